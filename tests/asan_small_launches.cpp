// tests/asan_small_launches.cpp -- the small launches of the hybrid build (round 10) under AddressSanitizer, as a stand-alone
// program over the emulator build of the product's kernels (device buffers are plain heap blocks there, so an out-of-bounds
// global load or store of a kernel is caught):
//   - k_byte_presence's slots and tickets in the radix scratch, the flag words behind the totals, the LUT its last workgroup writes;
//   - k_hist16_finish's sums over the first two rows of every stretch and the column stage's sixteen loads of them;
//   - the counter lines that the histogram sweep zeroes for k_tie_direct and k_tie_totals zeroes again.
// Host code only; `make -C tests/emu -f asan_small.mk` builds it, tests/test_asan_small_launches.py builds and runs it.
//
// The hooks (SFX_TINY=0, SFX_HYBRID_MIN=1, SFX_MAX_GRID) are set here, before the first call; they are read once per process, so
// the program's arguments are the grid cap and the order of the workgroups: "forward", or "reverse" (SFX_FINISH_REVERSE=1:
// workgroup i does the work of grid - 1 - i in every kernel with a last-arriver stage).
//   cap 3:  stretches of one row or none -- 1, 2, 3, 4 and 8-bit symbols, symbols that include 0x00 and 0xFF, a text one byte
//           behind a 16-byte boundary (the device entry point, twice into one workspace filled with 0xFF before each call);
//   cap 24: n = 24 * 16384 -- 24 rows of partial counts, three per stretch: the summed path (4-bit symbols), and
//           n = 24 * 16384 + 5 with 8-bit symbols: 20 rows, six stretches of three, one of two, one empty.
// Through the host-pointer entry sfx_build_sa_u32 unless said otherwise; each result against a std::sort of the suffix start positions.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "suffix_hip.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static const size_t T = 16384;

static void compare(const uint8_t* t, size_t n, const uint32_t* sa, const char* what);

static void run(const std::vector<uint8_t>& text, const char* what)
{
    const size_t n = text.size();
    // exactly n bytes and n entries on the heap: a byte or an entry beyond either is an error
    uint8_t* t = (uint8_t*)malloc(n);
    uint32_t* sa = (uint32_t*)malloc(n * sizeof(uint32_t));
    CHECK(t && sa);
    memcpy(t, text.data(), n);
    memset(sa, 0xA5, n * sizeof(uint32_t));
    CHECK(sfx_build_sa_u32(t, n, sa) == SFX_OK);
    compare(t, n, sa, what);
    free(sa);
    free(t);
}

// the device entry point (device memory is the heap here): the text `offset` bytes behind a 16-byte boundary, a workspace of
// exactly sfx_sa_workspace_bytes(n), and the same build twice into it, filled with 0xFF before each call
static void run_dev_twice(const std::vector<uint8_t>& text, const char* what, size_t offset)
{
    const size_t n = text.size();
    uint8_t* block = (uint8_t*)aligned_alloc(16, (offset + n + 15) / 16 * 16);
    uint32_t* sa = (uint32_t*)malloc(n * sizeof(uint32_t));
    const uint64_t ws_bytes = sfx_sa_workspace_bytes(n);
    void* ws = aligned_alloc(256, (ws_bytes + 255) / 256 * 256);
    CHECK(block && sa && ws);
    uint8_t* t = block + offset;
    memcpy(t, text.data(), n);
    for (int again = 0; again < 2; again++) {
        memset(ws, 0xFF, ws_bytes);
        memset(sa, 0xA5, n * sizeof(uint32_t));
        CHECK(sfx_build_sa_u32_dev(t, n, sa, ws, ws_bytes, nullptr) == SFX_OK);
        compare(t, n, sa, what);
    }
    free(ws);
    free(sa);
    free(block);
}

static void compare(const uint8_t* t, size_t n, const uint32_t* sa, const char* what)
{
    std::vector<uint32_t> want(n);
    for (size_t p = 0; p < n; p++) want[p] = (uint32_t)p;
    std::sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) {
        const size_t la = n - a, lb = n - b;
        const int c = memcmp(t + a, t + b, std::min(la, lb));
        return c ? c < 0 : la < lb;
    });
    for (size_t r = 0; r < n; r++) {
        if (sa[r] != want[r]) {
            fprintf(stderr, "%s: rank %zu: %u, expected %u\n", what, r, sa[r], want[r]);
            exit(1);
        }
    }
}

static std::vector<uint8_t> uniform(size_t n, unsigned sigma, unsigned seed, unsigned base = 40u)
{
    std::mt19937 rng(seed);
    std::vector<uint8_t> v(n);
    for (size_t p = 0; p < n; p++) v[p] = (uint8_t)(base + rng() % sigma);
    return v;
}

int main(int argc, char** argv)
{
    CHECK(argc == 3 && (!strcmp(argv[1], "3") || !strcmp(argv[1], "24")) && (!strcmp(argv[2], "forward") || !strcmp(argv[2], "reverse")));
    setenv("SFX_TINY", "0", 1);
    setenv("SFX_HYBRID_MIN", "1", 1);
    setenv("SFX_MAX_GRID", argv[1], 1);
    setenv("SFX_FINISH_REVERSE", !strcmp(argv[2], "reverse") ? "1" : "0", 1);
    int cases = 0;
    if (!strcmp(argv[1], "3")) {
        run(uniform(2 * T + 33, 2, 11), "sigma2");
        run(uniform(2 * T + 17, 4, 12), "dna");
        run(uniform(2 * T + 7, 6, 13), "sigma6");
        run(uniform(9 * T + 3 * 8 + 5, 16, 14), "sigma16");
        run(uniform(2 * T + 5, 200, 15), "bytes8");
        cases += 5;
        {
            std::vector<uint8_t> v = uniform(2 * T + 3, 16, 16, 0u);
            for (uint8_t& c : v) if (c == 15) c = 0xFF;
            run(v, "bytes-00-ff");
            cases++;
        }
        run_dev_twice(uniform(2 * T + 21, 4, 17), "dna-unaligned-twice", 1);
        cases++;
    } else {
        run(uniform(24 * T, 16, 21), "sigma16-rows3");
        run(uniform(24 * T + 5, 200, 22), "bytes8-rows3-2-0");
        run_dev_twice(uniform(24 * T, 4, 23), "dna-rows3-twice", 0);
        cases += 3;
    }
    sfx_release_cached_buffers();                                           // (the pool of staging buffers: no leak report)
    printf("asan_small_launches ok: cap %s, %s, %d cases\n", argv[1], argv[2], cases);
    return 0;
}
