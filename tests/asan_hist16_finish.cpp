// tests/asan_hist16_finish.cpp -- k_hist16_finish (column stage and last column) under AddressSanitizer, as a stand-alone
// program over the emulator build of the product's kernels (device buffers are plain heap blocks there, so an out-of-bounds
// global load or store of a kernel is caught: the columns' 16-byte loads and stores of the sub-bucket starts, the rows of
// low-digit sums and the statistics behind the cursors, the tickets behind the statistics).  Host code only;
// `make -C tests/emu -f asan_hist16.mk` builds it, tests/test_asan_hist16_finish.py builds and runs it.
//
// The hooks (SFX_TINY=0, SFX_HYBRID_MIN=1, SFX_MAX_GRID=3, SFX_HYBRID_CAP=100) are set here, before the first call; they are
// read once per process, so the order of the workgroups is the program's argument: "forward", or "reverse"
// (SFX_FINISH_REVERSE=1: workgroup i does the work of grid - 1 - i, and the first stretch and column 0 finish last).
// Through the host-pointer entry sfx_build_sa_u32: a 4-bit text whose lowest and highest symbol occur once each, as its last
// two bytes (the first and the last column of 2048 sub-buckets are empty), a DNA text with a planted sub-bucket of 300 suffixes
// (oversized under the lowered cap), and uniform texts of 1 and 4 bits per symbol; each result against a std::sort of the suffix
// start positions.
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
    std::vector<uint32_t> want(n);
    for (size_t p = 0; p < n; p++) want[p] = (uint32_t)p;
    // (two suffixes differ within a few dozen bytes; a suffix that is a prefix of the other sorts first)
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
    free(sa);
    free(t);
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
    CHECK(argc == 2 && (!strcmp(argv[1], "forward") || !strcmp(argv[1], "reverse")));
    setenv("SFX_TINY", "0", 1);
    setenv("SFX_HYBRID_MIN", "1", 1);
    setenv("SFX_MAX_GRID", "3", 1);
    setenv("SFX_HYBRID_CAP", "100", 1);
    setenv("SFX_FINISH_REVERSE", !strcmp(argv[1], "reverse") ? "1" : "0", 1);
    int cases = 0;
    {
        std::vector<uint8_t> v = uniform(2 * T + 77, 14, 1201, 41u);
        v[v.size() - 2] = 40;
        v[v.size() - 1] = 55;
        run(v, "empty-end-columns");
        cases++;
    }
    {
        std::vector<uint8_t> v = uniform(40000, 4, 5);
        const std::vector<uint8_t> tails = uniform(300 * 7, 4, 6);
        const uint8_t block[9] = {42, 40, 43, 43, 40, 41, 40, 42, 41};
        for (size_t k = 0; k < 300; k++) {
            v.insert(v.end(), block, block + 9);
            v.insert(v.end(), tails.begin() + 7 * k, tails.begin() + 7 * k + 7);
        }
        run(v, "planted-oversized");
        cases++;
    }
    run(uniform(2 * T + 33, 2, 11), "sigma2");
    cases++;
    run(uniform(9 * T + 3 * 8 + 5, 16, 12), "sigma16");
    cases++;
    sfx_release_cached_buffers();                                           // (the pool of staging buffers: no leak report)
    printf("asan_hist16_finish ok: %s, %d cases\n", argv[1], cases);
    return 0;
}
