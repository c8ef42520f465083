// tests/asan_compact_partition.cpp -- the compact-staging text-fed partition pass (k_partition_text) under AddressSanitizer, as
// a stand-alone program over the emulator build of the product's kernels (device buffers are plain heap blocks there, so an
// out-of-bounds global load or store of a kernel is caught: the tile loader's reads behind the text's last word, the short last
// tile's word-by-word loads, the rebuilt elements' stores).  Host code only; `make -C tests/emu -f asan_compact.mk` builds it,
// tests/test_asan_compact_partition.py builds and runs it.
//
// The hooks of tests/test_emu_compact_partition.py (SFX_TINY=0, SFX_HYBRID_MIN=1, SFX_MAX_GRID=3) are set here, before the first
// call.  Uniform texts of 2 and 8 bits per symbol through the host-pointer entry sfx_build_sa_u32, at n = 2 T + r (T = 16384:
// the kernel's tile) for a full last tile, one that holds a single position and one that ends inside a packed word, and a DNA
// text whose last positions all carry the largest code; each result against a std::sort of the suffix start positions.
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
    // (uniform symbols: two suffixes differ within a few bytes; a suffix that is a prefix of the other sorts first)
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

static std::vector<uint8_t> uniform(size_t n, unsigned sigma, unsigned seed)
{
    std::mt19937 rng(seed);
    std::vector<uint8_t> v(n);
    for (size_t p = 0; p < n; p++) v[p] = (uint8_t)(40u + rng() % sigma);
    return v;
}

int main()
{
    setenv("SFX_TINY", "0", 1);
    setenv("SFX_HYBRID_MIN", "1", 1);
    setenv("SFX_MAX_GRID", "3", 1);
    int cases = 0;
    const struct { unsigned sigma, spw; const char* name; } widths[] = {{4, 16, "dna"}, {200, 4, "bytes8"}};
    for (const auto& w : widths) {
        for (size_t r : {(size_t)0, (size_t)1, (size_t)w.spw + 1}) {
            char what[64];
            snprintf(what, sizeof(what), "%s-%zu", w.name, 2 * T + r);
            run(uniform(2 * T + r, w.sigma, 7u + (unsigned)r), what);
            cases++;
        }
    }
    {
        std::vector<uint8_t> v = uniform(2 * T + 15, 4, 99);
        for (size_t p = v.size() - 40; p < v.size(); p++) v[p] = 43;       // the largest code: windows into the spare words
        run(v, "dna-tail");
        cases++;
    }
    sfx_release_cached_buffers();                                           // (the pool of staging buffers: no leak report)
    printf("asan_compact_partition ok: %d cases\n", cases);
    return 0;
}
