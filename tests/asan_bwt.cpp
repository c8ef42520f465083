// tests/asan_bwt.cpp -- the Burrows-Wheeler entry points under AddressSanitizer, as a stand-alone program over the
// emulator build of the product's kernels (device buffers are plain heap blocks there, so an out-of-bounds global load
// or store of a kernel is caught).  Every buffer is allocated at exactly its size.  Host code only; by hand:
//
//     make -C tests/emu asan
//     clang++ -O1 -g -std=c++17 -fsanitize=address -I include tests/asan_bwt.cpp \
//         -L tests/emu/asan -lsuffix_emu -Wl,-rpath,$PWD/tests/emu/asan -o tests/emu/asan/asan_bwt
//     tests/emu/asan/asan_bwt              # prints "asan_bwt ok: <cases> cases"
//
// Per case (random texts of 0-300 bytes over 1-5 symbols, every step of {0, 1, 2, 8, 64, 512}): the forward transform
// through sfx_bwt_dev and sfx_bwt_u32 against the definition, the inverse through sfx_unbwt_dev (text, bwt and output at
// odd addresses, a workspace of exactly sfx_unbwt_workspace_bytes) and sfx_unbwt; then the inputs nobody checks: tables
// without a zero entry, with two, all n - 1; transforms with a flipped byte, samples of 0, n + 1 and 2^32 - 1 -- no
// input may take a kernel out of its arrays.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "suffix_hip.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

template <class T> struct Exact {                     // exactly n elements on the heap
    T* p;
    size_t n;
    explicit Exact(size_t n_) : p((T*)malloc(n_ ? n_ * sizeof(T) : 1)), n(n_) {}
    Exact(const Exact&) = delete;
    ~Exact() { free(p); }
};

int main()
{
    std::mt19937 rng(20261018);
    auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    static const uint32_t steps[6] = {0, 1, 2, 8, 64, 512};
    int cases = 0;
    for (int it = 0; it < 600; it++) {
        const int sigma = pick(1, 5);
        const unsigned char alpha[] = {'a', 'b', 0, 0xFF, 'z'};
        const uint64_t n = it % 11 == 0 ? (uint64_t)pick(0, 2) : (uint64_t)pick(1, 300);
        const uint32_t s = steps[it % 6];
        Exact<uint8_t> Traw(n + 1);
        uint8_t* T = Traw.p + 1;                       // an odd address
        for (uint64_t i = 0; i < n; i++) T[i] = alpha[pick(0, sigma - 1)];
        Exact<uint32_t> sa(n);
        CHECK(sfx_build_sa_u32(T, n, sa.p) == SFX_OK);

        // the definition
        const uint64_t cnt = sfx_bwt_sample_count(n, s);
        CHECK(cnt == (n == 0 ? 0 : s == 0 ? 1 : (n + s - 1) / s));
        std::vector<uint8_t> wb;
        std::vector<uint32_t> ws(cnt, 0);
        if (n) wb.push_back(T[n - 1]);
        for (uint64_t r = 0; r < n; r++) {
            if (sa.p[r]) wb.push_back(T[sa.p[r] - 1]);
            if (sa.p[r] == 0 || (s && sa.p[r] % s == 0)) ws[s ? sa.p[r] / s : 0] = (uint32_t)(r + 1);
        }
        CHECK(wb.size() == n);

        Exact<uint8_t> Braw(n + 1), B2(n);
        uint8_t* B = Braw.p + 1;
        Exact<uint32_t> M(cnt), M2(cnt);
        CHECK(sfx_bwt_dev(T, n, sa.p, s, B, M.p, nullptr) == SFX_OK);
        CHECK(sfx_bwt_u32(T, n, it % 2 ? sa.p : nullptr, s, B2.p, M2.p) == SFX_OK);
        CHECK(!n || (!memcmp(B, wb.data(), n) && !memcmp(B2.p, wb.data(), n)));
        CHECK(!cnt || (!memcmp(M.p, ws.data(), cnt * 4) && !memcmp(M2.p, ws.data(), cnt * 4)));

        const uint64_t wsb = sfx_unbwt_workspace_bytes(n);
        Exact<uint8_t> Oraw(n + 3), O2(n);
        uint8_t* O = Oraw.p + 3;
        void* W = nullptr;
        CHECK(posix_memalign(&W, 256, wsb ? wsb : 1) == 0);
        memset(W, 0xFF, wsb);
        CHECK(sfx_unbwt_dev(B, n, M.p, cnt, s, O, W, wsb, nullptr) == SFX_OK);
        CHECK(sfx_unbwt(B2.p, n, M2.p, cnt, s, O2.p) == SFX_OK);
        CHECK(!n || (!memcmp(O, T, n) && !memcmp(O2.p, T, n)));
        cases++;
        if (n == 0) { free(W); continue; }

        // tables nobody checks
        for (int kind = 0; kind < 4; kind++) {
            Exact<uint32_t> bad(n);
            memcpy(bad.p, sa.p, n * 4);
            const uint64_t zero = (uint64_t)(std::find(sa.p, sa.p + n, 0u) - sa.p);
            if (kind == 0) bad.p[zero] = (uint32_t)(n - 1);
            if (kind == 1) bad.p[(zero + 1) % n] = 0;
            if (kind == 2) std::fill(bad.p, bad.p + n, (uint32_t)(n - 1));
            if (kind == 3) std::fill(bad.p, bad.p + n, 0u);
            CHECK(sfx_bwt_dev(T, n, bad.p, s, B, M.p, nullptr) == SFX_OK);
            cases++;
        }
        // pairs nobody has made: whatever comes back is SFX_OK or SFX_ERR_ARG, and nothing leaves its array
        for (int kind = 0; kind < 5; kind++) {
            memcpy(B, wb.data(), n);
            memcpy(M.p, ws.data(), cnt * 4);
            if (kind == 0) B[pick(0, (int)n - 1)] ^= (uint8_t)pick(1, 255);
            if (kind == 1) for (uint64_t i = 0; i < n; i++) B[i] = (uint8_t)rng();
            if (kind == 2) M.p[pick(0, (int)cnt - 1)] = 0;
            if (kind == 3) M.p[pick(0, (int)cnt - 1)] = (uint32_t)(n + 1);
            if (kind == 4) M.p[pick(0, (int)cnt - 1)] = 0xFFFFFFFFu;
            memset(W, kind & 1 ? 0x00 : 0xFF, wsb);
            const int rc = sfx_unbwt_dev(B, n, M.p, cnt, s, O, W, wsb, nullptr);
            CHECK(rc == SFX_OK || rc == SFX_ERR_ARG);
            CHECK(kind < 2 || rc == SFX_ERR_ARG);
            cases++;
        }
        free(W);
    }
    sfx_release_cached_buffers();
    printf("asan_bwt ok: %d cases\n", cases);
    return 0;
}
