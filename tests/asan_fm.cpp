// tests/asan_fm.cpp -- the FM-index entry points under AddressSanitizer, as a stand-alone program over the emulator build
// of the product's kernels (device buffers are plain heap blocks there, so an out-of-bounds global load or store of a
// kernel is caught).  Every buffer is allocated at exactly its size.  Host code only; by hand:
//
//     make -C tests/emu asan -W ../../suffix_amd/csrc/sfx_api.hip   # (-W: sfx_fm.hip is part of sfx_api.hip's translation
//                                                                   #  unit and that Makefile does not name it)
//     clang++ -O1 -g -std=c++17 -fsanitize=address -I include tests/asan_fm.cpp \
//         -L tests/emu/asan -lsuffix_emu -Wl,-rpath,$PWD/tests/emu/asan -o tests/emu/asan/asan_fm
//     tests/emu/asan/asan_fm               # prints "asan_fm ok: <cases> cases" (1681 of them; about ten minutes: a fiber per lane)
//
// Per case (200 random texts of 0-300 bytes over 1-5 symbols and over all 256, every sample step of {0, 1, 2, 8, 64} with
// every occ_step of {0, 32, 64, 128, 4096}): the pair from sfx_bwt_u32, the index through sfx_fm_create_dev (the
// transform at an odd address) and sfx_fm_create, every interval against a scan of the text, every rank against the
// table; then the inputs creation does not prove: flipped bwt bytes, samples swapped and shifted inside [1, n] -- refused,
// or every answer in bounds -- and the refusals (samples of 0, n + 1 and 2^32 - 1, equal samples, ranks >= n).
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
    static const uint32_t steps[5] = {0, 1, 2, 8, 64}, occs[5] = {0, 32, 64, 128, 4096};
    int cases = 0;
    for (int it = 0; it < 200; it++) {
        const int sigma = it % 7 == 3 ? 256 : pick(1, 5);
        const unsigned char alpha[] = {'a', 'b', 0, 0xFF, 'z'};
        const uint32_t s = steps[it % 5], occ = occs[(it / 5) % 5];
        // (a fiber per lane: the whole text as one chain, or 64 lanes per rank, only on short texts)
        const uint64_t n = it % 11 == 0 ? (uint64_t)pick(0, 2) : (uint64_t)pick(1, s == 0 || occ == 4096 ? 80 : 300);
        std::string T(n, '\0');
        for (uint64_t i = 0; i < n; i++) T[i] = sigma == 256 ? (char)rng() : (char)alpha[pick(0, sigma - 1)];
        const uint8_t* Tp = reinterpret_cast<const uint8_t*>(T.data());
        Exact<uint32_t> sa(n);
        CHECK(sfx_build_sa_u32(Tp, n, sa.p) == SFX_OK);
        const uint64_t cnt = sfx_bwt_sample_count(n, s);
        Exact<uint8_t> Braw(n + 1);
        uint8_t* B = Braw.p + 1;                       // an odd address
        Exact<uint32_t> M(cnt);
        CHECK(sfx_bwt_u32(Tp, n, sa.p, s, B, M.p) == SFX_OK);

        // patterns: substrings, changed substrings, a foreign byte, one longer than the text, the empty one
        std::vector<std::string> qs = {"", std::string(1, '\x7e'), T + "a"};
        for (int k = 0; k < 24 && n; k++) {
            std::string q = T.substr((size_t)pick(0, (int)n - 1), (size_t)pick(1, 40));
            if (k % 3 == 2) q[(size_t)pick(0, (int)q.size() - 1)] = k % 2 ? '\x7e' : T[(size_t)pick(0, (int)n - 1)];
            qs.push_back(q);
        }
        std::string blob;
        Exact<uint64_t> off(qs.size() + 1);
        off.p[0] = 0;
        for (size_t k = 0; k < qs.size(); k++) { blob += qs[k]; off.p[k + 1] = blob.size(); }
        Exact<uint8_t> Qraw(blob.size() + 1);
        uint8_t* Q = Qraw.p + 1;
        memcpy(Q, blob.data(), blob.size());
        // the definition: the ranks whose suffix begins with q are contiguous
        std::vector<uint32_t> ws(qs.size(), 0), we(qs.size(), 0);
        for (size_t k = 0; k < qs.size(); k++) {
            if (qs[k].empty()) continue;
            uint64_t a = n, b = 0;
            for (uint64_t r = 0; r < n; r++)
                if (T.compare(sa.p[r], qs[k].size(), qs[k]) == 0) { a = std::min(a, r); b = r + 1; }
            if (b) { ws[k] = (uint32_t)a; we[k] = (uint32_t)b; }
        }
        for (int host = 0; host < 2; host++) {
            sfx_fm* fm = nullptr;
            CHECK((host ? sfx_fm_create(B, n, M.p, cnt, s, occ, &fm) : sfx_fm_create_dev(B, n, M.p, cnt, s, occ, nullptr, &fm)) == SFX_OK && fm);
            sfx_fm_info_t info;
            CHECK(sfx_fm_info(fm, &info) == SFX_OK && info.n == n && info.nsamples == cnt && info.sample_step == s);
            CHECK(n == 0 || info.bytes <= sfx_fm_bytes(n, s, occ));
            Exact<uint32_t> gs(qs.size()), ge(qs.size());
            CHECK((host ? sfx_fm_count(fm, Q, off.p, qs.size(), gs.p, ge.p) : sfx_fm_count_dev(fm, Q, off.p, qs.size(), gs.p, ge.p, nullptr)) == SFX_OK);
            CHECK(!memcmp(gs.p, ws.data(), qs.size() * 4) && !memcmp(ge.p, we.data(), qs.size() * 4));
            Exact<uint32_t> pos(n + 2), ranks(n + 2);
            CHECK((host ? sfx_fm_lookup(fm, nullptr, 0, n + 2, pos.p) : sfx_fm_lookup_dev(fm, nullptr, 0, n + 2, pos.p, nullptr)) == SFX_OK);
            CHECK(!n || !memcmp(pos.p, sa.p, n * 4));
            CHECK(pos.p[n] == 0xFFFFFFFFu && pos.p[n + 1] == 0xFFFFFFFFu);
            for (uint64_t i = 0; i < n + 2; i++) ranks.p[i] = (uint32_t)(n + 1 - i);
            CHECK(sfx_fm_lookup_dev(fm, ranks.p, 0, n + 2, pos.p, nullptr) == SFX_OK);
            for (uint64_t i = 2; i < n + 2; i++) CHECK(pos.p[i] == sa.p[n + 1 - i]);
            CHECK(pos.p[0] == 0xFFFFFFFFu && pos.p[1] == 0xFFFFFFFFu);
            CHECK(sfx_fm_count_dev(fm, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == SFX_OK);
            sfx_fm_destroy(fm);
            cases++;
        }
        if (n < 2) continue;
        // pairs nobody has made: refused, or every answer in bounds
        for (int kind = 0; kind < 7; kind++) {
            std::vector<uint8_t> b2(B, B + n);
            std::vector<uint32_t> m2(M.p, M.p + cnt);
            if (kind == 0) b2[(size_t)pick(0, (int)n - 1)] ^= (uint8_t)pick(1, 255);
            if (kind == 1) for (uint64_t i = 0; i < n; i++) b2[i] = (uint8_t)rng();
            if (kind == 2) std::swap(m2[(size_t)pick(0, (int)cnt - 1)], m2[(size_t)pick(0, (int)cnt - 1)]);
            if (kind == 3) m2[(size_t)pick(0, (int)cnt - 1)] = (uint32_t)pick(1, (int)n);
            if (kind == 4) m2[(size_t)pick(0, (int)cnt - 1)] = 0;
            if (kind == 5) m2[(size_t)pick(0, (int)cnt - 1)] = (uint32_t)(n + 1 + (uint64_t)pick(0, 1) * (0xFFFFFFFFull - n - 1));
            if (kind == 6 && cnt >= 2) m2[0] = m2[1];
            Exact<uint8_t> Bx(n);
            Exact<uint32_t> Mx(cnt);
            memcpy(Bx.p, b2.data(), n);
            memcpy(Mx.p, m2.data(), cnt * 4);
            sfx_fm* fm = nullptr;
            const int rc = sfx_fm_create_dev(Bx.p, n, Mx.p, cnt, s, occ, nullptr, &fm);
            CHECK(rc == SFX_OK || rc == SFX_ERR_ARG);
            CHECK((rc == SFX_OK) == (fm != nullptr));
            CHECK(!(kind == 4 || kind == 5 || (kind == 6 && cnt >= 2)) || rc == SFX_ERR_ARG);
            cases++;
            if (!fm) continue;
            Exact<uint32_t> gs(qs.size()), ge(qs.size()), pos(n + 1);
            CHECK(sfx_fm_count_dev(fm, Q, off.p, qs.size(), gs.p, ge.p, nullptr) == SFX_OK);
            for (size_t k = 0; k < qs.size(); k++) CHECK(gs.p[k] <= ge.p[k] && ge.p[k] <= n);
            CHECK(sfx_fm_lookup_dev(fm, nullptr, 0, n + 1, pos.p, nullptr) == SFX_OK);
            for (uint64_t i = 0; i <= n; i++) CHECK(pos.p[i] < n || pos.p[i] == 0xFFFFFFFFu);
            sfx_fm_destroy(fm);
        }
    }
    sfx_release_cached_buffers();
    printf("asan_fm ok: %d cases\n", cases);
    return 0;
}
