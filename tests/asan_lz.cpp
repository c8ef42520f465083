// tests/asan_lz.cpp -- the LZ77 entry points under AddressSanitizer, as a stand-alone program over the emulator build of
// the product's kernels (device buffers are plain heap blocks there, so an out-of-bounds global load or store of a kernel
// is caught).  Every buffer, the workspaces included, is allocated at exactly its size.  Host code only; by hand:
//
//     make -C tests/emu asan -W ../../suffix_amd/csrc/sfx_api.hip   # (-W: sfx_lz.hip is part of sfx_api.hip's translation
//                                                                   #  unit and that Makefile does not name it)
//     clang++ -O1 -g -std=c++17 -fsanitize=address -I include tests/asan_lz.cpp \
//         -L tests/emu/asan -lsuffix_emu -Wl,-rpath,$PWD/tests/emu/asan -o tests/emu/asan/asan_lz
//     SFX_LZ_TILE=8 SFX_LZ_LEVELS=2 SFX_MAX_GRID=3 SFX_LZ_ROUNDS_CHECK=1 tests/emu/asan/asan_lz
//     SFX_LZ_TILE=4 SFX_LZ_LEVELS=2 tests/emu/asan/asan_lz ; SFX_LZ_TILE=16 SFX_LZ_LEVELS=3 tests/emu/asan/asan_lz ; tests/emu/asan/asan_lz
//                                                                   # each prints "asan_lz ok: <cases> cases"
//
// Per text (300 random ones of 0-300 bytes over 1-4 symbols and over all 256, every third with its first half doubled, and
// "a" * n): the longest-previous-factor array by brute force, sfx_lz_parse_dev at min_len 1, 2, 3, 8 with capacity n, z - 1
// and 0 against the definition as a loop, sfx_lz_decode_dev back to the text; every tenth text through sfx_lz77_u32 and
// sfx_unlz.  Then what nobody computed: random rep / src arrays (entries past the text, sources that do not point
// backwards) -- refused, or parsed by the definition -- and damaged phrase lists (a zero length, a forward source, a wrong
// sum, a literal of 2 bytes), which must be refused with the output untouched.
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
static const uint32_t kNone = 0xFFFFFFFFu;

struct Phrases { std::vector<uint32_t> begin, len; std::vector<char> copy; };
static Phrases reference(const std::vector<uint32_t>& rep, uint32_t min_len)
{
    Phrases f;
    const uint64_t n = rep.size();
    for (uint64_t p = 0; p < n;) {
        const uint64_t r = std::min<uint64_t>(rep[p], n - p);
        const bool c = r >= min_len;
        f.begin.push_back((uint32_t)p);
        f.len.push_back((uint32_t)(c ? r : 1));
        f.copy.push_back(c);
        p += f.len.back();
    }
    return f;
}

// parse over exact buffers -> rc; the phrases written (up to capacity) land in len / src / lit / begin
static int parse(const std::vector<uint32_t>& rep, const std::vector<uint32_t>& src, const std::string& T, uint32_t min_len, uint64_t cap,
                 std::vector<uint32_t>* begin, std::vector<uint32_t>* len, std::vector<uint32_t>* psrc, std::vector<uint8_t>* lit, uint64_t* z)
{
    const uint64_t n = rep.size(), wsb = sfx_lz_parse_workspace_bytes(n);
    Exact<uint32_t> R(n), S(n), B(cap), L(cap), P(cap);
    Exact<uint8_t> X(n), C(cap), W(wsb);
    if (n) { memcpy(R.p, rep.data(), n * 4); memcpy(S.p, src.data(), n * 4); memcpy(X.p, T.data(), n); }
    memset(W.p, 0xA5, wsb);
    const int rc = sfx_lz_parse_dev(R.p, S.p, X.p, n, min_len, B.p, L.p, P.p, C.p, cap, z, W.p, wsb, nullptr);
    const uint64_t k = rc == SFX_OK ? std::min<uint64_t>(*z, cap) : 0;
    begin->assign(B.p, B.p + k);
    len->assign(L.p, L.p + k);
    psrc->assign(P.p, P.p + k);
    lit->assign(C.p, C.p + k);
    return rc;
}
static int decode(const std::vector<uint32_t>& len, const std::vector<uint32_t>& src, const std::vector<uint8_t>& lit, uint64_t n, std::string* out)
{
    const uint64_t z = len.size(), wsb = sfx_lz_decode_workspace_bytes(n, z);
    Exact<uint32_t> L(z), S(z);
    Exact<uint8_t> C(z), O(n), W(wsb);
    if (z) { memcpy(L.p, len.data(), z * 4); memcpy(S.p, src.data(), z * 4); memcpy(C.p, lit.data(), z); }
    memset(O.p, 0xEE, n);
    memset(W.p, 0x5A, wsb);
    const int rc = sfx_lz_decode_dev(L.p, S.p, C.p, z, n, O.p, W.p, wsb, nullptr);
    out->assign((const char*)O.p, n);
    return rc;
}

int main()
{
    std::mt19937 rng(20261019);
    auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    static const uint32_t min_lens[4] = {1, 2, 3, 8};
    int cases = 0;
    for (int it = 0; it < 300; it++) {
        const int sigma = it % 7 == 3 ? 256 : pick(1, 4);
        const unsigned char alpha[] = {'a', 'b', 0, 0xFF};
        uint64_t n = it % 11 == 0 ? (uint64_t)pick(0, 2) : (uint64_t)pick(1, 300);
        std::string T(n, '\0');
        for (uint64_t i = 0; i < n; i++) T[i] = sigma == 256 ? (char)rng() : (char)alpha[pick(0, sigma - 1)];
        if (it % 3 == 1) { T = T.substr(0, n / 2) + T.substr(0, n / 2) + T.substr(0, n - 2 * (n / 2)); }
        if (it % 29 == 5) T.assign(n, 'a');
        n = T.size();
        // the longest-previous-factor array and a witness, by brute force
        std::vector<uint32_t> rep(n, 0), src(n, kNone);
        for (uint64_t p = 0; p < n; p++)
            for (uint64_t q = 0; q < p; q++) {
                uint64_t l = 0;
                while (p + l < n && T[q + l] == T[p + l]) l++;
                if (l > rep[p]) { rep[p] = (uint32_t)l; src[p] = (uint32_t)q; }
            }
        for (uint32_t m : min_lens) {
            const Phrases want = reference(rep, m);
            const uint64_t zw = want.len.size();
            for (uint64_t cap : {n, zw ? zw - 1 : 0, (uint64_t)0}) {
                std::vector<uint32_t> b, l, s;
                std::vector<uint8_t> c;
                uint64_t z = 99;
                CHECK(parse(rep, src, T, m, cap, &b, &l, &s, &c, &z) == SFX_OK && z == zw);
                const uint64_t k = std::min(z, cap);
                CHECK(l.size() == k && std::equal(l.begin(), l.end(), want.len.begin()) && std::equal(b.begin(), b.end(), want.begin.begin()));
                for (uint64_t i = 0; i < k; i++)
                    CHECK(want.copy[i] ? (s[i] == src[b[i]] && c[i] == 0) : (s[i] == kNone && c[i] == (uint8_t)T[b[i]]));
                if (k == z && n) {
                    std::string back;
                    CHECK(decode(l, s, c, n, &back) == SFX_OK && back == T);
                }
                cases++;
            }
        }
        if (it % 10 == 0) {                                                        // the host entry points build the table themselves
            Exact<uint32_t> B(n), L(n), S(n);
            Exact<uint8_t> C(n), O(n);
            uint64_t z = 0;
            CHECK(sfx_lz77_u32((const uint8_t*)T.data(), n, nullptr, nullptr, 2, B.p, L.p, S.p, C.p, n, &z) == SFX_OK);
            const Phrases want = reference(rep, 2);
            CHECK(z == want.len.size() && std::equal(want.len.begin(), want.len.end(), L.p));
            CHECK(sfx_unlz(L.p, S.p, C.p, z, n, O.p) == SFX_OK && !memcmp(O.p, T.data(), n));
            cases++;
        }
        if (n < 2) continue;
        // arrays nobody computed: refused, or the definition's phrases
        for (int kind = 0; kind < 3; kind++) {
            std::vector<uint32_t> r2(n), s2(n);
            for (uint64_t p = 0; p < n; p++) {
                r2[p] = (uint32_t)pick(0, pick(0, 3) ? (int)std::min<uint64_t>(n - p, 9) : (int)(n - p));
                s2[p] = p ? (uint32_t)pick(0, (int)p - 1) : kNone;
            }
            r2[0] = 0;
            const uint32_t m = min_lens[pick(0, 3)];
            if (kind == 1) r2[(size_t)pick(0, (int)n - 1)] = pick(0, 1) ? kNone : (uint32_t)n + 1;
            const Phrases want = reference(r2, m);
            if (kind == 2) {
                const size_t k = (size_t)pick(0, (int)want.len.size() - 1);
                s2[want.begin[k]] = pick(0, 1) ? want.begin[k] : kNone - 1;
            }
            bool bad = false;
            for (uint64_t p = 0; p < n; p++) bad |= r2[p] > n - p;
            for (size_t k = 0; k < want.len.size(); k++) bad |= want.copy[k] && s2[want.begin[k]] >= want.begin[k];
            std::vector<uint32_t> b, l, s;
            std::vector<uint8_t> c;
            uint64_t z = 99;
            const int rc = parse(r2, s2, T, m, n, &b, &l, &s, &c, &z);
            CHECK(rc == (bad ? SFX_ERR_ARG : SFX_OK));
            if (!bad) {
                CHECK(z == want.len.size() && l == want.len && b == want.begin);
                std::string back;                                                  // (no factorization of T, but a valid list)
                CHECK(decode(l, s, c, n, &back) == SFX_OK);
            }
            cases++;
        }
        // damaged lists: refused, the output untouched
        {
            const Phrases want = reference(rep, 1);
            std::vector<uint32_t> b, l, s;
            std::vector<uint8_t> c;
            uint64_t z = 0;
            CHECK(parse(rep, src, T, 1, n, &b, &l, &s, &c, &z) == SFX_OK);
            for (int kind = 0; kind < 5; kind++) {
                std::vector<uint32_t> l2 = l, s2 = s;
                uint64_t n2 = n;
                const size_t k = (size_t)pick(0, (int)z - 1);
                if (kind == 0) l2[k] = 0;
                if (kind == 1) { s2[k] = b[k] + (uint32_t)pick(0, 1); }
                if (kind == 2) n2 = n + (pick(0, 1) ? 1 : (uint64_t)-1);
                if (kind == 3) { size_t j = 0; while (s[j] != kNone) j++; l2[j] = 2; n2 = n + 1; }
                if (kind == 4) s2[0] = 0;
                if (n2 == 0) continue;
                std::string back;
                CHECK(decode(l2, s2, c, n2, &back) == SFX_ERR_ARG);
                CHECK(back == std::string(n2, '\xEE'));
                cases++;
            }
        }
    }
    // the refusals
    uint64_t z = 0;
    CHECK(sfx_lz_parse_dev(nullptr, nullptr, nullptr, 0, 1, nullptr, nullptr, nullptr, nullptr, 0, &z, nullptr, 0, nullptr) == SFX_OK && z == 0);
    CHECK(sfx_lz_parse_dev(nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, &z, nullptr, 0, nullptr) == SFX_ERR_ARG);
    CHECK(sfx_lz_parse_dev(nullptr, nullptr, nullptr, 1ull << 32, 1, nullptr, nullptr, nullptr, nullptr, 0, &z, nullptr, 0, nullptr) == SFX_ERR_TOO_LARGE);
    CHECK(sfx_lz_decode_dev(nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, 0, nullptr) == SFX_OK);
    CHECK(sfx_lz_decode_dev(nullptr, nullptr, nullptr, 1, 1ull << 32, nullptr, nullptr, 0, nullptr) == SFX_ERR_TOO_LARGE);
    sfx_release_cached_buffers();
    printf("asan_lz ok: %d cases\n", cases);
    return 0;
}
