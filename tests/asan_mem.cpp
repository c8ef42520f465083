// tests/asan_mem.cpp -- the maximal-exact-match entry points under AddressSanitizer, as a stand-alone program over the
// emulator build of the product's kernels (device buffers are plain heap blocks there, so an out-of-bounds global load or
// store of a kernel is caught).  Every buffer, the workspace included, is allocated at exactly its size.  Host code only;
// by hand:
//
//     make -C tests/emu asan -W ../../suffix_amd/csrc/sfx_api.hip   # (-W: sfx_mem.hip is part of sfx_api.hip's translation
//                                                                   #  unit and that Makefile does not name it)
//     clang++ -O1 -g -std=c++17 -fsanitize=address -I include tests/asan_mem.cpp \
//         -L tests/emu/asan -lsuffix_emu -Wl,-rpath,$PWD/tests/emu/asan -o tests/emu/asan/asan_mem
//     SFX_MEM_TILE=8 SFX_MAX_GRID=3 tests/emu/asan/asan_mem ; SFX_MEM_TILE=8 SFX_MAX_GRID=3 SFX_MEM_BISECT=1 tests/emu/asan/asan_mem
//     SFX_MEM_TILE=5 SFX_MAX_GRID=16 tests/emu/asan/asan_mem               # each prints "asan_mem ok: <cases> cases"
//
// Per pair (16 random ones: T of 1-40 bytes and Q of 1-30 over 1-4 symbols, Q with a planted piece of T and a byte T
// lacks; every fifth T cut into documents, empty ones among them; and the runs a^n against a^m): the matches by the
// definition as a double loop, then sfx_mems_dev / sfx_index_mems_dev / sfx_gindex_mems_dev at min_len 1, 2 and 4 with both
// flag values and capacity Z, Z - 1 and 0, a pair limit of P and of P - 1 (refused: nothing written), and every fifth pair
// through sfx_index_mems / sfx_gindex_mems.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <tuple>
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
typedef std::tuple<uint32_t, uint32_t, uint32_t> Triple;

struct Text {
    std::string t;
    std::vector<uint64_t> starts;                     // one entry per document
    std::vector<uint32_t> sa, da;
    std::vector<uint64_t> lo, hi;                     // per position: its document's bounds
};
static void finish(Text* x)
{
    const size_t n = x->t.size();
    x->lo.assign(n, 0);
    x->hi.assign(n, n);
    x->da.assign(n, 0);
    std::vector<uint32_t> doc(n, 0);
    for (size_t d = 0; d < x->starts.size(); d++) {
        const uint64_t a = x->starts[d], b = d + 1 < x->starts.size() ? x->starts[d + 1] : n;
        for (uint64_t p = a; p < b; p++) { x->lo[p] = a; x->hi[p] = b; doc[p] = (uint32_t)d; }
    }
    x->sa.resize(n);
    for (size_t p = 0; p < n; p++) x->sa[p] = (uint32_t)p;
    // the truncated suffixes in their order; equal ones by document (the order of sfx_build_gsa_u32)
    std::sort(x->sa.begin(), x->sa.end(), [&](uint32_t a, uint32_t b) {
        const int c = x->t.compare(a, x->hi[a] - a, x->t, b, x->hi[b] - b);
        return c != 0 ? c < 0 : a < b;
    });
    for (size_t r = 0; r < n; r++) x->da[r] = doc[x->sa[r]];
}
static std::vector<Triple> brute(const Text& x, const std::string& q, uint32_t L, bool unique)
{
    const size_t n = x.t.size(), m = q.size();
    std::vector<uint32_t> rank(n);
    for (size_t r = 0; r < n; r++) rank[x.sa[r]] = (uint32_t)r;
    std::vector<Triple> out;
    for (size_t i = 0; i < m; i++) {
        std::vector<std::pair<uint32_t, Triple>> found;
        for (size_t p = 0; p < n; p++) {
            if (i > 0 && p > x.lo[p] && q[i - 1] == x.t[p - 1]) continue;
            size_t l = 0;
            while (i + l < m && p + l < x.hi[p] && q[i + l] == x.t[p + l]) l++;
            if (l < L) continue;
            if (unique) {
                size_t occ = 0;
                for (size_t s = 0; s < n; s++) occ += s + l <= x.hi[s] && x.t.compare(s, l, x.t, p, l) == 0;
                if (occ != 1) continue;
            }
            found.push_back({rank[p], Triple((uint32_t)i, (uint32_t)p, (uint32_t)l)});
        }
        std::sort(found.begin(), found.end());
        for (auto& f : found) out.push_back(f.second);
    }
    return out;
}

static long cases = 0;
// one `_dev` call over exact buffers; which: 0 table, 1 index, 2 collection index
static int call(int which, const Text& x, sfx_index* ix, sfx_gindex* gx, const std::string& q, uint32_t L, uint32_t flags, uint64_t limit,
                uint64_t cap, std::vector<Triple>* got, uint64_t* P, uint64_t* Z)
{
    const uint64_t n = x.t.size(), m = q.size(), wsb = sfx_mems_workspace_bytes(m, limit);
    Exact<uint8_t> T(n), Q(m), W(wsb);
    Exact<uint32_t> S(n), A(cap), B(cap), C(cap);
    memcpy(T.p, x.t.data(), n);
    memcpy(Q.p, q.data(), m);
    memcpy(S.p, x.sa.data(), n * 4);
    memset(W.p, 0xA5, wsb);
    memset(A.p, 0x5A, cap * 4);
    memset(B.p, 0x5A, cap * 4);
    memset(C.p, 0x5A, cap * 4);
    uint32_t *a = cap ? A.p : nullptr, *b = cap ? B.p : nullptr, *c = cap ? C.p : nullptr;
    int rc;
    if (which == 0) rc = sfx_mems_dev(T.p, n, S.p, Q.p, m, L, flags, limit, a, b, c, cap, P, Z, W.p, wsb, nullptr);
    else if (which == 1) rc = sfx_index_mems_dev(ix, Q.p, m, L, flags, limit, a, b, c, cap, P, Z, W.p, wsb, nullptr);
    else rc = sfx_gindex_mems_dev(gx, Q.p, m, L, flags, limit, a, b, c, cap, P, Z, W.p, wsb, nullptr);
    got->clear();
    const uint64_t k = rc == SFX_OK ? std::min<uint64_t>(*Z, cap) : 0;
    for (uint64_t j = 0; j < k; j++) got->push_back(Triple(A.p[j], B.p[j], C.p[j]));
    for (uint64_t j = k; j < cap; j++) CHECK(A.p[j] == 0x5A5A5A5Au && B.p[j] == 0x5A5A5A5Au && C.p[j] == 0x5A5A5A5Au);
    cases++;
    return rc;
}
static void exercise(const Text& x, const std::string& q, bool host_too)
{
    const uint64_t n = x.t.size(), m = q.size();
    const bool docs = x.starts.size() > 1;
    sfx_index* ix = nullptr;
    sfx_gindex* gx = nullptr;
    const uint8_t* t8 = reinterpret_cast<const uint8_t*>(x.t.data());
    if (!docs) CHECK(sfx_index_create(t8, n, x.sa.data(), &ix) == SFX_OK);
    CHECK(sfx_gindex_create(t8, n, x.starts.data(), x.starts.size(), x.sa.data(), x.da.data(), &gx) == SFX_OK);
    for (uint32_t L : {1u, 2u, 4u})
        for (uint32_t flags = 0; flags < 2; flags++) {
            const std::vector<Triple> want = brute(x, q, L, flags != 0);
            std::vector<Triple> got;
            uint64_t P = 0, Z = 0, P2 = 0, Z2 = 0;
            for (int which = docs ? 2 : 0; which < 3; which++) {
                CHECK(call(which, x, ix, gx, q, L, flags, m * n, want.size(), &got, &P, &Z) == SFX_OK);
                CHECK(Z == want.size() && got == want && P <= m * n);
                CHECK(call(which, x, ix, gx, q, L, flags, m * n, 0, &got, &P2, &Z2) == SFX_OK && P2 == P && Z2 == Z);
                if (Z) {
                    CHECK(call(which, x, ix, gx, q, L, flags, m * n, Z - 1, &got, &P2, &Z2) == SFX_OK && P2 == P && Z2 == Z);
                    CHECK(std::equal(got.begin(), got.end(), want.begin()) && got.size() == Z - 1);
                }
                if (P) {
                    CHECK(call(which, x, ix, gx, q, L, flags, P, want.size(), &got, &P2, &Z2) == SFX_OK && P2 == P && got == want);
                    if (P > 1) CHECK(call(which, x, ix, gx, q, L, flags, P - 1, want.size(), &got, &P2, &Z2) == SFX_OK && P2 == P && Z2 == 0 && got.empty());
                }
            }
            if (host_too) {
                std::vector<uint32_t> a(want.size() + 1), b(want.size() + 1), c(want.size() + 1);
                const uint8_t* q8 = reinterpret_cast<const uint8_t*>(q.data());
                const int rc = docs ? sfx_gindex_mems(gx, q8, m, L, flags, 1ull << 30, a.data(), b.data(), c.data(), a.size(), &P2, &Z2)
                                    : sfx_index_mems(ix, q8, m, L, flags, 1ull << 30, a.data(), b.data(), c.data(), a.size(), &P2, &Z2);
                CHECK(rc == SFX_OK && P2 == P && Z2 == want.size());
                for (size_t k = 0; k < want.size(); k++) CHECK(Triple(a[k], b[k], c[k]) == want[k]);
                cases++;
            }
        }
    if (ix) sfx_index_destroy(ix);
    sfx_gindex_destroy(gx);
}

int main()
{
    std::mt19937 rng(20261019);
    auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    for (int it = 0; it < 16; it++) {
        const int sigma = pick(1, 4);
        const char alpha[5] = {'a', 'b', (char)0, (char)255, 'z'};
        Text x;
        const int n = pick(1, 40);
        for (int k = 0; k < n; k++) x.t.push_back(alpha[pick(0, sigma - 1)]);
        std::string q;
        const int m = pick(1, 30);
        for (int k = 0; k < m; k++) q.push_back(alpha[pick(0, sigma)]);           // (one symbol the text lacks)
        if (it % 2) {
            const int a = pick(0, n - 1);
            q.insert((size_t)pick(0, m - 1), x.t.substr((size_t)a, (size_t)pick(1, 12)));
            q.resize(std::min<size_t>(q.size(), 30));
        }
        x.starts.push_back(0);
        if (it % 5 == 0)
            for (int p = pick(1, 9); p < n; p += pick(0, 9)) x.starts.push_back((uint64_t)p);   // (a step of 0: an empty document)
        finish(&x);
        exercise(x, q, it % 5 < 2);
    }
    for (int n : {1, 8, 9, 25})
        for (int m : {3, 8, 26}) {
            Text x;
            x.t.assign((size_t)n, 'a');
            x.starts.push_back(0);
            finish(&x);
            exercise(x, std::string((size_t)m, 'a'), true);
        }
    printf("asan_mem ok: %ld cases\n", cases);
    return 0;
}
