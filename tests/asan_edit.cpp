// tests/asan_edit.cpp -- the k-error pattern search under AddressSanitizer and UBSan, as a stand-alone program over the
// emulator build of the product's kernels (device buffers are plain heap blocks there, so an out-of-bounds global load or
// store of a kernel is caught).  Every buffer, the workspace included, is allocated at exactly its size -- the text and
// the pattern bytes too, so an extension that loads outside its window or past the last pattern is caught.  Host code
// only, no part of pytest; by hand:
//
//     make -C tests/emu asan -W ../../suffix_amd/csrc/sfx_api.hip   # (-W: sfx_edit.hip is part of sfx_api.hip's
//                                                                   #  translation unit and that Makefile does not name it)
//     clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include tests/asan_edit.cpp \
//         -L tests/emu/asan -lsuffix_emu -Wl,-rpath,$PWD/tests/emu/asan -o tests/emu/asan/asan_edit
//     SFX_ED_TILE=8 SFX_MAX_GRID=3 tests/emu/asan/asan_edit               # prints "asan_edit ok: <cases> cases"
//
// (The emulator's asan build carries AddressSanitizer; the undefined-behaviour checks cover this program's own code.)
//
// Per text (3 random ones: 1-60 bytes over 1-4 symbols; the first cut into documents, empty ones among them; and the
// run a^33): 6 patterns of up to 24 bytes (sampled with edits -- insertions and deletions among them --, random,
// longer than the text; those of at most k bytes are left out), the occurrences by Sellers' recurrence with max-start
// tracking per document, then sfx_edit_dev / sfx_index_edit_dev / sfx_gindex_edit_dev at k = 1 and 3 with capacity Z
// and first given, capacity Z - 1 and first NULL, capacity 0 (the table entry alone), the limits (C - 1, H) and
// (C, H - 1) (refused: nothing written), and three of the texts through sfx_index_edit / sfx_gindex_edit.  A call that
// finds hits runs the library's radix sort, seconds each under the sanitizer: hence the few texts.
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
typedef std::tuple<uint32_t, uint32_t, uint32_t, uint32_t> Quad;       // pattern, tbegin, tend, dist

struct Text {
    std::string t;
    std::vector<uint64_t> starts;                     // one entry per document
    std::vector<uint32_t> sa, da;
    std::vector<uint64_t> hi;                         // per position: its document's end
};
static void finish(Text* x)
{
    const size_t n = x->t.size();
    x->hi.assign(n, n);
    x->da.assign(n, 0);
    std::vector<uint32_t> doc(n, 0);
    for (size_t d = 0; d < x->starts.size(); d++) {
        const uint64_t a = x->starts[d], b = d + 1 < x->starts.size() ? x->starts[d + 1] : n;
        for (uint64_t p = a; p < b; p++) { x->hi[p] = b; doc[p] = (uint32_t)d; }
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
// Sellers' recurrence per document, a cell = (distance, -start): the least pair is the least distance from the largest start
static std::vector<Quad> brute(const Text& x, const std::vector<std::string>& pats, uint32_t k, std::vector<uint64_t>* first)
{
    typedef std::pair<int64_t, int64_t> Cell;
    const size_t n = x.t.size();
    std::vector<Quad> out;
    first->assign(1, 0);
    for (size_t j = 0; j < pats.size(); j++) {
        const std::string& q = pats[j];
        const size_t m = q.size();
        for (size_t d = 0; d < x.starts.size(); d++) {
            const uint64_t lo = x.starts[d], hi = d + 1 < x.starts.size() ? x.starts[d + 1] : n;
            std::vector<Cell> col(m + 1), prev(m + 1);
            for (size_t i = 0; i <= m; i++) prev[i] = Cell((int64_t)i, -(int64_t)lo);
            for (uint64_t e = lo + 1; e <= hi; e++) {
                col[0] = Cell(0, -(int64_t)e);
                for (size_t i = 1; i <= m; i++) {
                    Cell v(prev[i - 1].first + (q[i - 1] != x.t[e - 1]), prev[i - 1].second);
                    v = std::min(v, Cell(prev[i].first + 1, prev[i].second));
                    v = std::min(v, Cell(col[i - 1].first + 1, col[i - 1].second));
                    col[i] = v;
                }
                if (col[m].first <= (int64_t)k) out.push_back(Quad((uint32_t)j, (uint32_t)-col[m].second, (uint32_t)e, (uint32_t)col[m].first));
                prev = col;
            }
        }
        std::sort(out.begin() + (*first)[j], out.end(), [](const Quad& a, const Quad& b) { return std::get<2>(a) < std::get<2>(b); });
        first->push_back(out.size());
    }
    return out;
}

static long cases = 0;
// one `_dev` call over exact buffers; which: 0 table, 1 index, 2 collection index
static int call(int which, const Text& x, sfx_index* ix, sfx_gindex* gx, const std::vector<std::string>& pats, uint32_t k, uint64_t limit,
                uint64_t hlimit, uint64_t cap, bool want_first, std::vector<Quad>* got, std::vector<uint64_t>* first, uint64_t* C, uint64_t* H,
                uint64_t* Z)
{
    const uint64_t n = x.t.size(), nq = pats.size(), wsb = sfx_edit_workspace_bytes(nq, k, limit, hlimit);
    std::string blob;
    std::vector<uint64_t> off(1, 0);
    for (const std::string& q : pats) { blob += q; off.push_back(blob.size()); }
    Exact<uint8_t> T(n), Q(blob.size()), W(wsb), M(cap);
    Exact<uint32_t> S(n), A(cap), B(cap), E(cap);
    Exact<uint64_t> O(nq + 1), F(nq + 1);
    memcpy(T.p, x.t.data(), n);
    memcpy(Q.p, blob.data(), blob.size());
    memcpy(S.p, x.sa.data(), n * 4);
    memcpy(O.p, off.data(), (nq + 1) * 8);
    memset(W.p, 0xA5, wsb);
    memset(A.p, 0x5A, cap * 4);
    memset(B.p, 0x5A, cap * 4);
    memset(E.p, 0x5A, cap * 4);
    memset(M.p, 0x5A, cap);
    memset(F.p, 0x5A, (nq + 1) * 8);
    uint32_t *a = cap ? A.p : nullptr, *b = cap ? B.p : nullptr, *e = cap ? E.p : nullptr;
    uint8_t* mm = cap ? M.p : nullptr;
    uint64_t* f = want_first ? F.p : nullptr;
    int rc;
    if (which == 0) rc = sfx_edit_dev(T.p, n, S.p, Q.p, O.p, nq, k, limit, hlimit, a, b, e, mm, cap, f, C, H, Z, W.p, wsb, nullptr);
    else if (which == 1) rc = sfx_index_edit_dev(ix, Q.p, O.p, nq, k, limit, hlimit, a, b, e, mm, cap, f, C, H, Z, W.p, wsb, nullptr);
    else rc = sfx_gindex_edit_dev(gx, Q.p, O.p, nq, k, limit, hlimit, a, b, e, mm, cap, f, C, H, Z, W.p, wsb, nullptr);
    got->clear();
    first->clear();
    const bool refused = rc == SFX_OK && (*C > limit || *H > hlimit);
    const uint64_t z = rc == SFX_OK ? std::min<uint64_t>(*Z, cap) : 0;
    for (uint64_t j = 0; j < z; j++) got->push_back(Quad(A.p[j], B.p[j], E.p[j], M.p[j]));
    for (uint64_t j = z; j < cap; j++) CHECK(A.p[j] == 0x5A5A5A5Au && B.p[j] == 0x5A5A5A5Au && E.p[j] == 0x5A5A5A5Au && M.p[j] == 0x5A);
    if (want_first && rc == SFX_OK && !refused) first->assign(F.p, F.p + nq + 1);
    if (!want_first || refused)
        for (uint64_t j = 0; j <= nq; j++) CHECK(F.p[j] == 0x5A5A5A5A5A5A5A5Aull);
    cases++;
    return rc;
}
static void exercise(const Text& x, const std::vector<std::string>& all, bool host_too)
{
    const uint64_t n = x.t.size();
    const bool docs = x.starts.size() > 1;
    sfx_index* ix = nullptr;
    sfx_gindex* gx = nullptr;
    const uint8_t* t8 = reinterpret_cast<const uint8_t*>(x.t.data());
    if (!docs) CHECK(sfx_index_create(t8, n, x.sa.data(), &ix) == SFX_OK);
    CHECK(sfx_gindex_create(t8, n, x.starts.data(), x.starts.size(), x.sa.data(), x.da.data(), &gx) == SFX_OK);
    for (uint32_t k : {1u, 3u}) {
        std::vector<std::string> pats;
        for (const std::string& q : all)
            if (q.size() > k) pats.push_back(q);
        const uint64_t nq = pats.size();
        if (!nq) continue;
        std::vector<uint64_t> wfirst, first;
        const std::vector<Quad> want = brute(x, pats, k, &wfirst);
        const uint64_t most = nq * (k + 1) * n, hmost = std::min<uint64_t>(most * (2 * k + 1), 0xFFFFFFFFull);
        std::vector<Quad> got;
        uint64_t C = 0, H = 0, Z = 0, C2 = 0, H2 = 0, Z2 = 0;
        for (int which = docs ? 2 : 0; which < 3; which++) {
            CHECK(call(which, x, ix, gx, pats, k, most, hmost, want.size(), true, &got, &first, &C, &H, &Z) == SFX_OK);
            CHECK(Z == want.size() && got == want && first == wfirst && C <= most && H <= hmost && H >= Z);
            if (which == 0)
                CHECK(call(which, x, ix, gx, pats, k, most, hmost, 0, true, &got, &first, &C2, &H2, &Z2) == SFX_OK && C2 == C && H2 == H && Z2 == Z &&
                      first == wfirst);
            if (Z) {
                CHECK(call(which, x, ix, gx, pats, k, C, H, Z - 1, false, &got, &first, &C2, &H2, &Z2) == SFX_OK && C2 == C && H2 == H && Z2 == Z);
                CHECK(std::equal(got.begin(), got.end(), want.begin()) && got.size() == Z - 1);
            }
            if (C && H) {
                if (C > 1)
                    CHECK(call(which, x, ix, gx, pats, k, C - 1, H, want.size(), true, &got, &first, &C2, &H2, &Z2) == SFX_OK && C2 == C && H2 == 0 &&
                          Z2 == 0 && got.empty());
                if (H > 1)
                    CHECK(call(which, x, ix, gx, pats, k, C, H - 1, want.size(), true, &got, &first, &C2, &H2, &Z2) == SFX_OK && C2 == C && H2 == H &&
                          Z2 == 0 && got.empty());
            }
        }
        if (host_too) {
            std::string blob;
            std::vector<uint64_t> off(1, 0), f(nq + 1, 77);
            for (const std::string& q : pats) { blob += q; off.push_back(blob.size()); }
            std::vector<uint32_t> a(want.size() + 1), b(want.size() + 1), e(want.size() + 1);
            std::vector<uint8_t> c(want.size() + 1);
            const uint8_t* q8 = reinterpret_cast<const uint8_t*>(blob.data());
            const int rc = docs ? sfx_gindex_edit(gx, q8, off.data(), nq, k, 1ull << 30, 1ull << 24, a.data(), b.data(), e.data(), c.data(), a.size(),
                                                  f.data(), &C2, &H2, &Z2)
                                : sfx_index_edit(ix, q8, off.data(), nq, k, 1ull << 30, 1ull << 24, a.data(), b.data(), e.data(), c.data(), a.size(),
                                                 f.data(), &C2, &H2, &Z2);
            CHECK(rc == SFX_OK && C2 == C && H2 == H && Z2 == want.size() && f == wfirst);
            for (size_t i = 0; i < want.size(); i++) CHECK(Quad(a[i], b[i], e[i], c[i]) == want[i]);
            cases++;
        }
    }
    if (ix) sfx_index_destroy(ix);
    sfx_gindex_destroy(gx);
}

int main()
{
    std::mt19937 rng(20261020);
    auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    const char alpha[5] = {'a', 'b', (char)0, (char)255, 'z'};
    auto patterns = [&](const std::string& t, int sigma) {
        std::vector<std::string> pats;
        const int n = (int)t.size();
        for (int j = 0; j < 5; j++) {
            std::string q;
            const int m = pick(1, 24), a = pick(0, n - 1);
            if (j % 4 < 3) {
                q = t.substr((size_t)a, (size_t)m);
                for (int s = pick(0, 4); s > 0; s--) {
                    const int what = pick(0, 2);
                    if (what == 0 && q.size() > 1) q.erase((size_t)pick(0, (int)q.size() - 1), 1);
                    else if (what == 1) q.insert((size_t)pick(0, (int)q.size()), 1, alpha[pick(0, sigma)]);
                    else if (!q.empty()) q[(size_t)pick(0, (int)q.size() - 1)] = alpha[pick(0, sigma)];
                }
            } else
                for (int i = 0; i < m; i++) q.push_back(alpha[pick(0, sigma)]);      // (one symbol the text lacks)
            pats.push_back(q);
        }
        pats.push_back(t + "a");                                                    // longer than the text
        return pats;
    };
    for (int it = 0; it < 3; it++) {
        const int sigma = pick(1, 4);
        Text x;
        const int n = pick(1, 60);
        for (int i = 0; i < n; i++) x.t.push_back(alpha[pick(0, sigma - 1)]);
        x.starts.push_back(0);
        if (it % 4 == 0)
            for (int p = pick(1, 9); p < n; p += pick(0, 9)) x.starts.push_back((uint64_t)p);   // (a step of 0: an empty document)
        finish(&x);
        exercise(x, patterns(x.t, sigma), it % 4 < 2);
    }
    for (int n : {33}) {
        Text x;
        x.t.assign((size_t)n, 'a');
        x.starts.push_back(0);
        finish(&x);
        exercise(x, {std::string(32, 'a'), std::string(31, 'a') + "b", "b" + std::string(31, 'a'), "a", std::string(7, 'a'), std::string(9, 'a')}, true);
    }
    printf("asan_edit ok: %ld cases\n", cases);
    return 0;
}
