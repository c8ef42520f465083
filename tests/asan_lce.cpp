// tests/asan_lce.cpp -- the LCE index's entry points under AddressSanitizer, as a stand-alone program over the emulator
// build of the product's kernels (device buffers are plain heap blocks there, so an out-of-bounds global load or store
// of a kernel is caught).  Every buffer, the workspace included, is allocated at exactly its size.  Host code only; by
// hand:
//
//     make -C tests/emu asan -W ../../suffix_amd/csrc/sfx_api.hip   # (-W: sfx_lce.hip is part of sfx_api.hip's translation
//                                                                   #  unit and that Makefile does not name it)
//     clang++ -O1 -g -std=c++17 -fsanitize=address -I include tests/asan_lce.cpp \
//         -L tests/emu/asan -lsuffix_emu -Wl,-rpath,$PWD/tests/emu/asan -o tests/emu/asan/asan_lce
//     SFX_LCE_FAN=2 SFX_MAX_GRID=3 tests/emu/asan/asan_lce          # prints "asan_lce ok: <cases> cases"
//     SFX_LCE_FAN=4 SFX_MAX_GRID=3 SFX_LCE_VARIANT=team tests/emu/asan/asan_lce ; ... SFX_LCE_VARIANT=pyramid ...
//     SFX_PARTITION_MIN=50 tests/emu/asan/asan_lce                  # the partitioned scatter, the shipped fan
//
// Per text (random ones of 1 to 200 bytes over 1 to 4 symbols, every third cut into documents with empty ones among
// them, runs a^n, and sizes at the level edges 31 .. 65, 1023 .. 1025): the table and LCP by the definition; then
// sfx_inverse_table_dev / _u32, sfx_lce_create_dev / sfx_lce_create, all pairs or 400 random ones with 0, 1, 2 and 7
// mismatches through sfx_lce_query_dev / sfx_lce_query / sfx_lce_u32 against byte comparison, sfx_lce_range_min* over
// every kind of range against a plain loop, sfx_lce_ranks*; the same handle over a corrupted lcp (results within the
// ends); a table with an entry >= n and one with a repeated entry (refused).
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
    Exact(const std::vector<T>& v) : Exact(v.size()) { if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T)); }
    Exact(const Exact&) = delete;
    ~Exact() { free(p); }
};
static const uint32_t NONE = 0xFFFFFFFFu;

struct Text {
    std::string t;
    std::vector<uint64_t> starts;                     // empty: a plain text
    std::vector<uint32_t> sa, lcp;
    std::vector<uint64_t> hi;                         // per position: the end of its document
};
static void finish(Text* x)
{
    const size_t n = x->t.size();
    x->hi.assign(n, n);
    for (size_t d = 0; d < x->starts.size(); d++) {
        const uint64_t a = x->starts[d], b = d + 1 < x->starts.size() ? x->starts[d + 1] : n;
        for (uint64_t p = a; p < b; p++) x->hi[p] = b;
    }
    x->sa.resize(n);
    for (size_t p = 0; p < n; p++) x->sa[p] = (uint32_t)p;
    auto trunc = [&](uint32_t p) { return x->t.substr(p, x->hi[p] - p); };
    // the truncated suffixes in their order; equal ones by position (= by document)
    std::sort(x->sa.begin(), x->sa.end(), [&](uint32_t a, uint32_t b) {
        const int c = trunc(a).compare(trunc(b));
        return c ? c < 0 : a < b;
    });
    x->lcp.assign(n, 0);
    for (size_t r = 1; r < n; r++) {
        const std::string a = trunc(x->sa[r - 1]), b = trunc(x->sa[r]);
        uint32_t k = 0;
        while (k < a.size() && k < b.size() && a[k] == b[k]) k++;
        x->lcp[r] = k;
    }
}
static uint32_t brute(const Text& x, uint64_t i, uint64_t j, uint32_t k)
{
    const uint64_t n = x.t.size();
    if (i > n || j > n) return NONE;
    if (i == n || j == n) return 0;
    const uint64_t room = std::min(x.hi[i] - i, x.hi[j] - j);
    uint64_t l = 0;
    uint32_t miss = 0;
    for (; l < room; l++)
        if (x.t[i + l] != x.t[j + l] && miss++ == k) break;
    return (uint32_t)l;
}
static uint64_t room_of(const Text& x, uint64_t i, uint64_t j)
{
    return std::min(x.hi[i] - i, x.hi[j] - j);
}

static size_t cases = 0;

static void run_text(const Text& x, std::mt19937& rng, bool host_too)
{
    const uint64_t n = x.t.size(), nd = x.starts.size();
    Exact<uint32_t> sa(x.sa), lcp(x.lcp);
    Exact<uint64_t> starts(x.starts);
    const uint64_t* st = nd ? starts.p : nullptr;
    // the inverse table, exact-size workspace
    {
        const uint64_t wsb = sfx_inverse_table_workspace_bytes(n);
        void* ws = nullptr;
        CHECK(posix_memalign(&ws, 256, wsb ? wsb : 256) == 0);
        memset(ws, 0xA5, wsb);
        Exact<uint32_t> isa(n), isa2(n);
        CHECK(sfx_inverse_table_dev(sa.p, n, isa.p, ws, wsb, nullptr) == SFX_OK);
        CHECK(sfx_inverse_table_u32(sa.p, n, isa2.p) == SFX_OK);
        for (uint64_t r = 0; r < n; r++) CHECK(isa.p[x.sa[r]] == r && isa2.p[x.sa[r]] == r);
        free(ws);
        cases++;
    }
    // pairs: all of them where there are few, else random ones; positions n and above among them
    std::vector<uint32_t> a, b;
    if ((n + 2) * (n + 2) <= 400) {
        for (uint64_t i = 0; i <= n + 1; i++)
            for (uint64_t j = 0; j <= n + 1; j++) { a.push_back((uint32_t)i); b.push_back((uint32_t)j); }
    } else {
        for (int q = 0; q < 400; q++) { a.push_back((uint32_t)(rng() % (n + 2))); b.push_back((uint32_t)(rng() % (n + 2))); }
        for (uint64_t i : {(uint64_t)0, n - 1, n, n + 5}) { a.push_back((uint32_t)i); b.push_back((uint32_t)i); }
    }
    const uint64_t nq = a.size();
    Exact<uint32_t> da(a), db(b), out(nq);
    // ranges of every kind
    std::vector<uint32_t> lo, hi;
    for (uint64_t e = 0; e <= n + 1; e += (n > 300 ? 31 : 1)) {
        lo.push_back((uint32_t)e); hi.push_back((uint32_t)n);
        lo.push_back(0); hi.push_back((uint32_t)e);
        lo.push_back((uint32_t)e); hi.push_back((uint32_t)e + 1);
        lo.push_back((uint32_t)e); hi.push_back((uint32_t)(e + 33));
        lo.push_back((uint32_t)e); hi.push_back((uint32_t)e);
    }
    for (int q = 0; q < 200; q++) { lo.push_back((uint32_t)(rng() % (n + 1))); hi.push_back((uint32_t)(rng() % (n + 2))); }
    Exact<uint32_t> dlo(lo), dhi(hi), dmin(lo.size());
    for (int route = 0; route < (host_too ? 2 : 1); route++) {
        sfx_lce* lx = nullptr;
        if (route == 0) CHECK(sfx_lce_create_dev(sa.p, lcp.p, n, st, nd, nullptr, &lx) == SFX_OK);
        else CHECK(sfx_lce_create(sa.p, lcp.p, n, st, nd, &lx) == SFX_OK);
        CHECK(lx != nullptr);
        for (uint32_t k : {0u, 1u, 2u, 7u}) {
            memset(out.p, 0xA5, nq * 4);
            if (route == 0) CHECK(sfx_lce_query_dev(lx, da.p, db.p, nq, k, out.p, nullptr) == SFX_OK);
            else CHECK(sfx_lce_query(lx, da.p, db.p, nq, k, out.p) == SFX_OK);
            for (uint64_t q = 0; q < nq; q++) CHECK(out.p[q] == brute(x, a[q], b[q], k));
            cases++;
        }
        if (route == 0) CHECK(sfx_lce_range_min_dev(lx, dlo.p, dhi.p, lo.size(), dmin.p, nullptr) == SFX_OK);
        else CHECK(sfx_lce_range_min(lx, dlo.p, dhi.p, lo.size(), dmin.p) == SFX_OK);
        for (size_t q = 0; q < lo.size(); q++) {
            uint32_t m = NONE;
            if (lo[q] < hi[q] && hi[q] <= n)
                for (uint32_t r = lo[q]; r < hi[q]; r++) m = std::min(m, x.lcp[r]);
            CHECK(dmin.p[q] == m);
        }
        if (route == 0) CHECK(sfx_lce_ranks_dev(lx, da.p, nq, out.p, nullptr) == SFX_OK);
        else CHECK(sfx_lce_ranks(lx, da.p, nq, out.p) == SFX_OK);
        for (uint64_t q = 0; q < nq; q++) {
            if (a[q] >= n) CHECK(out.p[q] == NONE);
            else CHECK(x.sa[out.p[q]] == a[q]);
        }
        cases += 2;
        sfx_lce_destroy(lx);
    }
    // one shot
    memset(out.p, 0xA5, nq * 4);
    CHECK(sfx_lce_u32(sa.p, lcp.p, n, st, nd, da.p, db.p, nq, 1, out.p) == SFX_OK);
    for (uint64_t q = 0; q < nq; q++) CHECK(out.p[q] == brute(x, a[q], b[q], 1));
    cases++;
    // a corrupted lcp: within the ends, and the call returns
    for (int kind = 0; kind < 2; kind++) {
        Exact<uint32_t> bad(n);
        for (uint64_t r = 0; r < n; r++) bad.p[r] = kind ? NONE : (uint32_t)rng();
        sfx_lce* lx = nullptr;
        CHECK(sfx_lce_create_dev(sa.p, bad.p, n, st, nd, nullptr, &lx) == SFX_OK);
        for (uint32_t k : {0u, 3u, NONE}) {
            CHECK(sfx_lce_query_dev(lx, da.p, db.p, nq, k, out.p, nullptr) == SFX_OK);
            for (uint64_t q = 0; q < nq; q++) {
                if (a[q] > n || b[q] > n) CHECK(out.p[q] == NONE);
                else if (a[q] == n || b[q] == n) CHECK(out.p[q] == 0);
                else CHECK(out.p[q] <= room_of(x, a[q], b[q]));
            }
        }
        CHECK(sfx_lce_range_min_dev(lx, dlo.p, dhi.p, lo.size(), dmin.p, nullptr) == SFX_OK);
        sfx_lce_destroy(lx);
        cases++;
    }
    // refusals: an entry >= n, a repeated entry
    if (n >= 2) {
        for (int kind = 0; kind < 2; kind++) {
            std::vector<uint32_t> v = x.sa;
            if (kind) v[0] = v[n - 1]; else v[n / 2] = (uint32_t)n;
            Exact<uint32_t> bs(v), isa(n);
            sfx_lce* lx = nullptr;
            CHECK(sfx_lce_create_dev(bs.p, lcp.p, n, st, nd, nullptr, &lx) == SFX_ERR_ARG && !lx);
            CHECK(sfx_lce_create(bs.p, lcp.p, n, st, nd, &lx) == SFX_ERR_ARG && !lx);
            CHECK(sfx_inverse_table_u32(bs.p, n, isa.p) == SFX_ERR_ARG);
            cases++;
        }
    }
}

int main()
{
    std::mt19937 rng(12345);
    std::vector<Text> texts;
    for (int t = 0; t < 24; t++) {
        Text x;
        const int sigma = 1 + t % 4;
        const size_t n = t < 6 ? 1 + t : 1 + rng() % 200;
        for (size_t p = 0; p < n; p++) x.t.push_back((char)('a' + rng() % sigma));
        if (t % 3 == 2) {
            x.starts.push_back(0);
            for (uint64_t p = 0; p < n;) {
                p += rng() % 40;
                if (p < n) x.starts.push_back(p);
                if (rng() % 4 == 0 && p < n) x.starts.push_back(p);      // an empty document
            }
        }
        texts.push_back(x);
    }
    for (size_t n : {31, 32, 33, 63, 64, 65, 1023, 1024, 1025}) {
        Text x;
        x.t.assign(n, 'a');
        if (n % 2) for (size_t p = 0; p < n; p += 7) x.t[p] = 'b';
        texts.push_back(x);
    }
    // the empty text: a valid handle
    {
        sfx_lce* lx = nullptr;
        uint32_t a[2] = {0, 3}, b[2] = {0, 0}, out[2] = {7, 7};
        CHECK(sfx_lce_create_dev(nullptr, nullptr, 0, nullptr, 0, nullptr, &lx) == SFX_OK && lx);
        CHECK(sfx_lce_query_dev(lx, a, b, 2, 2, out, nullptr) == SFX_OK && out[0] == 0 && out[1] == NONE);
        CHECK(sfx_lce_range_min_dev(lx, a, b, 2, out, nullptr) == SFX_OK && out[0] == NONE && out[1] == NONE);
        sfx_lce_destroy(lx);
        cases++;
    }
    for (size_t t = 0; t < texts.size(); t++) {
        finish(&texts[t]);
        run_text(texts[t], rng, t % 4 == 0);
    }
    printf("asan_lce ok: %zu cases\n", cases);
    return 0;
}
