// tests/asan_runs.cpp -- the entry points of the maximal repetitions and the Lyndon array under AddressSanitizer, as a
// stand-alone program over the emulator build of the product's kernels (device buffers are plain heap blocks there, so an
// out-of-bounds global load or store of a kernel is caught).  Every buffer, the workspace included, is allocated at exactly
// its size.  Host code only; by hand:
//
//     make -C tests/emu asan -W ../../suffix_amd/csrc/sfx_api.hip   # (-W: sfx_runs.hip is part of sfx_api.hip's translation
//                                                                   #  unit and that Makefile does not name it)
//     clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -I include tests/asan_runs.cpp \
//         -L tests/emu/asan -lsuffix_emu -Wl,-rpath,$PWD/tests/emu/asan -o tests/emu/asan/asan_runs
//     SFX_MAX_GRID=3 SFX_LCE_FAN=2 SFX_RUNS_TILE=64 SFX_RUNS_LIST=5 tests/emu/asan/asan_runs    # prints "asan_runs ok: <cases> cases"
//     SFX_MAX_GRID=3 SFX_LCE_FAN=4 SFX_RUNS_TILE=128 SFX_RUNS_LIST=0 tests/emu/asan/asan_runs ; tests/emu/asan/asan_runs
//
// 16 texts (random ones of 1 to 150 bytes over 1 to 4 symbols and over 0x00 / 0xFF; a^n b and b a^n for n = 63, 65, 129,
// around the tiles of 64 and 128 words; a^65; a b^129; (ab)^70; the Fibonacci string of 233 bytes), sized so that the
// program ends within minutes under the sanitizer.  Per text: the table and LCP by the definition; sfx_runs_dev without a
// filter at capacity n, then with a filter of all three kinds or at capacity count - 1 (now and then an empty filter,
// capacity = count) against the runs enumerated from the definition; sfx_lyndon_array_dev of both orders against a plain
// double loop; every second text a corrupted lcp (every triple in bounds).  Every sixth text also sfx_runs_u32 (tables given, LCP built, both built in turn) and
// sfx_lyndon_array_u32; every third a table with an entry >= n or a repeated entry (refused).
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
    Exact(const std::vector<T>& v) : Exact(v.size()) { if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T)); }
    Exact(const Exact&) = delete;
    ~Exact() { free(p); }
};
struct Ws {                                           // an aligned workspace of exactly `bytes` bytes, dirty
    void* p = nullptr;
    uint64_t bytes;
    explicit Ws(uint64_t b) : bytes(b) { CHECK(posix_memalign(&p, 256, b ? b : 256) == 0); memset(p, 0xA5, b); }
    Ws(const Ws&) = delete;
    ~Ws() { free(p); }
};
static const uint32_t NONE = 0xFFFFFFFFu;
typedef std::tuple<uint32_t, uint32_t, uint32_t> Run;     // (begin, period, end): sorts as the output does

static std::vector<uint32_t> table_of(const std::string& t)
{
    std::vector<uint32_t> sa(t.size());
    for (size_t p = 0; p < t.size(); p++) sa[p] = (uint32_t)p;
    std::sort(sa.begin(), sa.end(), [&](uint32_t a, uint32_t b) { return t.compare(a, std::string::npos, t, b, std::string::npos) < 0; });
    return sa;
}
static std::vector<uint32_t> lcp_of(const std::string& t, const std::vector<uint32_t>& sa)
{
    std::vector<uint32_t> lcp(t.size(), 0);
    for (size_t r = 1; r < t.size(); r++) {
        uint32_t k = 0;
        while (sa[r - 1] + k < t.size() && sa[r] + k < t.size() && t[sa[r - 1] + k] == t[sa[r] + k]) k++;
        lcp[r] = k;
    }
    return lcp;
}
static bool primitive(const std::string& t, size_t b, size_t p)
{
    for (size_t q = 1; q < p; q++) {
        if (p % q) continue;
        bool same = true;
        for (size_t k = b; k + q < b + p && same; k++) same = t[k] == t[k + q];
        if (same) return false;
    }
    return true;
}
static std::vector<Run> brute(const std::string& t, uint32_t minp, uint32_t maxp, uint32_t minlen)
{
    const size_t n = t.size();
    std::vector<Run> out;
    for (size_t p = 1; 2 * p <= n; p++) {
        size_t k = 0;
        while (k + p < n) {
            if (t[k] != t[k + p]) { k++; continue; }
            const size_t s = k;
            while (k + p < n && t[k] == t[k + p]) k++;
            const size_t e = k + p;
            if (e - s >= 2 * p && primitive(t, s, p) && p >= minp && (maxp == 0 || p <= maxp) && e - s >= minlen)
                out.emplace_back((uint32_t)s, (uint32_t)p, (uint32_t)e);
        }
    }
    std::sort(out.begin(), out.end());
    return out;
}
static std::vector<uint32_t> lyndon_of(const std::string& t, int order)
{
    std::string u = t;
    if (order) for (char& c : u) c = (char)(255 - (unsigned char)c);
    const std::vector<uint32_t> sa = table_of(std::string(u.begin(), u.end()));
    std::vector<uint32_t> isa(t.size()), lyn(t.size());
    for (size_t r = 0; r < sa.size(); r++) isa[sa[r]] = (uint32_t)r;
    for (size_t i = 0; i < t.size(); i++) {
        size_t j = i + 1;
        while (j < t.size() && isa[j] > isa[i]) j++;
        lyn[i] = (uint32_t)(j - i);
    }
    return lyn;
}

static size_t cases = 0;

static void expect(const std::vector<Run>& want, uint64_t cap, uint64_t count, const Exact<uint32_t>& b, const Exact<uint32_t>& e,
                   const Exact<uint32_t>& p)
{
    CHECK(count == want.size());
    for (uint64_t k = 0; k < cap; k++) {
        if (k < count) CHECK(Run(b.p[k], p.p[k], e.p[k]) == want[k]);
        else CHECK(b.p[k] == 0xA5A5A5A5u && e.p[k] == 0xA5A5A5A5u && p.p[k] == 0xA5A5A5A5u);     // nothing behind the triples
    }
}

static void run_text(const std::string& t, std::mt19937& rng, size_t idx)
{
    const uint64_t n = t.size();
    const bool host_too = idx % 6 == 0;
    const std::vector<uint32_t> sav = table_of(t), lcpv = lcp_of(t, sav);
    Exact<uint32_t> sa(sav), lcp(lcpv);
    Exact<uint8_t> text(std::vector<uint8_t>(t.begin(), t.end()));
    // no filter at capacity n and count - 1 (or 0), one filter of all three kinds; every sixth text an empty filter and a host route
    const sfx_runs_filter_t all = {1, 0, 0, 0}, mixed = {2, 6, 9, 0}, none = {5, 4, 0, 0};
    const std::vector<Run> want_all = brute(t, 1, 0, 0);
    struct Call { const sfx_runs_filter_t* f; bool null_filter; uint64_t cap; };
    // (a call costs seconds under the sanitizer -- the radix sort's scan of its whole digit table -- so a text takes two or three)
    std::vector<Call> calls = {{&all, true, n}};
    if (idx % 2 == 0) calls.push_back({&mixed, false, n});
    else calls.push_back({&all, false, want_all.empty() ? 0 : want_all.size() - 1});
    if (idx % 6 == 1) calls.push_back({&none, false, n});
    if (idx % 6 == 2) calls.push_back({&all, true, want_all.size()});
    for (const Call& c : calls) {
        const std::vector<Run> want = brute(t, c.f->min_period, c.f->max_period, c.f->min_len);
        Exact<uint32_t> b(c.cap), e(c.cap), p(c.cap);
        for (Exact<uint32_t>* x : {&b, &e, &p}) memset(x->p, 0xA5, c.cap * 4);
        Ws ws(sfx_runs_workspace_bytes(n));
        uint64_t count = 99;
        CHECK(sfx_runs_dev(text.p, n, sa.p, lcp.p, c.null_filter ? nullptr : c.f, b.p, e.p, p.p, c.cap, &count, ws.p, ws.bytes, nullptr) == SFX_OK);
        expect(want, c.cap, count, b, e, p);
        cases++;
    }
    if (host_too) {                                     // tables given, LCP built, both built: one of the three per text
        const int given = (int)(idx / 6 % 3);
        Exact<uint32_t> b(n), e(n), p(n);
        for (Exact<uint32_t>* x : {&b, &e, &p}) memset(x->p, 0xA5, n * 4);
        uint64_t count = 99;
        CHECK(sfx_runs_u32(text.p, n, given ? sa.p : nullptr, given == 2 ? lcp.p : nullptr, &mixed, b.p, e.p, p.p, n, &count) == SFX_OK);
        expect(brute(t, 2, 6, 9), n, count, b, e, p);
        cases++;
    }
    // both Lyndon arrays
    for (int order = 0; order < 2; order++) {
        const std::vector<uint32_t> want = lyndon_of(t, order);
        std::string u = t;
        if (order) for (char& c : u) c = (char)(255 - (unsigned char)c);
        const std::vector<uint32_t> osa = table_of(u);
        std::vector<uint32_t> isav(n);
        for (size_t r = 0; r < n; r++) isav[osa[r]] = (uint32_t)r;
        Exact<uint32_t> isa(isav), lyn(n), os(osa);
        memset(lyn.p, 0xA5, n * 4);
        Ws ws(sfx_lyndon_array_workspace_bytes(n));
        CHECK(sfx_lyndon_array_dev(isa.p, n, lyn.p, ws.p, ws.bytes, nullptr) == SFX_OK);
        for (size_t i = 0; i < n; i++) CHECK(lyn.p[i] == want[i]);
        cases++;
        if (host_too) {
            memset(lyn.p, 0xA5, n * 4);
            CHECK(sfx_lyndon_array_u32(text.p, n, order ? nullptr : os.p, order, lyn.p) == SFX_OK);     // order 0: the table given; 1: built
            for (size_t i = 0; i < n; i++) CHECK(lyn.p[i] == want[i]);
            cases++;
        }
    }
    // a corrupted lcp (every second text, one kind each): every triple in bounds, and the call returns
    if (idx % 2 == 1) {
        const int kind = (int)(idx / 2 % 3);
        Exact<uint32_t> bad(n), b(n), e(n), p(n);
        for (uint64_t r = 0; r < n; r++) bad.p[r] = kind == 0 ? (uint32_t)rng() : kind == 1 ? NONE : (uint32_t)(rng() % (2 * n));
        Ws ws(sfx_runs_workspace_bytes(n));
        uint64_t count = 0;
        CHECK(sfx_runs_dev(text.p, n, sa.p, bad.p, nullptr, b.p, e.p, p.p, n, &count, ws.p, ws.bytes, nullptr) == SFX_OK);
        CHECK(count <= n);
        for (uint64_t k = 0; k < count; k++) CHECK(b.p[k] < e.p[k] && e.p[k] <= n && p.p[k] >= 1 && 2ull * p.p[k] <= e.p[k] - b.p[k]);
        cases++;
    }
    // refusals (every third text): an entry >= n or a repeated entry
    if (n >= 2 && idx % 3 == 1) {
        const int kind = (int)(idx / 3 % 2);
        std::vector<uint32_t> v = sav;
        if (kind) v[0] = v[n - 1]; else v[n / 2] = (uint32_t)n;
        Exact<uint32_t> bs(v), b(n), e(n), p(n), lyn(n);
        Ws ws(sfx_runs_workspace_bytes(n));
        uint64_t count = 0;
        CHECK(sfx_runs_dev(text.p, n, bs.p, lcp.p, nullptr, b.p, e.p, p.p, n, &count, ws.p, ws.bytes, nullptr) == SFX_ERR_ARG);
        if (kind) CHECK(sfx_runs_u32(text.p, n, bs.p, lcp.p, nullptr, b.p, e.p, p.p, n, &count) == SFX_ERR_ARG);
        else CHECK(sfx_lyndon_array_u32(text.p, n, bs.p, 0, lyn.p) == SFX_ERR_ARG);
        cases++;
    }
}

int main()
{
    std::mt19937 rng(4321);
    std::vector<std::string> texts;
    for (int t = 0; t < 6; t++) {
        const int sigma = 1 + t % 4;
        const size_t n = t < 2 ? 1 + t : 1 + rng() % 150;
        std::string x;
        for (size_t p = 0; p < n; p++) x.push_back((char)(t == 4 ? (rng() % sigma ? 0xFF : 0x00) : 'a' + rng() % sigma));
        texts.push_back(x);
    }
    for (size_t n : {63, 65, 129}) {                  // around the tiles of 64 and 128 words
        texts.push_back(std::string(n, 'a') + "b");   // every next-smaller answer leaves its tile: the list overflows
        texts.push_back("b" + std::string(n, 'a'));
    }
    texts.push_back(std::string(65, 'a'));
    texts.push_back("a" + std::string(129, 'b'));     // one Lyndon word over several tiles
    {
        std::string ab, f0 = "b", f1 = "a";
        for (int k = 0; k < 70; k++) ab += "ab";
        texts.push_back(ab);
        while (f1.size() < 233) { const std::string f2 = f1 + f0; f0 = f1; f1 = f2; }
        texts.push_back(f1);
    }
    // the empty text
    {
        uint64_t count = 9;
        CHECK(sfx_runs_dev(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &count, nullptr, 0, nullptr) == SFX_OK && count == 0);
        CHECK(sfx_runs_u32(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &count) == SFX_OK && count == 0);
        CHECK(sfx_lyndon_array_dev(nullptr, 0, nullptr, nullptr, 0, nullptr) == SFX_OK);
        CHECK(sfx_lyndon_array_u32(nullptr, 0, nullptr, 1, nullptr) == SFX_OK);
        cases++;
    }
    for (size_t t = 0; t < texts.size(); t++) run_text(texts[t], rng, t);
    printf("asan_runs ok: %zu cases\n", cases);
    return 0;
}
