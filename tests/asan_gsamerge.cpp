// tests/asan_gsamerge.cpp -- the GSA merge under AddressSanitizer and UBSan, as a stand-alone program over the emulator
// build of the product's kernels (device buffers are plain heap blocks there, so an out-of-bounds global load or store of
// a kernel is caught).  Every buffer, the workspace included, is allocated at exactly its size.  Host code only, no part
// of pytest; by hand, with every build product under $TMPDIR:
//
//     D=${TMPDIR:-/tmp}/sfx_asan_gsamerge
//     make -C tests/emu asan ASAN_DIR=$D -W ../../suffix_amd/csrc/sfx_api.hip   # (-W: sfx_gsamerge.hip is part of sfx_api.hip's
//                                                                               #  translation unit and that Makefile does not name it)
//     clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include tests/asan_gsamerge.cpp \
//         -L $D -lsuffix_emu -Wl,-rpath,$D -o $D/asan_gsamerge
//     $D/asan_gsamerge                                       # prints "asan_gsamerge ok: <cases> cases"
//     SFX_GM_TILE=5 SFX_MAX_GRID=3 $D/asan_gsamerge          # the same with small tiles and more tiles than workgroups
//
// (The emulator's asan build carries AddressSanitizer; the undefined-behaviour checks cover this program's own code.)
//
// The cases are tests/_gsamerge.py's 1, 3 and 4: the known answer, the ties and prefixes, and N, M around the scatter tile
// with the patterns that fill whole tiles from one side.  The arrays of either side and the expected arrays of the whole
// collection come from the definition (a comparison sort of the truncated suffixes, equal ones by position).  Each split
// runs through sfx_gsa_merge_dev with da given and NULL, with the da / lcp outputs NULL, with a match limit one below and
// at the longest old/new match, and through sfx_gsa_merge_u32 and sfx_gsa_extend_u32.
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
    Exact(const std::vector<T>& v) : Exact(v.size()) { if (n) memcpy(p, v.data(), n * sizeof(T)); }
    Exact(const Exact&) = delete;
    ~Exact() { free(p); }
};

struct Gsa { std::vector<uint32_t> sa, da, lcp; };
// the definition: truncated suffixes by their bytes, a proper prefix first, equal ones by position
static Gsa naive(const std::vector<std::string>& docs)
{
    std::string t;
    std::vector<uint32_t> doc, end;
    for (size_t d = 0; d < docs.size(); d++) {
        t += docs[d];
        doc.resize(t.size(), (uint32_t)d);
        end.resize(t.size(), (uint32_t)t.size());
    }
    const size_t n = t.size();
    Gsa g;
    g.sa.resize(n);
    for (size_t p = 0; p < n; p++) g.sa[p] = (uint32_t)p;
    std::sort(g.sa.begin(), g.sa.end(), [&](uint32_t a, uint32_t b) {
        const int c = t.compare(a, end[a] - a, t, b, end[b] - b);
        return c != 0 ? c < 0 : a < b;
    });
    g.da.resize(n);
    g.lcp.assign(n, 0);
    for (size_t r = 0; r < n; r++) {
        g.da[r] = doc[g.sa[r]];
        if (r == 0) continue;
        const uint32_t a = g.sa[r - 1], b = g.sa[r];
        uint32_t k = 0;
        while (a + k < end[a] && b + k < end[b] && t[a + k] == t[b + k]) k++;
        g.lcp[r] = k;
    }
    return g;
}

static int cases = 0;
static void one_split(const std::vector<std::string>& docs, size_t k)
{
    const std::vector<std::string> da_(docs.begin(), docs.begin() + k), db_(docs.begin() + k, docs.end());
    const Gsa A = naive(da_), B = naive(db_), W = naive(docs);
    std::string t;
    std::vector<uint64_t> st;
    for (const std::string& d : docs) { st.push_back(t.size()); t += d; }
    const uint64_t n = t.size(), na = A.sa.size(), nb = B.sa.size(), nd = docs.size();
    uint64_t want = 0;                                   // the longest (old, new) neighbour match
    for (size_t r = 1; r < n; r++)
        if ((W.sa[r - 1] < na) != (W.sa[r] < na)) want = std::max<uint64_t>(want, W.lcp[r]);
    Exact<uint8_t> text(n);
    if (n) memcpy(text.p, t.data(), n);
    Exact<uint64_t> starts(st);
    Exact<uint32_t> sa_a(A.sa), da_a(A.da), lcp_a(A.lcp), sa_b(B.sa), da_b(B.da), lcp_b(B.lcp);
    const uint64_t wsb = sfx_gsa_merge_workspace_bytes(na, nb);
    CHECK(wsb <= 12 * nb + (34u << 10));
    for (int variant = 0; variant < 5; variant++) {
        const bool with_da = variant != 1, outs = variant != 2;
        const uint32_t limit = variant == 3 ? (uint32_t)want : variant == 4 && want > 1 ? (uint32_t)want - 1 : 0;
        const bool refused = limit && want > limit;
        Exact<uint32_t> sa(n), da(n), lcp(n);
        Exact<uint8_t> ws(wsb);
        memset(ws.p, 0xC3, wsb);
        memset(sa.p, 0xEE, n * 4); memset(da.p, 0xEE, n * 4); memset(lcp.p, 0xEE, n * 4);
        uint64_t longest = 99;
        CHECK(sfx_gsa_merge_dev(text.p, starts.p, nd, k, sa_a.p, with_da ? da_a.p : nullptr, lcp_a.p, na, sa_b.p, with_da ? da_b.p : nullptr, lcp_b.p,
                                nb, limit, sa.p, outs ? da.p : nullptr, outs ? lcp.p : nullptr, &longest, ws.p, wsb, nullptr) == SFX_OK);
        CHECK(longest == (refused ? (uint64_t)limit + 1 : want));
        for (size_t r = 0; r < n; r++) {
            CHECK(sa.p[r] == (refused ? 0xEEEEEEEEu : W.sa[r]));
            CHECK(da.p[r] == (refused || !outs ? 0xEEEEEEEEu : W.da[r]));
            CHECK(lcp.p[r] == (refused || !outs ? 0xEEEEEEEEu : W.lcp[r]));
        }
        cases++;
    }
    {
        std::vector<uint32_t> sa(n), da(n), lcp(n);
        uint64_t longest = 99;
        CHECK(sfx_gsa_merge_u32(text.p, starts.p, nd, k, sa_a.p, da_a.p, lcp_a.p, na, sa_b.p, da_b.p, lcp_b.p, nb, 0, sa.data(), da.data(),
                                lcp.data(), &longest) == SFX_OK);
        CHECK(longest == want && sa == W.sa && da == W.da && lcp == W.lcp);
        uint32_t route = 99;
        std::fill(sa.begin(), sa.end(), 0u);
        CHECK(sfx_gsa_extend_u32(text.p, n, starts.p, nd, k, sa_a.p, nullptr, lcp_a.p, 0, 1, sa.data(), da.data(), lcp.data(), &longest, &route) == SFX_OK);
        CHECK(route == SFX_GSA_ROUTE_MERGE && longest == want && sa == W.sa && da == W.da && lcp == W.lcp);
        if (want > 1) {
            CHECK(sfx_gsa_extend_u32(text.p, n, starts.p, nd, k, sa_a.p, da_a.p, lcp_a.p, (uint32_t)want - 1, 1, sa.data(), da.data(), lcp.data(),
                                     &longest, &route) == SFX_OK);
            CHECK(route == SFX_GSA_ROUTE_REBUILD && longest == want && sa == W.sa && da == W.da && lcp == W.lcp);
        }
        cases += 2;
    }
}

static std::vector<std::string> cut(const std::string& t, size_t step)
{
    std::vector<std::string> out;
    for (size_t i = 0; i < t.size(); i += step) out.push_back(t.substr(i, step));
    return out;
}
static std::string bits(size_t n, unsigned seed)
{
    std::mt19937 rng(seed);
    std::string s(n, 'a');
    for (char& c : s) c = (char)('a' + (rng() & 1));
    return s;
}

int main()
{
    // 1. the known answer
    one_split({"banana", "ana"}, 1);
    {
        const Gsa w = naive({"banana", "ana"});
        CHECK((w.sa == std::vector<uint32_t>{5, 8, 3, 6, 1, 0, 4, 7, 2}) && (w.lcp == std::vector<uint32_t>{0, 1, 1, 3, 3, 0, 0, 2, 2}));
    }
    // 3. ties and prefixes
    const std::string a40(40, 'a'), zero3("\0\0\0", 3), zero1("\0", 1), mixed("a\0b\xff" "a", 5), mixed2("\0\xff" "a\0", 4);
    one_split({"xy", "b", "xy", "a", "xy"}, 3);
    one_split(std::vector<std::string>(10, a40), 7);
    {
        std::vector<std::string> d(7, a40);
        d.push_back(a40 + "a");
        one_split(d, 7);
    }
    one_split({"abcabc", "abcab", "abc", "ab"}, 2);
    one_split({"ab", "abc", "abcab", "abcabc"}, 2);
    one_split({"abab", "ba", zero3, zero1}, 2);
    one_split({"abab", "ba", "\xff\xff\xff", "\xff"}, 2);
    one_split({mixed, "\xff", mixed2, "b\xff", zero1}, 2);
    one_split({mixed, "\xff", mixed2, "b\xff", zero1}, 3);
    one_split({"", "ab", "", "", "ab", ""}, 3);
    one_split({"", ""}, 1);
    one_split({"q"}, 0);
    one_split({"q"}, 1);
    // 4. around the scatter tile
    const size_t sizes[] = {1, 2047, 2048, 2049, 4097};
    for (size_t na : sizes)
        for (size_t nb : sizes) {
            std::vector<std::string> docs = cut(bits(na, (unsigned)(10 * na)), 300);
            const size_t k = docs.size();
            for (const std::string& d : cut(bits(nb, (unsigned)(10 * nb + 1)), 300)) docs.push_back(d);
            one_split(docs, k);
        }
    {
        std::vector<std::string> words, order;                              // strict alternation of old and new slots
        for (int i = 0; i < 7 * 2100; i += 7) words.push_back(std::string{(char)('a' + i / 676), (char)('a' + i / 26 % 26), (char)('a' + i % 26), '~'});
        for (size_t i = 0; i < words.size(); i += 2) order.push_back(words[i]);
        for (size_t i = 1; i < words.size(); i += 2) order.push_back(words[i]);
        one_split(order, (words.size() + 1) / 2);
        std::vector<std::string> many;                                      // 2052 suffixes between "bab" and "z": one common p
        for (int i = 0; i < 513; i++) many.push_back(std::string{"mno"[i % 3], "mno"[i / 3 % 3], "mno"[i / 9 % 3], "mno"[i / 27 % 3]});
        std::vector<std::string> fm{"abab", "zz"}, mf(many);
        fm.insert(fm.end(), many.begin(), many.end());
        mf.push_back("abab");
        mf.push_back("zz");
        one_split(fm, 2);
        one_split(mf, many.size());                                         // the mirror: 2052 old ranks with no new one between
    }
    printf("asan_gsamerge ok: %d cases\n", cases);
    return 0;
}
