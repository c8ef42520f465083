// tests/asan_docs.cpp -- the document counts and the k-common substrings under AddressSanitizer, as a stand-alone program
// over the emulator build of the product's kernels (device buffers are plain heap blocks there, so an out-of-bounds
// global load or store of a kernel is caught).  Every buffer, the workspace included, is allocated at exactly its size.
// Host code only; by hand:
//
//     make -C tests/emu asan -W ../../suffix_amd/csrc/sfx_api.hip   # (-W: sfx_docs.hip is part of sfx_api.hip's translation
//                                                                   #  unit and that Makefile does not name it)
//     clang++ -O1 -g -std=c++17 -fsanitize=address -I include tests/asan_docs.cpp \
//         -L tests/emu/asan -lsuffix_emu -Wl,-rpath,$PWD/tests/emu/asan -o tests/emu/asan/asan_docs
//     tests/emu/asan/asan_docs                                      # prints "asan_docs ok: <cases> cases"
//     SFX_LCE_FAN=2 SFX_MAX_GRID=3 tests/emu/asan/asan_docs ; SFX_LCE_FAN=4 SFX_MAX_GRID=3 tests/emu/asan/asan_docs
//
// Per collection (random ones of 1 to 7 documents of 0 to 60 bytes over 1 to 3 symbols, empty documents and duplicates
// among them, and a^m twice for m at the node edges): the table, document array and LCP by the definition; then
// sfx_doc_counts_dev / _u32 against the set of documents of every boundary's interval and the definition of dup_prefix,
// sfx_common_substrings_dev / _u32 against a map of all substrings; the same arrays with lcp replaced by random words,
// by UINT32_MAX and by small values (the calls return, dup_prefix is still the definition's); da entries >= ndocs
// (refused); a df of random words; a workspace one byte short.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
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
struct Ws {                                           // exactly `bytes` bytes on a 256-byte boundary, dirty
    void* p = nullptr;
    uint64_t bytes;
    explicit Ws(uint64_t b, int fill) : bytes(b) { CHECK(posix_memalign(&p, 256, b ? b : 256) == 0); memset(p, fill, b); }
    ~Ws() { free(p); }
};
static const uint32_t NONE = 0xFFFFFFFFu;

struct Coll {
    std::vector<std::string> docs;
    std::vector<uint64_t> starts;
    std::vector<uint32_t> sa, da, lcp;
};
static void finish(Coll* c)
{
    std::vector<std::pair<uint32_t, uint32_t>> items;                    // (document, offset)
    uint64_t at = 0;
    for (size_t d = 0; d < c->docs.size(); d++) {
        c->starts.push_back(at);
        at += c->docs[d].size();
        for (size_t o = 0; o < c->docs[d].size(); o++) items.push_back({(uint32_t)d, (uint32_t)o});
    }
    auto suf = [&](const std::pair<uint32_t, uint32_t>& it) { return c->docs[it.first].substr(it.second); };
    std::sort(items.begin(), items.end(), [&](const auto& a, const auto& b) {
        const int k = suf(a).compare(suf(b));
        return k ? k < 0 : a.first < b.first;
    });
    for (size_t r = 0; r < items.size(); r++) {
        c->sa.push_back((uint32_t)(c->starts[items[r].first] + items[r].second));
        c->da.push_back(items[r].first);
        uint32_t k = 0;
        if (r) {
            const std::string a = suf(items[r - 1]), b = suf(items[r]);
            while (k < a.size() && k < b.size() && a[k] == b[k]) k++;
        }
        c->lcp.push_back(k);
    }
}
static std::vector<uint32_t> brute_df(const std::vector<uint32_t>& da, const std::vector<uint32_t>& lcp)
{
    const size_t n = da.size();
    std::vector<uint32_t> out(n);
    for (size_t p = 0; p < n; p++) {
        const uint32_t v = p ? lcp[p] : 0;
        size_t lb = 0, rb = n - 1;
        if (v) {
            lb = p - 1;
            while (lb > 0 && lcp[lb] >= v) lb--;
            rb = p;
            while (rb + 1 < n && lcp[rb + 1] >= v) rb++;
        }
        out[p] = (uint32_t)std::set<uint32_t>(da.begin() + lb, da.begin() + rb + 1).size();
    }
    return out;
}
static std::vector<uint32_t> brute_dup(const std::vector<uint32_t>& da, const std::vector<uint32_t>& lcp)
{
    const size_t n = da.size();
    std::vector<uint32_t> hits(n, 0);
    std::map<uint32_t, size_t> last;
    for (size_t r = 0; r < n; r++) {
        auto it = last.find(da[r]);
        if (it != last.end()) {
            size_t at = it->second + 1;
            for (size_t p = it->second + 1; p <= r; p++)
                if (lcp[p] <= lcp[at]) at = p;
            hits[at]++;
        }
        last[da[r]] = r;
    }
    for (size_t x = 1; x < n; x++) hits[x] += hits[x - 1];
    return hits;
}
static std::vector<uint32_t> brute_lens(const std::vector<std::string>& docs)
{
    std::map<std::string, std::set<size_t>> occ;
    for (size_t d = 0; d < docs.size(); d++)
        for (size_t i = 0; i < docs[d].size(); i++)
            for (size_t l = 1; i + l <= docs[d].size(); l++) occ[docs[d].substr(i, l)].insert(d);
    std::vector<uint32_t> len(docs.size(), 0);
    for (const auto& kv : occ)
        for (size_t k = 0; k < kv.second.size(); k++) len[k] = std::max(len[k], (uint32_t)kv.first.size());
    return len;
}

static size_t cases = 0;

static void run(const Coll& c, std::mt19937& rng, int t)
{
    const uint64_t n = c.sa.size(), nd = c.docs.size();
    Exact<uint32_t> sa(c.sa), da(c.da), lcp(c.lcp);
    Exact<uint64_t> starts(c.starts);
    const uint64_t wsb = sfx_doc_counts_workspace_bytes(n), cwsb = sfx_common_substrings_workspace_bytes(nd);
    const std::vector<uint32_t> exp_df = brute_df(c.da, c.lcp), exp_dup = brute_dup(c.da, c.lcp), exp_len = brute_lens(c.docs);
    std::string text;
    for (const auto& d : c.docs) text += d;
    {
        static const int fills[3] = {0x00, 0xFF, 0xA5};
        Ws ws(wsb, fills[t % 3]);
        Exact<uint32_t> df(n), dup(n), df2(n), dup2(n);
        CHECK(sfx_doc_counts_dev(da.p, lcp.p, n, nd, dup.p, df.p, ws.p, wsb, nullptr) == SFX_OK);
        CHECK(sfx_doc_counts_u32(da.p, lcp.p, n, nd, dup2.p, df2.p) == SFX_OK);
        for (uint64_t p = 0; p < n; p++) CHECK(df.p[p] == exp_df[p] && dup.p[p] == exp_dup[p] && df2.p[p] == exp_df[p] && dup2.p[p] == exp_dup[p]);
        CHECK(sfx_doc_counts_dev(da.p, lcp.p, n, nd, nullptr, df2.p, ws.p, wsb, nullptr) == SFX_OK);
        CHECK(sfx_doc_counts_dev(da.p, lcp.p, n, nd, dup2.p, nullptr, ws.p, wsb, nullptr) == SFX_OK);
        for (uint64_t p = 0; p < n; p++) CHECK(df2.p[p] == exp_df[p] && dup2.p[p] == exp_dup[p]);
        if (n) {
            Ws small(wsb - 1, 0xFF);
            CHECK(sfx_doc_counts_dev(da.p, lcp.p, n, nd, dup.p, df.p, small.p, wsb - 1, nullptr) == SFX_ERR_WORKSPACE);
        }
        Ws cws(cwsb, 0xFF);
        Exact<uint32_t> len(nd), pos(nd), len2(nd), pos2(nd);
        CHECK(sfx_common_substrings_dev(sa.p, lcp.p, df.p, n, starts.p, nd, len.p, pos.p, cws.p, cwsb, nullptr) == SFX_OK);
        CHECK(sfx_common_substrings_u32(sa.p, lcp.p, df.p, n, starts.p, nd, len2.p, pos2.p) == SFX_OK);
        for (uint64_t d = 0; d < nd; d++) {
            CHECK(len.p[d] == exp_len[d] && len2.p[d] == exp_len[d] && pos.p[d] == pos2.p[d]);
            if (!exp_len[d]) { CHECK(pos.p[d] == NONE); continue; }
            const std::string s = text.substr(pos.p[d], exp_len[d]);    // the string stands in at least d + 1 documents
            size_t in = 0;
            for (const auto& doc : c.docs) in += doc.find(s) != std::string::npos;
            CHECK(s.size() == exp_len[d] && in >= d + 1);
        }
        cases += 4;
    }
    if (!n) return;
    // arbitrary lcp contents: the calls return, dup_prefix is the definition's over what is stored
    for (int kind = 0; kind < 3; kind++) {
        std::vector<uint32_t> bad(n);
        for (uint64_t r = 0; r < n; r++) bad[r] = kind == 0 ? (uint32_t)rng() : kind == 1 ? NONE : (uint32_t)(rng() % 3);
        Exact<uint32_t> bl(bad), df(n), dup(n), len(nd), pos(nd);
        Ws ws(wsb, 0xA5), cws(cwsb, 0xA5);
        CHECK(sfx_doc_counts_dev(da.p, bl.p, n, nd, dup.p, df.p, ws.p, wsb, nullptr) == SFX_OK);
        const std::vector<uint32_t> e = brute_dup(c.da, bad);
        for (uint64_t p = 0; p < n; p++) CHECK(dup.p[p] == e[p]);
        CHECK(sfx_common_substrings_dev(sa.p, bl.p, df.p, n, starts.p, nd, len.p, pos.p, cws.p, cwsb, nullptr) == SFX_OK);
        // ... and a df of random words over it
        for (uint64_t p = 0; p < n; p++) df.p[p] = (uint32_t)rng() >> (rng() % 32);
        CHECK(sfx_common_substrings_dev(sa.p, bl.p, df.p, n, starts.p, nd, len.p, pos.p, cws.p, cwsb, nullptr) == SFX_OK);
        cases++;
    }
    // da entries out of range: refused, nothing out of bounds on the way
    for (int kind = 0; kind < 3; kind++) {
        std::vector<uint32_t> v = c.da;
        if (kind == 0) v[n / 2] = (uint32_t)nd;
        else if (kind == 1) v[rng() % n] = NONE;
        else for (auto& x : v) x = (uint32_t)rng();
        Exact<uint32_t> bd(v), df(n), dup(n);
        Ws ws(wsb, 0x00);
        CHECK(sfx_doc_counts_dev(bd.p, lcp.p, n, nd, dup.p, df.p, ws.p, wsb, nullptr) == SFX_ERR_ARG);
        CHECK(sfx_doc_counts_u32(bd.p, lcp.p, n, nd, dup.p, df.p) == SFX_ERR_ARG);
        cases++;
    }
    CHECK(sfx_doc_counts_dev(da.p, lcp.p, n, 0, nullptr, nullptr, nullptr, 0, nullptr) == SFX_ERR_ARG);
}

int main()
{
    std::mt19937 rng(4711);
    std::vector<Coll> colls;
    for (int t = 0; t < 60; t++) {
        Coll c;
        const int sigma = 1 + t % 3, m = 1 + (int)(rng() % 7);
        for (int d = 0; d < m; d++) {
            std::string s;
            const size_t len = rng() % 5 == 0 ? 0 : rng() % 61;
            for (size_t p = 0; p < len; p++) s.push_back((char)('a' + rng() % sigma));
            if (d && rng() % 6 == 0) s = c.docs[rng() % d];
            c.docs.push_back(s);
        }
        colls.push_back(c);
    }
    for (size_t m : {16, 17, 32, 33, 512, 513}) {                        // 2m ranks: the node edges of fan 32 (and of 2, 4 under the hook)
        Coll c;
        c.docs = {std::string(m, 'a'), std::string(m, 'a')};
        colls.push_back(c);
    }
    {
        Coll c;
        c.docs = {"", "", ""};
        colls.push_back(c);
    }
    CHECK(sfx_doc_counts_dev(nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, nullptr) == SFX_OK);
    for (size_t t = 0; t < colls.size(); t++) {
        finish(&colls[t]);
        if (colls[t].docs[0].size() > 100) {                             // (a^m twice: no map of all substrings)
            const Coll& c = colls[t];
            const uint64_t n = c.sa.size(), wsb = sfx_doc_counts_workspace_bytes(n);
            Exact<uint32_t> da(c.da), lcp(c.lcp), df(n), dup(n);
            Ws ws(wsb, 0xFF);
            CHECK(sfx_doc_counts_dev(da.p, lcp.p, n, 2, dup.p, df.p, ws.p, wsb, nullptr) == SFX_OK);
            for (uint64_t p = 0; p < n; p++) CHECK(df.p[p] == 2 && dup.p[p] == 2 * (p / 2));
            cases++;
            continue;
        }
        run(colls[t], rng, (int)t);
    }
    printf("asan_docs ok: %zu cases\n", cases);
    return 0;
}
