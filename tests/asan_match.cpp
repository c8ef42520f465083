// tests/asan_match.cpp -- the matching-statistics entry points under AddressSanitizer, as a stand-alone program over the
// emulator build of the product's kernels (device buffers are plain heap blocks there, so an out-of-bounds global load
// or store of a kernel is caught).  Every buffer is allocated at exactly its size.  Host code only; by hand:
//
//     make -C tests/emu asan
//     clang++ -O1 -g -std=c++17 -fsanitize=address -I include tests/asan_match.cpp \
//         -L tests/emu/asan -lsuffix_emu -Wl,-rpath,$PWD/tests/emu/asan -o tests/emu/asan/asan_match
//     tests/emu/asan/asan_match            # prints "asan_match ok: <cases> cases"
//
// Per case (random texts over 1-4 symbols, queries over one symbol more, caps 0 / 1 / 3 / 7, plain tables and
// collections with empty documents): all five entry points, every combination of the optional outputs, query bytes
// at an odd address; len is compared with the definition by brute force, start / end between the entry points.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "suffix_hip.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

template <class T> struct Exact {                     // exactly n elements on the heap; data() is NULL-safe for n == 0
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
    int cases = 0;
    for (int it = 0; it < 400; it++) {
        const int sigma = pick(1, 4);
        const char alpha[] = {'a', 'b', '\0', (char)0xFF, 'z'};
        // documents (one for a plain table); some empty
        const int ndocs = it % 2 ? pick(1, 6) : 1;
        std::string text;
        std::vector<uint64_t> starts;
        for (int d = 0; d < ndocs; d++) {
            starts.push_back(text.size());
            const int len = (ndocs > 1 && pick(0, 4) == 0) ? 0 : pick(it % 7 == 0 ? 0 : 1, 40);
            for (int k = 0; k < len; k++) text.push_back(alpha[pick(0, sigma - 1)]);
        }
        const uint64_t n = text.size();
        std::string query;
        for (int k = pick(1, 50); k > 0; k--) query.push_back(alpha[pick(0, sigma)]);
        if (n && pick(0, 1)) query.insert((size_t)pick(0, (int)query.size()), text.substr((size_t)pick(0, (int)n - 1), (size_t)pick(1, 20)));
        const uint64_t m = query.size();
        static const uint32_t caps[4] = {0, 1, 3, 7};
        const uint32_t cap = caps[it % 4];

        Exact<uint8_t> T(n), Q(m + 1);
        if (n) memcpy(T.p, text.data(), n);
        uint8_t* q = Q.p + 1;                          // an odd address
        memcpy(q, query.data(), m);
        Exact<uint64_t> S(starts.size());
        memcpy(S.p, starts.data(), starts.size() * 8);
        Exact<uint32_t> sa(n), da(n);
        CHECK(sfx_build_gsa_u32(T.p, n, S.p, starts.size(), sa.p, da.p, nullptr) == SFX_OK);

        // the definition: the longest prefix of query[i..] inside one document
        std::vector<uint32_t> want(m, 0);
        for (uint64_t i = 0; i < m; i++) {
            const uint64_t lim = cap ? std::min<uint64_t>(cap, m - i) : m - i;
            for (int d = 0; d < ndocs; d++) {
                const uint64_t b = starts[d], e = d + 1 < ndocs ? starts[d + 1] : n;
                for (uint64_t s = b; s < e; s++) {
                    uint64_t k = 0;
                    while (k < lim && s + k < e && (uint8_t)text[s + k] == q[i + k]) k++;
                    want[i] = std::max<uint32_t>(want[i], (uint32_t)k);
                }
            }
        }

        sfx_gindex* gx = nullptr;
        CHECK(sfx_gindex_create(T.p, n, S.p, starts.size(), sa.p, da.p, &gx) == SFX_OK);
        sfx_index* ix = nullptr;
        if (ndocs == 1) CHECK(sfx_index_create(T.p, n, sa.p, &ix) == SFX_OK);
        std::vector<uint32_t> first_start, first_end;
        for (int route = 0; route < 5; route++) {
            if (ndocs > 1 && route < 3) continue;      // the plain entries see one document only
            for (int combo = 0; combo < 4; combo++) {
                const bool want_src = combo & 1, want_iv = combo & 2;
                Exact<uint32_t> len(m), src(want_src ? m : 0), st(want_iv ? m : 0), en(want_iv ? m : 0);
                uint32_t *ps = want_src ? src.p : nullptr, *pa = want_iv ? st.p : nullptr, *pe = want_iv ? en.p : nullptr;
                int rc = -1;
                if (route == 0) rc = sfx_match_stats_dev(T.p, n, sa.p, q, m, cap, len.p, ps, pa, pe, nullptr);
                if (route == 1) rc = sfx_index_match_stats_dev(ix, q, m, cap, len.p, ps, pa, pe, nullptr);
                if (route == 2) rc = sfx_index_match_stats(ix, q, m, cap, len.p, ps, pa, pe);
                if (route == 3) rc = sfx_gindex_match_stats_dev(gx, q, m, cap, len.p, ps, pa, pe, nullptr);
                if (route == 4) rc = sfx_gindex_match_stats(gx, q, m, cap, len.p, ps, pa, pe);
                CHECK(rc == SFX_OK);
                for (uint64_t i = 0; i < m; i++) {
                    CHECK(len.p[i] == want[i]);
                    if (want_src) CHECK(want[i] ? src.p[i] < n && !memcmp(T.p + src.p[i], q + i, want[i]) : src.p[i] == 0xFFFFFFFFu);
                }
                if (want_iv) {
                    if (first_start.empty()) { first_start.assign(st.p, st.p + m); first_end.assign(en.p, en.p + m); }
                    CHECK(!memcmp(first_start.data(), st.p, m * 4) && !memcmp(first_end.data(), en.p, m * 4));
                }
                cases++;
            }
        }
        if (ix) sfx_index_destroy(ix);
        sfx_gindex_destroy(gx);
    }
    sfx_release_cached_buffers();
    printf("asan_match ok: %d cases\n", cases);
    return 0;
}
