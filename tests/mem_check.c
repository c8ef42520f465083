/* mem_check.c -- serial checker of a list of maximal exact matches (include/suffix_hip.h).
 * TEST INFRASTRUCTURE: needs no second engine.  T = text of n bytes (with doc_starts: a collection, a match lies inside
 * one document), sa = its table, Q = query of m bytes, L = min_len, (qpos, tpos, len)[z] = the list.
 *
 * For every triple: in range and len >= L (1), inside one document (2), equal bytes (3), not extendable to the left (4)
 * nor to the right (5); the list strictly ascending by (qpos, rank of tpos) (6), which also proves the triples
 * distinct; with flag bit 0 (unique) the bytes occur once: neither rank neighbour shares len bytes (7).
 * uniq_out (z bytes, may be NULL) receives that uniqueness test for every triple, whatever the flag.
 * *sum_out = the sum of (len - L + 1).  Returns 0, or the number of the first failed check with *where = its triple. */
#include <stdint.h>
#include <stdlib.h>

const char* mem_check_name(int code)
{
    static const char* names[] = {"ok", "range", "document", "bytes", "left-extendable", "right-extendable", "order", "not unique", "table"};
    return code >= 0 && code <= 8 ? names[code] : "?";
}

/* the document of position p: the last one that starts at or before p (empty documents share their start with the next) */
static void doc_bounds(const uint64_t* starts, uint64_t nd, uint64_t n, uint64_t p, uint64_t* lo, uint64_t* hi)
{
    if (!starts || nd == 0) { *lo = 0; *hi = n; return; }
    uint64_t a = 0, b = nd;                       /* starts[a] <= p < starts[b] */
    while (b - a > 1) {
        uint64_t mid = a + (b - a) / 2;
        if (starts[mid] <= p) a = mid; else b = mid;
    }
    *lo = starts[a];
    *hi = a + 1 < nd ? starts[a + 1] : n;
}
/* do the truncated suffixes at p and s share at least l bytes? (T[p .. p+l) lies inside p's document) */
static int shares(const uint8_t* T, const uint64_t* starts, uint64_t nd, uint64_t n, uint64_t p, uint64_t s, uint64_t l)
{
    uint64_t lo, hi;
    doc_bounds(starts, nd, n, s, &lo, &hi);
    if (hi - s < l) return 0;
    for (uint64_t k = 0; k < l; k++)
        if (T[p + k] != T[s + k]) return 0;
    return 1;
}

int mem_check(const uint8_t* T, uint64_t n, const uint32_t* sa, const uint64_t* starts, uint64_t nd, const uint8_t* Q, uint64_t m,
              uint32_t L, uint32_t flags, const uint32_t* qpos, const uint32_t* tpos, const uint32_t* len, uint64_t z,
              uint8_t* uniq_out, uint64_t* sum_out, int64_t* where)
{
    uint32_t* rank = (uint32_t*)malloc((n ? n : 1) * sizeof(uint32_t));
    uint64_t sum = 0;
    int rc = 0;
    *where = -1;
    for (uint64_t r = 0; r < n; r++) {
        if (sa[r] >= n) { free(rank); return 8; }
        rank[sa[r]] = (uint32_t)r;
    }
    for (uint64_t k = 0; k < z && !rc; k++) {
        const uint64_t i = qpos[k], p = tpos[k], l = len[k];
        uint64_t lo, hi;
        *where = (int64_t)k;
        if (l < L || l == 0 || i >= m || p >= n || i + l > m || p + l > n) { rc = 1; break; }
        doc_bounds(starts, nd, n, p, &lo, &hi);
        if (p + l > hi) { rc = 2; break; }
        for (uint64_t j = 0; j < l; j++)
            if (Q[i + j] != T[p + j]) { rc = 3; break; }
        if (rc) break;
        if (i > 0 && p > lo && Q[i - 1] == T[p - 1]) { rc = 4; break; }
        if (i + l < m && p + l < hi && Q[i + l] == T[p + l]) { rc = 5; break; }
        if (k > 0 && !(qpos[k - 1] < i || (qpos[k - 1] == i && rank[tpos[k - 1]] < rank[p]))) { rc = 6; break; }
        {
            const uint64_t r = rank[p];
            int uniq = 1;
            if (r > 0 && shares(T, starts, nd, n, p, sa[r - 1], l)) uniq = 0;
            if (r + 1 < n && shares(T, starts, nd, n, p, sa[r + 1], l)) uniq = 0;
            if (uniq_out) uniq_out[k] = (uint8_t)uniq;
            if ((flags & 1u) && !uniq) { rc = 7; break; }
        }
        sum += l - L + 1;
    }
    free(rank);
    *sum_out = sum;
    if (!rc) *where = -1;
    return rc;
}
