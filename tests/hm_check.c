/* hm_check.c -- serial checker of a k-mismatch occurrence list (include/suffix_hip.h).
 *
 * Reads the text, doc_starts, the patterns, k, the triples (pattern, tpos, mism) and first; needs no table and no second
 * engine.  In this order, stopping at the first wrong item (*where = its index):
 *   first      first[0] == 0, first never decreases, first[nq] == z, and pattern[i] == j for i in first[j] .. first[j+1]
 *   range      the pattern is not empty and the window [tpos, tpos + m) lies inside the text
 *   document   the window ends at or before the end of the document in which it starts
 *   count      mism is the number of differing bytes of the window
 *   mismatches mism <= k
 *   owner order within a pattern the owning pieces (the first piece of the cut b_t = floor(t m / (k + 1)) that matches
 *              exactly; an empty piece matches) never descend
 *   duplicate  no (pattern, tpos) appears twice
 *   missing    for every pattern j with complete[j] != 0: the number of windows with at most k mismatches, counted
 *              over the whole text, equals first[j+1] - first[j]  (*where = j)
 * Every listed triple is an occurrence, none is listed twice, and the counts agree: the list of a complete pattern IS
 * the set of its occurrences. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { HM_OK = 0, HM_FIRST, HM_RANGE, HM_DOCUMENT, HM_COUNT, HM_MISMATCHES, HM_OWNER, HM_DUPLICATE, HM_MISSING, HM_MEMORY };

const char* hm_check_name(int rc)
{
    static const char* names[] = {"ok", "first", "range", "document", "count", "mismatches", "owner order", "duplicate", "missing",
                                  "out of memory"};
    return rc >= 0 && rc <= HM_MEMORY ? names[rc] : "?";
}

/* the end of the document that holds position p (the last document starting at or before p); n without documents */
static uint64_t doc_end(uint64_t p, uint64_t n, const uint64_t* starts, uint64_t ndocs)
{
    if (!starts || ndocs == 0) return n;
    uint64_t lo = 0, hi = ndocs;                /* starts[lo] <= p < starts[hi] */
    while (hi - lo > 1) {
        uint64_t mid = lo + (hi - lo) / 2;
        if (starts[mid] <= p) lo = mid; else hi = mid;
    }
    return hi < ndocs ? starts[hi] : n;
}

static uint64_t differing(const uint8_t* a, const uint8_t* b, uint64_t lo, uint64_t hi)
{
    uint64_t c = 0;
    for (uint64_t i = lo; i < hi; i++) c += a[i] != b[i];
    return c;
}

/* windows of pattern (q, m) with at most k mismatches, inside one document each */
static uint64_t count_windows(const uint8_t* text, uint64_t n, const uint64_t* starts, uint64_t ndocs, const uint8_t* q, uint64_t m,
                              uint32_t k)
{
    uint64_t total = 0, nd = starts && ndocs ? ndocs : 1;
    for (uint64_t d = 0; d < nd; d++) {
        uint64_t lo = starts && ndocs ? starts[d] : 0, hi = starts && ndocs && d + 1 < ndocs ? starts[d + 1] : n;
        if (hi - lo < m) continue;
        for (uint64_t p = lo; p + m <= hi; p++) {
            uint32_t c = 0;
            const uint8_t* w = text + p;
            for (uint64_t i = 0; i < m; i++)
                if (w[i] != q[i] && ++c > k) break;
            total += c <= k;
        }
    }
    return total;
}

int hm_check(const uint8_t* text, uint64_t n, const uint64_t* starts, uint64_t ndocs, const uint8_t* qbytes, const uint64_t* qoff,
             uint64_t nq, uint32_t k, const uint32_t* pattern, const uint32_t* tpos, const uint8_t* mism, uint64_t z,
             const uint64_t* first, const uint8_t* complete, int64_t* where)
{
    *where = 0;
    if (first[0] != 0) return HM_FIRST;
    for (uint64_t j = 0; j < nq; j++) {
        *where = (int64_t)j;
        if (first[j + 1] < first[j] || first[j + 1] > z) return HM_FIRST;
    }
    *where = (int64_t)nq;
    if (first[nq] != z) return HM_FIRST;
    for (uint64_t j = 0; j < nq; j++)
        for (uint64_t i = first[j]; i < first[j + 1]; i++)
            if (pattern[i] != j) { *where = (int64_t)i; return HM_FIRST; }

    uint8_t* seen = (uint8_t*)calloc(n / 8 + 1, 1);
    if (!seen) return HM_MEMORY;
    int rc = HM_OK;
    for (uint64_t j = 0; j < nq && rc == HM_OK; j++) {
        const uint8_t* q = qbytes + qoff[j];
        const uint64_t m = qoff[j + 1] - qoff[j];
        uint64_t last_owner = 0;
        for (uint64_t i = first[j]; i < first[j + 1]; i++) {
            const uint64_t p = tpos[i];
            *where = (int64_t)i;
            if (m == 0 || p > n || m > n - p) { rc = HM_RANGE; break; }
            if (p + m > doc_end(p, n, starts, ndocs)) { rc = HM_DOCUMENT; break; }
            if (differing(q, text + p, 0, m) != mism[i]) { rc = HM_COUNT; break; }
            if (mism[i] > k) { rc = HM_MISMATCHES; break; }
            uint64_t owner = 0;                                  /* (<= k mismatches in k + 1 pieces: one of them matches) */
            while (owner <= k && differing(q, text + p, owner * m / (k + 1), (owner + 1) * m / (k + 1)) != 0) owner++;
            if (owner < last_owner) { rc = HM_OWNER; break; }
            last_owner = owner;
            if (seen[p >> 3] >> (p & 7) & 1) { rc = HM_DUPLICATE; break; }
            seen[p >> 3] |= (uint8_t)(1u << (p & 7));
        }
        if (rc != HM_OK) break;
        for (uint64_t i = first[j]; i < first[j + 1]; i++) seen[tpos[i] >> 3] = 0;      /* (this pattern's marks only) */
    }
    free(seen);
    if (rc != HM_OK) return rc;
    if (complete) {
        int64_t bad = -1;
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 1)
#endif
        for (int64_t j = 0; j < (int64_t)nq; j++) {
            if (!complete[j]) continue;
            const uint64_t m = qoff[j + 1] - qoff[j];
            const uint64_t have = first[j + 1] - first[j];
            const uint64_t want = m ? count_windows(text, n, starts, ndocs, qbytes + qoff[j], m, k) : 0;
            if (want != have) {
#ifdef _OPENMP
#pragma omp critical
#endif
                if (bad < 0 || j < bad) bad = j;
            }
        }
        if (bad >= 0) { *where = bad; return HM_MISSING; }
    }
    *where = -1;
    return HM_OK;
}
