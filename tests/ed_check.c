/* ed_check.c -- serial checker of a k-error occurrence list (include/suffix_hip.h).
 *
 * It reads the text, the document starts, the patterns and the quadruples (pattern, tbegin, tend, dist) with their CSR
 * array `first`, and nothing of the engine's.
 *   verify (always)  first is monotone, ends at z and files every quadruple under its pattern; inside a pattern the
 *                    ends ascend strictly (no duplicate, no swapped pair); tbegin <= tend <= n inside one document,
 *                    dist <= k; ed(P, T[tbegin..tend)) = dist by a full dynamic programme of its own over the
 *                    reversed strings, whose last column gives ed(P, T[s..tend)) for every s in [tend - m - k, tend]
 *                    at once: none is smaller than dist, and no s above tbegin reaches dist.
 *   sweep            for the patterns with sweep[j] != 0: Sellers' recurrence over every whole document; the ends
 *                    with a column minimum of at most k must be exactly the reported ones, with that distance.
 * Patterns are independent: with OpenMP they are spread over the threads; the fault reported is the one at the lowest
 * quadruple (for "missing": the lowest pattern), whatever the schedule.
 * -> 0 or the number of a rule (ed_check_name), *where = the quadruple (the pattern for "first" / "missing"). */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { ED_OK = 0, ED_FIRST, ED_RANGE, ED_ORDER, ED_DOCUMENT, ED_DISTANCE, ED_SMALLER, ED_BEGIN, ED_MISSING, ED_EXTRA, ED_MEMORY, ED_COUNT };

const char* ed_check_name(int rc)
{
    static const char* names[ED_COUNT] = {"ok", "first", "range", "order", "document", "distance", "smaller", "begin", "missing", "extra", "memory"};
    return rc >= 0 && rc < ED_COUNT ? names[rc] : "?";
}

/* the document that holds the text bytes before `end` (end > 0): the last one that starts below end */
static void doc_of(const uint64_t* starts, uint64_t ndocs, uint64_t n, uint64_t end, uint64_t* lo, uint64_t* hi)
{
    if (!starts || ndocs == 0) {
        *lo = 0;
        *hi = n;
        return;
    }
    uint64_t a = 0, b = ndocs;                          /* starts[a] < end <= starts[b] (b = ndocs: none) */
    while (b - a > 1) {
        const uint64_t mid = a + (b - a) / 2;
        if (starts[mid] < end) a = mid; else b = mid;
    }
    *lo = starts[a];
    *hi = a + 1 < ndocs ? starts[a + 1] : n;
}

/* col[u] = ed(P, T[end - u .. end)) for u = 0 .. umax: rows over the pattern read backwards, columns over the text read
 * backwards from end; two rows of umax + 1 cells */
static int backward_column(const uint8_t* p, uint64_t m, const uint8_t* text, uint64_t end, uint64_t umax, uint32_t* col)
{
    uint32_t* prev = (uint32_t*)malloc((umax + 1) * sizeof(uint32_t));
    if (!prev) return 0;
    for (uint64_t u = 0; u <= umax; u++) prev[u] = (uint32_t)u;
    for (uint64_t i = 1; i <= m; i++) {
        const uint8_t c = p[m - i];
        col[0] = (uint32_t)i;
        for (uint64_t u = 1; u <= umax; u++) {
            uint32_t v = prev[u - 1] + (text[end - u] != c);
            if (prev[u] + 1 < v) v = prev[u] + 1;
            if (col[u - 1] + 1 < v) v = col[u - 1] + 1;
            col[u] = v;
        }
        memcpy(prev, col, (umax + 1) * sizeof(uint32_t));
    }
    if (m == 0) memcpy(col, prev, (umax + 1) * sizeof(uint32_t));
    free(prev);
    return 1;
}

/* col[u] = ed(P, T[from .. from + u)) for u = 0 .. umax */
static int forward_column(const uint8_t* p, uint64_t m, const uint8_t* text, uint64_t from, uint64_t umax, uint32_t* col)
{
    uint32_t* prev = (uint32_t*)malloc((umax + 1) * sizeof(uint32_t));
    if (!prev) return 0;
    for (uint64_t u = 0; u <= umax; u++) prev[u] = col[u] = (uint32_t)u;
    for (uint64_t i = 1; i <= m; i++) {
        const uint8_t c = p[i - 1];
        col[0] = (uint32_t)i;
        for (uint64_t u = 1; u <= umax; u++) {
            uint32_t v = prev[u - 1] + (text[from + u - 1] != c);
            if (prev[u] + 1 < v) v = prev[u] + 1;
            if (col[u - 1] + 1 < v) v = col[u - 1] + 1;
            col[u] = v;
        }
        memcpy(prev, col, (umax + 1) * sizeof(uint32_t));
    }
    free(prev);
    return 1;
}

/* The candidate and hit counts of the definition for a plain text (include/suffix_hip.h): piece t of pattern j has the
 * exact interval [lo[j (k + 1) + t], hi[..]) of the table sa -- found by whoever calls, not by the engine under test.
 * Per candidate the left value L over its window and the right values R(e), each by a full table; a hit is an e with
 * L + R(e) <= k.  -> 0, or ED_MEMORY. */
int ed_counts(const uint8_t* text, uint64_t n, const uint32_t* sa, const uint8_t* qbytes, const uint64_t* qoff, uint64_t nq, uint32_t k,
              const uint32_t* lo, const uint32_t* hi, uint64_t* cands_out, uint64_t* hits_out)
{
    uint64_t C = 0, H = 0;
    int failed = 0;
    int64_t jj;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : C, H)
    for (jj = 0; jj < (int64_t)nq; jj++) {
        const uint64_t j = (uint64_t)jj, m = qoff[j + 1] - qoff[j];
        const uint8_t* p = qbytes + qoff[j];
        uint32_t* col = (uint32_t*)malloc((m + k + 1) * sizeof(uint32_t));
        if (!col) { failed = 1; continue; }
        for (uint64_t t = 0; t <= k; t++) {
            const uint64_t bt = t * m / (k + 1), bt1 = (t + 1) * m / (k + 1), e = j * (k + 1) + t;
            for (uint64_t r = lo[e]; r < hi[e]; r++) {
                const uint64_t q = sa[r], qe = q + (bt1 - bt);
                C++;
                if (qe > n) continue;
                uint64_t umax = bt + k < q ? bt + k : q;
                if (!backward_column(p, bt, text, q, umax, col)) { failed = 1; break; }
                uint32_t L = col[0];
                for (uint64_t u = 1; u <= umax; u++) L = col[u] < L ? col[u] : L;
                if (L > k) continue;
                umax = m - bt1 + k < n - qe ? m - bt1 + k : n - qe;
                if (!forward_column(p + bt1, m - bt1, text, qe, umax, col)) { failed = 1; break; }
                for (uint64_t u = 0; u <= umax; u++) H += L + col[u] <= k;
            }
        }
        free(col);
    }
    *cands_out = C;
    *hits_out = H;
    return failed ? ED_MEMORY : ED_OK;
}

/* Z of the definition: the ends with a column minimum of at most k, by Sellers' recurrence over every whole document,
 * for every pattern. */
int ed_occurrences(const uint8_t* text, uint64_t n, const uint64_t* starts, uint64_t ndocs, const uint8_t* qbytes, const uint64_t* qoff,
                   uint64_t nq, uint32_t k, uint64_t* count_out)
{
    uint64_t Z = 0;
    int failed = 0;
    int64_t jj;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : Z)
    for (jj = 0; jj < (int64_t)nq; jj++) {
        const uint64_t j = (uint64_t)jj, m = qoff[j + 1] - qoff[j];
        const uint8_t* p = qbytes + qoff[j];
        uint32_t* D = (uint32_t*)malloc((m + 1) * sizeof(uint32_t));
        if (!D) { failed = 1; continue; }
        const uint64_t nd = starts && ndocs ? ndocs : 1;
        for (uint64_t dn = 0; dn < nd; dn++) {
            const uint64_t lo = starts && ndocs ? starts[dn] : 0, hi = starts && ndocs ? (dn + 1 < ndocs ? starts[dn + 1] : n) : n;
            for (uint64_t r = 0; r <= m; r++) D[r] = (uint32_t)r;
            for (uint64_t e = lo + 1; e <= hi; e++) {
                const uint8_t c = text[e - 1];
                uint32_t diag = D[0];
                for (uint64_t r = 1; r <= m; r++) {
                    uint32_t v = diag + (p[r - 1] != c);
                    if (D[r] + 1 < v) v = D[r] + 1;
                    if (D[r - 1] + 1 < v) v = D[r - 1] + 1;
                    diag = D[r];
                    D[r] = v;
                }
                Z += D[m] <= k;
            }
        }
        free(D);
    }
    *count_out = Z;
    return failed ? ED_MEMORY : ED_OK;
}

static void fault(int rc, int64_t at, int* best_rc, int64_t* best_at)
{
#pragma omp critical(ed_check_fault)
    {
        if (*best_rc == ED_OK || at < *best_at) {
            *best_rc = rc;
            *best_at = at;
        }
    }
}

int ed_check(const uint8_t* text, uint64_t n, const uint64_t* starts, uint64_t ndocs, const uint8_t* qbytes, const uint64_t* qoff,
             uint64_t nq, uint32_t k, const uint32_t* pat, const uint32_t* tbegin, const uint32_t* tend, const uint8_t* dist, uint64_t z,
             const uint64_t* first, const uint8_t* sweep, int64_t* where)
{
    *where = -1;
    if (first[0] != 0) { *where = 0; return ED_FIRST; }
    for (uint64_t j = 0; j < nq; j++)
        if (first[j + 1] < first[j] || first[j + 1] > z) { *where = (int64_t)j; return ED_FIRST; }
    if (first[nq] != z) { *where = (int64_t)nq; return ED_FIRST; }
    for (uint64_t j = 0; j < nq; j++)
        for (uint64_t i = first[j]; i < first[j + 1]; i++)
            if (pat[i] != j) { *where = (int64_t)i; return ED_FIRST; }
    int rc = ED_OK;
    int64_t at = -1;
    int64_t jj;
#pragma omp parallel for schedule(dynamic, 1)
    for (jj = 0; jj < (int64_t)nq; jj++) {
        const uint64_t j = (uint64_t)jj;
        const uint8_t* p = qbytes + qoff[j];
        const uint64_t m = qoff[j + 1] - qoff[j];
        uint32_t* col = (uint32_t*)malloc((m + k + 1) * sizeof(uint32_t));
        if (!col) { fault(ED_MEMORY, (int64_t)first[j], &rc, &at); continue; }
        int bad = 0;
        for (uint64_t i = first[j]; i < first[j + 1] && !bad; i++) {
            const uint64_t b = tbegin[i], e = tend[i], d = dist[i];
            bad = 1;
            if (b > e || e > n || d > k || e == 0) { fault(ED_RANGE, (int64_t)i, &rc, &at); break; }
            if (i > first[j] && tend[i - 1] >= e) { fault(ED_ORDER, (int64_t)i, &rc, &at); break; }
            uint64_t lo, hi;
            doc_of(starts, ndocs, n, e, &lo, &hi);
            if (b < lo || e > hi) { fault(ED_DOCUMENT, (int64_t)i, &rc, &at); break; }
            uint64_t umax = m + k;
            if (umax > e - lo) umax = e - lo;
            if (e - b > umax) { fault(ED_DISTANCE, (int64_t)i, &rc, &at); break; }      /* |m - (e - b)| > k: more than k edits */
            if (!backward_column(p, m, text, e, umax, col)) { fault(ED_MEMORY, (int64_t)i, &rc, &at); break; }
            if (col[e - b] != d) { fault(ED_DISTANCE, (int64_t)i, &rc, &at); break; }
            int worse = 0;
            for (uint64_t u = 0; u <= umax && !worse; u++)
                if (col[u] < d) worse = ED_SMALLER;
            for (uint64_t u = 0; u < e - b && !worse; u++)
                if (col[u] == d) worse = ED_BEGIN;
            if (worse) { fault(worse, (int64_t)i, &rc, &at); break; }
            bad = 0;
        }
        free(col);
        if (bad || !sweep || !sweep[j]) continue;
        /* Sellers over every document: D[i] = the least ed(P[0..i), T[s..e)) over s, column by column */
        uint32_t* D = (uint32_t*)malloc((m + 1) * sizeof(uint32_t));
        if (!D) { fault(ED_MEMORY, (int64_t)first[j], &rc, &at); continue; }
        uint64_t i = first[j];
        const uint64_t nd = starts && ndocs ? ndocs : 1;
        for (uint64_t dn = 0; dn < nd && !bad; dn++) {
            const uint64_t lo = starts && ndocs ? starts[dn] : 0, hi = starts && ndocs ? (dn + 1 < ndocs ? starts[dn + 1] : n) : n;
            for (uint64_t r = 0; r <= m; r++) D[r] = (uint32_t)r;
            for (uint64_t e = lo + 1; e <= hi && !bad; e++) {
                const uint8_t c = text[e - 1];
                uint32_t diag = D[0];
                for (uint64_t r = 1; r <= m; r++) {
                    uint32_t v = diag + (p[r - 1] != c);
                    if (D[r] + 1 < v) v = D[r] + 1;
                    if (D[r - 1] + 1 < v) v = D[r - 1] + 1;
                    diag = D[r];
                    D[r] = v;
                }
                if (D[m] <= k) {
                    if (i >= first[j + 1] || tend[i] > e) { fault(ED_MISSING, (int64_t)j, &rc, &at); bad = 1; }
                    else if (tend[i] < e) { fault(ED_EXTRA, (int64_t)i, &rc, &at); bad = 1; }
                    else if (dist[i] != D[m]) { fault(ED_DISTANCE, (int64_t)i, &rc, &at); bad = 1; }
                    else i++;
                } else if (i < first[j + 1] && tend[i] == e) { fault(ED_EXTRA, (int64_t)i, &rc, &at); bad = 1; }
            }
        }
        if (!bad && i != first[j + 1]) fault(ED_EXTRA, (int64_t)i, &rc, &at);
        free(D);
    }
    *where = at;
    return rc;
}
