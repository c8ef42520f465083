/* tests/runs_check.c -- serial checker of reported maximal repetitions (runs): TEST INFRASTRUCTURE ONLY.
 *
 * It reads the text and the triples (begin, end, period) and nothing else -- no suffix array, no LCP array, no code of the
 * engine's.  Three checks (tests/_runs.py feeds the first two one fault per kind and must see each refused):
 *
 *   runs_check_verify   every triple is in bounds, periodic (T[k] == T[k+p] on [b, e-p)), at least two periods long, not
 *                       extendable to either side, primitive-rooted (for every prime f | p, T[b..b+p) does not have period
 *                       p / f -- with e - b >= 2p that is minimality of p, by Fine and Wilf), passes the filter, and the
 *                       list is strictly ascending by (b, p).
 *   runs_check_sweep    enumerates every run of period <= P straight from the definition: for each p the maximal stretches
 *                       of T[k] == T[k+p] of length >= p, kept when their smallest period is p.  The reported triples of
 *                       period <= P (the list is taken as ascending: verify first) must be exactly those that pass the filter.
 *                       P = n / 2 is the complete check.  *found = how many the sweep enumerated after the filter.  Only the
 *                       periods P_lo .. P are looked at, so that a caller may give every thread a range of its own.
 *   runs_check_lyndon   lyn[i] = (the next j > i with isa[j] < isa[i], or n) - i, by one pass with a stack.
 * All return 0 or the code of the first fault and its place in *where (an index into the reported list; for a missing run
 * the index where it should stand). */
#include <stdint.h>
#include <stdlib.h>

enum { RC_OK = 0, RC_BOUNDS, RC_PERIODIC, RC_SHORT, RC_LEFT, RC_RIGHT, RC_ROOT, RC_FILTER, RC_ORDER, RC_MISSING, RC_EXTRA, RC_MEMORY, RC_LYNDON };

const char* runs_check_name(int rc)
{
    static const char* names[] = {"ok", "out of bounds", "not periodic", "shorter than two periods", "extends to the left",
                                  "extends to the right", "not the smallest period", "fails the filter", "not ascending by (begin, period)",
                                  "a run is missing", "not a run of the sweep", "out of memory", "wrong Lyndon length"};
    return rc >= 0 && rc <= RC_LYNDON ? names[rc] : "?";
}

/* does T[b .. b+p) have period q (q | p)? */
static int has_period(const uint8_t* t, uint64_t b, uint64_t p, uint64_t q)
{
    for (uint64_t k = b; k + q < b + p; k++)
        if (t[k] != t[k + q]) return 0;
    return 1;
}
static int primitive_root(const uint8_t* t, uint64_t b, uint64_t p)
{
    uint64_t m = p;
    for (uint64_t f = 2; f * f <= m; f++) {
        if (m % f) continue;
        if (has_period(t, b, p, p / f)) return 0;
        while (m % f == 0) m /= f;
    }
    if (m > 1 && p > 1 && has_period(t, b, p, p / m)) return 0;
    return 1;
}
static int passes(uint64_t b, uint64_t e, uint64_t p, uint32_t min_period, uint32_t max_period, uint32_t min_len)
{
    return p >= min_period && (max_period == 0 || p <= max_period) && e - b >= min_len;
}

int runs_check_verify(const uint8_t* t, uint64_t n, const uint32_t* rb, const uint32_t* re, const uint32_t* rp, uint64_t cnt,
                      uint32_t min_period, uint32_t max_period, uint32_t min_len, int64_t* where)
{
    for (uint64_t i = 0; i < cnt; i++) {
        const uint64_t b = rb[i], e = re[i], p = rp[i];
        *where = (int64_t)i;
        if (!(b < e && e <= n && p >= 1)) return RC_BOUNDS;
        if (e - b < 2 * p) return RC_SHORT;
        for (uint64_t k = b; k + p < e; k++)
            if (t[k] != t[k + p]) return RC_PERIODIC;
        if (b > 0 && t[b - 1] == t[b - 1 + p]) return RC_LEFT;
        if (e < n && t[e] == t[e - p]) return RC_RIGHT;
        if (!primitive_root(t, b, p)) return RC_ROOT;
        if (!passes(b, e, p, min_period, max_period, min_len)) return RC_FILTER;
        if (i > 0 && !(rb[i - 1] < b || (rb[i - 1] == b && rp[i - 1] < p))) return RC_ORDER;
    }
    *where = -1;
    return RC_OK;
}

typedef struct { uint64_t key; uint32_t e; } found_t;
static int by_key(const void* a, const void* b)
{
    const uint64_t x = ((const found_t*)a)->key, y = ((const found_t*)b)->key;
    return x < y ? -1 : x > y;
}

int runs_check_sweep(const uint8_t* t, uint64_t n, const uint32_t* rb, const uint32_t* re, const uint32_t* rp, uint64_t cnt, uint64_t P_lo, uint64_t P,
                     uint32_t min_period, uint32_t max_period, uint32_t min_len, uint64_t* found, int64_t* where)
{
    uint64_t have = 0, room = 1024;
    found_t* f = (found_t*)malloc(room * sizeof(found_t));
    *found = 0;
    *where = -1;
    if (!f) return RC_MEMORY;
    for (uint64_t p = P_lo ? P_lo : 1; p <= P && 2 * p <= n; p++) {
        uint64_t k = 0;
        while (k + p < n) {
            if (t[k] != t[k + p]) { k++; continue; }
            const uint64_t s = k;
            while (k + p < n && t[k] == t[k + p]) k++;
            const uint64_t b = s, e = k + p;                     /* the stretch [s, k) of equal pairs: T[s .. k + p) has period p */
            if (e - b < 2 * p || !primitive_root(t, b, p) || !passes(b, e, p, min_period, max_period, min_len)) continue;
            if (have == room) {
                found_t* g = (found_t*)realloc(f, (room *= 2) * sizeof(found_t));
                if (!g) { free(f); return RC_MEMORY; }
                f = g;
            }
            f[have].key = b << 32 | p;
            f[have++].e = (uint32_t)e;
        }
    }
    qsort(f, have, sizeof(found_t), by_key);
    *found = have;
    uint64_t j = 0;
    int rc = RC_OK;
    for (uint64_t i = 0; i < cnt && rc == RC_OK; i++) {
        if (rp[i] > P || rp[i] < P_lo) continue;
        const uint64_t key = (uint64_t)rb[i] << 32 | rp[i];
        *where = (int64_t)i;
        if (j < have && f[j].key < key) rc = RC_MISSING;
        else if (j == have || f[j].key != key || f[j].e != re[i]) rc = RC_EXTRA;
        else j++;
    }
    if (rc == RC_OK && j < have) { rc = RC_MISSING; *where = (int64_t)cnt; }
    if (rc == RC_OK) *where = -1;
    free(f);
    return rc;
}

int runs_check_lyndon(const uint32_t* isa, uint64_t n, const uint32_t* lyn, int64_t* where)
{
    uint64_t* stack = (uint64_t*)malloc((n + 1) * sizeof(uint64_t));
    uint64_t top = 0;
    int rc = RC_OK;
    *where = -1;
    if (!stack) return RC_MEMORY;
    for (uint64_t j = 0; j <= n && rc == RC_OK; j++) {
        while (top && (j == n || isa[stack[top - 1]] > isa[j])) {
            const uint64_t i = stack[--top];
            if (lyn[i] != j - i) { rc = RC_LYNDON; *where = (int64_t)i; break; }
        }
        stack[top++] = j;
    }
    free(stack);
    return rc;
}
