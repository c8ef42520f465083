/* tests/ms_check.c -- serial, engine-independent checker of matching statistics (include/suffix_hip.h:
 * sfx_match_stats_dev and the index entries).  Built as a shared object into a temporary directory by tests/_match.py.
 *
 * Given the text T (n bytes), a table `sa` that the oracle has verified, optionally the document starts of a
 * collection (a suffix then ends with its document), the query text Q (m bytes), the cap max_len (0 = none) and the
 * four claimed arrays, ms_check returns 0 iff for every i, with lim = m - i or min(max_len, m - i):
 *   1  len <= lim;
 *   2  len == 0: Q[i] does not occur in T, the range is 0 / 0, src is NONE;
 *   3  otherwise 0 <= start < end <= n;
 *   4  the suffixes at ranks start and end - 1 begin with P = Q[i .. i + len) inside their document;
 *   5  those at ranks start - 1 and end do not;
 *   6  src < n and P stands at src;
 *   7  len < lim: a bisection inside [start, end) on the byte at depth len (a suffix that ends there sorts first)
 *      finds no Q[i + len] -- so no longer prefix occurs.
 * With a sorted table 3-5 pin the interval of P exactly, and 7 shows that P cannot be extended.  On a fault the number
 * of the failed check is returned and *where = i. */
#include <stdint.h>
#include <stddef.h>

#define NONE 0xFFFFFFFFu

typedef struct {
    const uint8_t* T;
    uint64_t n;
    const uint64_t* starts;
    uint64_t ndocs;
} Text;

/* length of the suffix at position s: to the end of its document (the last start <= s), or of the text */
static uint64_t suffix_len(const Text* t, uint64_t s)
{
    if (!t->starts || t->ndocs == 0) return t->n - s;
    uint64_t lo = 0, hi = t->ndocs;
    while (lo < hi) {
        uint64_t mid = (lo + hi) / 2;
        if (t->starts[mid] <= s) lo = mid + 1; else hi = mid;
    }
    return (lo < t->ndocs ? t->starts[lo] : t->n) - s;
}
static int begins_with(const Text* t, uint64_t s, const uint8_t* P, uint64_t len)
{
    if (s >= t->n || suffix_len(t, s) < len) return 0;
    for (uint64_t k = 0; k < len; k++)
        if (t->T[s + k] != P[k]) return 0;
    return 1;
}
/* the byte of the suffix at depth d, -1 if it ends there */
static int byte_at(const Text* t, uint64_t s, uint64_t d)
{
    return suffix_len(t, s) > d ? (int)t->T[s + d] : -1;
}

int ms_check(const uint8_t* T, uint64_t n, const uint32_t* sa, const uint64_t* starts, uint64_t ndocs,
             const uint8_t* Q, uint64_t m, uint32_t max_len,
             const uint32_t* len, const uint32_t* src, const uint32_t* start, const uint32_t* end, int64_t* where)
{
    Text t = {T, n, starts, ndocs};
    uint8_t present[256] = {0};
    for (uint64_t k = 0; k < n; k++) present[T[k]] = 1;
    for (uint64_t i = 0; i < m; i++) {
        *where = (int64_t)i;
        const uint64_t lim = (max_len && max_len < m - i) ? max_len : m - i;
        const uint64_t l = len[i];
        const uint8_t* P = Q + i;
        if (l > lim) return 1;
        if (l == 0) {
            if (present[P[0]] || start[i] != 0 || end[i] != 0 || src[i] != NONE) return 2;
            continue;
        }
        const uint64_t a = start[i], b = end[i];
        if (!(a < b && b <= n)) return 3;
        if (!begins_with(&t, sa[a], P, l) || !begins_with(&t, sa[b - 1], P, l)) return 4;
        if ((a > 0 && begins_with(&t, sa[a - 1], P, l)) || (b < n && begins_with(&t, sa[b], P, l))) return 5;
        if (src[i] >= n || !begins_with(&t, src[i], P, l)) return 6;
        if (l < lim) {
            const int c = P[l];
            uint64_t lo = a, hi = b;                       /* first rank of [a, b) whose byte at depth l is >= c */
            while (lo < hi) {
                uint64_t mid = (lo + hi) / 2;
                if (byte_at(&t, sa[mid], l) < c) lo = mid + 1; else hi = mid;
            }
            if (lo < b && byte_at(&t, sa[lo], l) == c) return 7;
        }
    }
    *where = -1;
    return 0;
}
