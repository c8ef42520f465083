/* TEST INFRASTRUCTURE: serial checker of the LCE index's answers (tests/_lce.py).
 *
 * lce_check       reads only the text, doc_starts, the pairs, k and the reported lengths: every length must be the
 *                 definition's -- the largest l with at most k differing places among the first l bytes, i + l and j + l
 *                 inside the text / the positions' documents; 0 for a position equal to n, 0xFFFFFFFF for one above.
 *                 Bytes are compared 8 per step.  The first wrong pair is named.
 * lce_check_min   out[q] = min lcp[lo .. hi) by a plain loop; 0xFFFFFFFF for lo >= hi or hi > n.
 * lce_check_isa   sa[isa[p]] == p for every p (and isa[p] < n).
 * No table is involved in lce_check, so a wrong table cannot hide a wrong answer. */
#include <stdint.h>
#include <string.h>

enum { LCE_OK = 0, LCE_TOO_SHORT, LCE_TOO_LONG, LCE_PAST_END, LCE_MARK, LCE_MIN, LCE_ISA, LCE_ARG };

const char* lce_check_name(int rc)
{
    switch (rc) {
    case LCE_OK: return "ok";
    case LCE_TOO_SHORT: return "the extension goes on";
    case LCE_TOO_LONG: return "more mismatches than allowed";
    case LCE_PAST_END: return "past an end";
    case LCE_MARK: return "wrong mark for a position >= n";
    case LCE_MIN: return "not the minimum";
    case LCE_ISA: return "not the inverse";
    default: return "bad arguments";
    }
}

/* the end of the document that holds p < n: the last d with starts[d] <= p */
static uint64_t end_of(uint64_t p, uint64_t n, const uint64_t* starts, uint64_t ndocs)
{
    if (!starts) return n;
    uint64_t lo = 0, hi = ndocs;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (starts[mid] <= p) lo = mid; else hi = mid;
    }
    return hi < ndocs ? starts[hi] : n;
}

/* equal bytes of x and y from offset `from` on, at most `room` in all */
static uint64_t agree(const uint8_t* x, const uint8_t* y, uint64_t from, uint64_t room)
{
    uint64_t l = from;
    while (l + 8 <= room) {
        uint64_t a, b;
        memcpy(&a, x + l, 8);
        memcpy(&b, y + l, 8);
        if (a != b) return l + (uint64_t)(__builtin_ctzll(a ^ b) >> 3);   /* little-endian: the lowest differing byte */
        l += 8;
    }
    while (l < room && x[l] == y[l]) l++;
    return l;
}

int lce_check(const uint8_t* text, uint64_t n, const uint64_t* starts, uint64_t ndocs, const uint32_t* a, const uint32_t* b, uint64_t nq,
              uint32_t k, const uint32_t* len, int64_t* where)
{
    if (starts && (ndocs == 0 || starts[0] != 0)) return LCE_ARG;
    for (uint64_t q = 0; q < nq; q++) {
        const uint64_t i = a[q], j = b[q], got = len[q];
        *where = (int64_t)q;
        if (i > n || j > n) {
            if (got != 0xFFFFFFFFu) return LCE_MARK;
            continue;
        }
        if (i == n || j == n) {
            if (got != 0) return LCE_MARK;
            continue;
        }
        const uint64_t ei = end_of(i, n, starts, ndocs), ej = end_of(j, n, starts, ndocs);
        const uint64_t room = ei - i < ej - j ? ei - i : ej - j;
        if (got > room) return LCE_PAST_END;
        if (i == j) {                                   /* every byte agrees with itself */
            if (got != room) return LCE_TOO_SHORT;
            continue;
        }
        /* walk the definition: the (k + 1)-th mismatch, or the end, is where the extension stops */
        uint64_t l = 0;
        uint32_t miss = 0;
        for (;;) {
            l = agree(text + i, text + j, l, room);
            if (l == room || miss == k) break;
            miss++;
            l++;                                        /* (l < room: the differing byte lies inside both ends) */
        }
        if (got < l) return LCE_TOO_SHORT;
        if (got > l) return LCE_TOO_LONG;
    }
    *where = -1;
    return LCE_OK;
}

int lce_check_min(const uint32_t* lcp, uint64_t n, const uint32_t* lo, const uint32_t* hi, uint64_t nq, const uint32_t* out, int64_t* where)
{
    for (uint64_t q = 0; q < nq; q++) {
        uint32_t m = 0xFFFFFFFFu;
        if (lo[q] < hi[q] && hi[q] <= n)
            for (uint64_t r = lo[q]; r < hi[q]; r++)
                if (lcp[r] < m) m = lcp[r];
        *where = (int64_t)q;
        if (out[q] != m) return LCE_MIN;
    }
    *where = -1;
    return LCE_OK;
}

int lce_check_isa(const uint32_t* sa, const uint32_t* isa, uint64_t n, int64_t* where)
{
    for (uint64_t p = 0; p < n; p++) {
        *where = (int64_t)p;
        if (isa[p] >= n || sa[isa[p]] != p) return LCE_ISA;
    }
    *where = -1;
    return LCE_OK;
}
