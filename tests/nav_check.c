/* TEST INFRASTRUCTURE: serial checker of the suffix-tree navigation calls (tests/_nav.py).
 *
 * Independent of the engine: it reads sa and lcp (the oracle's), builds the inverse table and a sparse table of LCP
 * minima, and then decides every answer in O(1) from the definitions.  B[p] = lcp[p] with B[0] = 0 whatever lcp[0] holds.
 * nav_check_substr  (pos, len) -> [lo, hi), depth is accepted iff lo <= isa[pos] < hi, B[lo] < len, hi == n or
 *                   lcp[hi] < len, hi - lo == 1 or min lcp(lo, hi) >= len, and depth is end(pos) - pos for one rank,
 *                   else that minimum.  len == 0, pos <= n: (0, n, 0).  Anything else: NONE three times.
 * nav_check_lca     the interval holds both ranks, depth is the minimum between them, and [lo, hi) is an lcp-interval of
 *                   exactly that depth (the root [0, n) for depth 0); i == j: the rank alone, depth end(i) - i.
 * nav_check_argmin  lcp[arg] is the minimum of lcp[lo .. hi) (lcp[0] as stored) and no smaller index attains it.
 * nav_check_slink   slink[k] = w is accepted iff node_depth[w] == d - 1, node_lb[w] <= isa[sa[r] + 1] <= node_rb[w] for
 *                   r = node_lb[k] and r = node_rb[k], and w == 0 iff d == 1; NONE for the root.  The ancestors of a leaf
 *                   have distinct depths, so this pins w.
 * The first wrong answer is named. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { NAV_OK = 0, NAV_RANK, NAV_LEFT, NAV_RIGHT, NAV_INSIDE, NAV_DEPTH, NAV_MARK, NAV_NOT_MIN, NAV_NOT_LEFTMOST, NAV_LINK_DEPTH, NAV_LINK_RANGE,
       NAV_LINK_ROOT, NAV_ARG };
#define NONE 0xFFFFFFFFu

const char* nav_check_name(int rc)
{
    switch (rc) {
    case NAV_OK: return "ok";
    case NAV_RANK: return "a rank lies outside the interval";
    case NAV_LEFT: return "the left boundary is not below";
    case NAV_RIGHT: return "the right boundary is not below";
    case NAV_INSIDE: return "a boundary inside is below";
    case NAV_DEPTH: return "wrong depth";
    case NAV_MARK: return "wrong mark";
    case NAV_NOT_MIN: return "not the minimum";
    case NAV_NOT_LEFTMOST: return "a smaller index attains the minimum";
    case NAV_LINK_DEPTH: return "the target's depth is not d - 1";
    case NAV_LINK_RANGE: return "the target does not hold the shortened suffix";
    case NAV_LINK_ROOT: return "the root is the target of depth 1 alone";
    default: return "bad arguments";
    }
}

typedef struct {
    uint64_t n, ndocs;
    const uint32_t *sa, *lcp;
    const uint64_t* starts;
    uint32_t* isa;
    uint32_t** tab;                                  /* tab[j][i] = min lcp[i .. i + 2^j) */
    int levels;
} nav_t;

void nav_close(void* h)
{
    nav_t* v = (nav_t*)h;
    if (!v) return;
    for (int j = 1; j < v->levels; j++) free(v->tab[j]);
    free(v->tab);
    free(v->isa);
    free(v);
}

/* sa must be a permutation of [0, n) (NULL otherwise); the arrays are borrowed */
void* nav_open(const uint32_t* sa, const uint32_t* lcp, uint64_t n, const uint64_t* starts, uint64_t ndocs)
{
    nav_t* v = (nav_t*)calloc(1, sizeof(nav_t));
    v->n = n, v->ndocs = ndocs, v->sa = sa, v->lcp = lcp, v->starts = starts;
    v->isa = (uint32_t*)malloc((n + 1) * sizeof(uint32_t));
    memset(v->isa, 0xFF, (n + 1) * sizeof(uint32_t));
    for (uint64_t r = 0; r < n; r++) {
        if (sa[r] >= n || v->isa[sa[r]] != NONE) { nav_close(v); return NULL; }
        v->isa[sa[r]] = (uint32_t)r;
    }
    v->levels = 1;
    while ((2ull << (v->levels - 1)) <= n) v->levels++;
    v->tab = (uint32_t**)calloc((size_t)v->levels, sizeof(uint32_t*));
    v->tab[0] = (uint32_t*)lcp;
    for (int j = 1; j < v->levels; j++) {
        const uint64_t half = 1ull << (j - 1), cnt = n - (2 * half) + 1;
        v->tab[j] = (uint32_t*)malloc(cnt * sizeof(uint32_t));
        for (uint64_t i = 0; i < cnt; i++) {
            const uint32_t a = v->tab[j - 1][i], b = v->tab[j - 1][i + half];
            v->tab[j][i] = a < b ? a : b;
        }
    }
    return v;
}

/* min lcp[l .. r), l < r <= n */
static uint32_t range_min(const nav_t* v, uint64_t l, uint64_t r)
{
    const int j = 63 - __builtin_clzll(r - l);
    const uint32_t a = v->tab[j][l], b = v->tab[j][r - (1ull << j)];
    return a < b ? a : b;
}

static uint64_t end_of(const nav_t* v, uint64_t p)
{
    if (!v->starts) return v->n;
    uint64_t lo = 0, hi = v->ndocs;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (v->starts[mid] <= p) lo = mid; else hi = mid;
    }
    return hi < v->ndocs ? v->starts[hi] : v->n;
}

/* is [lo, hi) bounded by values below d on both sides, with nothing below d inside?  B[0] = 0 */
static int interval_at(const nav_t* v, uint64_t lo, uint64_t hi, uint64_t d)
{
    if (lo >= hi || hi > v->n) return NAV_RANK;
    if (lo != 0 && v->lcp[lo] >= d) return NAV_LEFT;
    if (lo == 0 && d == 0) return NAV_LEFT;
    if (hi != v->n && v->lcp[hi] >= d) return NAV_RIGHT;
    if (hi - lo > 1 && range_min(v, lo + 1, hi) < d) return NAV_INSIDE;
    return NAV_OK;
}

int nav_check_substr(const void* h, const uint32_t* pos, const uint32_t* len, uint64_t nq, const uint32_t* lo, const uint32_t* hi,
                     const uint32_t* depth, int64_t* where)
{
    const nav_t* v = (const nav_t*)h;
    if (!v) return NAV_ARG;
    for (uint64_t q = 0; q < nq; q++) {
        const uint64_t p = pos[q], ln = len[q], n = v->n;
        *where = (int64_t)q;
        if (ln == 0 && p <= n) {
            if (lo[q] != 0 || hi[q] != n || depth[q] != 0) return NAV_MARK;
            continue;
        }
        const uint64_t room = p < n ? end_of(v, p) - p : 0;
        if (ln == 0 || p >= n || ln > room) {
            if (lo[q] != NONE || hi[q] != NONE || depth[q] != NONE) return NAV_MARK;
            continue;
        }
        const uint64_t l = lo[q], r = hi[q];
        if (l >= r || r > n || v->isa[p] < l || v->isa[p] >= r) return NAV_RANK;
        const int rc = interval_at(v, l, r, ln);
        if (rc != NAV_OK) return rc;
        if (depth[q] != (r - l == 1 ? room : range_min(v, l + 1, r))) return NAV_DEPTH;
    }
    *where = -1;
    return NAV_OK;
}

int nav_check_lca(const void* h, const uint32_t* a, const uint32_t* b, uint64_t nq, const uint32_t* lo, const uint32_t* hi, const uint32_t* depth,
                  int64_t* where)
{
    const nav_t* v = (const nav_t*)h;
    if (!v) return NAV_ARG;
    for (uint64_t q = 0; q < nq; q++) {
        const uint64_t i = a[q], j = b[q], n = v->n;
        *where = (int64_t)q;
        if (i >= n || j >= n) {
            if (lo[q] != NONE || hi[q] != NONE || depth[q] != NONE) return NAV_MARK;
            continue;
        }
        const uint64_t l = lo[q], r = hi[q];
        if (i == j) {
            if (l != v->isa[i] || r != l + 1) return NAV_RANK;
            if (depth[q] != end_of(v, i) - i) return NAV_DEPTH;
            continue;
        }
        const uint64_t ra = v->isa[i] < v->isa[j] ? v->isa[i] : v->isa[j], rb = v->isa[i] < v->isa[j] ? v->isa[j] : v->isa[i];
        if (l >= r || r > n || ra < l || rb >= r) return NAV_RANK;
        const uint64_t d = range_min(v, ra + 1, rb + 1);
        if (depth[q] != d) return NAV_DEPTH;
        if (d == 0) {
            if (l != 0) return NAV_LEFT;
            if (r != n) return NAV_RIGHT;
            continue;
        }
        const int rc = interval_at(v, l, r, d);                       /* (its minimum is d: it holds ra and rb) */
        if (rc != NAV_OK) return rc;
    }
    *where = -1;
    return NAV_OK;
}

int nav_check_argmin(const void* h, const uint32_t* lo, const uint32_t* hi, uint64_t nq, const uint32_t* arg, int64_t* where)
{
    const nav_t* v = (const nav_t*)h;
    if (!v) return NAV_ARG;
    for (uint64_t q = 0; q < nq; q++) {
        const uint64_t l = lo[q], r = hi[q], g = arg[q];
        *where = (int64_t)q;
        if (l >= r || r > v->n) {
            if (g != NONE) return NAV_MARK;
            continue;
        }
        if (g < l || g >= r) return NAV_RANK;
        const uint32_t m = range_min(v, l, r);
        if (v->lcp[g] != m) return NAV_NOT_MIN;
        if (g > l && range_min(v, l, g) <= m) return NAV_NOT_LEFTMOST;
    }
    *where = -1;
    return NAV_OK;
}

int nav_check_slink(const void* h, uint64_t nodes, const uint32_t* node_lb, const uint32_t* node_rb, const uint32_t* node_depth,
                    const uint32_t* slink, int64_t* where)
{
    const nav_t* v = (const nav_t*)h;
    if (!v || v->starts) return NAV_ARG;
    for (uint64_t k = 0; k < nodes; k++) {
        const uint64_t d = node_depth[k], w = slink[k];
        *where = (int64_t)k;
        if (node_lb[k] > node_rb[k] || node_rb[k] >= v->n) return NAV_ARG;
        if (d == 0) {
            if (w != NONE) return NAV_MARK;
            continue;
        }
        if (w >= nodes) return NAV_MARK;
        if ((w == 0) != (d == 1)) return NAV_LINK_ROOT;
        if (node_depth[w] != d - 1) return NAV_LINK_DEPTH;
        if (d == 1) continue;                                         /* (the root holds every rank) */
        const uint64_t ends[2] = {node_lb[k], node_rb[k]};
        for (int e = 0; e < 2; e++) {
            const uint64_t s = (uint64_t)v->sa[ends[e]] + 1;
            if (s >= v->n) return NAV_ARG;                            /* (a suffix under a node of depth >= 2 has two bytes) */
            if (v->isa[s] < node_lb[w] || v->isa[s] > node_rb[w]) return NAV_LINK_RANGE;
        }
    }
    *where = -1;
    return NAV_OK;
}
