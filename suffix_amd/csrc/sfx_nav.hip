// sfx_nav.hip -- suffix-tree navigation over the LCE index: substring loci, lowest common ancestors, the leftmost argmin
// of an LCP range and the suffix links of a node table (include/suffix_hip.h).
//
// Everything rests on one search over the min-tree an sfx_lce handle already holds (sfx_lce.hip): the nearest boundary to
// the left and to the right of a rank whose LCP value is below a threshold d,
//   bounds(r, d) = [lo, hi)   lo = the largest p <= r with B[p] < d, hi = the smallest p > r with B[p] < d (n if none),
// with B[0] = 0 whatever lcp[0] holds (boundary 0 always qualifies) and bounds(r, 0) = [0, n).
// One lane answers one query (section 21's A/B settled that for range minima; for this search it is an assumption).  From
// index r on level 0 the lane scans the words of r's node on the search side for the nearest one below d; if there is none
// it steps to the parent's neighbour on that side and repeats one level up; once a word below d is found above level 0 it
// descends, taking the nearest such word of every child node.  At most `levels` nodes up and `levels` - 1 down per side, a
// node being one 128-byte line; whole lines are read 16 bytes at a time where the alignment allows (lce_span_min's rule).
// The left search never evaluates lcp[0]: falling off the left gives 0, falling off the right n.  Every index stays below
// its level's count (a level's last node is partial).  A descent that finds no word below d -- possible only when the
// caller changed the borrowed lcp after creation -- takes the node's word nearest to r, so for ANY lcp contents nothing is
// read out of bounds and lo <= r < hi holds.
//
//   nav_substr   pos -> isa -> bounds(isa[pos], len) -> the depth of the lowest node at or below the locus
//   nav_lca      the fused range minimum between two ranks, then bounds
//   nav_argmin   the minimum of lcp[lo .. hi), then the first index at or right of lo that attains it (the same search)
//   nav_home     map[home(k)] = k for every node k below the root: home = the leftmost argmin of lcp[lb + 1 .. rb + 1)
//   nav_slink    per node of depth d >= 2: q = sa[lb] + 1, bounds(isa[q], d - 1), the home of that interval, the map
// No atomics, no read-back, nothing allocated.  An interval does not identify a node (in a unary text the root and the
// depth-1 node share [0, n)): a node is its home boundary, and the root is decided by d == 0, never by a lookup.
//
// Compiled as part of sfx_api.hip (which includes this file after sfx_lce.hip), like sfx_runs.hip.
#pragma once
#include "sfx_lce.hip"

namespace sfx {

constexpr uint64_t kNavOff = ~0ull;                    // a search that fell off its side

// the first / last index of [a, b) with L[i] <= t (b - a <= 32), kNavOff if none; only words of [a, b) are read.
// vec: L is 16-byte aligned
__device__ __forceinline__ uint64_t nav_first_le(const uint32_t* __restrict__ L, uint64_t a, uint64_t b, bool vec, uint32_t t)
{
    uint64_t i = a;
    if (vec) {
        for (; i < b && (i & 3); i++)
            if (L[i] <= t) return i;
        for (; i + 4 <= b; i += 4) {
            const uint4 w = *reinterpret_cast<const uint4*>(L + i);
            if (w.x <= t) return i;
            if (w.y <= t) return i + 1;
            if (w.z <= t) return i + 2;
            if (w.w <= t) return i + 3;
        }
    }
    for (; i < b; i++)
        if (L[i] <= t) return i;
    return kNavOff;
}
__device__ __forceinline__ uint64_t nav_last_le(const uint32_t* __restrict__ L, uint64_t a, uint64_t b, bool vec, uint32_t t)
{
    uint64_t i = b;
    if (vec) {
        for (; i > a && (i & 3); i--)
            if (L[i - 1] <= t) return i - 1;
        for (; i >= a + 4; i -= 4) {
            const uint4 w = *reinterpret_cast<const uint4*>(L + i - 4);
            if (w.w <= t) return i - 1;
            if (w.z <= t) return i - 2;
            if (w.y <= t) return i - 3;
            if (w.x <= t) return i - 4;
        }
    }
    for (; i > a; i--)
        if (L[i - 1] <= t) return i - 1;
    return kNavOff;
}
// level k of the handle and its word count, from n alone (as lce_walk derives them on its way up)
__device__ __forceinline__ const uint32_t* nav_level(const LceView& v, int k, uint64_t* cnt_out)
{
    if (k == 0) { *cnt_out = v.n; return v.lcp; }
    const uint64_t mask = (1ull << v.fan_log) - 1;
    const uint32_t* L = v.tree;
    uint64_t cnt = ((uint64_t)v.n + mask) >> v.fan_log;
    for (int j = 1; j < k; j++) {
        L += lce_line_up(cnt);
        cnt = (cnt + mask) >> v.fan_log;
    }
    *cnt_out = cnt;
    return L;
}
// RIGHT: the smallest p >= i with lcp[p] <= t; otherwise the largest p <= i with p >= 1 and lcp[p] <= t (lcp[0] is never
// evaluated).  kNavOff if there is none.  i < n for the left search; the right one takes any i <= n.
template <bool RIGHT> __device__ __forceinline__ uint64_t nav_search(const LceView& v, uint64_t i, uint32_t t)
{
    const int f = v.fan_log;
    const uint64_t mask = (1ull << f) - 1;
    const bool vec0 = (reinterpret_cast<uintptr_t>(v.lcp) & 15u) == 0;
    const uint32_t* L = v.lcp;
    uint64_t cnt = v.n, j;
    bool vec = vec0;
    int k = 0;
    for (;; k++) {                                                     // up: the rest of i's node on the search side
        if (RIGHT) {
            if (i >= cnt) return kNavOff;
            j = nav_first_le(L, i, dmin((i | mask) + 1, cnt), vec, t);
        } else {
            const uint64_t b = i & ~mask;
            j = nav_last_le(L, (k == 0 && b == 0) ? 1 : b, i + 1, vec, t);
        }
        if (j != kNavOff) break;
        if (k == v.levels - 1 || (!RIGHT && (i >> f) == 0)) return kNavOff;
        i = RIGHT ? (i >> f) + 1 : (i >> f) - 1;                       // the parent's neighbour
        L = k == 0 ? v.tree : L + lce_line_up(cnt);
        cnt = (cnt + mask) >> f;
        vec = true;
    }
    while (k > 0) {                                                    // down: the nearest such word of every child node
        k--;
        L = nav_level(v, k, &cnt);
        vec = k > 0 || vec0;
        const uint64_t a = j << f, e = dmin(a + mask + 1, cnt);        // (a < cnt: j is below the count of the level above)
        if (RIGHT) {
            const uint64_t p = nav_first_le(L, a, e, vec, t);
            j = p != kNavOff ? p : a;                                  // (none: lcp was changed after creation)
        } else {
            const bool first = k == 0 && a == 0;
            const uint64_t p = nav_last_le(L, first ? 1 : a, e, vec, t);
            if (p == kNavOff && first) return kNavOff;                 // the word stood for lcp[0] alone
            j = p != kNavOff ? p : e - 1;
        }
    }
    return j;
}
// bounds(r, d) for r < n: lo <= r < hi <= n for any lcp contents
__device__ __forceinline__ void nav_bounds(const LceView& v, uint32_t r, uint32_t d, uint32_t* lo, uint32_t* hi)
{
    if (d == 0) { *lo = 0; *hi = v.n; return; }
    const uint64_t l = nav_search<false>(v, r, d - 1), h = nav_search<true>(v, (uint64_t)r + 1, d - 1);
    *lo = l == kNavOff ? 0u : (uint32_t)l;
    *hi = h == kNavOff ? v.n : (uint32_t)h;
}
// the smallest index of [l, r) that attains min lcp[l .. r), 0 <= l < r <= n, lcp[0] as stored.  The search cannot leave
// [l, r) while the levels are those of lcp; if they are not, the answer is l
__device__ __forceinline__ uint32_t nav_argmin(const LceView& v, uint64_t l, uint64_t r)
{
    const uint32_t m = lce_walk<false>(v, l, r, 0);
    const uint64_t p = nav_search<true>(v, l, m);
    return p < r ? (uint32_t)p : (uint32_t)l;
}

__global__ void __launch_bounds__(kBlock)
k_nav_substr(LceView v, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ len, uint64_t nq, uint32_t* __restrict__ lo,
             uint32_t* __restrict__ hi, uint32_t* __restrict__ depth)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += stride) {
        const uint32_t p = pos[q], ln = len[q];
        uint32_t l = kLceNone, h = kLceNone, d = kLceNone;
        if (ln == 0) {
            if (p <= v.n) { l = 0; h = v.n; d = 0; }
        } else if (p < v.n) {
            const uint64_t room = lce_end_of(v, p) - p;
            if (ln <= room) {
                nav_bounds(v, v.isa[p], ln, &l, &h);
                d = h - l == 1 ? (uint32_t)room : lce_walk<false>(v, (uint64_t)l + 1, h, 0);
            }
        }
        lo[q] = l;
        hi[q] = h;
        if (depth) depth[q] = d;
    }
}
__global__ void __launch_bounds__(kBlock)
k_nav_lca(LceView v, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint64_t nq, uint32_t* __restrict__ lo,
          uint32_t* __restrict__ hi, uint32_t* __restrict__ depth)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += stride) {
        const uint32_t i = a[q], j = b[q];
        uint32_t l = kLceNone, h = kLceNone, d = kLceNone;
        if (i < v.n && j < v.n) {
            const uint32_t ri = v.isa[i], rj = i == j ? ri : v.isa[j];
            if (ri == rj) {                                             // (i != j only with a table that is not the handle's)
                l = ri;
                h = ri + 1;
                d = (uint32_t)(lce_end_of(v, i) - i);
            } else {
                const uint32_t ra = dmin(ri, rj), rb = dmax(ri, rj);
                d = lce_walk<false>(v, (uint64_t)ra + 1, (uint64_t)rb + 1, 0);
                nav_bounds(v, ra, d, &l, &h);
            }
        }
        lo[q] = l;
        hi[q] = h;
        if (depth) depth[q] = d;
    }
}
__global__ void __launch_bounds__(kBlock)
k_nav_argmin(LceView v, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi, uint64_t nq, uint32_t* __restrict__ out)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += stride) {
        const uint32_t l = lo[q], r = hi[q];
        out[q] = (l >= r || r > v.n) ? kLceNone : nav_argmin(v, l, r);
    }
}
// a node [lb, rb] (rb inclusive, as sfx_suffix_tree_dev writes it) the kernels look at: an interval of two ranks or more
__device__ __forceinline__ bool nav_node_ok(const LceView& v, uint32_t lb, uint32_t rb) { return lb < rb && rb < v.n; }
// map: n words of NONE on entry.  A table that is this lcp's gives every home to one node; with any other table a slot
// keeps one of the ids written to it, each of them below `nodes`
__global__ void __launch_bounds__(kBlock)
k_nav_home(LceView v, uint64_t nodes, const uint32_t* __restrict__ node_lb, const uint32_t* __restrict__ node_rb,
           const uint32_t* __restrict__ node_depth, uint32_t* __restrict__ map)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < nodes; k += stride) {
        const uint32_t lb = node_lb[k], rb = node_rb[k];
        if (node_depth[k] == 0 || !nav_node_ok(v, lb, rb)) continue;
        map[nav_argmin(v, (uint64_t)lb + 1, (uint64_t)rb + 1)] = (uint32_t)k;
    }
}
__global__ void __launch_bounds__(kBlock)
k_nav_slink(LceView v, const uint32_t* __restrict__ sa, uint64_t nodes, const uint32_t* __restrict__ node_lb,
            const uint32_t* __restrict__ node_rb, const uint32_t* __restrict__ node_depth, const uint32_t* __restrict__ map,
            uint32_t* __restrict__ slink)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < nodes; k += stride) {
        const uint32_t lb = node_lb[k], rb = node_rb[k], d = node_depth[k];
        uint32_t w = kLceNone;
        if (d == 1 && nav_node_ok(v, lb, rb)) {
            w = 0;
        } else if (d >= 2 && nav_node_ok(v, lb, rb)) {
            const uint64_t q = (uint64_t)sa[lb] + 1;                    // (q < n for this lcp's nodes: the suffix has d >= 2 bytes)
            if (q < v.n) {
                uint32_t l, h;
                nav_bounds(v, v.isa[q], d - 1, &l, &h);
                if (h - l >= 2) w = map[nav_argmin(v, (uint64_t)l + 1, h)];
                if (w != kLceNone && w >= nodes) w = kLceNone;
            }
        }
        slink[k] = w;
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
// what a query moves at most: its arguments and answers, one isa line, 2 levels - 1 lines per side of the search and two
// lines per level of a range minimum (DESIGN.md section 28 counts them)
static double nav_query_bytes(const sfx_lce* lx, uint64_t nq, int searches, int walks)
{
    return (double)nq * (20 + 128.0 * (1 + searches * (2 * lx->levels - 1) + walks * 2 * lx->levels));
}
int nav_substr_dev(const sfx_lce* lx, const uint32_t* d_pos, const uint32_t* d_len, uint64_t nq, uint32_t* d_lo, uint32_t* d_hi,
                   uint32_t* d_depth, hipStream_t st)
{
    if (!lx) return SFX_ERR_ARG;
    if (nq == 0) return SFX_OK;
    if (!d_pos || !d_len || !d_lo || !d_hi) return SFX_ERR_ARG;
    SFX_LAUNCH("nav_substr", nav_query_bytes(lx, nq, 2, 1), k_nav_substr, lce_grid(nq), kBlock, st, lce_view(lx), d_pos, d_len, nq, d_lo, d_hi,
               d_depth);
    return SFX_OK;
}
int nav_lca_dev(const sfx_lce* lx, const uint32_t* d_a, const uint32_t* d_b, uint64_t nq, uint32_t* d_lo, uint32_t* d_hi, uint32_t* d_depth,
                hipStream_t st)
{
    if (!lx) return SFX_ERR_ARG;
    if (nq == 0) return SFX_OK;
    if (!d_a || !d_b || !d_lo || !d_hi) return SFX_ERR_ARG;
    SFX_LAUNCH("nav_lca", nav_query_bytes(lx, nq, 2, 1) + (double)nq * 128, k_nav_lca, lce_grid(nq), kBlock, st, lce_view(lx), d_a, d_b, nq, d_lo,
               d_hi, d_depth);
    return SFX_OK;
}
int nav_argmin_dev(const sfx_lce* lx, const uint32_t* d_lo, const uint32_t* d_hi, uint64_t nq, uint32_t* d_arg, hipStream_t st)
{
    if (!lx) return SFX_ERR_ARG;
    if (nq == 0) return SFX_OK;
    if (!d_lo || !d_hi || !d_arg) return SFX_ERR_ARG;
    SFX_LAUNCH("nav_argmin", nav_query_bytes(lx, nq, 1, 1), k_nav_argmin, lce_grid(nq), kBlock, st, lce_view(lx), d_lo, d_hi, nq, d_arg);
    return SFX_OK;
}
// [map n u32]: boundary -> dense id of the node whose home it is
uint64_t suffix_links_workspace_bytes(uint64_t n)
{
    if (n == 0 || n > 0xFFFFFFFFull) return 0;
    ArenaSizer z;
    z.take<uint32_t>(n);
    return z.used;
}
int suffix_links_dev(const sfx_lce* lx, const uint32_t* d_sa, uint64_t nodes, const uint32_t* d_node_lb, const uint32_t* d_node_rb,
                     const uint32_t* d_node_depth, uint32_t* d_slink, void* ws, uint64_t ws_bytes, hipStream_t st)
{
    if (!lx || lx->starts) return SFX_ERR_ARG;                           // (a collection's nodes have several terminals: no node table)
    if (nodes == 0 || lx->n == 0) return SFX_OK;
    if (nodes > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;                 // (ids are 32 bits wide)
    if (!d_sa || !d_node_lb || !d_node_rb || !d_node_depth || !d_slink) return SFX_ERR_ARG;
    if (!ws || ws_bytes < suffix_links_workspace_bytes(lx->n)) return SFX_ERR_WORKSPACE;
    Arena a(ws, ws_bytes);
    uint32_t* map = a.take<uint32_t>(lx->n);
    if (a.overflow) return SFX_ERR_INTERNAL;
    SFX_HIP(hipMemsetAsync(map, 0xFF, lx->n * sizeof(uint32_t), st));
    SFX_LAUNCH("nav_home", nav_query_bytes(lx, nodes, 1, 1), k_nav_home, lce_grid(nodes), kBlock, st, lce_view(lx), nodes, d_node_lb, d_node_rb,
               d_node_depth, map);
    SFX_LAUNCH("nav_slink", nav_query_bytes(lx, nodes, 3, 1) + (double)nodes * 256, k_nav_slink, lce_grid(nodes), kBlock, st, lce_view(lx), d_sa,
               nodes, d_node_lb, d_node_rb, d_node_depth, (const uint32_t*)map, d_slink);
    return SFX_OK;
}

}  // namespace sfx
