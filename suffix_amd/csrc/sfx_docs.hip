// sfx_docs.hip -- how many distinct documents lie under every lcp-interval of a collection, and the longest strings common
// to at least d documents (include/suffix_hip.h).
//
// PREV[r] = the previous rank of r's document.  The suffixes at PREV[r] and r are the same document seen twice inside every
// interval that holds both, and the deepest such interval is the one of p(r) = the RIGHTMOST boundary of (PREV[r], r] with
// the minimum of lcp over that range.  dup[x] = #{r : p(r) <= x}; for an interval [lb, rb] whose inner boundaries are all
// deeper than its two outer ones, a pair (PREV[r], r) lies inside exactly when lb < p(r) <= rb, so
//   df = (rb - lb + 1) - (dup[rb] - dup[lb])
// is the number of distinct documents among da[lb .. rb] -- one subtraction per node, or per pattern interval.
//
//   docs_check    any da[r] >= ndocs
//   (gsa_prev)    PREV by the stable key sort of da (sfx_tree.hip's builder)
//   (lce_levels)  the 32-ary min-tree over lcp (sfx_lce.hip's levels, in the workspace)
//   docs_argmin   p(r) per rank: up the tree from level 0 over at most two lines per level, remembering where the rightmost
//                 minimum was seen, then down from there through one line per level; PREV[r] == r - 1 reads nothing
//   (radix sort)  the p(r) sorted: equal targets become runs
//   docs_runs     count[v] = length of v's run, from the run's two ends -- at most two adds per address, whatever the input
//   (gsa_scan)    inclusive prefix sum = dup
//   docs_counts   dup_prefix out; df[p] from lb[p] / rb[p] of the interval search (tree_pyramid, tree_intervals)
// The accumulation is a sort, not atomics on the p(r): on many short documents nearly every p(r) is one of a few hundred
// shallow boundaries, and one add per rank onto those words is the queue DESIGN.md section 10 (round 6, lesson b) measured.
// No address depends on a value read from lcp: values are only compared, every index is bounded by n and the level sizes.
//
//   docs_longest     the longest document, (length << 32 | ~document) by one maximum per wave
//   docs_best        per df value the maximum of (lcp[p] << 32 | ~p): 1024 boundaries per wave, every lane keeps the best
//                    of its current df, a wave whose lanes agree reduces first, and nothing that does not beat the slot's
//                    present value touches it
//   docs_suffix_max  one workgroup: the suffix maximum over d, decoded into len / pos
//
// Compiled as part of sfx_api.hip (which includes this file after sfx_lce.hip, whose levels it uses).
#pragma once
#include "sfx_host.hpp"
#include "sfx_lce.hip"

namespace sfx {

constexpr uint32_t kDocsNone = 0xFFFFFFFFu;
constexpr unsigned kDocsFlagWords = 64;                 // [0] a da entry >= ndocs / a bad doc start
constexpr unsigned kDocsBestPerLane = 16;               // docs_best: boundaries per lane and wave segment

// the min-tree of sfx_lce.hip in a workspace: level 0 = lcp (borrowed), level k >= 1 at tree + docs_level_off(k)
struct DocsTree {
    const uint32_t* lcp;
    const uint32_t* tree;
    uint32_t n;
    int f, levels;
};
// entries of level k: ceil(n / F^k)
__device__ __forceinline__ uint64_t docs_level_cnt(const DocsTree& t, int k)
{
    const int s = t.f * k;
    return ((uint64_t)t.n + (1ull << s) - 1) >> s;
}
// words in front of level k >= 1 (lce_layout's order: every level padded to whole lines)
__device__ __forceinline__ uint64_t docs_level_off(const DocsTree& t, int k)
{
    uint64_t off = 0;
    for (int j = 1; j < k; j++) off += lce_line_up(docs_level_cnt(t, j));
    return off;
}
// the RIGHTMOST minimum of L[a .. b), a < b, b - a <= 32; only words of [a, b) are read.  vec: L is 16-byte aligned
__device__ __forceinline__ void docs_span_argmin(const uint32_t* __restrict__ L, uint64_t a, uint64_t b, bool vec, uint32_t* val, uint64_t* at)
{
    uint32_t m = kDocsNone;
    uint64_t w = a, i = a;
    auto take = [&](uint32_t x, uint64_t j) { if (x <= m) { m = x; w = j; } };
    if (vec) {
        for (; i < b && (i & 3); i++) take(L[i], i);
        for (; i + 4 <= b; i += 4) {
            const uint4 v = *reinterpret_cast<const uint4*>(L + i);
            take(v.x, i);
            take(v.y, i + 1);
            take(v.z, i + 2);
            take(v.w, i + 3);
        }
    }
    for (; i < b; i++) take(L[i], i);
    *val = m;
    *at = w;
}
// the rightmost p in [l, r) with lcp[p] = min lcp[l .. r), for 1 <= l < r <= n.  The way up is lce_walk's: at every level
// the words from l to the end of l's node and from the start of r's node to r, then the nodes strictly between one level
// up.  In text order the spans are: the left ones (higher levels further right), the last span, the right ones (higher
// levels further left) -- so a right span replaces the candidate only with a smaller value, a left span also with an equal
// one.  The way down takes the rightmost minimum of the candidate's node at every level below.
__device__ __forceinline__ uint64_t docs_argmin_right(const DocsTree& t, uint64_t l, uint64_t r)
{
    const int f = t.f;
    const uint64_t mask = (1ull << f) - 1;
    const bool vec0 = (reinterpret_cast<uintptr_t>(t.lcp) & 15u) == 0;
    const uint32_t* L = t.lcp;
    bool vec = vec0;
    uint64_t cnt = t.n, off = 0;
    uint32_t vl = 0, vm = 0, vr = 0, v;
    uint64_t il = 0, im = 0, ir = 0, i;
    int kl = -1, km = -1, kr = -1;
    for (int k = 0;; k++) {
        if (((l ^ (r - 1)) >> f) == 0 || k == t.levels - 1) {
            docs_span_argmin(L, l, r, vec, &vm, &im);
            km = k;
            break;
        }
        if (l & mask) {
            const uint64_t e = (l | mask) + 1;
            docs_span_argmin(L, l, e, vec, &v, &i);
            if (kl < 0 || v <= vl) { vl = v; il = i; kl = k; }
            l = e;
        }
        if (r & mask) {
            const uint64_t b = r & ~mask;
            docs_span_argmin(L, b, r, vec, &v, &i);
            if (kr < 0 || v < vr) { vr = v; ir = i; kr = k; }
            r = b;
        }
        if (l >= r) break;
        l >>= f;
        r >>= f;
        off = k == 0 ? 0 : off + lce_line_up(cnt);
        cnt = (cnt + mask) >> f;
        L = t.tree + off;
        vec = true;
    }
    uint32_t m = kDocsNone;
    if (kr >= 0) m = dmin(m, vr);
    if (km >= 0) m = dmin(m, vm);
    if (kl >= 0) m = dmin(m, vl);
    int k;
    if (kr >= 0 && vr == m) { k = kr; i = ir; }
    else if (km >= 0 && vm == m) { k = km; i = im; }
    else { k = kl; i = il; }
    while (k > 0) {                                                   // node i of level k: its words on level k - 1
        k--;
        const uint64_t cb = i << f, ce = dmin(cb + mask + 1, docs_level_cnt(t, k));
        docs_span_argmin(k == 0 ? t.lcp : t.tree + docs_level_off(t, k), cb, ce, k == 0 ? vec0 : true, &v, &i);
    }
    return i;
}

// ---- document counts ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_docs_check(const uint32_t* __restrict__ da, uint64_t n, uint64_t ndocs, uint32_t* __restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    bool bad = false;
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) bad |= da[r] >= ndocs;
    if (bad) flags[0] = 1u;
}
// key[r] = p(r), or n for a rank without an earlier one of its document
__global__ void __launch_bounds__(kBlock)
k_docs_argmin(DocsTree t, const uint32_t* __restrict__ prev, uint64_t* __restrict__ key)
{
    const uint64_t n = t.n, stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) {
        const uint64_t q = prev[r];
        uint64_t p = n;
        if (q < r) {                                                  // (kGsaNone is not below r)
            p = q + 1 == r ? r : docs_argmin_right(t, q + 1, r + 1);
            if (p <= q || p > r) p = r;                               // (cannot happen: the tree is this call's own)
        }
        key[r] = p;
    }
}
// sorted keys -> count[v] = how many keys equal v < n: the last of a run adds its place + 1, the first takes its place
// off again (mod 2^32, in either order); count is cleared by the caller
__global__ void __launch_bounds__(kBlock)
k_docs_runs(const uint64_t* __restrict__ key, uint64_t n, uint32_t* __restrict__ count)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const uint64_t v = key[i];
        if (v >= n) continue;
        const bool first = i == 0 || key[i - 1] != v, last = i + 1 == n || key[i + 1] != v;
        if (first && last) count[v] = 1u;
        else if (last) atomicAdd(&count[v], (uint32_t)(i + 1));
        else if (first) atomicSub(&count[v], (uint32_t)i);
    }
}
// inc[x] = dup[x] (the scan's output, shifted by one).  df of boundary p from its interval [lb[p], rb[p]]
__global__ void __launch_bounds__(kBlock)
k_docs_counts(const uint32_t* __restrict__ inc, uint64_t n, const uint32_t* __restrict__ lb, const uint32_t* __restrict__ rb,
              uint32_t* __restrict__ dup, uint32_t* __restrict__ df)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += stride) {
        if (dup) dup[p] = inc[p];
        if (df) {
            const uint64_t b = dmin<uint64_t>(rb[p], n - 1), a = dmin<uint64_t>(lb[p], b);
            df[p] = (uint32_t)(b - a + 1) - (inc[b] - inc[a]);
        }
    }
}

// ---- k-common substrings ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void docs_raise(unsigned long long* __restrict__ slot, unsigned long long v)
{
    if (v > *slot) atomicMax(slot, v);                                // (a stale read only costs an atomic: slots never fall)
}
__device__ __forceinline__ unsigned long long docs_wave_max(unsigned long long v)
{
    for (int d = 32; d >= 1; d >>= 1) v = dmax(v, (unsigned long long)__shfl_xor(v, d));
    return v;
}
// best[0] = max (length << 32 | ~d) over the documents; doc_starts checked as k_gsa_check_docs does
__global__ void __launch_bounds__(kBlock)
k_docs_longest(const uint64_t* __restrict__ starts, uint64_t ndocs, uint64_t n, unsigned long long* __restrict__ best,
               uint32_t* __restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t t0 = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned long long m = 0;
    bool bad = false;
    for (uint64_t base = t0 - threadIdx.x % kWave; base < ndocs; base += stride) {    // (the same trip count for a wave's lanes)
        const uint64_t d = base + threadIdx.x % kWave;
        if (d >= ndocs) continue;
        const uint64_t s = starts[d], e = d + 1 < ndocs ? starts[d + 1] : n;
        if (s > n || e > n || e < s || (d == 0 && s != 0)) { bad = true; continue; }
        m = dmax(m, (unsigned long long)((e - s) << 32 | (uint32_t)~(uint32_t)d));
    }
    if (bad) flags[0] = 1u;
    m = docs_wave_max(m);
    if (lane_id() == 0 && m) docs_raise(&best[0], m);
}
// best[d] = max (lcp[p] << 32 | ~p) over the boundaries p >= 1 with df[p] == d in 1 .. ndocs and lcp[p] > 0
__global__ void __launch_bounds__(kBlock)
k_docs_best(const uint32_t* __restrict__ lcp, const uint32_t* __restrict__ df, uint64_t n, uint64_t ndocs,
            unsigned long long* __restrict__ best)
{
    const uint64_t seg_len = (uint64_t)kWave * kDocsBestPerLane;
    const uint64_t nseg = (n + seg_len - 1) / seg_len;
    const uint64_t waves = (uint64_t)gridDim.x * kWavesPerBlock;
    const unsigned lane = lane_id();
    for (uint64_t seg = (uint64_t)blockIdx.x * kWavesPerBlock + wave_id(); seg < nseg; seg += waves) {
        uint32_t cur_d = 0;
        unsigned long long cur = 0;
        for (unsigned i = 0; i < kDocsBestPerLane; i++) {
            const uint64_t p = seg * seg_len + (uint64_t)i * kWave + lane;
            if (p >= n) break;
            if (p == 0) continue;
            const uint32_t v = lcp[p], d = df[p];
            if (v == 0 || d == 0 || d > ndocs) continue;
            const unsigned long long pk = (unsigned long long)v << 32 | (uint32_t)~(uint32_t)p;
            if (d != cur_d) {
                if (cur_d) docs_raise(&best[cur_d], cur);
                cur_d = d;
                cur = pk;
            } else {
                cur = dmax(cur, pk);
            }
        }
        const unsigned long long have = __ballot(cur_d != 0);
        if (!have) continue;
        const int leader = __ffsll((long long)have) - 1;
        const uint32_t d0 = (uint32_t)__shfl((int)cur_d, leader);
        if (__all(cur_d == 0 || cur_d == d0)) {
            const unsigned long long m = docs_wave_max(cur);
            if ((int)lane == leader) docs_raise(&best[d0], m);
        } else if (cur_d) {
            docs_raise(&best[cur_d], cur);
        }
    }
}
// one workgroup: len[d - 1] / pos[d - 1] from max best[d ..]; d == 1 also takes the whole documents (best[0])
__global__ void __launch_bounds__(kBlock)
k_docs_suffix_max(const unsigned long long* __restrict__ best, uint64_t ndocs, const uint32_t* __restrict__ sa,
                  const uint64_t* __restrict__ starts, uint32_t* __restrict__ len, uint32_t* __restrict__ pos)
{
    __shared__ unsigned long long sh[kBlock];
    const uint64_t chunk = (ndocs + kBlock - 1) / kBlock;
    const uint64_t b = 1 + threadIdx.x * chunk, e = dmin(b + chunk, ndocs + 1);
    unsigned long long m = 0;
    for (uint64_t d = b; d < e; d++) m = dmax(m, best[d]);
    sh[threadIdx.x] = m;
    __syncthreads();
    unsigned long long carry = 0;
    for (unsigned t = threadIdx.x + 1; t < (unsigned)kBlock; t++) carry = dmax(carry, sh[t]);
    for (uint64_t d = e; d > b;) {
        d--;
        carry = dmax(carry, best[d]);
        uint32_t l = (uint32_t)(carry >> 32);
        uint32_t at = l ? sa[(uint32_t)~(uint32_t)carry] : kDocsNone;
        if (d == 1) {                                                 // (a document is at least as long as any lcp of the collection)
            const unsigned long long doc = best[0];
            if ((uint32_t)(doc >> 32) > l) {
                l = (uint32_t)(doc >> 32);
                at = (uint32_t)starts[(uint32_t)~(uint32_t)doc];
            }
        }
        len[d - 1] = l;
        pos[d - 1] = at;
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// [flags | prev n u32 | K0 n u64 | V0 n u32 | K1 n u64 | V1 n u32 | radix scratch | count n + 1 u32 | scan partials | the levels
//  above lcp | the interval search's workspace]; lb and rb of the interval search lie in K0, node in K1 (the sorts are over)
struct DocsWs {
    uint32_t *flags, *prev, *V0, *V1, *scratch, *count, *part, *tree;
    uint64_t *K0, *K1;
    uint8_t* iv;
    uint64_t iv_bytes;
};
template <class A> static void docs_carve(A& a, uint64_t n, int fan_log, DocsWs* w)
{
    w->flags = a.template take<uint32_t>(kDocsFlagWords);
    w->prev = a.template take<uint32_t>(n);
    w->K0 = a.template take<uint64_t>(n);
    w->V0 = a.template take<uint32_t>(n);
    w->K1 = a.template take<uint64_t>(n);
    w->V1 = a.template take<uint32_t>(n);
    w->scratch = a.template take<uint32_t>(radix_scratch_words(n));
    w->count = a.template take<uint32_t>(n + 1);
    w->part = a.template take<uint32_t>(kMaxGrid + 64);
    w->tree = a.template take<uint32_t>(lce_layout(n, fan_log).tree_words);
    w->iv_bytes = lcp_intervals_workspace_bytes(n);
    w->iv = a.template take<uint8_t>(w->iv_bytes);
}
uint64_t doc_counts_workspace_bytes(uint64_t n)
{
    if (n == 0 || n > 0xFFFFFFFFull) return 0;
    LceSizer z;
    DocsWs w;
    docs_carve(z, n, lce_fan_log(), &w);
    return z.used;
}
int doc_counts_dev(const uint32_t* d_da, const uint32_t* d_lcp, uint64_t n, uint64_t ndocs, uint32_t* d_dup, uint32_t* d_df, void* ws,
                   uint64_t ws_bytes, hipStream_t st)
{
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (ndocs == 0 || !d_da || !d_lcp) return SFX_ERR_ARG;
    if (!ws || ws_bytes < doc_counts_workspace_bytes(n)) return SFX_ERR_WORKSPACE;
    const int f = lce_fan_log();
    Arena a(ws, ws_bytes);
    DocsWs w;
    docs_carve(a, n, f, &w);
    if (a.overflow) return SFX_ERR_INTERNAL;
    const unsigned grid = lce_grid(n);
    SFX_HIP(hipMemsetAsync(w.flags, 0, kDocsFlagWords * sizeof(uint32_t), st));
    SFX_LAUNCH("docs_check", (double)n * 4, k_docs_check, grid, kBlock, st, d_da, n, ndocs, w.flags);
    // (da is u32: more than 2^32 documents sort like 2^32)
    SFX_TRY(gsa_prev_dev(d_da, n, dmin<uint64_t>(ndocs, 1ull << 32), w.prev, w.K0, w.V0, w.K1, w.V1, w.scratch, st));
    const LceLayout L = lce_layout(n, f);
    {
        const uint32_t* in = d_lcp;
        uint32_t* out = w.tree;
        uint64_t cnt = n;
        for (int k = 1; k < L.levels; k++) {
            const uint64_t cnt_out = (cnt + (1ull << f) - 1) >> f;
            SFX_LAUNCH("lce_levels", (double)cnt * 4 + (double)cnt_out * 4, k_lce_levels, lce_grid(cnt), kBlock, st, in, cnt, out, f);
            in = out;
            out += lce_line_up(cnt_out);
            cnt = cnt_out;
        }
    }
    const DocsTree t{d_lcp, w.tree, (uint32_t)n, f, L.levels};
    // a PREV line, and about two tree lines per level on the way up, one on the way down, for the ranks that walk
    SFX_LAUNCH("docs_argmin", (double)n * (12 + 3.0 * 128 * L.levels), k_docs_argmin, grid, kBlock, st, t, (const uint32_t*)w.prev, w.K0);
    int in1 = 0;
    SFX_TRY(radix_sort_kv64(w.K0, w.V0, w.K1, w.V1, n, 0, bits_for(n), w.scratch, st, &in1, nullptr, nullptr));
    SFX_HIP(hipMemsetAsync(w.count, 0, (n + 1) * sizeof(uint32_t), st));
    SFX_LAUNCH("docs_runs", (double)n * 12, k_docs_runs, grid, kBlock, st, (const uint64_t*)(in1 ? w.K1 : w.K0), n, w.count);
    SFX_TRY(scan_u32_excl_dev(w.count, n, w.count, w.part, st));      // count[x + 1] = dup[x]
    uint32_t *lb = nullptr, *rb = nullptr;
    if (d_df) {
        lb = reinterpret_cast<uint32_t*>(w.K0);
        rb = lb + n;
        SFX_TRY(lcp_interval_bounds_dev(d_lcp, n, lb, rb, reinterpret_cast<uint32_t*>(w.K1), w.iv, w.iv_bytes, st));
    }
    if (d_dup || d_df)
        SFX_LAUNCH("docs_counts", (double)n * (d_df ? 16 + 2 * 128 : 8), k_docs_counts, grid, kBlock, st, (const uint32_t*)(w.count + 1), n,
                   (const uint32_t*)lb, (const uint32_t*)rb, d_dup, d_df);
    uint32_t flag = 0;
    SFX_TRY(read_back(&flag, w.flags, sizeof(flag), st));             // the one synchronisation of the call
    return flag ? SFX_ERR_ARG : SFX_OK;
}

// [flags | best ndocs + 1 u64]
uint64_t common_substrings_workspace_bytes(uint64_t ndocs)
{
    if (ndocs == 0 || ndocs > 0xFFFFFFFFull) return 0;
    ArenaSizer z;
    z.take<uint32_t>(kDocsFlagWords);
    z.take<uint64_t>(ndocs + 1);
    return z.used;
}
int common_substrings_dev(const uint32_t* d_sa, const uint32_t* d_lcp, const uint32_t* d_df, uint64_t n, const uint64_t* d_starts,
                          uint64_t ndocs, uint32_t* d_len, uint32_t* d_pos, void* ws, uint64_t ws_bytes, hipStream_t st)
{
    if (n > 0xFFFFFFFFull || ndocs > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (ndocs == 0) return n ? SFX_ERR_ARG : SFX_OK;
    if (!d_starts || !d_len || !d_pos || (n && (!d_sa || !d_lcp || !d_df))) return SFX_ERR_ARG;
    if (!ws || ws_bytes < common_substrings_workspace_bytes(ndocs)) return SFX_ERR_WORKSPACE;
    Arena a(ws, ws_bytes);
    uint32_t* flags = a.take<uint32_t>(kDocsFlagWords);
    unsigned long long* best = reinterpret_cast<unsigned long long*>(a.take<uint64_t>(ndocs + 1));
    if (a.overflow) return SFX_ERR_INTERNAL;
    SFX_HIP(hipMemsetAsync(flags, 0, kDocsFlagWords * sizeof(uint32_t), st));
    SFX_HIP(hipMemsetAsync(best, 0, (ndocs + 1) * sizeof(uint64_t), st));
    SFX_LAUNCH("docs_longest", (double)ndocs * 8, k_docs_longest, lce_grid(ndocs), kBlock, st, d_starts, ndocs, n, best, flags);
    if (n) {
        const uint64_t per_block = (uint64_t)kWave * kDocsBestPerLane * kWavesPerBlock;
        const unsigned grid = (unsigned)dmax<uint64_t>(1, dmin<uint64_t>((n + per_block - 1) / per_block, dmin<unsigned>(kMaxGrid, grid_cap())));
        SFX_LAUNCH("docs_best", (double)n * 8, k_docs_best, grid, kBlock, st, d_lcp, d_df, n, ndocs, best);
    }
    uint32_t flag = 0;
    SFX_TRY(read_back(&flag, flags, sizeof(flag), st));               // the one synchronisation: doc_starts before anything indexes by it
    if (flag) return SFX_ERR_ARG;
    SFX_LAUNCH("docs_suffix_max", (double)ndocs * 16, k_docs_suffix_max, 1, kBlock, st, (const unsigned long long*)best, ndocs, d_sa, d_starts,
               d_len, d_pos);
    return SFX_OK;
}

}  // namespace sfx
