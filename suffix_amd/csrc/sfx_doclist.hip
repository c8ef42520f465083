// sfx_doclist.hip -- which documents lie in a rank interval of a collection and how often each of them occurs there, in document
// order or ranked by term frequency, with a top-k cut (include/suffix_hip.h).
//
// The index: one stable sort of (da, rank) gives PREV[r] = the previous rank of r's document and R = the ranks ordered by
// (document, rank).  Every text position contributes exactly one suffix, so document d's ranks are R[doc_starts[d] ..
// doc_end(d)): no offset array.  Creation verifies exactly that: slot k of the sorted keys names the document that owns
// text position k.
//   tf_j(d) = lower_bound(R_d, e_j) - lower_bound(R_d, s_j), both bisections inside d's slice of R.
//
// A batch of intervals becomes one line of work items: interval j has e - s of them (route A, by occurrence: item i is
// rank s + i, which counts iff PREV[r] is none or < s) or ndocs of them (route B, by document, for e - s > occ_cut: item i
// is document i, which counts iff it has a rank in [s, e)).  Tiles of 2048 items are expanded through LDS (mem_expand of
// sfx_mem.hip); every workgroup owns a contiguous run of tiles.
//   doclist_work     the items per interval; s > e or e > n raises the flag
//   (gsa_scan)       their offsets
//   doclist_count    per workgroup the items that count: one word per workgroup, never one per interval
//   doclist_offsets  one workgroup: the scan of those words, Z_full
//   doclist_emit     the same walk again with the running offset: (j << docbits | d, tf) per counting item, in item order
//                    -- ascending by j; nothing when Z_full exceeds the limit
//   doclist_first    where list j starts among the entries: a bisection per interval
//   doclist_cut      min(|D_j|, top_k) per interval;  (gsa_scan) = first;  doclist_publish: first out, Z
//   --- the one read-back: (Z_full, Z, flags).  What follows is queued behind it and sized by Z_full ---
//   doclist_keys     BY_TF: the sort key (j, n - tf, d) -- in one word when the three fields fit 64 bits, else in two stable sorts
//   (radix_sort_kv64)
//   doclist_write    entry i of list j goes to first[j] + its place in the list, if below top_k and capacity
// An index whose occ_cut is at least n has no interval for route B: its calls launch doclist_count / doclist_emit, instances
// without the by-document code.  Every other index launches doclist_count_docs / doclist_emit_docs, which take either route
// item by item -- so the profile shows which routes a call could take.
//
// Compiled as part of sfx_api.hip (which includes this file after sfx_docs.hip).
#pragma once
#include "sfx_host.hpp"
#include "sfx_mem.hip"
#include "sfx_docs.hip"

struct sfx_doclist {
    uint64_t n = 0, ndocs = 0, occ_cut = 0, bytes = 0;
    void* mem = nullptr;                    // [PREV n u32 | R n u32], each on a 256-byte boundary (nullptr: n == 0)
    void* own_da = nullptr;                 // the host route's copies (nullptr: borrowed)
    void* own_starts = nullptr;
    const uint32_t* da = nullptr;
    const uint64_t* starts = nullptr;
    const uint32_t* prev = nullptr;
    const uint32_t* R = nullptr;
};

namespace sfx {

constexpr uint32_t kDlTile = kMemTile;                   // items per tile
constexpr uint32_t kDlGroup = kBlock * 4;                // a thread takes 4 consecutive items: one 16-byte load of PREV
constexpr unsigned kDlResWords = 64;                     // [0,1] Z_full  [2,3] Z  [4] a bad interval / a bad index
constexpr unsigned kDlResZfull = 0, kDlResZ = 2, kDlResBad = 4;
constexpr uint64_t kDlMaxEntries = 0xFFFFFFFFull;        // what one sort takes
static_assert(kDlTile % kDlGroup == 0, "whole groups per tile");

// test hook, read at every listing call: SFX_DOCLIST_SPLIT=1 takes the two-sort form of the BY_TF key whatever the widths
static bool dl_split_hook()
{
    const char* e = dev_env("SFX_DOCLIST_SPLIT");
    return e && atoi(e) != 0;
}

// what the kernels need of the handle, by value
struct DlView {
    const uint32_t* da;
    const uint32_t* prev;
    const uint32_t* R;
    const uint64_t* starts;
    uint64_t n, ndocs, occ_cut;
};
struct DlIn {
    DlView v;
    const uint32_t* start;
    const uint32_t* end;
    uint64_t nq;
    const uint64_t* off;                                 // nq + 1: the first item of every interval
    uint64_t limit;                                      // entries the call may write to its key / value arrays
    int docbits;
};

__device__ __forceinline__ uint64_t dl_doc_end(const uint64_t* __restrict__ starts, uint64_t ndocs, uint64_t n, uint64_t d)
{
    return d + 1 < ndocs ? starts[d + 1] : n;
}

// ---- creation --------------------------------------------------------------------------------------------------------------
// slot k of the sorted (da, rank) pairs: its document exists and owns text position k; R[k] = the rank.  doc_starts as
// k_gsa_check_docs wants them.  Nothing is indexed by a value that was not compared first.
__global__ void __launch_bounds__(kBlock)
k_dl_check(const uint64_t* __restrict__ K, const uint32_t* __restrict__ V, uint64_t n, const uint64_t* __restrict__ starts, uint64_t ndocs,
           uint32_t* __restrict__ R, uint32_t* __restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t t0 = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    bool bad = false;
    for (uint64_t d = t0; d < ndocs; d += stride) {
        const uint64_t v = starts[d];
        bad |= v > n || (d == 0 ? v != 0 : v < starts[d - 1]);
    }
    for (uint64_t k = t0; k < n; k += stride) {
        const uint64_t d = K[k];
        const uint32_t r = V[k];
        if (d >= ndocs) bad = true;
        else bad |= starts[d] > k || dl_doc_end(starts, ndocs, n, d) <= k;
        R[k] = r;
    }
    if (bad) flags[0] = 1u;
}

// ---- the items -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool dl_by_doc(const DlView& v, uint32_t s, uint32_t e) { return (uint64_t)(e - s) > v.occ_cut; }
// the first slot of R[lo .. hi) that holds a rank >= x
__device__ __forceinline__ uint64_t dl_lower(const uint32_t* __restrict__ R, uint64_t lo, uint64_t hi, uint32_t x)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (R[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint32_t dl_tf(const DlView& v, uint64_t d, uint32_t s, uint32_t e)
{
    const uint64_t lo = v.starts[d], hi = dl_doc_end(v.starts, v.ndocs, v.n, d);
    const uint64_t a = dl_lower(v.R, lo, hi, s);
    return (uint32_t)(dl_lower(v.R, a, hi, e) - a);
}
__device__ __forceinline__ bool dl_doc_present(const DlView& v, uint64_t d, uint32_t s, uint32_t e)
{
    const uint64_t lo = v.starts[d], hi = dl_doc_end(v.starts, v.ndocs, v.n, d);
    const uint64_t a = dl_lower(v.R, lo, hi, s);
    return a < hi && v.R[a] < e;
}
__global__ void __launch_bounds__(kBlock)
k_dl_work(DlView v, const uint32_t* __restrict__ start, const uint32_t* __restrict__ end, uint64_t nq, uint32_t* __restrict__ w,
          uint32_t* __restrict__ res)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    bool bad = false;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < nq; j += stride) {
        const uint32_t s = start[j], e = end[j];
        uint32_t items = 0;
        if (s > e || e > v.n) bad = true;
        else items = dl_by_doc(v, s, e) ? (uint32_t)v.ndocs : e - s;
        w[j] = items;
    }
    if (bad) res[kDlResBad] = 1u;
}
// bit x: item base + x of the tile counts.  DOCS: the index has intervals for route B (else every item is a rank).
// pos[] = the interval of every item of the tile (mem_expand), cnt = the items the tile has, k0 = its first item.
template <bool DOCS> __device__ __forceinline__ uint32_t dl_keep4(const DlIn& in, const uint32_t* __restrict__ pos, uint32_t base,
                                                                     uint32_t cnt, uint64_t k0)
{
    if (base >= cnt) return 0u;
    const uint32_t m = dmin(4u, cnt - base);
    if (m == 4 && pos[base + 3] == pos[base]) {                       // four ranks of one interval: one load where they align
        const uint32_t j = pos[base], s = in.start[j], e = in.end[j];
        const uint64_t r0 = s + (k0 + base - in.off[j]);
        if ((r0 & 3u) == 0 && !(DOCS && dl_by_doc(in.v, s, e))) {                                         // (PREV starts on a 256-byte boundary)
            const uint4 p = *reinterpret_cast<const uint4*>(in.v.prev + r0);
            return (p.x == kDocsNone || p.x < s ? 1u : 0u) | (p.y == kDocsNone || p.y < s ? 2u : 0u) |
                   (p.z == kDocsNone || p.z < s ? 4u : 0u) | (p.w == kDocsNone || p.w < s ? 8u : 0u);
        }
    }
    uint32_t bits = 0;
    for (uint32_t x = 0; x < m; x++) {
        const uint32_t j = pos[base + x], s = in.start[j], e = in.end[j];
        const uint64_t i = k0 + base + x - in.off[j];
        bool keep;
        if (DOCS && dl_by_doc(in.v, s, e)) {
            keep = dl_doc_present(in.v, i, s, e);
        } else {
            const uint32_t p = in.v.prev[s + i];
            keep = p == kDocsNone || p < s;
        }
        bits |= keep ? 1u << x : 0u;
    }
    return bits;
}
// the tiles of workgroup b: [*t0, *t1) of ceil(W / kDlTile)
__device__ __forceinline__ void dl_chunk(uint64_t W, uint64_t* t0, uint64_t* t1)
{
    const uint64_t nt = (W + kDlTile - 1) / kDlTile, chunk = (nt + gridDim.x - 1) / gridDim.x;
    *t0 = dmin(nt, (uint64_t)blockIdx.x * chunk);
    *t1 = dmin(nt, *t0 + chunk);
}
__device__ __forceinline__ MemIn dl_expander(const DlIn& in)
{
    MemIn e = {};
    e.m = in.nq;
    e.off = in.off;
    e.tile = kDlTile;
    return e;
}
// bcnt[b] = the counting items of workgroup b's tiles
template <bool DOCS> __global__ void __launch_bounds__(kBlock)
k_dl_count(DlIn in, unsigned long long* __restrict__ bcnt)
{
    __shared__ uint32_t pos[kDlTile];
    __shared__ uint32_t part[kWavesPerBlock];
    __shared__ unsigned long long sums[kWavesPerBlock];
    __shared__ uint64_t first;
    const uint64_t W = in.off[in.nq];
    const MemIn ex = dl_expander(in);
    uint64_t t0, t1;
    dl_chunk(W, &t0, &t1);
    unsigned long long mine = 0;
    for (uint64_t t = t0; t < t1; t++) {
        const uint32_t cnt = mem_expand(ex, W, t, pos, part, &first);
        for (uint32_t g = 0; g < kDlTile; g += kDlGroup) mine += __popc(dl_keep4<DOCS>(in, pos, g + threadIdx.x * 4, cnt, t * kDlTile));
        __syncthreads();
    }
    for (int d = 32; d >= 1; d >>= 1) mine += (unsigned long long)__shfl_xor(mine, d);
    if (lane_id() == 0) sums[wave_id()] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
        for (unsigned k = 0; k < (unsigned)kWavesPerBlock; k++) all += sums[k];
        bcnt[blockIdx.x] = all;
    }
}
// one workgroup: boff = the exclusive scan of bcnt, Z_full
__global__ void __launch_bounds__(kBlock)
k_dl_offsets(const unsigned long long* __restrict__ bcnt, unsigned nwords, unsigned long long* __restrict__ boff, uint32_t* __restrict__ res)
{
    __shared__ unsigned long long sh[kWavesPerBlock];
    unsigned long long carry = 0;
    for (unsigned base = 0; base < nwords; base += kBlock) {
        const unsigned i = base + threadIdx.x;
        unsigned long long total;
        const unsigned long long ex = block_scan_add_excl<unsigned long long>(i < nwords ? bcnt[i] : 0ull, sh, total);
        if (i < nwords) boff[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        boff[nwords] = carry;
        res[kDlResZfull] = (uint32_t)carry;
        res[kDlResZfull + 1] = (uint32_t)(carry >> 32);
    }
}
// true: the call writes nothing (a bad interval, or more entries than the limit)
__device__ __forceinline__ bool dl_refused(const uint32_t* __restrict__ res, uint64_t limit)
{
    const uint64_t z = (uint64_t)res[kDlResZfull + 1] << 32 | res[kDlResZfull];
    return res[kDlResBad] != 0 || z > limit;
}
template <bool DOCS> __global__ void __launch_bounds__(kBlock)
k_dl_emit(DlIn in, const unsigned long long* __restrict__ boff, const uint32_t* __restrict__ res, uint64_t* __restrict__ K, uint32_t* __restrict__ V)
{
    __shared__ uint32_t pos[kDlTile];
    __shared__ uint32_t part[kWavesPerBlock];
    __shared__ uint64_t first;
    if (dl_refused(res, in.limit)) return;                            // (uniform)
    const uint64_t W = in.off[in.nq];
    const MemIn ex = dl_expander(in);
    uint64_t t0, t1;
    dl_chunk(W, &t0, &t1);
    uint64_t run = boff[blockIdx.x];
    for (uint64_t t = t0; t < t1; t++) {
        const uint32_t cnt = mem_expand(ex, W, t, pos, part, &first);
        for (uint32_t g = 0; g < kDlTile; g += kDlGroup) {
            const uint32_t base = g + threadIdx.x * 4;
            const uint32_t bits = dl_keep4<DOCS>(in, pos, base, cnt, t * kDlTile);
            uint32_t total;
            uint64_t o = run + block_scan_add_excl<uint32_t>(__popc(bits), part, total);
            for (uint32_t x = 0; x < 4; x++) {
                if (!(bits >> x & 1u)) continue;
                const uint32_t j = pos[base + x], s = in.start[j], e = in.end[j];
                const uint64_t i = t * kDlTile + base + x - in.off[j];
                const uint64_t d = DOCS && dl_by_doc(in.v, s, e) ? i : in.v.da[s + i];
                if (o < in.limit) {                                   // (always: the count saw the same items)
                    K[o] = (uint64_t)j << in.docbits | d;
                    V[o] = dl_tf(in.v, d, s, e);
                }
                o++;
            }
            run += total;
        }
        __syncthreads();
    }
}
// ffirst[j] = the first entry of an interval >= j among the Z_full entries (ascending by interval), j = 0 .. nq
__global__ void __launch_bounds__(kBlock)
k_dl_first(const uint64_t* __restrict__ K, int docbits, uint64_t nq, uint64_t limit, const uint32_t* __restrict__ res, uint64_t* __restrict__ ffirst)
{
    const bool off = dl_refused(res, limit);
    const uint64_t z = off ? 0 : (uint64_t)res[kDlResZfull + 1] << 32 | res[kDlResZfull];
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j <= nq; j += stride) {
        uint64_t lo = 0, hi = z;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if ((K[mid] >> docbits) < j) lo = mid + 1; else hi = mid;
        }
        ffirst[j] = lo;
    }
}
__global__ void __launch_bounds__(kBlock)
k_dl_cut(const uint64_t* __restrict__ ffirst, uint64_t nq, uint32_t top_k, uint32_t* __restrict__ c)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < nq; j += stride) {
        const uint64_t len = ffirst[j + 1] - ffirst[j];               // (<= ndocs < 2^32)
        c[j] = (uint32_t)(top_k ? dmin<uint64_t>(len, top_k) : len);
    }
}
__global__ void __launch_bounds__(kBlock)
k_dl_publish(const uint64_t* __restrict__ wfirst, uint64_t nq, uint64_t limit, uint64_t* __restrict__ first, uint32_t* __restrict__ res)
{
    if (dl_refused(res, limit)) return;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j <= nq; j += stride) {
        if (first) first[j] = wfirst[j];
        if (j == nq) {
            res[kDlResZ] = (uint32_t)wfirst[nq];
            res[kDlResZ + 1] = (uint32_t)(wfirst[nq] >> 32);
        }
    }
}
// ---- the order -------------------------------------------------------------------------------------------------------------
// BY_TF keys from (j << docbits | d, tf).  mode 0: (j, n - tf, d) in one word, tf stays the value.  mode 1: (n - tf, d) with
// j as the value, for the first of two stable sorts.  mode 2, over the result of that sort: back to (j << docbits | d, tf).
__global__ void __launch_bounds__(kBlock)
k_dl_keys(uint64_t* __restrict__ K, uint32_t* __restrict__ V, uint64_t z, int mode, int docbits, int tfbits, uint64_t n)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock, dmask = (1ull << docbits) - 1;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < z; i += stride) {
        const uint64_t k = K[i];
        const uint32_t v = V[i];
        if (mode == 0) {
            K[i] = ((k >> docbits) << tfbits | (n - v)) << docbits | (k & dmask);
        } else if (mode == 1) {
            K[i] = (n - v) << docbits | (k & dmask);
            V[i] = (uint32_t)(k >> docbits);
        } else {
            K[i] = (uint64_t)v << docbits | (k & dmask);
            V[i] = (uint32_t)(n - (k >> docbits));
        }
    }
}
// entry i of the sorted lists: list j = K >> jshift occupies [ffirst[j], ffirst[j + 1]) before and after the sort
__global__ void __launch_bounds__(kBlock)
k_dl_write(const uint64_t* __restrict__ K, const uint32_t* __restrict__ V, uint64_t z, int jshift, int docbits,
           const uint64_t* __restrict__ ffirst, const uint64_t* __restrict__ wfirst, uint32_t top_k, uint64_t capacity,
           uint32_t* __restrict__ doc, uint32_t* __restrict__ tf)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock, dmask = (1ull << docbits) - 1;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < z; i += stride) {
        const uint64_t k = K[i], j = jshift < 64 ? k >> jshift : 0, place = i - ffirst[j];   // (64: one interval, its field is empty)
        if (top_k && place >= top_k) continue;
        const uint64_t o = wfirst[j] + place;
        if (o >= capacity) continue;
        doc[o] = (uint32_t)(k & dmask);
        tf[o] = V[i];
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static uint64_t dl_line_up(uint64_t bytes) { return (bytes + kArenaAlign - 1) & ~(kArenaAlign - 1); }
uint64_t doclist_bytes(uint64_t n)
{
    if (n == 0 || n > 0xFFFFFFFFull) return 0;
    return 2 * dl_line_up(n * sizeof(uint32_t));
}
// [flags | K0 n u64 | V0 n u32 | K1 n u64 | V1 n u32 | radix scratch]
struct DlCreateWs {
    uint32_t *flags, *V0, *V1, *scratch;
    uint64_t *K0, *K1;
};
template <class A> static void dl_create_carve(A& a, uint64_t n, DlCreateWs* w)
{
    w->flags = a.template take<uint32_t>(kDocsFlagWords);
    w->K0 = a.template take<uint64_t>(n);
    w->V0 = a.template take<uint32_t>(n);
    w->K1 = a.template take<uint64_t>(n);
    w->V1 = a.template take<uint32_t>(n);
    w->scratch = a.template take<uint32_t>(radix_scratch_words(n));
}
uint64_t doclist_create_workspace_bytes(uint64_t n)
{
    if (n == 0 || n > 0xFFFFFFFFull) return 0;
    LceSizer z;
    DlCreateWs w;
    dl_create_carve(z, n, &w);
    return z.used;
}
void doclist_destroy(sfx_doclist* dx)
{
    if (!dx) return;
    if (dx->mem) (void)dev_free(dx->mem);
    if (dx->own_da) (void)dev_free(dx->own_da);
    if (dx->own_starts) (void)dev_free(dx->own_starts);
    delete dx;
}
uint64_t doclist_auto_cut(uint64_t ndocs)
{
    // route A streams 1/32 of a line per rank, route B pays about four random lines per document: the line model says
    // 32 * ndocs * 4.  Measured (profiles/doclist_times.json): the best threshold is 50 - 100 ndocs for
    // 10^4 documents of 10 KB and 21 - 43 ndocs for 390 625 documents of 256 bytes, which lose 2x at 128 ndocs; a threshold
    // above the optimum costs far more than one below it, and 32 ndocs is within 3 % of the best on both
    return dmax<uint64_t>(1, ndocs) * 32;
}
// own: d_da / d_starts were allocated for this handle, which frees them (the host route).  ws: doclist_create_workspace_bytes(n)
// bytes for the duration of the call, free again when this returns SFX_OK (the read-back is the last thing queued)
int doclist_create_dev(const uint32_t* d_da, uint64_t n, const uint64_t* d_starts, uint64_t ndocs, uint64_t occ_cut, void* ws,
                       uint64_t ws_bytes, hipStream_t st, bool own, sfx_doclist** out)
{
    if (!out) return SFX_ERR_ARG;
    *out = nullptr;
    if (n > 0xFFFFFFFFull || ndocs > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n && (!d_da || !d_starts || ndocs == 0)) return SFX_ERR_ARG;
    if (n && (!ws || ws_bytes < doclist_create_workspace_bytes(n))) return SFX_ERR_WORKSPACE;
    sfx_doclist* dx = new sfx_doclist;
    dx->n = n;
    dx->ndocs = n ? ndocs : 0;
    dx->occ_cut = occ_cut ? occ_cut : doclist_auto_cut(ndocs);
    int rc = SFX_OK;
    if (n) {
        rc = [&]() -> int {
            Arena a(ws, ws_bytes);
            DlCreateWs w;
            dl_create_carve(a, n, &w);
            if (a.overflow) return SFX_ERR_INTERNAL;
            dx->bytes = doclist_bytes(n);
            SFX_HIP(dev_malloc(&dx->mem, dx->bytes));
            uint32_t* prev = (uint32_t*)dx->mem;
            uint32_t* R = (uint32_t*)((char*)dx->mem + dx->bytes / 2);
            dx->prev = prev;
            dx->R = R;
            dx->da = d_da;
            dx->starts = d_starts;
            SFX_HIP(hipMemsetAsync(w.flags, 0, kDocsFlagWords * sizeof(uint32_t), st));
            const uint64_t* keys = nullptr;
            const uint32_t* ranks = nullptr;
            SFX_TRY(gsa_prev_sorted_dev(d_da, n, ndocs, prev, w.K0, w.V0, w.K1, w.V1, w.scratch, st, &keys, &ranks));
            SFX_LAUNCH("doclist_check", (double)n * 16 + (double)ndocs * 8, k_dl_check, lce_grid(dmax(n, ndocs)), kBlock, st, keys, ranks, n,
                       d_starts, ndocs, R, w.flags);
            uint32_t flag = 0;
            SFX_TRY(read_back(&flag, w.flags, sizeof(flag), st));     // the one synchronisation of a create
            return flag ? SFX_ERR_ARG : SFX_OK;
        }();
    }
    if (rc != SFX_OK) {
        doclist_destroy(dx);
        return rc;
    }
    if (own) {
        dx->own_da = const_cast<uint32_t*>(d_da);
        dx->own_starts = const_cast<uint64_t*>(d_starts);
    }
    *out = dx;
    return SFX_OK;
}

// [res 64 u32 | w nq u32 | off nq + 1 u64 | scan partials u64 | bcnt G u64 | boff G + 1 u64 | ffirst nq + 1 u64 | c nq u32 |
//  wfirst nq + 1 u64 | K0 L u64 | V0 L u32 | K1 L u64 | V1 L u32 | radix scratch(L)],  G = kMaxGrid, L = min(list_limit, 2^32 - 1)
struct DlWs {
    uint32_t *res, *w, *c, *V0, *V1, *scratch;
    uint64_t *off, *part, *bcnt, *boff, *ffirst, *wfirst, *K0, *K1;
};
template <class A> static void dl_carve(A& a, uint64_t nq, uint64_t L, DlWs* w)
{
    w->res = a.template take<uint32_t>(kDlResWords);
    w->w = a.template take<uint32_t>(nq);
    w->off = a.template take<uint64_t>(nq + 1);
    w->part = a.template take<uint64_t>(kMaxGrid + 64);
    w->bcnt = a.template take<uint64_t>(kMaxGrid);
    w->boff = a.template take<uint64_t>(kMaxGrid + 1);
    w->ffirst = a.template take<uint64_t>(nq + 1);
    w->c = a.template take<uint32_t>(nq);
    w->wfirst = a.template take<uint64_t>(nq + 1);
    w->K0 = a.template take<uint64_t>(L);
    w->V0 = a.template take<uint32_t>(L);
    w->K1 = a.template take<uint64_t>(L);
    w->V1 = a.template take<uint32_t>(L);
    w->scratch = a.template take<uint32_t>(radix_scratch_words(L));
}
uint64_t doclist_workspace_bytes(uint64_t nq, uint64_t list_limit)
{
    if (nq == 0 || nq > 0xFFFFFFFFull) return 0;
    LceSizer z;
    DlWs w;
    dl_carve(z, nq, dmin(list_limit, kDlMaxEntries), &w);
    return z.used;
}
int doclist_list_dev(const sfx_doclist* dx, const uint32_t* d_start, const uint32_t* d_end, uint64_t nq, uint32_t order, uint32_t top_k,
                     uint64_t list_limit, uint32_t* d_doc, uint32_t* d_tf, uint64_t capacity, uint64_t* d_first, uint64_t* listed_out,
                     uint64_t* count_out, void* ws, uint64_t ws_bytes, hipStream_t st)
{
    if (!dx || !listed_out || !count_out || order > SFX_DOCLIST_BY_TF) return SFX_ERR_ARG;
    *listed_out = *count_out = 0;
    if (nq > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (capacity && (!d_doc || !d_tf)) return SFX_ERR_ARG;
    if (nq == 0 || dx->n == 0) {
        if (d_first) SFX_HIP(hipMemsetAsync(d_first, 0, (nq + 1) * sizeof(uint64_t), st));
        return SFX_OK;
    }
    if (!d_start || !d_end) return SFX_ERR_ARG;
    if (!ws || ws_bytes < doclist_workspace_bytes(nq, list_limit)) return SFX_ERR_WORKSPACE;
    const uint64_t L = dmin(list_limit, kDlMaxEntries);
    Arena a(ws, ws_bytes);
    DlWs w;
    dl_carve(a, nq, L, &w);
    if (a.overflow) return SFX_ERR_INTERNAL;
    const unsigned cap = dmin<unsigned>(kMaxGrid, grid_cap());
    const unsigned qgrid = (unsigned)dmin<uint64_t>((nq + 1 + kBlock - 1) / kBlock, cap);
    const DlView v{dx->da, dx->prev, dx->R, dx->starts, dx->n, dx->ndocs, dx->occ_cut};
    const int docbits = bits_for(dx->ndocs - 1), jbits = bits_for(nq - 1), tfbits = bits_for(dx->n);
    SFX_HIP(hipMemsetAsync(w.res, 0, kDlResWords * sizeof(uint32_t), st));
    SFX_LAUNCH("doclist_work", (double)nq * 12, k_dl_work, qgrid, kBlock, st, v, d_start, d_end, nq, w.w, w.res);
    SFX_TRY(scan_u32_to_u64_excl_dev(w.w, nq, w.off, w.part, st));
    const DlIn in{v, d_start, d_end, nq, w.off, L, docbits};
    // (the number of items is on the device: the grid is sized by its bound, the kernels read the real one)
    // That bound is nearly always the grid cap, so doclist_offsets scans cap words even for one short interval (a few
    // microseconds); a tighter grid would need the sum of min(e - s, ...) on the host, a second read-back.  For the same
    // reason count and emit report 0 algorithmic bytes: the host does not know how many items they walk.
    const double bound = (double)nq * (double)dmax(dx->n, dx->ndocs);
    const unsigned grid = (unsigned)dmax(1.0, dmin((double)cap, bound / kDlTile + 1.0));
    const bool docs = dx->occ_cut < dx->n;                            // (else no interval is long enough for route B)
    unsigned long long* const bcnt = reinterpret_cast<unsigned long long*>(w.bcnt);
    unsigned long long* const boff = reinterpret_cast<unsigned long long*>(w.boff);
    if (docs) SFX_LAUNCH("doclist_count_docs", 0.0, k_dl_count<true>, grid, kBlock, st, in, bcnt);
    else SFX_LAUNCH("doclist_count", 0.0, k_dl_count<false>, grid, kBlock, st, in, bcnt);
    SFX_LAUNCH("doclist_offsets", (double)grid * 16, k_dl_offsets, 1, kBlock, st, (const unsigned long long*)bcnt, grid, boff, w.res);
    if (docs) SFX_LAUNCH("doclist_emit_docs", 0.0, k_dl_emit<true>, grid, kBlock, st, in, (const unsigned long long*)boff, (const uint32_t*)w.res, w.K0, w.V0);
    else SFX_LAUNCH("doclist_emit", 0.0, k_dl_emit<false>, grid, kBlock, st, in, (const unsigned long long*)boff, (const uint32_t*)w.res, w.K0, w.V0);
    SFX_LAUNCH("doclist_first", (double)nq * 8, k_dl_first, qgrid, kBlock, st, (const uint64_t*)w.K0, docbits, nq, L, (const uint32_t*)w.res, w.ffirst);
    SFX_LAUNCH("doclist_cut", (double)nq * 12, k_dl_cut, qgrid, kBlock, st, (const uint64_t*)w.ffirst, nq, top_k, w.c);
    SFX_TRY(scan_u32_to_u64_excl_dev(w.c, nq, w.wfirst, w.part, st));
    SFX_LAUNCH("doclist_publish", (double)nq * 16, k_dl_publish, qgrid, kBlock, st, (const uint64_t*)w.wfirst, nq, L, d_first, w.res);
    uint32_t back[5] = {0, 0, 0, 0, 0};                               // Z_full, Z, the flag: the one read-back
    SFX_TRY(read_back(back, w.res, sizeof(back), st));
    if (back[kDlResBad]) return SFX_ERR_ARG;
    const uint64_t zfull = (uint64_t)back[1] << 32 | back[0];
    *listed_out = zfull;
    if (zfull > L) return SFX_OK;                                     // refused: nothing was written
    *count_out = (uint64_t)back[3] << 32 | back[2];
    if (zfull == 0 || capacity == 0) return SFX_OK;
    // the order, queued behind the read-back and sized by it
    const unsigned zgrid = (unsigned)dmax<uint64_t>(1, dmin<uint64_t>((zfull + kBlock - 1) / kBlock, cap));
    uint64_t *K = w.K0, *Kx = w.K1;
    uint32_t *V = w.V0, *Vx = w.V1;
    int in1 = 0, jshift = docbits;
    auto sorted = [&](int lo, int hi) -> int {
        SFX_TRY(radix_sort_kv64(K, V, Kx, Vx, zfull, lo, hi, w.scratch, st, &in1, nullptr, nullptr));
        if (in1) {
            uint64_t* tk = K; K = Kx; Kx = tk;
            uint32_t* tv = V; V = Vx; Vx = tv;
        }
        return SFX_OK;
    };
    if (order == SFX_DOCLIST_BY_DOC) {
        SFX_TRY(sorted(0, docbits + jbits));
    } else if (docbits + tfbits + jbits <= 64 && !dl_split_hook()) {
        SFX_LAUNCH("doclist_keys", (double)zfull * 24, k_dl_keys, zgrid, kBlock, st, K, V, zfull, 0, docbits, tfbits, dx->n);
        SFX_TRY(sorted(0, docbits + tfbits + jbits));
        jshift = docbits + tfbits;
    } else {
        SFX_LAUNCH("doclist_keys", (double)zfull * 24, k_dl_keys, zgrid, kBlock, st, K, V, zfull, 1, docbits, tfbits, dx->n);
        SFX_TRY(sorted(0, docbits + tfbits));
        SFX_LAUNCH("doclist_keys", (double)zfull * 24, k_dl_keys, zgrid, kBlock, st, K, V, zfull, 2, docbits, tfbits, dx->n);
        SFX_TRY(sorted(docbits, docbits + jbits));
    }
    SFX_LAUNCH("doclist_write", (double)zfull * 20, k_dl_write, zgrid, kBlock, st, (const uint64_t*)K, (const uint32_t*)V, zfull, jshift, docbits,
               (const uint64_t*)w.ffirst, (const uint64_t*)w.wfirst, top_k, capacity, d_doc, d_tf);
    return SFX_OK;
}

}  // namespace sfx
