// sfx_lce.hip -- longest common extensions between two positions of the indexed text, from SA + LCP alone
// (include/suffix_hip.h).
//
// LCE(i, j) = min lcp[lo + 1 .. hi] with lo < hi the ranks of i and j, so the index is two things:
//   isa       the inverse table, isa[sa[r]] = r, 4n bytes.  Creation proves that sa is a permutation of [0, n): lce_check
//             rejects an entry >= n, the scatter writes over a table cleared to 0xFFFFFFFF, lce_verify finds a slot that
//             was never written -- n writes below n that fill n slots are a bijection.
//   min-tree  F-ary (F = 32), level 0 = the LCP array itself (borrowed), L[k + 1][b] = min L[k][F b .. F b + F).  Every
//             level above 0 starts on a 128-byte line, so a node of 32 words IS one line.  Levels are added while the
//             last one has more than F entries.  The levels lie one behind the other, each padded to whole lines, so a
//             query derives a level's place from n alone: no table of offsets is read.
// A query [l, r) walks up from level 0: where l and r - 1 lie in one node (or on the top level) it scans l .. r and is
// done; otherwise it scans from l to the end of l's node and from the start of r's node to r -- at most two lines per
// level -- and continues with the nodes strictly between them one level up.  One lane answers one query; a run of words
// is read 16 bytes at a time wherever it is 16-byte aligned (always above level 0; on level 0 when the caller's lcp is).
//
//   lce_check     any sa[r] >= n, any doc_starts entry out of order
//   lce_scatter   isa[sa[r]] = r (entries >= n are skipped: nothing is written out of bounds on any input); from
//                 partitioned_scatter_min() entries on: (sa[r], r) pairs for the engine's partitioned scatter
//   lce_verify    one streaming pass: any slot still 0xFFFFFFFF
//   lce_levels    one level from the one below: a wave reads 64 consecutive words per step and reduces each group of F
//                 lanes with cross-lane moves
//   lce_query     two isa reads, the document ends by bisection (collections), max_mismatches + 1 rounds, every round
//                 clamped to the ends
//   lce_range_min / lce_ranks   the two halves on their own
// Creation reads the two flags back once; queries need no workspace and no synchronisation.  lcp is not verified: every
// index a query forms is bounded by n and by the level sizes (never by a value read from lcp), and every result is clamped
// to the distance to the ends, so a foreign lcp gives unspecified values and nothing else.
//
// Compiled as part of sfx_api.hip (which includes this file), like sfx_fm.hip, sfx_lz.hip and sfx_mem.hip.
#pragma once
#include "sfx_host.hpp"

struct sfx_lce {
    uint64_t n = 0, ndocs = 0, bytes = 0;
    void* mem = nullptr;                    // [isa | levels 1 ..] (nullptr: n == 0)
    void* own_lcp = nullptr;                // the host route's copies (nullptr: borrowed)
    void* own_starts = nullptr;
    const uint32_t* isa = nullptr;
    const uint32_t* lcp = nullptr;          // level 0
    const uint32_t* tree = nullptr;         // level 1
    const uint64_t* starts = nullptr;       // nullptr: a plain table
    int fan_log = 5, levels = 1;
#ifdef SFX_DEV_HOOKS
    void* pyr_mem = nullptr;                // hooked builds: the 64-ary pyramid of the baseline variant (nullptr: not built)
    sfx::Pyramid py = {};
#endif
};

namespace sfx {

constexpr int kLceFanLog = 5;                           // F = 32 words = one 128-byte line
constexpr uint32_t kLceNone = 0xFFFFFFFFu;
constexpr uint64_t kLceLineWords = 32;
constexpr unsigned kLceFlagWords = 64;                  // [0] a bad entry / doc start, [1] an empty slot

// test hook, read at every create: SFX_LCE_FAN=<2|4|8|16|32>, so that a few thousand entries have 6 to 12 levels
static int lce_fan_log()
{
    const char* e = dev_env("SFX_LCE_FAN");
    const int f = e ? atoi(e) : 0;
    for (int b = 1; b <= kLceFanLog; b++)
        if (f == 1 << b) return b;
    return kLceFanLog;
}
// test hook, read at every create and query: SFX_LCE_VARIANT=<lane|team|pyramid>; a handle answers through the pyramid
// only if it was created under that value (the pyramid is built then)
static int lce_variant_hook()
{
    const char* e = dev_env("SFX_LCE_VARIANT");
    if (!e) return -1;
    return !strcmp(e, "lane") ? 0 : !strcmp(e, "team") ? 1 : !strcmp(e, "pyramid") ? 2 : -1;
}
__host__ __device__ __forceinline__ uint64_t lce_line_up(uint64_t words) { return (words + kLceLineWords - 1) & ~(kLceLineWords - 1); }

struct LceLayout {
    int levels;                                         // level 0 included
    uint64_t tree_words, tree_off, bytes;
};
static LceLayout lce_layout(uint64_t n, int fan_log)
{
    LceLayout L{1, 0, 0, 0};
    for (uint64_t cnt = n; cnt > (1ull << fan_log); L.levels++) {
        cnt = (cnt + (1ull << fan_log) - 1) >> fan_log;
        L.tree_words += lce_line_up(cnt);
    }
    L.tree_off = lce_line_up(n) * 4;
    L.bytes = L.tree_off + L.tree_words * 4;
    return L;
}

// what the kernels need of the handle, by value
struct LceView {
    const uint32_t* isa;
    const uint32_t* lcp;
    const uint32_t* tree;
    const uint64_t* starts;
    uint64_t ndocs;
    uint32_t n;
    int fan_log, levels;
#ifdef SFX_DEV_HOOKS
    Pyramid py;                                         // hooked builds, SFX_LCE_VARIANT=pyramid at creation: the baseline's levels
#endif
};

// ---- build ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_lce_check(const uint32_t* __restrict__ sa, uint64_t n, const uint64_t* __restrict__ starts, uint64_t ndocs, uint32_t* __restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t t0 = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    bool bad = false;
    for (uint64_t r = t0; r < n; r += stride) bad |= sa[r] >= n;
    for (uint64_t d = t0; d < ndocs; d += stride) {                  // (as k_gsa_check_docs)
        const uint64_t v = starts[d];
        bad |= v > n || (d == 0 ? v != 0 : v < starts[d - 1]);
    }
    if (bad) flags[0] = 1u;
}
__global__ void __launch_bounds__(kBlock)
k_lce_scatter(const uint32_t* __restrict__ sa, uint64_t n, uint32_t* __restrict__ isa)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) {
        const uint32_t p = sa[r];
        if (p < n) isa[p] = (uint32_t)r;
    }
}
// (suffix << 32 | rank) in rank order for scatter_pairs_u32; an entry >= n (the call fails anyway) becomes a pair for
// slot 0 that writes the empty mark
__global__ void __launch_bounds__(kBlock)
k_lce_scatter_pairs(const uint32_t* __restrict__ sa, uint64_t n, uint64_t* __restrict__ pairs)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) {
        const uint32_t p = sa[r];
        pairs[r] = p < n ? (uint64_t)p << 32 | r : (uint64_t)kLceNone;
    }
}
__global__ void __launch_bounds__(kBlock)
k_lce_verify(const uint32_t* __restrict__ isa, uint64_t n, uint32_t* __restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    bool bad = false;
    for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += stride) bad |= isa[p] == kLceNone;
    if (bad) flags[1] = 1u;
}
// out[b] = min in[b << f .. (b + 1) << f) for the n_out = ceil(n_in >> f) nodes.  A wave takes 64 consecutive words per
// step (one coalesced read of two lines), every group of 1 << f lanes reduces with f exchanges and its first lane writes.
// The trip count is the same for all lanes of a wave, so every lane takes part in every exchange.
__global__ void __launch_bounds__(kBlock)
k_lce_levels(const uint32_t* __restrict__ in, uint64_t n_in, uint32_t* __restrict__ out, int f)
{
    const unsigned lane = threadIdx.x & (kWave - 1);
    const uint64_t wave = (uint64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock * kWave;
    for (uint64_t base = wave * kWave; base < n_in; base += stride) {
        const uint64_t i = base + lane;
        uint32_t v = i < n_in ? in[i] : kLceNone;
        for (int d = 1; d < (1 << f); d <<= 1) v = dmin(v, (uint32_t)__shfl_xor(v, d));
        if (i < n_in && (lane & ((1u << f) - 1)) == 0) out[i >> f] = v;
    }
}

// ---- queries ----------------------------------------------------------------------------------------------------------
// The shipped kernels answer one query per lane (kLceLane).  Builds with SFX_DEV_HOOKS also carry the two alternatives the
// shipped one is measured against (scripts/gpu_lce_time.py, SFX_LCE_VARIANT=lane|team|pyramid):
//   team      32 lanes per query: lane t reads word t of a span, so a node is fetched as one line by one instruction; the
//             lanes keep partial minima over all spans of a walk and exchange them once per round
//   pyramid   one lane per query through the 64-ary Pyramid / range_min of sfx_tree.hip: the baseline
constexpr int kLceLane = 0, kLceTeam = 1, kLcePyramid = 2;
constexpr int kLceShipped = kLceLane;
constexpr unsigned kLceTeamLanes = 32;

// min(m, L[a .. b)), b - a <= 32; only words of [a, b) are read.  vec: L is 16-byte aligned
__device__ __forceinline__ uint32_t lce_span_min(const uint32_t* __restrict__ L, uint64_t a, uint64_t b, bool vec, uint32_t m)
{
    uint64_t i = a;
    if (vec) {
        for (; i < b && (i & 3); i++) m = dmin(m, L[i]);
        for (; i + 4 <= b; i += 4) {
            const uint4 v = *reinterpret_cast<const uint4*>(L + i);
            m = dmin(dmin(m, v.x), dmin(dmin(v.y, v.z), v.w));
        }
    }
    for (; i < b; i++) m = dmin(m, L[i]);
    return m;
}
// min lcp[l .. r) for 0 <= l < r <= n.  Level k has cnt = ceil(n / F^k) words; r never exceeds it (r is a multiple of F
// when it is divided), so no index leaves a level.  TEAM: lane tl of 32 reads word tl of every span and returns its own
// partial minimum (the caller exchanges); otherwise the whole minimum.
template <bool TEAM> __device__ __forceinline__ uint32_t lce_walk(const LceView& v, uint64_t l, uint64_t r, unsigned tl)
{
    const int f = v.fan_log;
    const uint64_t mask = (1ull << f) - 1;
    const uint32_t* L = v.lcp;
    bool vec = (reinterpret_cast<uintptr_t>(L) & 15u) == 0;
    uint64_t cnt = v.n;
    uint32_t m = kLceNone;
    auto span = [&](uint64_t a, uint64_t b) {
        if (TEAM) {
            if (a + tl < b) m = dmin(m, L[a + tl]);
        } else {
            m = lce_span_min(L, a, b, vec, m);
        }
    };
    for (int k = 0;; k++) {
        if (((l ^ (r - 1)) >> f) == 0 || k == v.levels - 1) {
            span(l, r);
            return m;
        }
        if (l & mask) {
            const uint64_t e = (l | mask) + 1;
            span(l, e);
            l = e;
        }
        if (r & mask) {
            const uint64_t b = r & ~mask;
            span(b, r);
            r = b;
        }
        if (l >= r) return m;
        l >>= f;
        r >>= f;
        L = k == 0 ? v.tree : L + lce_line_up(cnt);
        cnt = (cnt + mask) >> f;
        vec = true;
    }
}
// one lane's answer to [l, r), 0 <= l < r <= n
template <int V> __device__ __forceinline__ uint32_t lce_range_min(const LceView& v, uint64_t l, uint64_t r)
{
#ifdef SFX_DEV_HOOKS
    if (V == kLcePyramid) return range_min(v.py, l, r - 1);
#endif
    return lce_walk<false>(v, l, r, 0);
}
// the end of the document that holds position p < n: the last d with starts[d] <= p (empty documents share a start)
__device__ __forceinline__ uint64_t lce_end_of(const LceView& v, uint64_t p)
{
    if (!v.starts) return v.n;
    uint64_t lo = 0, hi = v.ndocs;                                   // starts[lo] <= p < starts[hi]  (starts[0] = 0)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (v.starts[mid] <= p) lo = mid; else hi = mid;
    }
    return hi < v.ndocs ? v.starts[hi] : v.n;
}
// a query's state between rounds: done, or the next round compares the suffixes at i + len and j + len
struct LceState {
    uint64_t i, j, room, len;
    uint32_t miss;
    bool done;
};
__device__ __forceinline__ LceState lce_begin(const LceView& v, uint32_t i, uint32_t j)
{
    LceState s{i, j, 0, 0, 0, true};
    if (i > v.n || j > v.n) { s.len = kLceNone; return s; }
    if (i == v.n || j == v.n) return s;
    const uint64_t ei = lce_end_of(v, i), ej = i == j ? ei : lce_end_of(v, j);
    s.room = dmin(ei - i, ej - j);
    if (i == j) { s.len = s.room; return s; }
    s.done = false;
    return s;
}
// the ranks of the round's two suffixes, sorted: the range is [lo + 1, hi + 1)
__device__ __forceinline__ void lce_round_ranks(const LceView& v, const LceState& s, uint32_t* lo, uint32_t* hi)
{
    const uint32_t ra = v.isa[s.i + s.len], rb = v.isa[s.j + s.len];
    *lo = dmin(ra, rb);
    *hi = dmax(ra, rb);
}
// m = the round's range minimum: the extension is clamped to the room left, then a mismatch is stepped over while the
// budget and the room last -- at most k + 1 rounds, and len never exceeds room whatever m is
__device__ __forceinline__ void lce_advance(LceState& s, uint32_t m, uint32_t k)
{
    s.len += dmin<uint64_t>(m, s.room - s.len);
    if (s.miss < k && s.len < s.room) {                               // (len < room: a mismatch inside both ends)
        s.miss++;
        s.len++;
        s.done = s.len >= s.room;
    } else {
        s.done = true;
    }
}
template <int V> __global__ void __launch_bounds__(kBlock)
k_lce_query(LceView v, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint64_t nq, uint32_t k, uint32_t* __restrict__ len)
{
    if (V != kLceTeam) {
        const uint64_t stride = (uint64_t)gridDim.x * kBlock;
        for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += stride) {
            LceState s = lce_begin(v, a[q], b[q]);
            while (!s.done) {
                uint32_t lo, hi;
                lce_round_ranks(v, s, &lo, &hi);
                // (lo == hi only with a table that is not the handle's: stay bounded)
                lce_advance(s, lo == hi ? kLceNone : lce_range_min<V>(v, (uint64_t)lo + 1, (uint64_t)hi + 1), k);
            }
            len[q] = (uint32_t)s.len;
        }
        return;
    }
    // two teams per wave; the trip counts are the same for all lanes of a wave, so every lane takes part in every exchange
    const unsigned lane = threadIdx.x & (kWave - 1), tl = lane & (kLceTeamLanes - 1);
    constexpr unsigned per = kWave / kLceTeamLanes;
    const uint64_t wave = (uint64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock * per;
    for (uint64_t base = wave * per; base < nq; base += stride) {
        const uint64_t q = base + lane / kLceTeamLanes;
        LceState s{0, 0, 0, 0, 0, true};
        if (q < nq) s = lce_begin(v, a[q], b[q]);
        while (__any(!s.done)) {
            uint32_t m = kLceNone;
            if (!s.done) {
                uint32_t lo, hi;
                lce_round_ranks(v, s, &lo, &hi);
                if (lo != hi) m = lce_walk<true>(v, (uint64_t)lo + 1, (uint64_t)hi + 1, tl);
            }
            for (unsigned d = 1; d < kLceTeamLanes; d <<= 1) m = dmin(m, (uint32_t)__shfl_xor(m, (int)d));
            if (!s.done) lce_advance(s, m, k);
        }
        if (q < nq && tl == 0) len[q] = (uint32_t)s.len;
    }
}
template <int V> __global__ void __launch_bounds__(kBlock)
k_lce_range_min(LceView v, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi, uint64_t nq, uint32_t* __restrict__ out)
{
    if (V != kLceTeam) {
        const uint64_t stride = (uint64_t)gridDim.x * kBlock;
        for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += stride) {
            const uint32_t l = lo[q], r = hi[q];
            out[q] = (l >= r || r > v.n) ? kLceNone : lce_range_min<V>(v, l, r);
        }
        return;
    }
    const unsigned lane = threadIdx.x & (kWave - 1), tl = lane & (kLceTeamLanes - 1);
    constexpr unsigned per = kWave / kLceTeamLanes;
    const uint64_t wave = (uint64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock * per;
    for (uint64_t base = wave * per; base < nq; base += stride) {
        const uint64_t q = base + lane / kLceTeamLanes;
        uint32_t m = kLceNone;
        if (q < nq) {
            const uint32_t l = lo[q], r = hi[q];
            if (l < r && r <= v.n) m = lce_walk<true>(v, l, r, tl);
        }
        for (unsigned d = 1; d < kLceTeamLanes; d <<= 1) m = dmin(m, (uint32_t)__shfl_xor(m, (int)d));
        if (q < nq && tl == 0) out[q] = m;
    }
}
__global__ void __launch_bounds__(kBlock)
k_lce_ranks(LceView v, const uint32_t* __restrict__ pos, uint64_t nq, uint32_t* __restrict__ rank)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += stride) {
        const uint32_t p = pos[q];
        rank[q] = p < v.n ? v.isa[p] : kLceNone;
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
static unsigned lce_grid(uint64_t items)
{
    return (unsigned)dmax<uint64_t>(1, dmin<uint64_t>((items + kBlock - 1) / kBlock, dmin<unsigned>(kMaxGrid, grid_cap())));
}
// [flags 64 u32 | from partitioned_scatter_min() entries on: pairs n u64 | tmp n u64 | radix scratch]
struct LceWs {
    uint32_t* flags;
    uint64_t *pairs, *tmp;
    uint32_t* scratch;
};
struct LceSizer {                                      // ArenaSizer with pointer-returning take
    uint64_t used = 0;
    template <class T> T* take(uint64_t count) { used += (count * sizeof(T) + kArenaAlign - 1) & ~(kArenaAlign - 1); return nullptr; }
};
template <class A> static void lce_carve(A& a, uint64_t n, LceWs* w)
{
    w->flags = a.template take<uint32_t>(kLceFlagWords);
    w->pairs = w->tmp = nullptr;
    w->scratch = nullptr;
    if (n >= partitioned_scatter_min()) {
        w->pairs = a.template take<uint64_t>(n);
        w->tmp = a.template take<uint64_t>(n);
        w->scratch = a.template take<uint32_t>(radix_scratch_words(n));
    }
}
uint64_t inverse_table_workspace_bytes(uint64_t n)
{
    if (n == 0 || n > 0xFFFFFFFFull) return 0;
    LceSizer z;
    LceWs w;
    lce_carve(z, n, &w);
    return z.used;
}
// queues check, clear, scatter and verify; the two flags are left in w.flags for the caller's one read-back
static int lce_isa_queue(const uint32_t* d_sa, uint64_t n, const uint64_t* d_starts, uint64_t ndocs, uint32_t* d_isa, const LceWs& w,
                         hipStream_t st)
{
    const unsigned grid = lce_grid(n);
    SFX_HIP(hipMemsetAsync(w.flags, 0, kLceFlagWords * sizeof(uint32_t), st));
    SFX_LAUNCH("lce_check", (double)n * 4 + (double)ndocs * 8, k_lce_check, lce_grid(dmax(n, ndocs)), kBlock, st, d_sa, n, d_starts,
               d_starts ? ndocs : 0, w.flags);
    SFX_HIP(hipMemsetAsync(d_isa, 0xFF, n * sizeof(uint32_t), st));
    if (w.pairs) {
        SFX_LAUNCH("lce_scatter", (double)n * 12, k_lce_scatter_pairs, grid, kBlock, st, d_sa, n, w.pairs);
        SFX_TRY(scatter_pairs_u32(w.pairs, w.tmp, n, n, d_isa, w.scratch, st, nullptr));
    } else {
        SFX_LAUNCH("lce_scatter", (double)n * 8, k_lce_scatter, grid, kBlock, st, d_sa, n, d_isa);
    }
    SFX_LAUNCH("lce_verify", (double)n * 4, k_lce_verify, grid, kBlock, st, (const uint32_t*)d_isa, n, w.flags);
    return SFX_OK;
}
int inverse_table_dev(const uint32_t* d_sa, uint64_t n, uint32_t* d_isa, void* ws, uint64_t ws_bytes, hipStream_t st)
{
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!d_sa || !d_isa) return SFX_ERR_ARG;
    if (!ws || ws_bytes < inverse_table_workspace_bytes(n)) return SFX_ERR_WORKSPACE;
    Arena a(ws, ws_bytes);
    LceWs w;
    lce_carve(a, n, &w);
    if (a.overflow) return SFX_ERR_INTERNAL;
    SFX_TRY(lce_isa_queue(d_sa, n, nullptr, 0, d_isa, w, st));
    uint32_t flags[2] = {0, 0};
    SFX_TRY(read_back(flags, w.flags, sizeof(flags), st));
    return (flags[0] | flags[1]) ? SFX_ERR_ARG : SFX_OK;
}

uint64_t lce_bytes(uint64_t n)
{
    if (n == 0 || n > 0xFFFFFFFFull) return 0;
    return lce_layout(n, lce_fan_log()).bytes;
}
static LceView lce_view(const sfx_lce* lx)
{
    LceView v{lx->isa, lx->lcp, lx->tree, lx->starts, lx->ndocs, (uint32_t)lx->n, lx->fan_log, lx->levels};
#ifdef SFX_DEV_HOOKS
    v.py = lx->py;
#endif
    return v;
}
// the variant a query launch takes: the shipped one; in hooked builds what SFX_LCE_VARIANT names
static int lce_variant(const sfx_lce* lx)
{
    int v = kLceShipped;
#ifdef SFX_DEV_HOOKS
    const int h = lce_variant_hook();
    if (h >= 0) v = h;
    if (v == kLcePyramid && !lx->pyr_mem) v = kLceShipped;
#endif
    (void)lx;
    return v;
}
void lce_destroy(sfx_lce* lx)
{
    if (!lx) return;
    if (lx->mem) (void)dev_free(lx->mem);
    if (lx->own_lcp) (void)dev_free(lx->own_lcp);
    if (lx->own_starts) (void)dev_free(lx->own_starts);
#ifdef SFX_DEV_HOOKS
    if (lx->pyr_mem) (void)dev_free(lx->pyr_mem);
#endif
    delete lx;
}
// scratch: inverse_table_workspace_bytes(n) bytes of the caller's, free again when this returns SFX_OK (the read-back is
// the last thing queued); after an error the caller drains the stream before reusing it
static int lce_build(sfx_lce* lx, const uint32_t* d_sa, hipStream_t st, void* scratch, uint64_t scratch_bytes)
{
    const uint64_t n = lx->n;
    const LceLayout L = lce_layout(n, lx->fan_log);
    if (!scratch || scratch_bytes < inverse_table_workspace_bytes(n)) return SFX_ERR_WORKSPACE;
    SFX_HIP(dev_malloc(&lx->mem, L.bytes));
    lx->bytes = L.bytes;
    lx->levels = L.levels;
    uint32_t* isa = (uint32_t*)lx->mem;
    uint32_t* tree = (uint32_t*)((char*)lx->mem + L.tree_off);
    lx->isa = isa;
    lx->tree = tree;
    Arena a(scratch, scratch_bytes);
    LceWs w;
    lce_carve(a, n, &w);
    if (a.overflow) return SFX_ERR_INTERNAL;
    SFX_TRY(lce_isa_queue(d_sa, n, lx->starts, lx->ndocs, isa, w, st));
    // the levels, each from the one below; the padding behind a level keeps the empty mark (never read)
    if (L.tree_words) SFX_HIP(hipMemsetAsync(tree, 0xFF, L.tree_words * 4, st));
    const uint32_t* in = lx->lcp;
    uint32_t* out = tree;
    uint64_t cnt = n;
    for (int k = 1; k < L.levels; k++) {
        const uint64_t cnt_out = (cnt + (1ull << lx->fan_log) - 1) >> lx->fan_log;
        const unsigned grid = (unsigned)dmax<uint64_t>(1, dmin<uint64_t>((cnt + kBlock - 1) / kBlock, dmin<unsigned>(kMaxGrid, grid_cap())));
        SFX_LAUNCH("lce_levels", (double)cnt * 4 + (double)cnt_out * 4, k_lce_levels, grid, kBlock, st, in, cnt, out, lx->fan_log);
        in = out;
        out += lce_line_up(cnt_out);
        cnt = cnt_out;
    }
#ifdef SFX_DEV_HOOKS
    if (lce_variant_hook() == kLcePyramid) {
        SFX_HIP(dev_malloc(&lx->pyr_mem, (lcp_pyramid_words(n) + 64) * sizeof(uint32_t)));
        SFX_TRY(lcp_pyramid_build_dev(lx->lcp, n, (uint32_t*)lx->pyr_mem, st, &lx->py));
    }
#endif
    uint32_t flags[2] = {0, 0};
    SFX_TRY(read_back(flags, w.flags, sizeof(flags), st));            // the one synchronisation of a create
    return (flags[0] | flags[1]) ? SFX_ERR_ARG : SFX_OK;
}
// own: d_lcp / d_starts were allocated with hipMalloc for this handle, which frees them (the host route).
// scratch: inverse_table_workspace_bytes(n) bytes of device memory for the duration of the call (n == 0: none)
int lce_create_dev(const uint32_t* d_sa, const uint32_t* d_lcp, uint64_t n, const uint64_t* d_starts, uint64_t ndocs, hipStream_t st,
                   bool own, void* scratch, uint64_t scratch_bytes, sfx_lce** out)
{
    if (!out) return SFX_ERR_ARG;
    *out = nullptr;
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n && (!d_sa || !d_lcp)) return SFX_ERR_ARG;
    if (d_starts ? ndocs == 0 : ndocs != 0) return SFX_ERR_ARG;
    sfx_lce* lx = new sfx_lce;
    lx->n = n;
    lx->fan_log = lce_fan_log();
    int rc = SFX_OK;
    if (n) {
        lx->lcp = d_lcp;
        lx->starts = d_starts;
        lx->ndocs = d_starts ? ndocs : 0;
        rc = lce_build(lx, d_sa, st, scratch, scratch_bytes);
        if (own) {
            lx->own_lcp = const_cast<uint32_t*>(d_lcp);
            lx->own_starts = const_cast<uint64_t*>(d_starts);
        }
    }
    if (rc != SFX_OK) {
        if (own) lx->own_lcp = lx->own_starts = nullptr;               // (the caller's to free after a failure)
        lce_destroy(lx);
        return rc;
    }
    *out = lx;
    return SFX_OK;
}
int lce_query_dev(const sfx_lce* lx, const uint32_t* d_a, const uint32_t* d_b, uint64_t nq, uint32_t k, uint32_t* d_len, hipStream_t st)
{
    if (!lx) return SFX_ERR_ARG;
    if (nq == 0) return SFX_OK;
    if (!d_a || !d_b || !d_len) return SFX_ERR_ARG;
    // two isa lines and about eight tree lines per round (DESIGN.md section 21 counts them)
    const double bytes = (double)nq * (12 + 10 * 128);
    const int var = lce_variant(lx);
    if (var == kLceShipped) {
        const unsigned grid = lce_grid(kLceShipped == kLceTeam ? nq * kLceTeamLanes : nq);
        SFX_LAUNCH("lce_query", bytes, k_lce_query<kLceShipped>, grid, kBlock, st, lce_view(lx), d_a, d_b, nq, k, d_len);
    }
#ifdef SFX_DEV_HOOKS
    else if (var == kLceLane) SFX_LAUNCH("lce_query", bytes, k_lce_query<kLceLane>, lce_grid(nq), kBlock, st, lce_view(lx), d_a, d_b, nq, k, d_len);
    else if (var == kLceTeam)
        SFX_LAUNCH("lce_query", bytes, k_lce_query<kLceTeam>, lce_grid(nq * kLceTeamLanes), kBlock, st, lce_view(lx), d_a, d_b, nq, k, d_len);
    else SFX_LAUNCH("lce_query", bytes, k_lce_query<kLcePyramid>, lce_grid(nq), kBlock, st, lce_view(lx), d_a, d_b, nq, k, d_len);
#endif
    return SFX_OK;
}
int lce_range_min_dev(const sfx_lce* lx, const uint32_t* d_lo, const uint32_t* d_hi, uint64_t nq, uint32_t* d_min, hipStream_t st)
{
    if (!lx) return SFX_ERR_ARG;
    if (nq == 0) return SFX_OK;
    if (!d_lo || !d_hi || !d_min) return SFX_ERR_ARG;
    const double bytes = (double)nq * (12 + 8 * 128);
    const int var = lce_variant(lx);
    if (var == kLceShipped) {
        const unsigned grid = lce_grid(kLceShipped == kLceTeam ? nq * kLceTeamLanes : nq);
        SFX_LAUNCH("lce_range_min", bytes, k_lce_range_min<kLceShipped>, grid, kBlock, st, lce_view(lx), d_lo, d_hi, nq, d_min);
    }
#ifdef SFX_DEV_HOOKS
    else if (var == kLceLane)
        SFX_LAUNCH("lce_range_min", bytes, k_lce_range_min<kLceLane>, lce_grid(nq), kBlock, st, lce_view(lx), d_lo, d_hi, nq, d_min);
    else if (var == kLceTeam)
        SFX_LAUNCH("lce_range_min", bytes, k_lce_range_min<kLceTeam>, lce_grid(nq * kLceTeamLanes), kBlock, st, lce_view(lx), d_lo, d_hi, nq, d_min);
    else SFX_LAUNCH("lce_range_min", bytes, k_lce_range_min<kLcePyramid>, lce_grid(nq), kBlock, st, lce_view(lx), d_lo, d_hi, nq, d_min);
#endif
    return SFX_OK;
}
int lce_ranks_dev(const sfx_lce* lx, const uint32_t* d_pos, uint64_t nq, uint32_t* d_rank, hipStream_t st)
{
    if (!lx) return SFX_ERR_ARG;
    if (nq == 0) return SFX_OK;
    if (!d_pos || !d_rank) return SFX_ERR_ARG;
    SFX_LAUNCH("lce_ranks", (double)nq * (8 + 128), k_lce_ranks, lce_grid(nq), kBlock, st, lce_view(lx), d_pos, nq, d_rank);
    return SFX_OK;
}

}  // namespace sfx
