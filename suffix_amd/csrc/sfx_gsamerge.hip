// sfx_gsamerge.hip -- merge of two generalized suffix arrays: a collection A and the documents B added behind it
// (include/suffix_hip.h).
//
// Truncated suffixes are ordered by their bytes and equal ones by position, so a document behind the collection never moves
// an old suffix relative to another old one and sorts after every old suffix equal to it:
//   GSA(A || B) = the stable merge of GSA(A) and GSA(B), the old entry first on equal strings.
// For the new suffix x_j at B-rank j: p[j] = the number of old suffixes <= x_j, left[j] / right[j] = its common prefix with
// the old suffixes at ranks p[j] - 1 / p[j] (0 where there is none).  x_j goes to slot p[j] + j, old rank r to slot
// r + #{j : p[j] <= r}.  A pair of merged neighbours that was adjacent inside A or inside B keeps that array's lcp; an
// (old, new) seam gets left[j], a (new, old) seam right[j] of the last j in front of it.
//
//   gmerge_check    doc_starts as k_gsa_check_docs wants them and with the split at n_a; every sa_a[r] < n_a, sa_b[j] < n_b,
//                   da_a[r] < ndocs_a, da_b[j] < ndocs - ndocs_a.  One read-back; nothing else runs on arrays that fail.
//   gmerge_rank     one lane per new suffix, grid-stride, no LDS: the upper-bound bisection over the old table ("old <= new"
//                   moves the lower bound), both bounds carrying their common prefix with x_j as ms_search does, ms_extend
//                   comparing 8 bytes per step from the smaller of the two.  A lane whose common prefix exceeds match_limit
//                   stops and reports match_limit + 1.  p, left, right per suffix; the maximum of max(left, right) per WAVE
//                   (a shuffle reduction: four words per workgroup, no LDS, no atomics).
//                   A second launch under the same name takes the maximum of those words and proves p non-decreasing.
//                   One read-back: (p out of order, longest).
//   gmerge_scatter  one workgroup per tile of output slots: the first new suffix at or after the tile by a bisection of
//                   q[j] = p[j] + j (computed on the fly), the tile's new slots marked in LDS, an LDS scan that gives every
//                   slot its source index, then sa / da / lcp written with full-width stores.
// Arrays that pass gmerge_check but are no GSAs give some answer; every index is bounded first: a suffix length is clamped to
// [0, doc end - position], p <= n_a by construction, p is proven non-decreasing before gmerge_scatter runs, and a slot's source
// index is its slot number less a count of marks -- never a value read from an input array.
//
// Compiled as part of sfx_api.hip.
#pragma once
#include "sfx_host.hpp"

namespace sfx {

constexpr uint32_t kGmTile = 2048;                      // output slots per workgroup of gmerge_scatter
constexpr unsigned kGmFlagWords = 64;                   // [0] a failed check  [1] p out of order  [2] longest
enum { kGmBad = 0, kGmOrder = 1, kGmLongest = 2 };

// test hook, read at every call: SFX_GM_TILE=<slots> in [1, 2048]
static uint32_t gm_tile()
{
    const char* e = dev_env("SFX_GM_TILE");
    const int t = e ? atoi(e) : 0;
    return t >= 1 && t <= (int)kGmTile ? (uint32_t)t : kGmTile;
}

// what the three kernels read: the whole collection's text and document starts, the two array sets
struct GmIn {
    const uint8_t* text;                                // n = na + nb bytes
    const uint64_t* starts;                             // ndocs, over the whole collection
    uint64_t ndocs, nda, n, na, nb;
    const uint32_t *sa_a, *da_a, *lcp_a;                // na each; da_a may be NULL
    const uint32_t *sa_b, *da_b, *lcp_b;                // nb each, relative to B; da_b may be NULL
};

// the document of position p: the last start <= p (as gsa_doc_of of sfx_tree.hip)
__device__ __forceinline__ uint64_t gm_doc_of(const uint64_t* __restrict__ starts, uint64_t ndocs, uint64_t p)
{
    uint64_t lo = 0, hi = ndocs;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (starts[mid] <= p) lo = mid + 1; else hi = mid;
    }
    return lo ? lo - 1 : 0;
}
// bytes from position s to the end of document d < ndocs; 0 for a position that does not lie in front of that end
__device__ __forceinline__ uint64_t gm_rest(const GmIn& in, uint64_t d, uint64_t s)
{
    const uint64_t e = d + 1 < in.ndocs ? in.starts[d + 1] : in.n;
    return e > s ? e - s : 0;
}
__device__ __forceinline__ uint64_t gm_doc_a(const GmIn& in, uint64_t r, uint64_t s)
{
    return in.da_a ? in.da_a[r] : gm_doc_of(in.starts, in.ndocs, s);
}
// the document of the new suffix at B-rank j, position s of the whole text, numbered in the whole collection
__device__ __forceinline__ uint64_t gm_doc_b(const GmIn& in, uint64_t j, uint64_t s)
{
    return in.da_b ? in.nda + in.da_b[j] : gm_doc_of(in.starts, in.ndocs, s);
}

__global__ void __launch_bounds__(kBlock)
k_gm_check(GmIn in, uint32_t* __restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock, ndb = in.ndocs - in.nda;
    const uint64_t items = dmax(in.ndocs, dmax(in.na, in.nb));
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < items; i += stride) {
        if (i < in.ndocs) {
            const uint64_t v = in.starts[i];
            bad |= v > in.n || (i == 0 ? v != 0 : v < in.starts[i - 1]);
            bad |= i == in.nda && v != in.na;                         // the split lies where the caller says
        }
        if (i < in.na) {
            bad |= in.sa_a[i] >= in.na;
            if (in.da_a) bad |= in.da_a[i] >= in.nda;
        }
        if (i < in.nb) {
            bad |= in.sa_b[i] >= in.nb;
            if (in.da_b) bad |= in.da_b[i] >= ndb;
        }
    }
    if (bad) flags[kGmBad] = 1u;                                      // (every writer stores the same word)
}

// p / left / right of every new suffix; wmax[4 * block + wave] = the largest max(left, right) the wave saw, limit + 1 for
// a lane that stopped at the match limit (limit 0: none)
__global__ void __launch_bounds__(kBlock)
k_gm_rank(GmIn in, uint32_t limit, uint32_t* __restrict__ p_out, uint32_t* __restrict__ left_out, uint32_t* __restrict__ right_out,
          uint32_t* __restrict__ wmax)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t t0 = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t seen = 0;
    for (uint64_t j = t0; j < in.nb; j += stride) {
        const uint64_t sx = in.na + in.sa_b[j];
        const uint64_t lx = gm_rest(in, gm_doc_b(in, j, sx), sx);
        const uint8_t* const x = in.text + sx;
        uint64_t lo = 0, hi = in.na, l = 0, r = 0;
        bool stopped = false;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            const uint64_t s = in.sa_a[mid];
            const uint64_t slen = gm_rest(in, gm_doc_a(in, mid, s), s);
            const uint64_t both = dmin(lx, slen);
            const uint64_t lim = limit ? dmin<uint64_t>(both, (uint64_t)limit + 1) : both;
            const uint64_t k = ms_extend(x, in.text + s, dmin(dmin(l, r), lim), lim);
            if (limit && k > limit) { stopped = true; break; }
            // old <= new: the old suffix ends here (a prefix of the new one, or equal to it), or its next byte is the smaller
            const bool le = k == slen || (k < lx && in.text[s + k] < x[k]);
            if (le) { lo = mid + 1; l = k; } else { hi = mid; r = k; }
        }
        if (lo == 0) l = 0;
        if (lo == in.na) r = 0;
        p_out[j] = (uint32_t)lo;
        left_out[j] = (uint32_t)l;
        right_out[j] = (uint32_t)r;
        seen = dmax(seen, stopped ? limit + 1 : (uint32_t)dmax(l, r));
    }
    for (int d = 32; d >= 1; d >>= 1) seen = dmax(seen, (uint32_t)__shfl_xor((int)seen, d));
    if (lane_id() == 0) wmax[(uint64_t)blockIdx.x * kWavesPerBlock + wave_id()] = seen;
}
// flags[kGmOrder] = 1 where p decreases; workgroup 0 also writes flags[kGmLongest] = max wmax[0 .. nw)
__global__ void __launch_bounds__(kBlock)
k_gm_rank_finish(const uint32_t* __restrict__ p, uint64_t nb, const uint32_t* __restrict__ wmax, unsigned nw, uint32_t* __restrict__ flags)
{
    __shared__ uint32_t sh[kWavesPerBlock];
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    bool bad = false;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x + 1; j < nb; j += stride) bad |= p[j - 1] > p[j];
    if (bad) flags[kGmOrder] = 1u;
    if (blockIdx.x != 0) return;
    uint32_t m = 0;
    for (unsigned i = threadIdx.x; i < nw; i += kBlock) m = dmax(m, wmax[i]);
    for (int d = 32; d >= 1; d >>= 1) m = dmax(m, (uint32_t)__shfl_xor((int)m, d));
    if (lane_id() == 0) sh[wave_id()] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWavesPerBlock; w++) m = dmax(m, sh[w]);
        flags[kGmLongest] = m;
    }
}

// Tile t holds the output slots [t * tile, min(n, (t + 1) * tile)).  mark[1 + i] = (the number of new slots among the tile's
// first i) << 1 | (slot i is new); mark[0] = is the slot in front of the tile new.
__global__ void __launch_bounds__(kBlock)
k_gm_scatter(GmIn in, const uint32_t* __restrict__ p, const uint32_t* __restrict__ left, const uint32_t* __restrict__ right,
             uint32_t tile, uint64_t ntiles, uint32_t* __restrict__ sa, uint32_t* __restrict__ da, uint32_t* __restrict__ lcp)
{
    __shared__ uint32_t mark[kGmTile + 1];
    __shared__ uint32_t part[kWavesPerBlock];
    const uint32_t per = (tile + kBlock - 1) / kBlock;                // slots per thread of the scan
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t s0 = t * tile;
        const uint32_t cnt = (uint32_t)dmin<uint64_t>(tile, in.n - s0);
        // the first new suffix whose slot is not in front of the tile (q is increasing; every lane takes the same steps)
        uint64_t a = 0, b = in.nb;
        while (a < b) {
            const uint64_t mid = (a + b) >> 1;
            if ((uint64_t)p[mid] + mid < s0) a = mid + 1; else b = mid;
        }
        const uint64_t j0 = a;
        for (uint32_t i = threadIdx.x; i <= cnt; i += kBlock) mark[i] = 0;
        __syncthreads();
        if (threadIdx.x == 0 && j0 > 0 && (uint64_t)p[j0 - 1] + j0 == s0) mark[0] = 1u;       // q[j0 - 1] == s0 - 1
        for (uint64_t j = j0 + threadIdx.x; j < in.nb && j - j0 < cnt; j += kBlock) {
            const uint64_t q = (uint64_t)p[j] + j;
            if (q >= s0 && q - s0 < cnt) mark[1 + (q - s0)] = 1u;     // (q >= s0 from j0 on)
        }
        __syncthreads();
        const uint32_t c0 = dmin(threadIdx.x * per, cnt), c1 = dmin(c0 + per, cnt);
        uint32_t mine = 0;
        for (uint32_t i = c0; i < c1; i++) mine += mark[1 + i];
        uint32_t total;
        uint32_t run = block_scan_add_excl<uint32_t>(mine, part, total);
        for (uint32_t i = c0; i < c1; i++) {
            const uint32_t m = mark[1 + i];
            mark[1 + i] = run << 1 | m;
            run += m;
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < cnt; i += kBlock) {
            const uint32_t v = mark[1 + i];
            const bool prev_new = (mark[i] & 1u) != 0;
            const uint64_t jn = j0 + (v >> 1);                        // new suffixes in front of this slot
            uint32_t pos, len = 0;
            uint64_t doc = 0;
            if (v & 1u) {
                const uint64_t j = dmin(jn, in.nb - 1);               // (jn < nb: the slot was marked by suffix jn)
                pos = (uint32_t)(in.na + in.sa_b[j]);
                if (da) doc = gm_doc_b(in, j, pos);
                if (lcp) len = prev_new ? in.lcp_b[j] : left[j];
            } else {
                const uint64_t r = dmin(s0 + i - jn, in.na - 1);      // (< na: n slots hold nb new ones)
                pos = in.sa_a[r];
                if (da) doc = gm_doc_a(in, r, pos);
                if (lcp) len = prev_new ? right[jn - 1] : in.lcp_a[r];
            }
            sa[s0 + i] = pos;
            if (da) da[s0 + i] = (uint32_t)doc;
            if (lcp) lcp[s0 + i] = len;
        }
        __syncthreads();                                              // mark is cleared for the next tile
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// [flags 256 B | p nb u32 | left nb u32 | right nb u32 | wave maxima 4 kMaxGrid u32] <= 12 nb + 34 KiB
struct GmWs { uint32_t *flags, *p, *left, *right, *wmax; };
template <class A> static void gm_carve(A& a, uint64_t nb, GmWs* w)
{
    w->flags = a.template take<uint32_t>(kGmFlagWords);
    w->p = a.template take<uint32_t>(nb);
    w->left = a.template take<uint32_t>(nb);
    w->right = a.template take<uint32_t>(nb);
    w->wmax = a.template take<uint32_t>((uint64_t)kMaxGrid * kWavesPerBlock);
}
struct GmSizer {
    uint64_t used = 0;
    template <class T> T* take(uint64_t count) { used += (count * sizeof(T) + kArenaAlign - 1) & ~(kArenaAlign - 1); return nullptr; }
};
uint64_t gsa_merge_workspace_bytes(uint64_t na, uint64_t nb)
{
    if (na > 0xFFFFFFFFull || nb > 0xFFFFFFFFull || na + nb > 0xFFFFFFFFull) return 0;
    GmSizer z;
    GmWs w;
    gm_carve(z, nb, &w);
    return z.used;
}
static bool gm_overlap(const void* a, uint64_t abytes, const void* b, uint64_t bbytes)
{
    if (!a || !b || !abytes || !bbytes) return false;
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bbytes && y < x + abytes;
}
static unsigned gm_grid(uint64_t items)
{
    return (unsigned)dmax<uint64_t>(1, dmin<uint64_t>((items + kBlock - 1) / kBlock, dmin<unsigned>(kMaxGrid, grid_cap())));
}
int gsa_merge_dev(const GmIn& in, uint32_t match_limit, uint32_t* d_sa, uint32_t* d_da, uint32_t* d_lcp, uint64_t* longest_out, void* ws,
                  uint64_t ws_bytes, hipStream_t st)
{
    if (in.na > 0xFFFFFFFFull || in.nb > 0xFFFFFFFFull || in.n > 0xFFFFFFFFull || in.ndocs > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (!longest_out || in.nda > in.ndocs) return SFX_ERR_ARG;
    *longest_out = 0;
    if (in.n == 0) return SFX_OK;
    if (in.ndocs == 0 || !in.text || !in.starts || !d_sa) return SFX_ERR_ARG;
    if ((in.na && (in.nda == 0 || !in.sa_a || (d_lcp && !in.lcp_a))) || (in.nb && (in.nda == in.ndocs || !in.sa_b || (d_lcp && !in.lcp_b))))
        return SFX_ERR_ARG;
    if (!ws || ws_bytes < gsa_merge_workspace_bytes(in.na, in.nb)) return SFX_ERR_WORKSPACE;
    const uint64_t bytes = in.n * sizeof(uint32_t);
    for (const uint32_t* out : {d_sa, d_da, d_lcp}) {
        const struct { const void* p; uint64_t b; } ins[] = {
            {in.text, in.n}, {in.starts, in.ndocs * sizeof(uint64_t)}, {in.sa_a, in.na * 4}, {in.da_a, in.na * 4}, {in.lcp_a, in.na * 4},
            {in.sa_b, in.nb * 4}, {in.da_b, in.nb * 4}, {in.lcp_b, in.nb * 4}, {ws, ws_bytes}};
        for (const auto& x : ins)
            if (gm_overlap(out, bytes, x.p, x.b)) return SFX_ERR_ARG;
    }
    Arena a(ws, ws_bytes);
    GmWs w;
    gm_carve(a, in.nb, &w);
    if (a.overflow) return SFX_ERR_INTERNAL;
    SFX_HIP(hipMemsetAsync(w.flags, 0, kGmFlagWords * sizeof(uint32_t), st));
    const uint64_t items = dmax(in.ndocs, dmax(in.na, in.nb));
    SFX_LAUNCH("gmerge_check", (double)in.ndocs * 8 + (double)in.n * (4 + (in.da_a ? 4 : 0)), k_gm_check, gm_grid(items), kBlock, st, in, w.flags);
    uint32_t flags[4] = {0, 0, 0, 0};
    SFX_TRY(read_back(flags, w.flags, sizeof(flags), st));            // nothing indexes by an entry that was not checked
    if (flags[kGmBad]) return SFX_ERR_ARG;
    if (in.nb) {
        const unsigned grid = gm_grid(in.nb);
        // per bisection step a table entry, its document's end and a line of text, all dependent
        SFX_LAUNCH("gmerge_rank", (double)in.nb * (16 + (double)bits_for(in.na) * 3 * 64), k_gm_rank, grid, kBlock, st, in, match_limit, w.p,
                   w.left, w.right, w.wmax);
        SFX_LAUNCH("gmerge_rank", (double)in.nb * 4, k_gm_rank_finish, grid, kBlock, st, (const uint32_t*)w.p, in.nb, (const uint32_t*)w.wmax,
                   grid * (unsigned)kWavesPerBlock, w.flags);
        SFX_TRY(read_back(flags, w.flags, sizeof(flags), st));
        *longest_out = flags[kGmLongest];
        if (match_limit && flags[kGmLongest] > match_limit) return SFX_OK;   // refused: nothing is written (a lane that stopped left no p)
        if (flags[kGmOrder]) return SFX_ERR_ARG;
    }
    const uint32_t tile = gm_tile();
    const uint64_t ntiles = (in.n + tile - 1) / tile;
    const unsigned sgrid = (unsigned)dmin<uint64_t>(ntiles, grid_cap() < kMaxGrid ? grid_cap() : ntiles);
    SFX_LAUNCH("gmerge_scatter", (double)in.n * (12 + 4 * (1 + (d_da ? 1 : 0) + (d_lcp ? 1 : 0))), k_gm_scatter, sgrid, kBlock, st, in,
               (const uint32_t*)w.p, (const uint32_t*)w.left, (const uint32_t*)w.right, tile, ntiles, d_sa, d_da, d_lcp);
    return SFX_OK;
}

}  // namespace sfx
