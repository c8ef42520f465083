// sfx_mem.hip -- maximal exact matches of a query text against a table (include/suffix_hip.h).
//
// T = the indexed text of n bytes with table sa, Q = the query of m bytes, L = min_len.  A candidate pair (i, r) is a
// query position and a rank whose suffix shares at least L bytes with Q[i..]; the capped matching statistics
// (max_len = L) give exactly those ranks as one interval [start_i, end_i) per position whose capped length reaches L.
// Pairs are numbered k = off[i] + (r - start_i), off = the exclusive sum of the interval sizes: ascending by i, then by
// rank -- the order of the output.  P = off[m] pairs in all.  Pair (i, r) with p = sa[r] is the left end of a maximal
// match iff it cannot be extended to the left (i == 0, p at the start of the text / its document, or
// Q[i-1] != T[p-1]); its length is then found by extending to the right from byte L on.
//
//   mem_cand    cand[i] = len[i] == L ? end[i] - start[i] : 0, in place over len
//   scan        off = the 64-bit exclusive sum of cand (the three-phase scan of sfx_tree.hip); P stays on the device
//   mem_count   tiles of K consecutive pairs: positions are expanded to pairs through LDS, every pair is tested for
//               left-maximality (and, with SFX_MEM_UNIQUE, extended and compared with its rank neighbours); per tile
//               the number of matches and one bit per pair
//   scan        tile offsets, 64-bit
//   mem_emit    the marked pairs of a tile, compacted in pair order, are extended and written at tile_off + rank
//               while that is below `capacity`; the first lane posts (P, Z) for the one read-back
// A P above pair_limit makes mem_count write zero counts and nothing else, so that mem_emit writes nothing.
// No workgroup waits for another and nothing is counted with atomics; every loop is bounded by m, n or K.
//
// Compiled as part of sfx_api.hip (which includes this file), like sfx_fm.hip and sfx_lz.hip.
#pragma once
#include "sfx_host.hpp"

namespace sfx {

constexpr uint32_t kMemTile = 2048;                     // K: pairs per tile = kBlock x 8, one mask byte per thread
constexpr uint32_t kMemKnownFlags = SFX_MEM_UNIQUE;
static_assert(kMemTile == kBlock * 8, "a thread packs the flags of its 8 consecutive slots into one byte");

struct MemGeom {
    uint32_t tile;                                      // in [1, kMemTile]
    bool bisect;                                        // every slot bisects off itself instead of the LDS expansion
};
// test hooks, read at every call: SFX_MEM_TILE=<pairs> in [1, 2048]; SFX_MEM_BISECT=1 (the baseline the expansion was
// measured against, scripts/gpu_mem_time.py)
static MemGeom mem_geom()
{
    MemGeom v{kMemTile, false};
    const char* e = dev_env("SFX_MEM_TILE");
    const int t = e ? atoi(e) : 0;
    if (t >= 1 && t <= (int)kMemTile) v.tile = (uint32_t)t;
    e = dev_env("SFX_MEM_BISECT");
    v.bisect = e && atoi(e) != 0;
    return v;
}

// what the pair kernels read; starts / da / ndocs are read by the collection's instances (DOCS) only
struct MemIn {
    const uint8_t* text;
    uint64_t n;
    const uint32_t* sa;
    const uint64_t* starts;
    const uint32_t* da;
    uint64_t ndocs;
    const uint8_t* q;
    uint64_t m;
    const uint64_t* off;                                // m + 1
    const uint32_t* start;                              // m
    uint32_t L, flags, tile;
    uint64_t pair_limit, ntiles_max;
#ifdef SFX_DEV_HOOKS
    bool bisect;                                        // hooked builds only: the baseline of the comparison in DESIGN.md section 20
#endif
};

__global__ void __launch_bounds__(kBlock)
k_mem_cand(uint32_t* __restrict__ len, const uint32_t* __restrict__ start, const uint32_t* __restrict__ end, uint64_t m, uint32_t L)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += stride)
        len[i] = len[i] == L ? end[i] - start[i] : 0u;
}

// the position whose pairs hold pair k < P: off[i] <= k < off[i + 1]  (off[0] = 0, off[m] = P; <= 32 steps)
__device__ __forceinline__ uint64_t mem_position_of(const uint64_t* __restrict__ off, uint64_t m, uint64_t k)
{
    uint64_t lo = 0, hi = m;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= k) lo = mid; else hi = mid;
    }
    return lo;
}
// pos[j] = the query position of pair t * K + j, for the cnt pairs of tile t.  One lane bisects for the tile's first
// position; the positions behind it that begin inside the tile mark their first slot (positions with pairs have
// distinct offsets, and none but the first reaches slot 0), reading off in chunks of kBlock until it reaches the
// tile's end; a max-scan over the slots then carries the position index forward.  A stretch of positions without
// pairs costs its off reads, a position that covers many tiles one bisection per tile.
__device__ __forceinline__ uint32_t mem_expand(const MemIn& in, uint64_t P, uint64_t t, uint32_t* __restrict__ pos,
                                               uint32_t* __restrict__ part, uint64_t* __restrict__ first)
{
    const uint32_t K = in.tile, per = (K + kBlock - 1) / kBlock;
    const uint64_t k0 = t * K, k1 = dmin<uint64_t>(k0 + K, P);
    const uint32_t cnt = (uint32_t)(k1 - k0);
#ifdef SFX_DEV_HOOKS
    if (in.bisect) {
        for (uint32_t j = threadIdx.x; j < cnt; j += kBlock) pos[j] = (uint32_t)mem_position_of(in.off, in.m, k0 + j);
        __syncthreads();
        return cnt;
    }
#endif
    if (threadIdx.x == 0) *first = mem_position_of(in.off, in.m, k0);
    for (uint32_t j = threadIdx.x; j < K; j += kBlock) pos[j] = 0u;
    __syncthreads();
    const uint64_t i0 = *first;
    if (threadIdx.x == 0) pos[0] = (uint32_t)i0;
    for (uint64_t base = i0 + 1; base < in.m; base += kBlock) {
        const uint64_t i = base + threadIdx.x;
        if (i < in.m) {
            const uint64_t a = in.off[i];
            if (a < k1 && in.off[i + 1] > a) pos[a - k0] = (uint32_t)i;               // (a > k0: i lies behind i0)
        }
        if (in.off[dmin<uint64_t>(base + kBlock, in.m)] >= k1) break;                 // (the same word for every lane)
    }
    __syncthreads();
    const uint32_t s0 = dmin(threadIdx.x * per, K), s1 = dmin(s0 + per, K);
    uint32_t v = 0;
    for (uint32_t s = s0; s < s1; s++) v = dmax(v, pos[s]);
    uint32_t all;
    uint32_t carry = block_scan_max_excl(v, part, all);
    for (uint32_t s = s0; s < s1; s++) {
        carry = dmax(carry, pos[s]);
        pos[s] = carry;
    }
    __syncthreads();
    return cnt;
}
// the bounds of the suffix at rank r: its document's for a collection (the truncated-suffix model), the text's otherwise
template <bool DOCS> __device__ __forceinline__ void mem_bounds(const MemIn& in, uint64_t r, uint64_t* lo, uint64_t* hi)
{
    if (!DOCS) {
        *lo = 0;
        *hi = in.n;
        return;
    }
    const uint64_t d = in.da[r];
    *lo = in.starts[d];
    *hi = d + 1 < in.ndocs ? in.starts[d + 1] : in.n;
}
struct MemPair {
    uint64_t i, r, end;                                 // end = end_i, the end of position i's interval
    uint32_t p;
    uint64_t dlo, dhi;
};
template <bool DOCS> __device__ __forceinline__ MemPair mem_pair(const MemIn& in, uint64_t i, uint64_t k)
{
    MemPair a;
    const uint64_t o = in.off[i];
    a.i = i;
    a.r = in.start[i] + (k - o);
    a.end = in.start[i] + (in.off[i + 1] - o);
    a.p = in.sa[a.r];
    mem_bounds<DOCS>(in, a.r, &a.dlo, &a.dhi);
    return a;
}
__device__ __forceinline__ bool mem_left_maximal(const MemIn& in, const MemPair& a)
{
    return a.i == 0 || a.p == a.dlo || in.q[a.i - 1] != in.text[a.p - 1];
}
// the pair's first L bytes are equal (its rank lies in the interval): from there on, to the ends of Q and of T / the document
__device__ __forceinline__ uint32_t mem_length(const MemIn& in, const MemPair& a)
{
    return (uint32_t)ms_extend(in.q + a.i, in.text + a.p, in.L, dmin<uint64_t>(in.m - a.i, a.dhi - a.p));
}
// Do the ell bytes occur once?  The suffixes that begin with them are a run of ranks around r, so the two neighbours
// decide; one outside [start_i, end_i) shares fewer than L bytes.
template <bool DOCS> __device__ __forceinline__ bool mem_unique(const MemIn& in, const MemPair& a, uint32_t ell)
{
    const uint64_t lo = in.start[a.i];
    for (int side = 0; side < 2; side++) {
        if (side == 0 ? a.r == lo : a.r + 1 >= a.end) continue;
        const uint64_t nb = side == 0 ? a.r - 1 : a.r + 1;
        const uint32_t s = in.sa[nb];
        uint64_t dlo, dhi;
        mem_bounds<DOCS>(in, nb, &dlo, &dhi);
        if (dhi - s >= ell && ms_extend(in.q + a.i, in.text + s, in.L, ell) == ell) return false;
    }
    return true;
}

// Pairs are dealt to lanes striped (pair j of the tile to lane j % kBlock: a run of ranks is read coalesced); the flags
// go through LDS so that a thread packs its 8 consecutive slots into the byte the emit pass reads.
template <bool DOCS> __global__ void __launch_bounds__(kBlock)
k_mem_count(MemIn in, uint32_t* __restrict__ tcnt, uint8_t* __restrict__ mask)
{
    __shared__ uint32_t pos[kMemTile];
    __shared__ uint8_t hit[kMemTile];
    __shared__ uint32_t part[kWavesPerBlock];
    __shared__ uint64_t first;
    const uint64_t P = in.off[in.m];
    const uint32_t K = in.tile, per = (K + kBlock - 1) / kBlock;
    const uint64_t nt = P > in.pair_limit ? 0 : (P + K - 1) / K;
    // the tiles the limit allows for but P does not fill (all of them after a refusal) count nothing: one lane each
    for (uint64_t t = nt + (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < in.ntiles_max; t += (uint64_t)gridDim.x * kBlock) tcnt[t] = 0u;
    for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
        const uint32_t cnt = mem_expand(in, P, t, pos, part, &first);
        for (uint32_t j = threadIdx.x; j < K; j += kBlock) {
            bool ok = false;
            if (j < cnt) {
                const MemPair a = mem_pair<DOCS>(in, pos[j], t * K + j);
                ok = mem_left_maximal(in, a);
                if (ok && (in.flags & SFX_MEM_UNIQUE)) ok = mem_unique<DOCS>(in, a, mem_length(in, a));
            }
            hit[j] = ok ? 1 : 0;
        }
        __syncthreads();
        const uint32_t s0 = dmin(threadIdx.x * per, K), s1 = dmin(s0 + per, K);
        uint32_t bits = 0;
        for (uint32_t s = s0; s < s1; s++) bits |= (uint32_t)hit[s] << (s - s0);
        mask[t * kBlock + threadIdx.x] = (uint8_t)bits;
        uint32_t total;
        block_scan_add_excl<uint32_t>(__popc(bits), part, total);                    // (two barriers: LDS is free again)
        if (threadIdx.x == 0) tcnt[t] = total;
    }
}
template <bool DOCS> __global__ void __launch_bounds__(kBlock)
k_mem_emit(MemIn in, const uint64_t* __restrict__ toff, const uint8_t* __restrict__ mask, uint32_t* __restrict__ qpos,
           uint32_t* __restrict__ tpos, uint32_t* __restrict__ len, uint64_t capacity, uint64_t* __restrict__ result)
{
    __shared__ uint32_t pos[kMemTile];
    __shared__ uint16_t list[kMemTile];
    __shared__ uint32_t part[kWavesPerBlock];
    __shared__ uint64_t first;
    const uint64_t P = in.off[in.m];
    const uint32_t K = in.tile, per = (K + kBlock - 1) / kBlock;
    const uint64_t nt = P > in.pair_limit ? 0 : (P + K - 1) / K;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        result[0] = P;
        result[1] = toff[in.ntiles_max];                                              // (0 after a refusal)
    }
    for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
        const uint64_t o = toff[t];
        if (o >= capacity || toff[t + 1] == o) continue;                              // (uniform)
        mem_expand(in, P, t, pos, part, &first);
        const uint32_t bits = mask[t * kBlock + threadIdx.x];
        uint32_t total;
        uint32_t rank = block_scan_add_excl<uint32_t>(__popc(bits), part, total);
        for (uint32_t b = 0; b < per; b++)
            if (bits >> b & 1u) list[rank++] = (uint16_t)(threadIdx.x * per + b);
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < total && o + j < capacity; j += kBlock) {
            const uint32_t slot = list[j];
            const MemPair a = mem_pair<DOCS>(in, pos[slot], t * K + slot);
            qpos[o + j] = (uint32_t)a.i;
            tpos[o + j] = a.p;
            len[o + j] = mem_length(in, a);
        }
        __syncthreads();
    }
}

// [result 64 u32 | len -> cand m | start m | end m | off m + 1 (u64) | scan partials (u64) | tile counts | tile offsets
//  + total (u64) | one mask byte per thread and tile]
struct MemWs {
    uint32_t *result, *len, *start, *end;
    uint64_t *off, *part;
    uint32_t* tcnt;
    uint64_t* toff;
    uint8_t* mask;
};
struct MemSizer {                                      // ArenaSizer with pointer-returning take
    uint64_t used = 0;
    template <class T> T* take(uint64_t count) { used += (count * sizeof(T) + kArenaAlign - 1) & ~(kArenaAlign - 1); return nullptr; }
};
// tiles the pairs of one call can fill: pair_limit of them, and no more than every position against every rank
static uint64_t mem_tiles(uint64_t m, uint64_t n, uint64_t pair_limit, uint32_t tile)
{
    const uint64_t pairs = dmin(pair_limit, m * dmin<uint64_t>(n, 0xFFFFFFFFull));    // (m <= u32::MAX: no overflow)
    return pairs / tile + (pairs % tile ? 1 : 0);
}
template <class A> static void mem_carve(A& a, uint64_t m, uint64_t ntiles, MemWs* w)
{
    w->result = a.template take<uint32_t>(64);
    w->len = a.template take<uint32_t>(m);
    w->start = a.template take<uint32_t>(m);
    w->end = a.template take<uint32_t>(m);
    w->off = a.template take<uint64_t>(m + 1);
    w->part = a.template take<uint64_t>(kMaxGrid + 64);
    w->tcnt = a.template take<uint32_t>(ntiles);
    w->toff = a.template take<uint64_t>(ntiles + 1);
    w->mask = a.template take<uint8_t>(ntiles * kBlock);
}
uint64_t mems_workspace_bytes(uint64_t m, uint64_t pair_limit)
{
    if (m == 0 || m > 0xFFFFFFFFull || pair_limit == 0) return 0;
    MemSizer z;
    MemWs w;
    mem_carve(z, m, mem_tiles(m, 0xFFFFFFFFull, pair_limit, mem_geom().tile), &w);
    return z.used;
}
// where the candidates come from: dir != nullptr: through the index's directory; starts != nullptr: a collection
struct MemSource {
    const uint8_t* text;
    uint64_t n;
    const uint32_t* sa;
    const uint32_t* dir;
    const uint16_t* lut;
    int bits, k, dbits;
    const uint64_t* starts;
    const uint32_t* da;
    uint64_t ndocs;
};
int mems_dev(const MemSource& s, const uint8_t* d_q, uint64_t m, uint32_t min_len, uint32_t flags, uint64_t pair_limit, uint32_t* d_qpos,
             uint32_t* d_tpos, uint32_t* d_len, uint64_t capacity, uint64_t* pairs_out, uint64_t* count_out, void* ws, uint64_t ws_bytes,
             hipStream_t st)
{
    if (!pairs_out || !count_out || min_len == 0 || pair_limit == 0 || (flags & ~kMemKnownFlags)) return SFX_ERR_ARG;
    *pairs_out = *count_out = 0;
    if (m > 0xFFFFFFFFull || s.n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (capacity && (!d_qpos || !d_tpos || !d_len)) return SFX_ERR_ARG;
    if (m == 0 || s.n == 0 || min_len > dmin(m, s.n)) return SFX_OK;
    if (!d_q || !s.text || !s.sa || (s.starts && (!s.da || s.ndocs == 0))) return SFX_ERR_ARG;
    if (!ws || ws_bytes < mems_workspace_bytes(m, pair_limit)) return SFX_ERR_WORKSPACE;
    const MemGeom g = mem_geom();
    const uint64_t ntiles = mem_tiles(m, s.n, pair_limit, g.tile);                    // (>= 1, and no more than the sizer's)
    Arena a(ws, ws_bytes);
    MemWs w;
    mem_carve(a, m, ntiles, &w);
    if (a.overflow) return SFX_ERR_INTERNAL;
    if (s.starts)
        SFX_TRY(gindex_match_stats_dev(s.text, s.n, s.starts, s.ndocs, s.sa, s.da, d_q, m, min_len, w.len, nullptr, w.start, w.end, st));
    else if (s.dir)
        SFX_TRY(match_stats_dir_dev(s.text, s.n, s.sa, s.dir, s.lut, s.bits, s.k, s.dbits, d_q, m, min_len, w.len, nullptr, w.start, w.end,
                                    st));
    else
        SFX_TRY(match_stats_dev(s.text, s.n, s.sa, d_q, m, min_len, w.len, nullptr, w.start, w.end, st));
    const unsigned cap = dmin<unsigned>(kMaxGrid, grid_cap());
    SFX_LAUNCH("mem_cand", (double)m * 16, k_mem_cand, (unsigned)dmin<uint64_t>((m + kBlock - 1) / kBlock, cap), kBlock, st, w.len,
               (const uint32_t*)w.start, (const uint32_t*)w.end, m, min_len);
    SFX_TRY(scan_u32_to_u64_excl_dev(w.len, m, w.off, w.part, st));
    MemIn in = {s.text, s.n, s.sa, s.starts, s.da, s.ndocs, d_q, m, w.off, w.start, min_len, flags, g.tile, pair_limit, ntiles};
#ifdef SFX_DEV_HOOKS
    in.bisect = g.bisect;
#endif
    const unsigned grid = (unsigned)dmin<uint64_t>(ntiles, cap);
    // P stays on the device, so the host has no byte estimate for the two pair kernels: they report 0 algorithmic bytes
    // (no bandwidth column in the profile; DESIGN.md section 20 has the bytes per pair and per match)
    if (s.starts)
        SFX_LAUNCH("mem_count", 0.0, k_mem_count<true>, grid, kBlock, st, in, w.tcnt, w.mask);
    else
        SFX_LAUNCH("mem_count", 0.0, k_mem_count<false>, grid, kBlock, st, in, w.tcnt, w.mask);
    SFX_TRY(scan_u32_to_u64_excl_dev(w.tcnt, ntiles, w.toff, w.part, st));
    if (s.starts)
        SFX_LAUNCH("mem_emit", 0.0, k_mem_emit<true>, grid, kBlock, st, in, (const uint64_t*)w.toff, (const uint8_t*)w.mask, d_qpos,
                   d_tpos, d_len, capacity, reinterpret_cast<uint64_t*>(w.result));
    else
        SFX_LAUNCH("mem_emit", 0.0, k_mem_emit<false>, grid, kBlock, st, in, (const uint64_t*)w.toff, (const uint8_t*)w.mask, d_qpos,
                   d_tpos, d_len, capacity, reinterpret_cast<uint64_t*>(w.result));
    uint32_t back[4] = {0, 0, 0, 0};                                                  // P, Z: one read-back
    SFX_TRY(read_back(back, w.result, sizeof(back), st));
    *pairs_out = (uint64_t)back[1] << 32 | back[0];
    *count_out = *pairs_out > pair_limit ? 0 : (uint64_t)back[3] << 32 | back[2];
    return SFX_OK;
}

}  // namespace sfx
