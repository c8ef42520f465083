// sfx_lz.hip -- greedy LZ77 factorization from the longest-previous-factor array, and its decoder
// (include/suffix_hip.h).
//
// rep / src are what sfx_repeat_lens_dev(SFX_REP_EARLIER) writes.  r(p) = min(rep[p], n - p); step(p) = r(p) if
// r(p) >= min_len, else 1; next(p) = p + step(p).  The phrases are the chain 0, next(0), next(next(0)), ... below n.
// next(p) > p for every input, so every chain ends; nothing else is assumed of it (it is monotone only for a true LPF
// array at min_len = 1).
//
// Parse: the chain's members are found without one lane walking it.
//   lz_exit         per tile of B positions: next() in LDS, pointer jumping inside the tile, exit1[p] = the first chain
//                   position at or beyond the tile's end reached from p
//   lz_hop x K      level k pairs groups of 2^k tiles: the left half follows its exit once more (G[p] = G[G[p]] when
//                   G[p] is still inside the pair); afterwards G[p] leaves p's group of 2^K tiles
//   lz_walk_groups  one lane follows G from 0: the entry of every group the chain enters (<= n / (B << K) steps)
//   lz_walk_tiles   one lane per entered group follows exit1: the entry of every tile the chain enters (<= 2^K steps)
//   lz_count        one lane per entered tile follows next() and counts its phrases (<= B steps)
//   scan            the three-phase exclusive scan of sfx_tree.hip over the tile counts
//   lz_emit         the same walk again, writing the phrases at their offsets, below `capacity` only
// Decode: begin = the exclusive sum of len (64-bit, so that unchecked lengths cannot wrap), the phrase list is checked
// and refused before anything is written; every position gets its origin org[i] = src[k] + i - begin[k] < i (a literal
// is its own origin and writes its byte); pointer jumping org[i] = org[org[i]] takes every position to the literal its
// byte comes from in <= 32 rounds; one last pass copies the bytes.  The rounds touch org alone, never the output.
//
// Compiled as part of sfx_api.hip (which includes this file), so that every build of the C ABI -- the product's and the
// emulator's of tests/emu -- carries it without a source list of its own.
#pragma once
#include "sfx_host.hpp"

namespace sfx {

constexpr uint32_t kLzTile = 4096;                      // B: positions per tile = SFX_LZ_MAX_STEPS
constexpr uint32_t kLzLevels = 8;                       // K: a group is 2^K tiles = 2^20 positions
constexpr uint32_t kLzNone = 0xFFFFFFFFu;
constexpr int kLzDecodeRounds = 33;                     // copy chains are < 2^32 deep: 32 doublings and one to see it
static_assert(kLzTile == SFX_LZ_MAX_STEPS, "a tile walk is the longest dependent walk of a lane");
static_assert((1u << kLzLevels) <= SFX_LZ_MAX_STEPS, "a group walk visits at most 2^K tiles");
static_assert((0xFFFFFFFFull >> 20) < SFX_LZ_MAX_STEPS && kLzTile << kLzLevels == 1u << 20, "groups of a text below 2^32");

struct LzGeom {
    uint32_t tile, levels;                              // tile: a power of two in [4, kLzTile]
};
// test hooks: SFX_LZ_TILE=<positions> (a power of two in [4, 4096]) and SFX_LZ_LEVELS=<K> (0 .. 16), read once
static LzGeom lz_geom()
{
    static const LzGeom g = [] {
        LzGeom v{kLzTile, kLzLevels};
        const char* e = dev_env("SFX_LZ_TILE");
        const int t = e ? atoi(e) : 0;
        if (t >= 4 && t <= (int)kLzTile && (t & (t - 1)) == 0) v.tile = (uint32_t)t;
        e = dev_env("SFX_LZ_LEVELS");
        const int k = e ? atoi(e) : -1;
        if (k >= 0 && k <= 16) v.levels = (uint32_t)k;
        return v;
    }();
    return g;
}
static bool lz_rounds_check()
{
    static const bool v = [] { const char* e = dev_env("SFX_LZ_ROUNDS_CHECK"); return e && atoi(e) != 0; }();
    return v;
}

// step(p) for p < n; *bad is raised for an entry that reaches past the text (it is clipped either way)
__device__ __forceinline__ uint32_t lz_step(const uint32_t* __restrict__ rep, uint64_t p, uint64_t n, uint32_t min_len, bool* copy)
{
    const uint32_t r = (uint32_t)dmin<uint64_t>(rep[p], n - p);
    *copy = r >= min_len;                               // (min_len >= 1: a copy has r >= 1)
    return *copy ? r : 1u;
}

// ---- parse --------------------------------------------------------------------------------------------------
// One workgroup per tile.  e[i] starts as next(tb + i); a round replaces a pointer that is still inside the tile by
// its target's pointer.  Pointers only ever move forward along the chain of their position, so a lane that reads a
// neighbour another lane has already updated in the same round only gets further; after round k every pointer is at
// least 2^k links on or out of the tile, and a tile holds at most `tile` links.
__global__ void __launch_bounds__(kBlock)
k_lz_exit(const uint32_t* __restrict__ rep, uint64_t n, uint32_t min_len, uint32_t tile, uint32_t log_tile, uint64_t ntiles,
          uint32_t* __restrict__ exit1, uint32_t* __restrict__ G, uint32_t* __restrict__ flags)
{
    __shared__ uint32_t e[kLzTile];
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t tb = t * tile, tend = dmin<uint64_t>(tb + tile, n);
        const uint32_t cnt = (uint32_t)(tend - tb);
        bool bad = false;
        for (uint32_t i = threadIdx.x; i < cnt; i += kBlock) {
            const uint64_t p = tb + i;
            bool copy;
            e[i] = (uint32_t)(p + lz_step(rep, p, n, min_len, &copy));          // (<= n < 2^32)
            bad |= rep[p] > n - p;
        }
        if (bad) flags[0] = 1u;
        __syncthreads();
        for (uint32_t round = 0; round < log_tile; round++) {
            for (uint32_t i = threadIdx.x; i < cnt; i += kBlock) {
                const uint32_t v = e[i];
                if (v < tend) e[i] = e[v - (uint32_t)tb];
            }
            __syncthreads();
        }
        for (uint32_t i = threadIdx.x; i < cnt; i += kBlock) {
            const uint32_t v = e[i];
            exit1[tb + i] = v;
            G[tb + i] = v;
        }
        __syncthreads();
    }
}
// Level `hs - log_tile`: half = 1 << hs positions.  Item i is the i-th position that lies in the left half of its pair.
// A left position whose pointer is still inside the pair points into the right half, which no lane writes at this
// level: in place without a race.
__global__ void __launch_bounds__(kBlock)
k_lz_hop(uint32_t* __restrict__ G, uint64_t n, uint32_t hs)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock, low = (1ull << hs) - 1;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;; i += stride) {
        const uint64_t p = ((i >> hs) << (hs + 1)) | (i & low);
        if (p >= n) break;                                                        // (p grows with i)
        const uint64_t gend = dmin<uint64_t>(((p >> (hs + 1)) + 1) << (hs + 1), n);
        const uint32_t q = G[p];
        if (q < gend) G[p] = G[q];
    }
}
__global__ void __launch_bounds__(kWave)
k_lz_walk_groups(const uint32_t* __restrict__ G, uint64_t n, uint32_t gs, uint32_t* __restrict__ group_entry)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (uint64_t p = 0; p < n; p = G[p]) group_entry[p >> gs] = (uint32_t)p;      // (G[p] >= the end of p's group)
}
__global__ void __launch_bounds__(kBlock)
k_lz_walk_tiles(const uint32_t* __restrict__ exit1, uint64_t n, uint32_t gs, uint32_t log_tile, uint64_t ngroups,
                const uint32_t* __restrict__ group_entry, uint32_t* __restrict__ tile_entry)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < ngroups; g += stride) {
        uint64_t p = group_entry[g];
        if (p == kLzNone) continue;
        const uint64_t gend = dmin<uint64_t>((g + 1) << gs, n);
        for (; p < gend; p = exit1[p]) tile_entry[p >> log_tile] = (uint32_t)p;   // (exit1[p] >= the end of p's tile)
    }
}
// One lane per tile the chain enters.  EMIT = false: the number of phrases that begin in the tile.  EMIT = true: the
// phrases themselves from offset off[t] on; flags[1] is raised for a copy that does not point backwards; the lane of tile 0
// leaves the total where the read-back finds it.
template <bool EMIT>
__device__ __forceinline__ void
lz_tile_walk(const uint32_t* __restrict__ rep, const uint32_t* __restrict__ src, const uint8_t* __restrict__ text, uint64_t n,
               uint32_t min_len, uint32_t log_tile, uint64_t ntiles, const uint32_t* __restrict__ tile_entry, uint32_t* __restrict__ off,
               uint32_t* __restrict__ begin, uint32_t* __restrict__ len, uint32_t* __restrict__ psrc, uint8_t* __restrict__ lit,
               uint64_t capacity, uint32_t* __restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < ntiles; t += stride) {
        if (EMIT && t == 0) flags[2] = off[ntiles];
        uint64_t p = tile_entry[t];
        const uint64_t tend = dmin<uint64_t>((t + 1) << log_tile, n);
        if (p == kLzNone) p = tend;
        uint64_t k = EMIT ? off[t] : 0;
        bool bad = false;
        while (p < tend) {
            bool copy;
            const uint32_t s = lz_step(rep, p, n, min_len, &copy);
            if (EMIT && k < capacity) {
                const uint32_t from = copy ? src[p] : kLzNone;
                bad |= copy && from >= p;
                if (begin) begin[k] = (uint32_t)p;
                len[k] = s;
                psrc[k] = from;
                if (text) lit[k] = copy ? (uint8_t)0 : text[p];
            } else if (EMIT && copy) {
                bad |= src[p] >= p;
            }
            k++;
            p += s;
        }
        if (!EMIT) off[t] = (uint32_t)k;
        if (EMIT && bad) flags[1] = 1u;
    }
}
__global__ void __launch_bounds__(kBlock)
k_lz_count(const uint32_t* __restrict__ rep, uint64_t n, uint32_t min_len, uint32_t log_tile, uint64_t ntiles,
           const uint32_t* __restrict__ tile_entry, uint32_t* __restrict__ off)
{
    lz_tile_walk<false>(rep, nullptr, nullptr, n, min_len, log_tile, ntiles, tile_entry, off, nullptr, nullptr, nullptr, nullptr, 0, nullptr);
}
__global__ void __launch_bounds__(kBlock)
k_lz_emit(const uint32_t* __restrict__ rep, const uint32_t* __restrict__ src, const uint8_t* __restrict__ text, uint64_t n,
          uint32_t min_len, uint32_t log_tile, uint64_t ntiles, const uint32_t* __restrict__ tile_entry, uint32_t* __restrict__ off,
          uint32_t* __restrict__ begin, uint32_t* __restrict__ len, uint32_t* __restrict__ psrc, uint8_t* __restrict__ lit,
          uint64_t capacity, uint32_t* __restrict__ flags)
{
    lz_tile_walk<true>(rep, src, text, n, min_len, log_tile, ntiles, tile_entry, off, begin, len, psrc, lit, capacity, flags);
}

// [flags 64 | exit1 n | G n | group entries | tile entries | tile counts / offsets + total | scan partials]
struct LzParseWs {
    uint32_t *flags, *exit1, *G, *group_entry, *tile_entry, *off, *part;
};
template <class A> static void lz_parse_carve(A& a, uint64_t n, const LzGeom& g, LzParseWs* w)
{
    const uint64_t ntiles = (n + g.tile - 1) / g.tile, ngroups = (ntiles + (1ull << g.levels) - 1) >> g.levels;
    w->flags = a.template take<uint32_t>(64);
    w->exit1 = a.template take<uint32_t>(n);
    w->G = a.template take<uint32_t>(n);
    w->group_entry = a.template take<uint32_t>(ngroups);
    w->tile_entry = a.template take<uint32_t>(ntiles);
    w->off = a.template take<uint32_t>(ntiles + 1);
    w->part = a.template take<uint32_t>(kMaxGrid + 64);
}
struct LzSizer {                                   // ArenaSizer with pointer-returning take
    uint64_t used = 0;
    template <class T> T* take(uint64_t count) { used += (count * sizeof(T) + kArenaAlign - 1) & ~(kArenaAlign - 1); return nullptr; }
};
uint64_t lz_parse_workspace_bytes(uint64_t n)
{
    if (n == 0 || n > 0xFFFFFFFFull) return 0;
    LzSizer z;
    LzParseWs w;
    lz_parse_carve(z, n, lz_geom(), &w);
    return z.used;
}
static uint32_t lz_log2(uint32_t v)
{
    uint32_t l = 0;
    while ((1u << l) < v) l++;
    return l;
}
int lz_parse_dev(const uint32_t* d_rep, const uint32_t* d_src, const uint8_t* d_text, uint64_t n, uint32_t min_len, uint32_t* d_begin,
                 uint32_t* d_len, uint32_t* d_psrc, uint8_t* d_lit, uint64_t capacity, uint64_t* count_out, void* ws, uint64_t ws_bytes,
                 hipStream_t st)
{
    if (!count_out || min_len == 0) return SFX_ERR_ARG;
    *count_out = 0;
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!d_rep || !d_src || (capacity && (!d_len || !d_psrc || (d_text && !d_lit)))) return SFX_ERR_ARG;
    if (!ws || ws_bytes < lz_parse_workspace_bytes(n)) return SFX_ERR_WORKSPACE;
    const LzGeom g = lz_geom();
    Arena a(ws, ws_bytes);
    LzParseWs w;
    lz_parse_carve(a, n, g, &w);
    if (a.overflow) return SFX_ERR_INTERNAL;
    const uint32_t log_tile = lz_log2(g.tile), gs = log_tile + g.levels;
    const uint64_t ntiles = (n + g.tile - 1) / g.tile, ngroups = (ntiles + (1ull << g.levels) - 1) >> g.levels;
    SFX_HIP(hipMemsetAsync(w.flags, 0, 64 * sizeof(uint32_t), st));
    SFX_HIP(hipMemsetAsync(w.group_entry, 0xFF, ngroups * sizeof(uint32_t), st));
    SFX_HIP(hipMemsetAsync(w.tile_entry, 0xFF, ntiles * sizeof(uint32_t), st));
    const unsigned cap = dmin<unsigned>(kMaxGrid, grid_cap());
    SFX_LAUNCH("lz_exit", (double)n * 12, k_lz_exit, (unsigned)dmin<uint64_t>(ntiles, cap), kBlock, st, d_rep, n, min_len, g.tile, log_tile,
               ntiles, w.exit1, w.G, w.flags);
    for (uint32_t k = 0; k < g.levels && ((uint64_t)g.tile << k) < n; k++) {          // (a pair with an empty right half has nothing to do)
        const unsigned grid = (unsigned)dmin<uint64_t>((n / 2 + kBlock) / kBlock, cap);
        SFX_LAUNCH("lz_hop", (double)n * 6, k_lz_hop, grid, kBlock, st, w.G, n, log_tile + k);
    }
    SFX_LAUNCH("lz_walk_groups", (double)ngroups * 8, k_lz_walk_groups, 1, kWave, st, (const uint32_t*)w.G, n, gs, w.group_entry);
    SFX_LAUNCH("lz_walk_tiles", (double)ntiles * 8, k_lz_walk_tiles, (unsigned)dmin<uint64_t>((ngroups + kBlock - 1) / kBlock, cap), kBlock, st,
               (const uint32_t*)w.exit1, n, gs, log_tile, ngroups, (const uint32_t*)w.group_entry, w.tile_entry);
    const unsigned tgrid = (unsigned)dmin<uint64_t>((ntiles + kBlock - 1) / kBlock, cap);
    SFX_LAUNCH("lz_count", (double)n * 4, k_lz_count, tgrid, kBlock, st, d_rep, n, min_len, log_tile, ntiles, (const uint32_t*)w.tile_entry,
               w.off);
    SFX_TRY(scan_u32_excl_dev(w.off, ntiles, w.off, w.part, st));
    SFX_LAUNCH("lz_emit", (double)n * 8, k_lz_emit, tgrid, kBlock, st, d_rep, d_src, d_text, n, min_len, log_tile, ntiles,
               (const uint32_t*)w.tile_entry, w.off, d_begin, d_len, d_psrc, d_lit, capacity, w.flags);
    uint32_t back[4] = {0, 0, 0, 0};                                                  // bad rep, bad src, z: one read-back
    SFX_TRY(read_back(back, w.flags, sizeof(back), st));
    if (back[0] || back[1]) return SFX_ERR_ARG;
    *count_out = back[2];
    return SFX_OK;
}

// ---- decode -------------------------------------------------------------------------------------------------
// flags[0]: len == 0; [1]: a literal whose len is not 1; [2]: a copy with src >= begin; [3]: the lengths do not sum to n
__global__ void __launch_bounds__(kBlock)
k_lz_unscan_check(const uint32_t* __restrict__ len, const uint32_t* __restrict__ psrc, const uint64_t* __restrict__ begin, uint64_t z,
               uint64_t n, uint32_t* __restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < z; k += stride) {
        const uint32_t l = len[k], s = psrc[k];
        if (l == 0) flags[0] = 1u;
        if (s == kLzNone) {
            if (l != 1) flags[1] = 1u;
        } else if (s >= begin[k]) {
            flags[2] = 1u;
        }
        if (k == 0 && begin[z] != n) flags[3] = 1u;
    }
}
// One lane per position: the phrase it lies in by bisection of begin (begin[0] = 0 <= i < n = begin[z], lengths > 0),
// then its origin.  Work is dealt per position because one phrase may be anything from 1 to n - 1 bytes.
__global__ void __launch_bounds__(kBlock)
k_lz_unorigin(const uint32_t* __restrict__ psrc, const uint8_t* __restrict__ lit, const uint64_t* __restrict__ begin, uint64_t z,
                uint64_t n, uint32_t* __restrict__ org, uint8_t* __restrict__ out)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        uint64_t lo = 0, hi = z;                                        // begin[lo] <= i < begin[hi]
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (begin[mid] <= i) lo = mid; else hi = mid;
        }
        const uint32_t s = psrc[lo];
        if (s == kLzNone) {
            out[i] = lit[lo];
            org[i] = (uint32_t)i;
        } else {
            org[i] = (uint32_t)(s + (i - begin[lo]));                   // (< i: the list was checked)
        }
    }
}
// org[i] = org[org[i]] until it reaches a literal (its own origin).  Origins strictly decrease along a chain and
// every value org[t] ever held lies on t's chain towards that literal, so a lane that reads a neighbour's value of
// this round, of the round before or a cached older one still gets a position on its own chain: only progress can
// vary, and a launch boundary makes every round at least double what the round before it had reached.
__global__ void __launch_bounds__(kBlock)
k_lz_unjump(uint32_t* __restrict__ org, uint64_t n, uint32_t* __restrict__ left)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    bool any = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const uint32_t t = org[i];
        if (t == i) continue;
        const uint32_t tt = org[t];
        if (tt != t) {
            org[i] = tt;
            any = true;
        }
    }
    if (any) *left = 1u;
}
__global__ void __launch_bounds__(kBlock)
k_lz_unfill(const uint32_t* __restrict__ org, uint64_t n, uint8_t* out)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const uint32_t t = org[i];
        if (t != i) out[i] = out[t];                                    // (out[t]: a literal's byte, written a launch ago, never here)
    }
}

// [flags 64: 4 check words, then one "anything left" word per round | begin z + 1 (u64) | scan partials (u64) | org n]
struct LzDecodeWs {
    uint32_t* flags;
    uint64_t *begin, *part;
    uint32_t* org;
};
template <class A> static void lz_decode_carve(A& a, uint64_t n, uint64_t z, LzDecodeWs* w)
{
    w->flags = a.template take<uint32_t>(64);
    w->begin = a.template take<uint64_t>(z + 1);
    w->part = a.template take<uint64_t>(kMaxGrid + 64);
    w->org = a.template take<uint32_t>(n);
}
uint64_t lz_decode_workspace_bytes(uint64_t n, uint64_t z)
{
    if (n == 0 || n > 0xFFFFFFFFull || z > 0xFFFFFFFFull) return 0;
    LzSizer s;
    LzDecodeWs w;
    lz_decode_carve(s, n, z, &w);
    return s.used;
}
static bool lz_overlap(const void* a, uint64_t abytes, const void* b, uint64_t bbytes)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && abytes && bbytes && x < y + bbytes && y < x + abytes;
}
int lz_decode_dev(const uint32_t* d_len, const uint32_t* d_psrc, const uint8_t* d_lit, uint64_t z, uint64_t n, uint8_t* d_out, void* ws,
                  uint64_t ws_bytes, hipStream_t st)
{
    if (n > 0xFFFFFFFFull || z > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return z == 0 ? SFX_OK : SFX_ERR_ARG;
    if (z == 0 || z > n || !d_len || !d_psrc || !d_lit || !d_out) return SFX_ERR_ARG;
    if (lz_overlap(d_out, n, d_len, z * 4) || lz_overlap(d_out, n, d_psrc, z * 4) || lz_overlap(d_out, n, d_lit, z)) return SFX_ERR_ARG;
    if (!ws || ws_bytes < lz_decode_workspace_bytes(n, z)) return SFX_ERR_WORKSPACE;
    Arena a(ws, ws_bytes);
    LzDecodeWs w;
    lz_decode_carve(a, n, z, &w);
    if (a.overflow) return SFX_ERR_INTERNAL;
    SFX_HIP(hipMemsetAsync(w.flags, 0, 64 * sizeof(uint32_t), st));
    SFX_TRY(scan_u32_to_u64_excl_dev(d_len, z, w.begin, w.part, st));
    const unsigned zgrid = (unsigned)dmin<uint64_t>((z + kBlock - 1) / kBlock, kMaxGrid);
    SFX_LAUNCH("unlz_scan", (double)z * 16, k_lz_unscan_check, zgrid, kBlock, st, d_len, d_psrc, (const uint64_t*)w.begin, z, n, w.flags);
    uint32_t bad[4] = {0, 0, 0, 0};
    SFX_TRY(read_back(bad, w.flags, sizeof(bad), st));
    if (bad[0] || bad[1] || bad[2] || bad[3]) return SFX_ERR_ARG;                  // (nothing has been written to d_out)
    const unsigned grid = (unsigned)dmin<uint64_t>((n + kBlock - 1) / kBlock, kMaxGrid);
    SFX_LAUNCH("unlz_origin", (double)n * 5, k_lz_unorigin, grid, kBlock, st, d_psrc, d_lit, (const uint64_t*)w.begin, z, n, w.org, d_out);
    const int every = lz_rounds_check() ? 1 : 4;
    bool done = false;
    for (int r = 0; r < kLzDecodeRounds && !done; r++) {
        SFX_LAUNCH("unlz_jump", (double)n * 12, k_lz_unjump, grid, kBlock, st, w.org, n, w.flags + 4 + r);
        if ((r + 1) % every == 0 || r + 1 == kLzDecodeRounds) {
            uint32_t left = 0;
            SFX_TRY(read_back(&left, w.flags + 4 + r, sizeof(left), st));
            done = left == 0;
        }
    }
    if (!done) return SFX_ERR_INTERNAL;                                            // (no checked list is 2^32 deep)
    SFX_LAUNCH("unlz_fill", (double)n * 6, k_lz_unfill, grid, kBlock, st, (const uint32_t*)w.org, n, d_out);
    return SFX_OK;
}

}  // namespace sfx
