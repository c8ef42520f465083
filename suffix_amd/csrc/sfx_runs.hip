// sfx_runs.hip -- the maximal repetitions (runs) of a plain text, its Lyndon arrays and through them its tandem repeats, from
// SA + LCP (include/suffix_hip.h).  After Bannai, I, Inenaga, Nakashima, Takeda, Tsuruta, "The runs
// theorem" (2017): every run (b, e, p) holds, under one of the two byte orders, a Lyndon word of length p that is the longest
// Lyndon word starting at its position -- so the candidates are the pairs (i, lyn_o[i]), 2n of them, and each is settled by
// longest common extensions to the right and to the left.
//
//   lyn_o[i] = nss_o(i) - i, nss_o(i) = the least j > i with isa_o[j] < isa_o[i], or n.  isa_1 is the inverse table of the
//   complemented text (byte -> 255 - byte): in both orders a proper prefix is smaller than its extension.
//
//   runs_complement      the text under order 1
//   (the SA build)       its table; no LCP
//   runs_check / runs_scatter / runs_verify   the inverse tables (the kernels of sfx_lce.hip: the caller's table is proven a
//                        permutation, ours is only scattered)
//   runs_levels          F-ary min-trees (k_lce_levels): over the caller's LCP array for the extensions, over each inverse
//                        table for the next-smaller walks that leave a tile
//   runs_lyndon_tile     a workgroup stages a tile of 2048 inverse-table words in LDS under a binary min-tree and answers
//                        next-smaller inside the tile with <= 2 log2 2048 LDS reads; positions whose answer leaves the tile
//                        are listed (one reservation per 256 positions); what does not fit the list is finished right there
//   runs_lyndon_open     the listed positions, one per lane, through the global min-tree: up from the tile's end to the first
//                        node whose minimum is smaller, down to its first such leaf -- at most 2 F words per level
//   runs_candidates      per (order, position): r = LCE(i, i + p); the left extension has to reach need = p - r, which one
//                        more LCE at distance need decides.  Survivors keep r; per workgroup one count word
//   runs_offsets         one workgroup: the scan of those words
//   runs_compact         the survivors, dense and in position order (wave ballot + the workgroup's offset)
//   runs_extend          l = the largest k <= min(i, p) with LCE(i - k, i + p - k) >= k (monotone in k): doubling from need,
//                        then bisection.  Accepted iff l < p and (order 0 or e < n) -- every run exactly once -- and the filters
//                        hold; (b << 32 | p, e) per survivor, one count word per workgroup
//   runs_gather          the accepted triples, dense
//   --- the one read-back: (count, flags).  What follows is queued behind it and sized by it ---
//   (radix_sort_kv64)    ascending by (b, p)
//   runs_write           the first min(count, capacity) triples
// lcp is not verified: no address is formed from it, every extension is clamped to the room left, and l <= i, so every triple
// has 0 <= b < e <= n and 2p <= e - b whatever lcp holds.
//
// Compiled as part of sfx_api.hip (which includes this file after sfx_lce.hip).
#pragma once
#include "sfx_host.hpp"
#include "sfx_lce.hip"

namespace sfx {

constexpr uint32_t kRunsTile = 2048;                     // inverse-table words per Lyndon tile (a power of two)
constexpr unsigned kRunsResWords = 64;                   // [0,1] count  [2,3] the count before the last gather  [4] a bad table
constexpr unsigned kRunsResZ = 0, kRunsResBase = 2, kRunsResFlags = 4, kRunsResOpen = 6;   // entry [5] an empty slot [6] listed positions
constexpr unsigned kRunsResSurvive = 8, kRunsResAccept = 10;   // [8], [9] survivors of the first extension per order; [10], [11] accepted per order
constexpr uint64_t kRunsNoKey = ~0ull;
constexpr uint64_t kRunsMaxN = 0xFFFFFFFEull;            // n < 2^32 - 1: n itself and the empty mark stay apart

// test hooks, read at every call: SFX_RUNS_TILE=<64 .. 2048, a power of two>, SFX_RUNS_LIST=<entries the open list holds>
static uint32_t runs_tile_hook()
{
    const char* e = dev_env("SFX_RUNS_TILE");
    const long v = e ? atol(e) : 0;
    for (uint32_t t = 64; t <= kRunsTile; t <<= 1)
        if (v == (long)t) return t;
    return kRunsTile;
}
static uint64_t runs_list_hook(uint64_t n)
{
    const char* e = dev_env("SFX_RUNS_LIST");
    if (!e) return n;
    const long long v = atoll(e);
    return v < 0 ? n : dmin<uint64_t>((uint64_t)v, n);
}

// ---- Lyndon array: all next smaller values of an inverse table ------------------------------------------------------------
// the F-ary min-tree over isa, laid out as the LCE index lays out its levels (lce_layout)
struct RunsTree {
    const uint32_t* isa;
    const uint32_t* tree;
    uint64_t n;
    int fan_log, levels;
};
// the least j >= start with isa[j] < v, or n.  Up: the rest of start's node, then its parent's right siblings, ...; the top
// level is scanned to its end.  Down: the first child below v.  At most 2 F reads per level on any input.
__device__ __forceinline__ uint64_t runs_nss_walk(const RunsTree& t, uint64_t start, uint32_t v)
{
    const int f = t.fan_log;
    const uint64_t mask = (1ull << f) - 1;
    const uint32_t* L = t.isa;
    uint64_t p = start, cnt = t.n;
    int k = 0;
    bool found = false;
    for (;;) {
        if (p >= cnt) return t.n;
        const bool top = k == t.levels - 1;
        if (top || (p & mask)) {
            const uint64_t e = top ? cnt : dmin(cnt, (p | mask) + 1);
            for (; p < e; p++)
                if (L[p] < v) { found = true; break; }
            if (found) break;
            if (top || p >= cnt) return t.n;
        }
        p >>= f;
        L = k == 0 ? t.tree : L + lce_line_up(cnt);
        cnt = (cnt + mask) >> f;
        k++;
    }
    while (k > 0) {
        k--;
        const uint64_t below = (t.n + (1ull << (f * k)) - 1) >> (f * k);       // the words of level k
        L = k == 0 ? t.isa : L - lce_line_up(below);
        const uint64_t b = p << f, e = dmin(below, b + mask + 1);
        uint64_t q = b;
        while (q < e && L[q] >= v) q++;
        if (q >= e) return t.n;                                                // (a node without its minimum: not a tree of ours)
        p = q;
    }
    return p;
}
// the first index > j of the tile with a value < v, or T.  tr: the binary min-tree, level k (T >> k words) behind level k - 1
__device__ __forceinline__ uint32_t runs_tile_nss(const uint32_t* tr, uint32_t T, uint32_t j, uint32_t v)
{
    uint32_t idx = j, off = 0, cnt = T;
    bool found = false;
    while (cnt > 1) {
        if (!(idx & 1u) && tr[off + idx + 1] < v) { idx++; found = true; break; }
        idx >>= 1;
        off += cnt;
        cnt >>= 1;
    }
    if (!found) return T;
    while (off > 0) {
        cnt <<= 1;
        off -= cnt;
        idx <<= 1;
        if (tr[off + idx] >= v) idx++;
    }
    return idx;
}
__global__ void __launch_bounds__(kBlock)
k_runs_lyndon_tile(RunsTree t, uint32_t T, uint32_t* __restrict__ lyn, uint32_t* __restrict__ list, uint64_t list_cap, uint32_t* __restrict__ open_count)
{
    __shared__ uint32_t tr[2 * kRunsTile];
    __shared__ uint32_t part[kWavesPerBlock];
    __shared__ uint32_t slot0;
    const uint64_t n = t.n, ntiles = (n + T - 1) / T;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t g0 = tile * T;
        for (uint32_t j = threadIdx.x; j < T; j += kBlock) tr[j] = g0 + j < n ? t.isa[g0 + j] : kLceNone;
        __syncthreads();
        for (uint32_t off = 0, cnt = T; cnt > 1; off += cnt, cnt >>= 1) {
            for (uint32_t j = threadIdx.x; j < cnt / 2; j += kBlock) tr[off + cnt + j] = dmin(tr[off + 2 * j], tr[off + 2 * j + 1]);
            __syncthreads();
        }
        const bool last = g0 + T >= n;                                   // nothing lies behind the last tile: the answer is n
        for (uint32_t base = 0; base < T; base += kBlock) {
            const uint32_t j = base + threadIdx.x;
            const uint64_t g = g0 + j;
            bool open = false;
            uint32_t v = 0;
            if (j < T && g < n) {
                v = tr[j];
                const uint32_t q = runs_tile_nss(tr, T, j, v);
                if (q < T) lyn[g] = q - j;
                else if (last) lyn[g] = (uint32_t)(n - g);
                else open = true;
            }
            const unsigned long long b = __ballot(open);
            const uint32_t below = lanes_below(b);
            if (lane_id() == 0) part[wave_id()] = (uint32_t)__popcll(b);
            __syncthreads();
            uint32_t rank = below, total = 0;
            for (unsigned w = 0; w < (unsigned)kWavesPerBlock; w++) {
                if (w < wave_id()) rank += part[w];
                total += part[w];
            }
            if (threadIdx.x == 0 && total) slot0 = atomicAdd(open_count, total);
            __syncthreads();
            if (open) {
                const uint64_t slot = (uint64_t)slot0 + rank;
                if (slot < list_cap) list[slot] = (uint32_t)g;
                else lyn[g] = (uint32_t)(runs_nss_walk(t, g0 + T, v) - g);   // the list is full: finished here
            }
        }
        __syncthreads();
    }
}
__global__ void __launch_bounds__(kBlock)
k_runs_lyndon_open(RunsTree t, uint32_t T, uint32_t* __restrict__ lyn, const uint32_t* __restrict__ list, uint64_t list_cap,
                   const uint32_t* __restrict__ open_count)
{
    const uint64_t m = dmin<uint64_t>(*open_count, list_cap), stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < m; q += stride) {
        const uint64_t g = list[q];
        if (g >= t.n) continue;                                          // (never: the list is ours)
        lyn[g] = (uint32_t)(runs_nss_walk(t, (g / T + 1) * T, t.isa[g]) - g);
    }
}

// ---- candidates -----------------------------------------------------------------------------------------------------------
struct RunsFilter { uint32_t min_period, max_period, min_len; };
// LCE(i, j) over the caller's tables, i, j <= n.  A rank >= n (a table that is not a permutation: the call fails) reads nothing
__device__ __forceinline__ uint32_t runs_lce(const LceView& v, uint32_t i, uint32_t j)
{
    LceState s = lce_begin(v, i, j);
    while (!s.done) {
        uint32_t lo, hi;
        lce_round_ranks(v, s, &lo, &hi);
        lce_advance(s, lo == hi ? kLceNone : hi >= v.n ? 0u : lce_range_min<kLceShipped>(v, (uint64_t)lo + 1, (uint64_t)hi + 1), 0);
    }
    return (uint32_t)s.len;
}
// the items of workgroup b: [*lo, *hi) of N, whole steps of kBlock
__device__ __forceinline__ void runs_chunk(uint64_t N, uint64_t* lo, uint64_t* hi)
{
    const uint64_t steps = (N + kBlock - 1) / kBlock, per = (steps + gridDim.x - 1) / gridDim.x;
    *lo = dmin(N, (uint64_t)blockIdx.x * per * kBlock);
    *hi = dmin(N, *lo + per * kBlock);
}
__device__ __forceinline__ void runs_block_sum(unsigned long long mine, unsigned long long* sums, unsigned long long* out)
{
    for (int d = 32; d >= 1; d >>= 1) mine += (unsigned long long)__shfl_xor(mine, d);
    if (lane_id() == 0) sums[wave_id()] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
        for (unsigned k = 0; k < (unsigned)kWavesPerBlock; k++) all += sums[k];
        *out = all;
    }
}
// the place of a flagged lane among the workgroup's flagged lanes, and how many there are
__device__ __forceinline__ uint32_t runs_block_rank(bool f, uint32_t* part, uint32_t& total)
{
    const unsigned long long b = __ballot(f);
    const uint32_t below = lanes_below(b);
    if (lane_id() == 0) part[wave_id()] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t rank = below, tot = 0;
    for (unsigned w = 0; w < (unsigned)kWavesPerBlock; w++) {
        if (w < wave_id()) rank += part[w];
        tot += part[w];
    }
    __syncthreads();
    total = tot;
    return rank;
}
// rr[i] = r for the candidates (i, lyn[i]) that can still be a run, the empty mark for the others
__global__ void __launch_bounds__(kBlock)
k_runs_candidates(LceView v, const uint32_t* __restrict__ lyn, int order, RunsFilter flt, uint32_t* __restrict__ rr,
                  unsigned long long* __restrict__ bcnt)
{
    __shared__ unsigned long long sums[kWavesPerBlock];
    const uint64_t n = v.n;
    uint64_t lo, hi;
    runs_chunk(n, &lo, &hi);
    unsigned long long mine = 0;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += kBlock) {
        const uint64_t p = lyn[i];
        uint32_t keep = kLceNone;
        if (p >= 1 && p <= n - i && p >= flt.min_period && p <= flt.max_period) {
            const uint32_t r = i + p == n ? 0u : runs_lce(v, (uint32_t)i, (uint32_t)(i + p));
            const uint64_t need = p > r ? p - r : 0, room = dmin<uint64_t>(i, p - 1);
            bool ok = need <= room && !(order == 1 && i + p + r == n);
            if (ok && need) ok = runs_lce(v, (uint32_t)(i - need), (uint32_t)(i + p - need)) >= need;
            if (ok) keep = r;
        }
        rr[i] = keep;
        mine += keep != kLceNone;
    }
    runs_block_sum(mine, sums, &bcnt[blockIdx.x]);
}
// one workgroup: boff = the exclusive scan of bcnt, boff[nwords] = the total, also kept in res[note] for whoever times the
// call; accepted: the running count moves on by it
__global__ void __launch_bounds__(kBlock)
k_runs_offsets(const unsigned long long* __restrict__ bcnt, unsigned nwords, unsigned long long* __restrict__ boff, uint32_t* __restrict__ res,
               unsigned note, bool accepted)
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
        res[note] = (uint32_t)carry;
        if (accepted) {
            const unsigned long long z = (unsigned long long)res[kRunsResZ + 1] << 32 | res[kRunsResZ];
            res[kRunsResBase] = (uint32_t)z;
            res[kRunsResBase + 1] = (uint32_t)(z >> 32);
            res[kRunsResZ] = (uint32_t)(z + carry);
            res[kRunsResZ + 1] = (uint32_t)((z + carry) >> 32);
        }
    }
}
__global__ void __launch_bounds__(kBlock)
k_runs_compact(const uint32_t* __restrict__ rr, uint64_t n, const unsigned long long* __restrict__ boff, uint32_t* __restrict__ pos,
               uint32_t* __restrict__ rl)
{
    __shared__ uint32_t part[kWavesPerBlock];
    uint64_t lo, hi;
    runs_chunk(n, &lo, &hi);
    uint64_t run = boff[blockIdx.x];
    for (uint64_t base = lo; base < hi; base += kBlock) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t r = i < hi ? rr[i] : kLceNone;
        uint32_t total;
        const uint32_t rank = runs_block_rank(r != kLceNone, part, total);
        if (r != kLceNone) {
            pos[run + rank] = (uint32_t)i;
            rl[run + rank] = r;
        }
        run += total;
    }
}
// l = the largest k in [need, min(i, p)] with LCE(i - k, i + p - k) >= k; k = need holds (runs_candidates)
__device__ __forceinline__ uint32_t runs_left(const LceView& v, uint32_t i, uint32_t p, uint32_t need)
{
    const uint32_t cap = dmin(i, p);
    uint32_t lo = need, hi = cap;
    for (uint32_t step = 1; lo < cap; step <<= 1) {
        const uint32_t k = cap - lo <= step ? cap : lo + step;
        if (runs_lce(v, i - k, i + p - k) >= k) {
            lo = k;
            if (step > 0x7FFFFFFFu) break;
        } else {
            hi = k - 1;
            break;
        }
    }
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (runs_lce(v, i - mid, i + p - mid) >= mid) lo = mid; else hi = mid - 1;
    }
    return lo;
}
__global__ void __launch_bounds__(kBlock)
k_runs_extend(LceView v, const uint32_t* __restrict__ lyn, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ rl,
              const unsigned long long* __restrict__ scount, int order, RunsFilter flt, uint64_t* __restrict__ tK, uint32_t* __restrict__ tV,
              unsigned long long* __restrict__ bcnt)
{
    __shared__ unsigned long long sums[kWavesPerBlock];
    const uint64_t n = v.n, S = dmin<uint64_t>(*scount, n);
    uint64_t lo, hi;
    runs_chunk(S, &lo, &hi);
    unsigned long long mine = 0;
    for (uint64_t s = lo + threadIdx.x; s < hi; s += kBlock) {
        const uint32_t i = pos[s], r = rl[s];
        uint64_t key = kRunsNoKey;
        uint32_t e = 0;
        if (i < n) {
            const uint64_t p = lyn[i];
            if (p >= 1 && p <= n - i && r <= n - i - p) {                 // (always: both arrays are ours)
                const uint32_t need = p > r ? (uint32_t)(p - r) : 0u;
                if (need <= dmin<uint64_t>(i, p - 1)) {
                    const uint32_t l = runs_left(v, i, (uint32_t)p, need);
                    e = (uint32_t)(i + p + r);
                    if (l < p && (order == 0 || e < n) && (uint64_t)e - (i - l) >= flt.min_len) key = (uint64_t)(i - l) << 32 | p;
                }
            }
        }
        tK[s] = key;
        tV[s] = e;
        mine += key != kRunsNoKey;
    }
    runs_block_sum(mine, sums, &bcnt[blockIdx.x]);
}
__global__ void __launch_bounds__(kBlock)
k_runs_gather(const uint64_t* __restrict__ tK, const uint32_t* __restrict__ tV, const unsigned long long* __restrict__ scount, uint64_t n,
              const unsigned long long* __restrict__ boff, const uint32_t* __restrict__ res, uint64_t* __restrict__ K, uint32_t* __restrict__ V)
{
    __shared__ uint32_t part[kWavesPerBlock];
    const uint64_t S = dmin<uint64_t>(*scount, n);
    uint64_t lo, hi;
    runs_chunk(S, &lo, &hi);
    uint64_t run = ((uint64_t)res[kRunsResBase + 1] << 32 | res[kRunsResBase]) + boff[blockIdx.x];
    for (uint64_t base = lo; base < hi; base += kBlock) {
        const uint64_t s = base + threadIdx.x;
        const uint64_t key = s < hi ? tK[s] : kRunsNoKey;
        uint32_t total;
        const uint32_t rank = runs_block_rank(key != kRunsNoKey, part, total);
        if (key != kRunsNoKey && run + rank < n) {                        // (fewer than n runs; a foreign lcp may claim more)
            K[run + rank] = key;
            V[run + rank] = tV[s];
        }
        run += total;
    }
}
__global__ void __launch_bounds__(kBlock)
k_runs_write(const uint64_t* __restrict__ K, const uint32_t* __restrict__ V, uint64_t count, uint32_t* __restrict__ begin,
             uint32_t* __restrict__ end, uint32_t* __restrict__ period)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < count; q += stride) {
        const uint64_t k = K[q];
        begin[q] = (uint32_t)(k >> 32);
        end[q] = V[q];
        period[q] = (uint32_t)k;
    }
}
__global__ void __launch_bounds__(kBlock)
k_runs_complement(const uint8_t* text, uint64_t n, uint8_t* out)          // (out may be text: the host route's own copy)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) out[i] = (uint8_t)(255u - text[i]);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// isa[sa[r]] = r.  flags (two words, cleared by the caller): the table is checked and the result verified as lce_isa_queue
// does; nullptr: a table of ours, scattered only
static int runs_isa_queue(const uint32_t* d_sa, uint64_t n, uint32_t* d_isa, uint32_t* flags, hipStream_t st)
{
    const unsigned grid = lce_grid(n);
    if (flags) SFX_LAUNCH("runs_check", (double)n * 4, k_lce_check, grid, kBlock, st, d_sa, n, (const uint64_t*)nullptr, (uint64_t)0, flags);
    SFX_HIP(hipMemsetAsync(d_isa, 0xFF, n * sizeof(uint32_t), st));
    SFX_LAUNCH("runs_scatter", (double)n * 8, k_lce_scatter, grid, kBlock, st, d_sa, n, d_isa);
    if (flags) SFX_LAUNCH("runs_verify", (double)n * 4, k_lce_verify, grid, kBlock, st, (const uint32_t*)d_isa, n, flags);
    return SFX_OK;
}
// the levels above `in` (n words), lce_layout(n, fan_log).tree_words words at tree
static int runs_levels_queue(const uint32_t* in, uint64_t n, uint32_t* tree, int fan_log, hipStream_t st)
{
    const LceLayout L = lce_layout(n, fan_log);
    if (L.tree_words) SFX_HIP(hipMemsetAsync(tree, 0xFF, L.tree_words * 4, st));
    uint32_t* out = tree;
    uint64_t cnt = n;
    for (int k = 1; k < L.levels; k++) {
        const uint64_t cnt_out = (cnt + (1ull << fan_log) - 1) >> fan_log;
        SFX_LAUNCH("runs_levels", (double)cnt * 4 + (double)cnt_out * 4, k_lce_levels, lce_grid(cnt), kBlock, st, in, cnt, out, fan_log);
        in = out;
        out += lce_line_up(cnt_out);
        cnt = cnt_out;
    }
    return SFX_OK;
}
// lyn from isa: tree = lce_layout(n, fan_log).tree_words words, list = list_cap words, open_count = one word (all scratch)
static int runs_lyndon_queue(const uint32_t* d_isa, uint64_t n, uint32_t* d_lyn, uint32_t* tree, uint32_t* list, uint64_t list_cap,
                             uint32_t* open_count, int fan_log, hipStream_t st)
{
    const uint32_t T = runs_tile_hook();
    SFX_TRY(runs_levels_queue(d_isa, n, tree, fan_log, st));
    SFX_HIP(hipMemsetAsync(open_count, 0, sizeof(uint32_t), st));
    const RunsTree t{d_isa, tree, n, fan_log, lce_layout(n, fan_log).levels};
    const unsigned cap = dmin<unsigned>(kMaxGrid, grid_cap());
    const unsigned tgrid = (unsigned)dmax<uint64_t>(1, dmin<uint64_t>((n + T - 1) / T, cap));
    SFX_LAUNCH("runs_lyndon_tile", (double)n * 8, k_runs_lyndon_tile, tgrid, kBlock, st, t, T, d_lyn, list, list_cap, open_count);
    // (the number of listed positions is on the device: the grid is sized by its bound)
    if (list_cap) SFX_LAUNCH("runs_lyndon_open", 0.0, k_runs_lyndon_open, lce_grid(list_cap), kBlock, st, t, T, d_lyn, (const uint32_t*)list, list_cap,
                             (const uint32_t*)open_count);
    return SFX_OK;
}

// [res 64 u32 | tree | list n u32]
struct LyndonWs { uint32_t *res, *tree, *list; };
template <class A> static void lyndon_carve(A& a, uint64_t n, int fan_log, LyndonWs* w)
{
    w->res = a.template take<uint32_t>(kRunsResWords);
    w->tree = a.template take<uint32_t>(lce_layout(n, fan_log).tree_words);
    w->list = a.template take<uint32_t>(n);
}
uint64_t lyndon_array_workspace_bytes(uint64_t n)
{
    if (n == 0 || n > kRunsMaxN) return 0;
    LceSizer z;
    LyndonWs w;
    lyndon_carve(z, n, lce_fan_log(), &w);
    return z.used;
}
// no read-back, no synchronisation: d_lyn is complete in stream order.  d_isa is not verified: its values are only compared
int lyndon_array_dev(const uint32_t* d_isa, uint64_t n, uint32_t* d_lyn, void* ws, uint64_t ws_bytes, hipStream_t st)
{
    if (n > kRunsMaxN) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!d_isa || !d_lyn) return SFX_ERR_ARG;
    if (!ws || ws_bytes < lyndon_array_workspace_bytes(n)) return SFX_ERR_WORKSPACE;
    const int f = lce_fan_log();
    Arena a(ws, ws_bytes);
    LyndonWs w;
    lyndon_carve(a, n, f, &w);
    if (a.overflow) return SFX_ERR_INTERNAL;
    return runs_lyndon_queue(d_isa, n, d_lyn, w.tree, w.list, runs_list_hook(n), w.res + kRunsResOpen, f, st);
}
// the host route's middle: the inverse table of d_sa into d_isa (checked), then lyn; one read-back for the flags
int lyndon_from_table_dev(const uint32_t* d_sa, uint64_t n, uint32_t* d_isa, uint32_t* d_lyn, void* ws, uint64_t ws_bytes, hipStream_t st)
{
    if (n > kRunsMaxN) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!ws || ws_bytes < lyndon_array_workspace_bytes(n)) return SFX_ERR_WORKSPACE;
    uint32_t* const res = (uint32_t*)ws;
    SFX_HIP(hipMemsetAsync(res, 0, kRunsResWords * sizeof(uint32_t), st));
    SFX_TRY(runs_isa_queue(d_sa, n, d_isa, res + kRunsResFlags, st));
    SFX_TRY(lyndon_array_dev(d_isa, n, d_lyn, ws, ws_bytes, st));
    uint32_t flags[2] = {0, 0};
    SFX_TRY(read_back(flags, res + kRunsResFlags, sizeof(flags), st));
    return (flags[0] | flags[1]) ? SFX_ERR_ARG : SFX_OK;
}

// (the first 64 words of the workspace are res: a timing script reads the survivor counts there after the call)
// [res | bcntA | boffA | bcntB | boffB | comp n u8 | X n u32 | isa0 | isa1 | lyn0 | lyn1 | lcp tree | U],  U = the larger of
// the SA build's workspace and [isa tree | list n u32 | K0 n u64 | V0 n u32 | K1 n u64 | V1 n u32 | radix scratch(n)].
// X: the complement's table, then the survivors' positions; isa1: after the second Lyndon pass the survivors' r; list: after the
// Lyndon passes r per position; K1 / V1: until the sort the survivors' triples
struct RunsWs {
    uint32_t *res, *X, *isa0, *isa1, *lyn0, *lyn1, *lcptree;
    unsigned long long *bcntA, *boffA, *bcntB, *boffB;
    uint8_t *comp, *U;
    uint64_t ubytes;
};
struct RunsLate {
    uint32_t *isatree, *list, *V0, *V1, *scratch;
    uint64_t *K0, *K1;
};
template <class A> static void runs_late_carve(A& a, uint64_t n, int fan_log, RunsLate* w)
{
    w->isatree = a.template take<uint32_t>(lce_layout(n, fan_log).tree_words);
    w->list = a.template take<uint32_t>(n);
    w->K0 = a.template take<uint64_t>(n);
    w->V0 = a.template take<uint32_t>(n);
    w->K1 = a.template take<uint64_t>(n);
    w->V1 = a.template take<uint32_t>(n);
    w->scratch = a.template take<uint32_t>(radix_scratch_words(n));
}
template <class A> static void runs_carve(A& a, uint64_t n, int fan_log, RunsWs* w)
{
    w->res = a.template take<uint32_t>(kRunsResWords);
    w->bcntA = a.template take<unsigned long long>(kMaxGrid);
    w->boffA = a.template take<unsigned long long>(kMaxGrid + 1);
    w->bcntB = a.template take<unsigned long long>(kMaxGrid);
    w->boffB = a.template take<unsigned long long>(kMaxGrid + 1);
    w->comp = a.template take<uint8_t>(n);
    w->X = a.template take<uint32_t>(n);
    w->isa0 = a.template take<uint32_t>(n);
    w->isa1 = a.template take<uint32_t>(n);
    w->lyn0 = a.template take<uint32_t>(n);
    w->lyn1 = a.template take<uint32_t>(n);
    w->lcptree = a.template take<uint32_t>(lce_layout(n, fan_log).tree_words);
    LceSizer z;
    RunsLate late;
    runs_late_carve(z, n, fan_log, &late);
    w->ubytes = dmax(z.used, (sa_workspace_bytes(n) + kArenaAlign - 1) & ~(kArenaAlign - 1));
    w->U = a.template take<uint8_t>(w->ubytes);
}
uint64_t runs_workspace_bytes(uint64_t n)
{
    if (n == 0 || n > kRunsMaxN) return 0;
    LceSizer z;
    RunsWs w;
    runs_carve(z, n, lce_fan_log(), &w);
    return z.used;
}
// Queues on st and synchronises it once for (count, flags), apart from the read-backs of the SA build of the complement.  The
// sort and the copy into the three arrays are queued behind that read-back: they are complete in stream order, and the
// workspace must stay untouched until the stream has passed them.
int runs_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint32_t* d_lcp, const sfx_runs_filter_t* filter, uint32_t* d_begin,
             uint32_t* d_end, uint32_t* d_period, uint64_t capacity, uint64_t* count_out, void* ws, uint64_t ws_bytes, hipStream_t st)
{
    if (!count_out) return SFX_ERR_ARG;
    *count_out = 0;
    if (n > kRunsMaxN) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!d_text || !d_sa || !d_lcp || (capacity && (!d_begin || !d_end || !d_period))) return SFX_ERR_ARG;
    if (!ws || ws_bytes < runs_workspace_bytes(n)) return SFX_ERR_WORKSPACE;
    RunsFilter flt{1u, (uint32_t)n, 0u};
    if (filter) {
        flt.min_period = dmax(1u, filter->min_period);
        if (filter->max_period) flt.max_period = filter->max_period;
        flt.min_len = filter->min_len;
    }
    const int f = lce_fan_log();
    Arena a(ws, ws_bytes);
    RunsWs w;
    runs_carve(a, n, f, &w);
    if (a.overflow) return SFX_ERR_INTERNAL;
    Arena la(w.U, w.ubytes);
    RunsLate late;
    runs_late_carve(la, n, f, &late);
    if (la.overflow) return SFX_ERR_INTERNAL;
    const unsigned grid = lce_grid(n);
    SFX_HIP(hipMemsetAsync(w.res, 0, kRunsResWords * sizeof(uint32_t), st));
    // the table of order 1, both inverse tables, the LCP tree
    SFX_LAUNCH("runs_complement", (double)n * 2, k_runs_complement, grid, kBlock, st, d_text, n, w.comp);
    SFX_TRY(build_sa_u32_dev(w.comp, n, w.X, w.U, w.ubytes, st));
    SFX_TRY(runs_isa_queue(w.X, n, w.isa1, nullptr, st));
    SFX_TRY(runs_isa_queue(d_sa, n, w.isa0, w.res + kRunsResFlags, st));
    SFX_TRY(runs_levels_queue(d_lcp, n, w.lcptree, f, st));
    // both Lyndon arrays (the isa tree and the list serve one pass after the other)
    const uint64_t list_cap = runs_list_hook(n);
    SFX_TRY(runs_lyndon_queue(w.isa0, n, w.lyn0, late.isatree, late.list, list_cap, w.res + kRunsResOpen, f, st));
    SFX_TRY(runs_lyndon_queue(w.isa1, n, w.lyn1, late.isatree, late.list, list_cap, w.res + kRunsResOpen, f, st));
    LceView v = {};
    v.isa = w.isa0;
    v.lcp = d_lcp;
    v.tree = w.lcptree;
    v.n = (uint32_t)n;
    v.fan_log = f;
    v.levels = lce_layout(n, f).levels;
    uint32_t *const rr = late.list, *const pos = w.X, *const rl = w.isa1;
    for (int order = 0; order < 2; order++) {
        const uint32_t* lyn = order ? w.lyn1 : w.lyn0;
        // two isa lines and about eight tree lines per extension (as lce_query counts them)
        SFX_LAUNCH("runs_candidates", (double)n * (8 + 10 * 128), k_runs_candidates, grid, kBlock, st, v, lyn, order, flt, rr, w.bcntA);
        SFX_LAUNCH("runs_offsets", (double)grid * 16, k_runs_offsets, 1, kBlock, st, (const unsigned long long*)w.bcntA, grid, w.boffA, w.res,
                   kRunsResSurvive + (unsigned)order, false);
        SFX_LAUNCH("runs_compact", (double)n * 4, k_runs_compact, grid, kBlock, st, (const uint32_t*)rr, n, (const unsigned long long*)w.boffA, pos, rl);
        // (the number of survivors is on the device: the grids are sized by its bound, the kernels read the real one)
        const unsigned long long* scount = w.boffA + grid;
        SFX_LAUNCH("runs_extend", 0.0, k_runs_extend, grid, kBlock, st, v, lyn, (const uint32_t*)pos, (const uint32_t*)rl, scount, order, flt, late.K1,
                   late.V1, w.bcntB);
        SFX_LAUNCH("runs_offsets", (double)grid * 16, k_runs_offsets, 1, kBlock, st, (const unsigned long long*)w.bcntB, grid, w.boffB, w.res,
                   kRunsResAccept + (unsigned)order, true);
        SFX_LAUNCH("runs_gather", 0.0, k_runs_gather, grid, kBlock, st, (const uint64_t*)late.K1, (const uint32_t*)late.V1, scount, n,
                   (const unsigned long long*)w.boffB, (const uint32_t*)w.res, late.K0, late.V0);
    }
    uint32_t back[6] = {0, 0, 0, 0, 0, 0};                             // the count and the two flags: the one read-back
    SFX_TRY(read_back(back, w.res, sizeof(back), st));
    if (back[kRunsResFlags] | back[kRunsResFlags + 1]) return SFX_ERR_ARG;
    const uint64_t count = dmin((uint64_t)back[kRunsResZ + 1] << 32 | back[kRunsResZ], n);
    *count_out = count;
    const uint64_t wr = dmin(count, capacity);
    if (wr == 0) return SFX_OK;
    // the order, queued behind the read-back and sized by it
    uint64_t* K = late.K0;
    uint32_t* V = late.V0;
    int in1 = 0;
    SFX_TRY(radix_sort_kv64(late.K0, late.V0, late.K1, late.V1, count, 0, 32 + bits_for(n), late.scratch, st, &in1, nullptr, nullptr));
    if (in1) { K = late.K1; V = late.V1; }
    SFX_LAUNCH("runs_write", (double)wr * 24, k_runs_write, lce_grid(wr), kBlock, st, (const uint64_t*)K, (const uint32_t*)V, wr, d_begin, d_end, d_period);
    return SFX_OK;
}

}  // namespace sfx
