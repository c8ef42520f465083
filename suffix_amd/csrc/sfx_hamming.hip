// sfx_hamming.hip -- k-mismatch (Hamming) occurrences of a batch of patterns (include/suffix_hip.h).
//
// T = the indexed text of n bytes with table sa; pattern j has m_j bytes and is cut at b_t = floor(t m_j / (k + 1)),
// t = 0 .. k + 1, into k + 1 pieces.  An occurrence (at most k differing bytes) has a piece that matches exactly -- the
// first such piece OWNS it.  A candidate is (piece e = j (k + 1) + t, rank r in the exact interval of the piece); it
// survives iff the window p = sa[r] - b_t has room, no earlier piece matches exactly and the window differs in <= k bytes.
// Every occurrence is thus produced by exactly one candidate, and the output -- the survivors in candidate order -- needs
// neither a sort nor a duplicate filter.
//
//   hm_pieces   po[e] = qoff[j] + b_t, nq (k + 1) + 1 of them: a qoff for the batch search; a decreasing qoff or a
//               pattern above u32::MAX raises a flag
//   hm_guard    a raised flag empties every piece (po = 0), so that the search reads no pattern byte
//   search      the index's own batch search over (qbytes, po): [start, end) per piece
//   hm_cand     cand = end - start; an empty piece of a non-empty pattern: all n ranks; written over end
//   scan        off = the 64-bit exclusive sum of cand; C = off[pieces] stays on the device
//   hm_count    tiles of K consecutive candidates, expanded from the pieces through LDS (mem_expand of sfx_mem.hip);
//               per tile the number of survivors and one bit per candidate
//   scan        tile offsets, 64-bit
//   hm_emit     the marked candidates of a tile, compacted in candidate order, written at tile offset + rank while that
//               is below `capacity`; the first lane posts (C, Z, flags) for the one read-back
//   hm_first    first[j] = the tile offset of the tile with pattern j's first candidate + the marks below its slot
// A C above cand_limit makes hm_count write zero counts and nothing else; hm_emit and hm_first then write nothing.
// No workgroup waits for another and nothing is counted with atomics; every loop is bounded by m_j, k + 1, K or the
// piece count.
//
// Compiled as part of sfx_api.hip (which includes this file behind sfx_mem.hip).
#pragma once
#include "sfx_mem.hip"

namespace sfx {

constexpr uint32_t kHmMaxK = 255;

// test hook, read at every call: SFX_HM_TILE=<candidates> in [1, 2048]
static uint32_t hm_tile()
{
    const char* e = dev_env("SFX_HM_TILE");
    const int t = e ? atoi(e) : 0;
    return t >= 1 && t <= (int)kMemTile ? (uint32_t)t : kMemTile;
}

// what the candidate kernels read.  e: the expansion's view -- m = the number of pieces, off / start per piece, q = the
// pattern bytes, tile = K, pair_limit = cand_limit
struct HmIn {
    MemIn e;
    const uint64_t* qoff;                               // nq + 1
    const uint64_t* po;                                 // pieces + 1
    uint32_t k, kp1;
};

enum { kHmResC = 0, kHmResZ = 2, kHmResBadOrder = 4, kHmResTooLong = 5 };      // u32 words of the result block

__global__ void __launch_bounds__(kBlock)
k_hm_pieces(const uint64_t* __restrict__ qoff, uint64_t nq, uint32_t kp1, uint64_t* __restrict__ po, uint32_t* __restrict__ result)
{
    const uint64_t np = nq * kp1, stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e <= np; e += stride) {
        if (e == np) {
            po[e] = qoff[nq];
            continue;
        }
        const uint64_t j = e / kp1, t = e - j * kp1, a = qoff[j], b = qoff[j + 1];
        const uint64_t m = b >= a ? b - a : 0;
        if (t == 0 && b < a) result[kHmResBadOrder] = 1u;                             // (every writer stores the same word)
        if (t == 0 && m > 0xFFFFFFFFull) result[kHmResTooLong] = 1u;
        po[e] = a + (m > 0xFFFFFFFFull ? 0 : t * m / kp1);                            // (t <= 255, m < 2^32: no overflow)
    }
}
__global__ void __launch_bounds__(kBlock)
k_hm_guard(uint64_t np, uint64_t* __restrict__ po, const uint32_t* __restrict__ result)
{
    if (!(result[kHmResBadOrder] | result[kHmResTooLong])) return;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e <= np; e += stride) po[e] = 0;
}
__global__ void __launch_bounds__(kBlock)
k_hm_cand(const uint64_t* __restrict__ qoff, const uint64_t* __restrict__ po, uint64_t np, uint32_t kp1, uint64_t n,
          uint32_t* __restrict__ start, uint32_t* __restrict__ end, const uint32_t* __restrict__ result)
{
    const bool bad = (result[kHmResBadOrder] | result[kHmResTooLong]) != 0;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < np; e += stride) {
        uint32_t c = 0;
        if (!bad) {
            const uint64_t j = e / kp1, m = qoff[j + 1] - qoff[j];
            if (m != 0 && m <= n) {                                                   // (a pattern longer than the text has no window)
                if (po[e + 1] == po[e]) {
                    start[e] = 0u;
                    c = (uint32_t)n;
                } else {
                    const uint32_t a = start[e], b = end[e];
                    if (b > a && b <= n) c = b - a;
                }
            }
        }
        end[e] = c;
    }
}

// the number of differing bytes of a[lo..hi) and b[lo..hi), 8 bytes at a time; gives up once the count passes `budget`
// (what it returns then is only known to be above it)
__device__ __forceinline__ uint32_t hm_diff(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint64_t lo, uint64_t hi,
                                            uint32_t budget)
{
    uint32_t c = 0;
    while (lo + 8 <= hi) {
        uint64_t x, y;
        __builtin_memcpy(&x, a + lo, 8);
        __builtin_memcpy(&y, b + lo, 8);
        uint64_t d = x ^ y;
        if (d) {
            d |= d >> 4;
            d |= d >> 2;
            d |= d >> 1;
            c += (uint32_t)__popcll(d & 0x0101010101010101ull);                       // one bit per differing byte
            if (c > budget) return c;
        }
        lo += 8;
    }
    for (; lo < hi; lo++) c += a[lo] != b[lo];
    return c;
}
struct HmCand {
    uint64_t j, qo, m;                                  // pattern, its first byte in qbytes, its length
    uint32_t t, bt, p;                                  // own piece, its offset in the pattern, the window's start
    bool room;                                          // the window lies inside the text / the document of sa[r]
};
// candidate c of piece e: rank start[e] + (c - off[e])
template <bool DOCS> __device__ __forceinline__ HmCand hm_candidate(const HmIn& in, uint64_t e, uint64_t c)
{
    HmCand a;
    a.j = e / in.kp1;
    a.t = (uint32_t)(e - a.j * in.kp1);
    a.qo = in.qoff[a.j];
    a.m = in.qoff[a.j + 1] - a.qo;
    a.bt = (uint32_t)(in.po[e] - a.qo);
    const uint64_t r = in.e.start[e] + (c - in.e.off[e]);                             // (< n: hm_cand admitted end <= n only)
    const uint32_t q = in.e.sa[r];
    uint64_t lo, hi;
    mem_bounds<DOCS>(in.e, r, &lo, &hi);
    a.p = q - a.bt;
    a.room = q < in.e.n && q >= a.bt && (uint64_t)q - a.bt >= lo && hi <= in.e.n && (uint64_t)a.p + a.m <= hi;
    return a;
}
// The window's mismatches, piece by piece; the candidate's own piece matches and is skipped.  -> the count, or k + 1 as
// soon as it passes k or an earlier piece turns out to match exactly (the candidate does not own the window).
__device__ __forceinline__ uint32_t hm_window(const HmIn& in, const HmCand& a)
{
    const uint8_t* __restrict__ pat = in.e.q + a.qo;
    const uint8_t* __restrict__ win = in.e.text + a.p;
    const uint64_t* __restrict__ cut = in.po + a.j * in.kp1;
    uint32_t total = 0;
    uint64_t b0 = 0;
    for (uint32_t s = 0; s < in.kp1; s++) {
        const uint64_t b1 = cut[s + 1] - a.qo;
        if (s != a.t) {
            const uint32_t d = hm_diff(pat, win, b0, b1, in.k - total);
            if (d == 0 && s < a.t) return in.k + 1;
            total += d;
            if (total > in.k) return in.k + 1;
        }
        b0 = b1;
    }
    return total;
}

// Candidates are dealt to lanes striped (candidate j of the tile to lane j % kBlock: a run of ranks reads sa coalesced);
// the flags go through LDS so that a thread packs its consecutive slots into the byte the emit pass reads.
template <bool DOCS> __global__ void __launch_bounds__(kBlock)
k_hm_count(HmIn in, uint32_t* __restrict__ tcnt, uint8_t* __restrict__ mask)
{
    __shared__ uint32_t pos[kMemTile];
    __shared__ uint8_t hit[kMemTile];
    __shared__ uint32_t part[kWavesPerBlock];
    __shared__ uint64_t first;
    const uint64_t C = in.e.off[in.e.m];
    const uint32_t K = in.e.tile, per = (K + kBlock - 1) / kBlock;
    const uint64_t nt = C > in.e.pair_limit ? 0 : (C + K - 1) / K;
    // the tiles the limit allows for but C does not fill (all of them after a refusal) count nothing: one lane each
    for (uint64_t t = nt + (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < in.e.ntiles_max; t += (uint64_t)gridDim.x * kBlock) tcnt[t] = 0u;
    for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
        const uint32_t cnt = mem_expand(in.e, C, t, pos, part, &first);
        for (uint32_t j = threadIdx.x; j < K; j += kBlock) {
            bool ok = false;
            if (j < cnt) {
                const HmCand a = hm_candidate<DOCS>(in, pos[j], t * K + j);
                ok = a.room && hm_window(in, a) <= in.k;
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
k_hm_emit(HmIn in, const uint64_t* __restrict__ toff, const uint8_t* __restrict__ mask, uint32_t* __restrict__ pattern,
          uint32_t* __restrict__ tpos, uint8_t* __restrict__ mism, uint64_t capacity, uint32_t* __restrict__ result)
{
    __shared__ uint32_t pos[kMemTile];
    __shared__ uint16_t list[kMemTile];
    __shared__ uint32_t part[kWavesPerBlock];
    __shared__ uint64_t first;
    const uint64_t C = in.e.off[in.e.m];
    const uint32_t K = in.e.tile, per = (K + kBlock - 1) / kBlock;
    const uint64_t nt = C > in.e.pair_limit ? 0 : (C + K - 1) / K;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t Z = toff[in.e.ntiles_max];                                     // (0 after a refusal)
        result[kHmResC] = (uint32_t)C;
        result[kHmResC + 1] = (uint32_t)(C >> 32);
        result[kHmResZ] = (uint32_t)Z;
        result[kHmResZ + 1] = (uint32_t)(Z >> 32);
    }
    for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
        const uint64_t o = toff[t];
        if (o >= capacity || toff[t + 1] == o) continue;                              // (uniform)
        mem_expand(in.e, C, t, pos, part, &first);
        const uint32_t bits = mask[t * kBlock + threadIdx.x];
        uint32_t total;
        uint32_t rank = block_scan_add_excl<uint32_t>(__popc(bits), part, total);
        for (uint32_t b = 0; b < per; b++)
            if (bits >> b & 1u) list[rank++] = (uint16_t)(threadIdx.x * per + b);
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < total && o + j < capacity; j += kBlock) {
            const uint32_t slot = list[j];
            const HmCand a = hm_candidate<DOCS>(in, pos[slot], t * K + slot);
            pattern[o + j] = (uint32_t)a.j;
            tpos[o + j] = a.p;
            mism[o + j] = (uint8_t)hm_window(in, a);                                  // (marked: room, owner, <= k <= 255)
        }
        __syncthreads();
    }
}
// One lane per pattern (and one for first[nq] = Z).  Pattern j's first candidate is number off[j (k + 1)]; the marks of
// its tile below that slot are at most kBlock mask bytes: whole bytes for the threads below the slot's, then a part.
__global__ void __launch_bounds__(kBlock)
k_hm_first(HmIn in, uint64_t nq, const uint64_t* __restrict__ toff, const uint8_t* __restrict__ mask, uint64_t* __restrict__ first,
           const uint32_t* __restrict__ result)
{
    const uint64_t C = in.e.off[in.e.m];
    if (C > in.e.pair_limit || (result[kHmResBadOrder] | result[kHmResTooLong])) return;   // (refused: first stays as it is)
    const uint32_t K = in.e.tile, per = (K + kBlock - 1) / kBlock;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j <= nq; j += stride) {
        const uint64_t c = j < nq ? in.e.off[j * in.kp1] : C;
        if (c >= C) {
            first[j] = toff[in.e.ntiles_max];
            continue;
        }
        const uint64_t t = c / K;
        const uint32_t slot = (uint32_t)(c - t * K), whole = slot / per;
        const uint8_t* __restrict__ mk = mask + t * kBlock;
        uint32_t below = 0, x = 0;
        for (; x + 8 <= whole; x += 8) {                                              // (mk is 256-byte aligned)
            uint64_t w;
            __builtin_memcpy(&w, mk + x, 8);
            below += (uint32_t)__popcll(w);
        }
        for (; x < whole; x++) below += (uint32_t)__popc(mk[x]);
        below += (uint32_t)__popc(mk[whole] & ((1u << (slot - whole * per)) - 1u));
        first[j] = toff[t] + below;
    }
}

// [result 64 u32 | po pieces + 1 (u64) | start | end -> cand | off pieces + 1 (u64) | scan partials (u64) | tile counts |
//  tile offsets + total (u64) | one mask byte per thread and tile]
struct HmWs {
    uint32_t* result;
    uint64_t* po;
    uint32_t *start, *end;
    uint64_t *off, *part;
    uint32_t* tcnt;
    uint64_t* toff;
    uint8_t* mask;
};
template <class A> static void hm_carve(A& a, uint64_t np, uint64_t ntiles, HmWs* w)
{
    w->result = a.template take<uint32_t>(64);
    w->po = a.template take<uint64_t>(np + 1);
    w->start = a.template take<uint32_t>(np);
    w->end = a.template take<uint32_t>(np);
    w->off = a.template take<uint64_t>(np + 1);
    w->part = a.template take<uint64_t>(kMaxGrid + 64);
    w->tcnt = a.template take<uint32_t>(ntiles);
    w->toff = a.template take<uint64_t>(ntiles + 1);
    w->mask = a.template take<uint8_t>(ntiles * kBlock);
}
// 0: nothing can run (no pattern, k above 255, 2^32 pieces or more, no limit)
static uint64_t hm_piece_count(uint64_t nq, uint32_t k)
{
    if (nq == 0 || k > kHmMaxK || nq > 0xFFFFFFFFull) return 0;
    const uint64_t np = nq * (k + 1);
    return np > 0xFFFFFFFFull ? 0 : np;
}
uint64_t hamming_workspace_bytes(uint64_t nq, uint32_t k, uint64_t cand_limit)
{
    const uint64_t np = hm_piece_count(nq, k);
    if (np == 0 || cand_limit == 0) return 0;
    MemSizer z;
    HmWs w;
    hm_carve(z, np, mem_tiles(np, 0xFFFFFFFFull, cand_limit, hm_tile()), &w);
    return z.used;
}
// the text, its table and, for a collection, its documents; `search(qbytes, po, pieces, start, end, stream)` is the
// exact batch search of whoever calls
struct HmSource {
    const uint8_t* text;
    uint64_t n;
    const uint32_t* sa;
    const uint64_t* starts;
    const uint32_t* da;
    uint64_t ndocs;
};
template <class Search>
int hamming_dev(const HmSource& s, Search search, const uint8_t* d_q, const uint64_t* d_qoff, uint64_t nq, uint32_t k, uint64_t cand_limit,
                uint32_t* d_pattern, uint32_t* d_tpos, uint8_t* d_mism, uint64_t capacity, uint64_t* d_first, uint64_t* cands_out,
                uint64_t* count_out, void* ws, uint64_t ws_bytes, hipStream_t st)
{
    if (!cands_out || !count_out || cand_limit == 0 || k > kHmMaxK) return SFX_ERR_ARG;
    *cands_out = *count_out = 0;
    if (s.n > 0xFFFFFFFFull || (nq && hm_piece_count(nq, k) == 0)) return SFX_ERR_TOO_LARGE;
    if (capacity && (!d_pattern || !d_tpos || !d_mism)) return SFX_ERR_ARG;
    if (nq == 0 || s.n == 0) {
        if (d_first) SFX_HIP(hipMemsetAsync(d_first, 0, (nq + 1) * sizeof(uint64_t), st));
        return SFX_OK;
    }
    if (!d_q || !d_qoff || !s.text || !s.sa || (s.starts && (!s.da || s.ndocs == 0))) return SFX_ERR_ARG;
    if (!ws || ws_bytes < hamming_workspace_bytes(nq, k, cand_limit)) return SFX_ERR_WORKSPACE;
    const uint32_t kp1 = k + 1, tile = hm_tile();
    const uint64_t np = nq * kp1, ntiles = mem_tiles(np, s.n, cand_limit, tile);      // (>= 1, and no more than the sizer's)
    Arena a(ws, ws_bytes);
    HmWs w;
    hm_carve(a, np, ntiles, &w);
    if (a.overflow) return SFX_ERR_INTERNAL;
    const unsigned cap = dmin<unsigned>(kMaxGrid, grid_cap());
    const unsigned pgrid = (unsigned)dmin<uint64_t>((np + 1 + kBlock - 1) / kBlock, cap);
    SFX_HIP(hipMemsetAsync(w.result, 0, 64 * sizeof(uint32_t), st));
    SFX_LAUNCH("hm_pieces", (double)np * 16, k_hm_pieces, pgrid, kBlock, st, d_qoff, nq, kp1, w.po, w.result);
    SFX_LAUNCH("hm_guard", 0.0, k_hm_guard, pgrid, kBlock, st, np, w.po, (const uint32_t*)w.result);
    SFX_TRY(search(d_q, (const uint64_t*)w.po, np, w.start, w.end, st));
    SFX_LAUNCH("hm_cand", (double)np * 32, k_hm_cand, pgrid, kBlock, st, d_qoff, (const uint64_t*)w.po, np, kp1, s.n, w.start, w.end,
               (const uint32_t*)w.result);
    SFX_TRY(scan_u32_to_u64_excl_dev(w.end, np, w.off, w.part, st));
    HmIn in;
    in.e = MemIn{s.text, s.n, s.sa, s.starts, s.da, s.ndocs, d_q, np, w.off, w.start, 0u, 0u, tile, cand_limit, ntiles};
#ifdef SFX_DEV_HOOKS
    in.e.bisect = false;
#endif
    in.qoff = d_qoff;
    in.po = w.po;
    in.k = k;
    in.kp1 = kp1;
    const unsigned grid = (unsigned)dmin<uint64_t>(ntiles, cap);
    // C stays on the device, so the host has no byte estimate for the candidate kernels: they report 0 algorithmic bytes
    if (s.starts)
        SFX_LAUNCH("hm_count", 0.0, k_hm_count<true>, grid, kBlock, st, in, w.tcnt, w.mask);
    else
        SFX_LAUNCH("hm_count", 0.0, k_hm_count<false>, grid, kBlock, st, in, w.tcnt, w.mask);
    SFX_TRY(scan_u32_to_u64_excl_dev(w.tcnt, ntiles, w.toff, w.part, st));
    if (s.starts)
        SFX_LAUNCH("hm_emit", 0.0, k_hm_emit<true>, grid, kBlock, st, in, (const uint64_t*)w.toff, (const uint8_t*)w.mask, d_pattern, d_tpos,
                   d_mism, capacity, w.result);
    else
        SFX_LAUNCH("hm_emit", 0.0, k_hm_emit<false>, grid, kBlock, st, in, (const uint64_t*)w.toff, (const uint8_t*)w.mask, d_pattern, d_tpos,
                   d_mism, capacity, w.result);
    if (d_first)
        SFX_LAUNCH("hm_first", (double)nq * 24, k_hm_first, (unsigned)dmin<uint64_t>((nq + 1 + kBlock - 1) / kBlock, cap), kBlock, st, in, nq,
                   (const uint64_t*)w.toff, (const uint8_t*)w.mask, d_first, (const uint32_t*)w.result);
    uint32_t back[6] = {0, 0, 0, 0, 0, 0};                                            // C, Z, the two flags: one read-back
    SFX_TRY(read_back(back, w.result, sizeof(back), st));
    if (back[kHmResBadOrder]) return SFX_ERR_ARG;
    if (back[kHmResTooLong]) return SFX_ERR_TOO_LARGE;
    *cands_out = (uint64_t)back[1] << 32 | back[0];
    *count_out = *cands_out > cand_limit ? 0 : (uint64_t)back[3] << 32 | back[2];
    return SFX_OK;
}

}  // namespace sfx
