// sfx_edit.hip -- k-error (edit distance) occurrences of a batch of patterns (include/suffix_hip.h).
//
// T = the indexed text of n bytes with table sa; pattern j has m_j >= k + 1 bytes and is cut into k + 1 pieces as in
// sfx_hamming.hip.  An alignment with at most k edits leaves a piece untouched, so it passes through a candidate
// (piece e = j (k + 1) + t, rank r in the exact interval of the piece): q = sa[r], qe = q + |piece|.  The candidate
// extends to the left (P[0 .. b_t) against the text before q, reversed) and to the right (P[b_(t+1) .. m) against the
// text from qe on); L = the best left cost, s* the largest start that attains it, R(e) the right cost up to end e.
// Every e with L + R(e) <= k is a hit (j, e, L + R(e), s*); an occurrence (j, e) is found by several hits and keeps the
// least cost and, among those, the largest s*.
//
//   hm_pieces, hm_guard   sfx_hamming.hip's: po[e] = qoff[j] + b_t; a flag empties every piece
//   ed_short    a pattern with m_j <= k raises a flag
//   search      the index's own batch search over (qbytes, po): [start, end) per piece
//   ed_cand     cand = end - start, written over end; nothing after a flag
//   scan        off = the 64-bit exclusive sum of cand; C = off[pieces] stays on the device
//   ed_count    tiles of K consecutive candidates (mem_expand); per tile the number of hits and one bit per candidate
//   scan        tile offsets, 64-bit: H
//   ed_emit     the marked candidates again: key = pattern << 32 | tend, the hit's number, dist and s* at tile offset +
//               rank; posts (C, H) for the read-back
//   (radix_sort_kv64)     the hit numbers ascending by (pattern, tend), sized by H behind the read-back
//   ed_heads    the first hit of every (pattern, tend), counted per workgroup
//   scan        workgroup offsets: Z
//   ed_reduce   one lane per head: the least dist of its run, then the largest s*; the head's rank for ed_first
//   ed_first    first[j] by bisection over the sorted keys
// A C above cand_limit makes ed_count write zero counts and nothing else; an H above hit_limit makes ed_emit write
// nothing.  No workgroup waits for another and nothing is counted with atomics; every loop is bounded by m_j, 2 k + 1, K,
// the piece count or the length of a run of equal keys.
//
// The extension is an anchored banded dynamic programme over the 2 k + 1 diagonals around the seed, kept as vertical
// differences in two 64-bit words (Myers 1999 in the diagonal form of Hyyro 2003): the text runs down the word, one
// pattern byte is consumed per step and the band slides one text byte.  Rows before the start of the text window are
// given the values of a programme that may only walk along them (vertical -1, horizontal +1), rows past its end never
// match and are not read out; both are consistent with the recurrence, so the formulas need no special case.
//
// Compiled as part of sfx_api.hip (which includes this file behind sfx_hamming.hip).
#pragma once
#include "sfx_hamming.hip"

namespace sfx {

constexpr uint32_t kEdMaxK = 31;                        // 2 k + 1 <= 63 diagonals: one word per lane
constexpr uint64_t kEdMaxHits = 0xFFFFFFFFull;          // hits are numbered in 32 bits (the sort's values)

// test hook, read at every call: SFX_ED_TILE=<candidates> in [1, 2048]
static uint32_t ed_tile()
{
    const char* e = dev_env("SFX_ED_TILE");
    const int t = e ? atoi(e) : 0;
    return t >= 1 && t <= (int)kMemTile ? (uint32_t)t : kMemTile;
}

// u32 words of the result block; words 4 and 5 are sfx_hamming.hip's flags (hm_pieces raises them)
enum { kEdResC = 0, kEdResH = 2, kEdResShort = 6, kEdResZ = 8 };

__global__ void __launch_bounds__(kBlock)
k_ed_short(const uint64_t* __restrict__ qoff, uint64_t nq, uint32_t k, uint32_t* __restrict__ result)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < nq; j += stride) {
        const uint64_t a = qoff[j], b = qoff[j + 1];
        if (b >= a && b - a <= k) result[kEdResShort] = 1u;                           // (every writer stores the same word)
    }
}
__global__ void __launch_bounds__(kBlock)
k_ed_cand(uint64_t np, uint64_t n, const uint32_t* __restrict__ start, uint32_t* __restrict__ end, const uint32_t* __restrict__ result)
{
    const bool bad = (result[kHmResBadOrder] | result[kHmResTooLong] | result[kEdResShort]) != 0;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < np; e += stride) {
        const uint32_t a = start[e], b = end[e];
        end[e] = !bad && b > a && b <= n ? b - a : 0u;
    }
}

// The band after the last pattern byte: bit b stands for the text prefix of u = a - k + b bytes, vp / vn = the cost
// rises / falls by one from u - 1 to u, diag = the cost at u = a.
struct EdBand {
    uint64_t vp, vn;
    uint32_t diag;
    bool alive;                                         // false: abandoned, every cost is above the budget
};
// the cost at bit 0; the one at bit b follows by adding (vp >> b & 1) - (vn >> b & 1) for 1 .. b
__device__ __forceinline__ int32_t ed_val0(const EdBand& d, uint32_t k)
{
    const uint64_t low = ((1ull << (k + 1)) - 1ull) & ~1ull;                          // bits 1 .. k
    return (int32_t)d.diag - (int32_t)__popcll(d.vp & low) + (int32_t)__popcll(d.vn & low);
}
__device__ __forceinline__ int32_t ed_band_min(const EdBand& d, uint32_t k)
{
    int32_t v = ed_val0(d, k), mn = v;
    for (uint32_t b = 1; b <= 2 * k; b++) {
        v += (int32_t)(d.vp >> b & 1ull) - (int32_t)(d.vn >> b & 1ull);
        mn = v < mn ? v : mn;
    }
    return mn;
}
// ed(A[0 .. i), X[0 .. u)) inside the band |i - u| <= k, anchored at (0, 0), after all a bytes of A.  !REV: A[i] = pat[i],
// X[u] = txt[u]; REV: A[i] = pat[a - 1 - i], X[u] = txt[-1 - u].  avail = the bytes of X that exist; none at or beyond
// min(avail, a + k) is read, 8 at a time where 8 remain.  Costs of at most k are exact, larger ones are not below k + 1.
// Gives up (alive = false) once no cell of the band is within `budget`: tested every row while the band has at most 9
// cells, every 8th row for a wider one.
template <bool REV> __device__ __forceinline__ EdBand ed_extend(const uint8_t* __restrict__ pat, uint32_t a, const uint8_t* __restrict__ txt,
                                                                uint64_t avail, uint32_t k, uint32_t budget)
{
    const uint64_t mask = (1ull << (2 * k + 1)) - 1ull, top = 1ull << (2 * k);
    EdBand d;
    d.vn = (1ull << (k + 1)) - 1ull;                                                  // u <= 0: the cost falls towards u = 0
    d.vp = ((1ull << k) - 1ull) << (k + 1);
    d.diag = 0;
    d.alive = true;
    const int64_t kk = k, lim = (int64_t)dmin<uint64_t>(avail, (uint64_t)a + k);
    const uint32_t every = 2 * k + 1 <= 9 ? 0u : 7u;
    for (uint32_t v = 1; v <= a; v++) {
        const uint8_t c = REV ? pat[a - v] : pat[v - 1];
        const uint64_t cc = (uint64_t)c * 0x0101010101010101ull;
        const int64_t base = (int64_t)v - kk - 1;                                     // the text byte of bit 0
        int64_t i = base > 0 ? base : 0;
        const int64_t i1 = (int64_t)v + kk < lim ? (int64_t)v + kk : lim;
        uint64_t eq = 0;
        for (; i + 8 <= i1; i += 8) {
            uint64_t w;
            if (REV) {
                __builtin_memcpy(&w, txt - 8 - i, 8);
                w = __builtin_bswap64(w);
            } else {
                __builtin_memcpy(&w, txt + i, 8);
            }
            uint64_t x = w ^ cc;
            x |= x >> 4;
            x |= x >> 2;
            x |= x >> 1;
            const uint64_t f = ~x & 0x0101010101010101ull;                           // one bit per equal byte
            eq |= ((f * 0x0102040810204080ull) >> 56) << (i - base);                  // gathered into 8 adjacent bits
        }
        for (; i < i1; i++) eq |= (uint64_t)((REV ? txt[-1 - i] : txt[i]) == c) << (i - base);
        const uint64_t vp = (d.vp >> 1) | top, vn = d.vn >> 1;                        // the band slides one text byte
        const uint64_t d0 = (((eq & vp) + vp) ^ vp) | eq | vn;
        const uint64_t hp = vn | ~(d0 | vp), hn = vp & d0;
        d.diag += 1u - (uint32_t)(d0 >> k & 1ull);
        const uint64_t xp = (hp << 1) | 1ull, xn = hn << 1;
        d.vp = (xn | ~(d0 | xp)) & mask;
        d.vn = xp & d0 & mask;
        if ((v & every) == 0 && ed_band_min(d, k) > (int32_t)budget) {
            d.alive = false;
            return d;
        }
    }
    return d;
}

// what the candidate kernels read.  e: the expansion's view -- m = the number of pieces, off / start per piece, q = the
// pattern bytes, tile = K, pair_limit = cand_limit
struct EdIn {
    MemIn e;
    const uint64_t* qoff;                               // nq + 1
    const uint64_t* po;                                 // pieces + 1
    uint32_t k, kp1;
    uint64_t hit_limit;
};
struct EdEval {
    uint64_t j;
    uint32_t qe, sstar, L, hits;
    int32_t u0;                                         // the text prefix of bit 0 of the right band
    uint64_t avail;                                     // text bytes behind qe
    EdBand r;
};
// candidate c of piece e: rank start[e] + (c - off[e]).  Bounds first: no byte is read before they hold.
template <bool DOCS> __device__ __forceinline__ EdEval ed_eval(const EdIn& in, uint64_t e, uint64_t c)
{
    EdEval a;
    a.hits = 0;
    a.j = e / in.kp1;
    const uint64_t qo = in.qoff[a.j], m = in.qoff[a.j + 1] - qo;
    const uint32_t bt = (uint32_t)(in.po[e] - qo), bt1 = (uint32_t)(in.po[e + 1] - qo);
    const uint64_t r = in.e.start[e] + (c - in.e.off[e]);                             // (< n: ed_cand admitted end <= n only)
    const uint32_t q = in.e.sa[r];
    uint64_t lo, hi;
    mem_bounds<DOCS>(in.e, r, &lo, &hi);
    if (!(q < in.e.n && hi <= in.e.n && lo <= q && (uint64_t)q + (bt1 - bt) <= hi)) return a;
    a.qe = q + (bt1 - bt);
    const uint8_t* __restrict__ pat = in.e.q + qo;
    const uint32_t k = in.k;
    const EdBand l = ed_extend<true>(pat, bt, in.e.text + q, q - lo, k, k);
    if (!l.alive) return a;
    {   // the least cost of the last row, at the fewest text bytes (the largest start)
        const uint64_t av = q - lo;
        int32_t v = ed_val0(l, k), best = 0x7FFFFFFF;
        uint32_t at = 0;
        for (uint32_t b = 0; b <= 2 * k; b++) {
            if (b) v += (int32_t)(l.vp >> b & 1ull) - (int32_t)(l.vn >> b & 1ull);
            const int64_t u = (int64_t)bt - k + b;
            if (u >= 0 && (uint64_t)u <= av && v < best) {
                best = v;
                at = (uint32_t)u;
            }
        }
        if (best > (int32_t)k) return a;
        a.L = (uint32_t)best;
        a.sstar = q - at;
    }
    const uint32_t rb = (uint32_t)(m - bt1);
    a.avail = hi - a.qe;
    a.r = ed_extend<false>(pat + bt1, rb, in.e.text + a.qe, a.avail, k, k - a.L);
    if (!a.r.alive) return a;
    a.u0 = (int32_t)((int64_t)rb - k);
    int32_t v = ed_val0(a.r, k);
    for (uint32_t b = 0; b <= 2 * k; b++) {
        if (b) v += (int32_t)(a.r.vp >> b & 1ull) - (int32_t)(a.r.vn >> b & 1ull);
        const int64_t u = (int64_t)a.u0 + b;
        a.hits += u >= 0 && (uint64_t)u <= a.avail && v + (int32_t)a.L <= (int32_t)k;
    }
    return a;
}

// Candidates are dealt to lanes striped, as in hm_count; a slot's hit count (at most 2 k + 1 <= 63) goes through LDS so
// that a thread packs the flags of its consecutive slots into the byte the emit pass reads.
template <bool DOCS> __global__ void __launch_bounds__(kBlock)
k_ed_count(EdIn in, uint32_t* __restrict__ tcnt, uint8_t* __restrict__ mask)
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
        for (uint32_t j = threadIdx.x; j < K; j += kBlock) hit[j] = j < cnt ? (uint8_t)ed_eval<DOCS>(in, pos[j], t * K + j).hits : (uint8_t)0;
        __syncthreads();
        const uint32_t s0 = dmin(threadIdx.x * per, K), s1 = dmin(s0 + per, K);
        uint32_t bits = 0, sum = 0;
        for (uint32_t s = s0; s < s1; s++) {
            bits |= (uint32_t)(hit[s] != 0) << (s - s0);
            sum += hit[s];
        }
        mask[t * kBlock + threadIdx.x] = (uint8_t)bits;
        uint32_t total;
        block_scan_add_excl<uint32_t>(sum, part, total);                             // (two barriers: LDS is free again)
        if (threadIdx.x == 0) tcnt[t] = total;
    }
}
// The marked candidates of a tile, kBlock at a time in candidate order: each is evaluated again, a scan of the hit counts
// ranks its hits, and it writes them ascending by end.
template <bool DOCS> __global__ void __launch_bounds__(kBlock)
k_ed_emit(EdIn in, const uint64_t* __restrict__ toff, const uint8_t* __restrict__ mask, uint64_t* __restrict__ key, uint32_t* __restrict__ val,
          uint8_t* __restrict__ dist, uint32_t* __restrict__ sst, uint32_t* __restrict__ result)
{
    __shared__ uint32_t pos[kMemTile];
    __shared__ uint16_t list[kMemTile];
    __shared__ uint32_t part[kWavesPerBlock];
    __shared__ uint64_t first;
    const uint64_t C = in.e.off[in.e.m], H = toff[in.e.ntiles_max];                   // (H = 0 after a refusal of C)
    const uint32_t K = in.e.tile, per = (K + kBlock - 1) / kBlock;
    const uint64_t nt = C > in.e.pair_limit || H > in.hit_limit ? 0 : (C + K - 1) / K;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        result[kEdResC] = (uint32_t)C;
        result[kEdResC + 1] = (uint32_t)(C >> 32);
        result[kEdResH] = (uint32_t)H;
        result[kEdResH + 1] = (uint32_t)(H >> 32);
    }
    for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
        uint64_t o = toff[t];
        if (toff[t + 1] == o) continue;                                               // (uniform)
        mem_expand(in.e, C, t, pos, part, &first);
        const uint32_t bits = mask[t * kBlock + threadIdx.x];
        uint32_t marked;
        uint32_t rank = block_scan_add_excl<uint32_t>(__popc(bits), part, marked);
        for (uint32_t b = 0; b < per; b++)
            if (bits >> b & 1u) list[rank++] = (uint16_t)(threadIdx.x * per + b);
        __syncthreads();
        for (uint32_t j0 = 0; j0 < marked; j0 += kBlock) {                            // (uniform)
            const uint32_t j = j0 + threadIdx.x;
            EdEval a;
            a.hits = 0;
            if (j < marked) {
                const uint32_t slot = list[j];
                a = ed_eval<DOCS>(in, pos[slot], t * K + slot);
            }
            uint32_t total;
            uint64_t h = o + block_scan_add_excl<uint32_t>(a.hits, part, total);
            if (a.hits) {
                int32_t v = ed_val0(a.r, in.k);
                for (uint32_t b = 0; b <= 2 * in.k; b++) {
                    if (b) v += (int32_t)(a.r.vp >> b & 1ull) - (int32_t)(a.r.vn >> b & 1ull);
                    const int64_t u = (int64_t)a.u0 + b;
                    if (u >= 0 && (uint64_t)u <= a.avail && v + (int32_t)a.L <= (int32_t)in.k) {
                        key[h] = a.j << 32 | (uint64_t)(a.qe + (uint32_t)u);
                        val[h] = (uint32_t)h;                                         // (H <= hit_limit < 2^32)
                        dist[h] = (uint8_t)(v + (int32_t)a.L);
                        sst[h] = a.sstar;
                        h++;
                    }
                }
            }
            o += total;
        }
        __syncthreads();
    }
}

// Workgroup g owns the sorted hits [g chunk, (g + 1) chunk); a head is a hit whose key differs from the one before it.
__global__ void __launch_bounds__(kBlock)
k_ed_heads(const uint64_t* __restrict__ key, uint64_t H, uint64_t chunk, uint32_t* __restrict__ bcnt)
{
    __shared__ uint32_t part[kWavesPerBlock];
    const uint64_t i0 = (uint64_t)blockIdx.x * chunk, i1 = dmin<uint64_t>(i0 + chunk, H);
    uint32_t c = 0;
    for (uint64_t i = i0 + threadIdx.x; i < i1; i += kBlock) c += i == 0 || key[i] != key[i - 1];
    uint32_t total;
    block_scan_add_excl<uint32_t>(c, part, total);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = total;
}
// One lane per head, in hit order: its rank is the workgroup's offset plus the heads before it; the run of its key (at
// most (k + 1)(2 k + 1) hits, it may reach into the next workgroups' hits) gives the least dist and then the largest s*.
// hrank[i] = the heads before hit i, for ed_first.
__global__ void __launch_bounds__(kBlock)
k_ed_reduce(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val, const uint8_t* __restrict__ dist, const uint32_t* __restrict__ sst,
            uint64_t H, uint64_t chunk, const uint64_t* __restrict__ boff, uint64_t capacity, uint32_t* __restrict__ pattern,
            uint32_t* __restrict__ tbegin, uint32_t* __restrict__ tend, uint8_t* __restrict__ dout, uint32_t* __restrict__ hrank,
            uint32_t* __restrict__ result)
{
    __shared__ uint32_t part[kWavesPerBlock];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t Z = boff[gridDim.x];
        result[kEdResZ] = (uint32_t)Z;
        result[kEdResZ + 1] = (uint32_t)(Z >> 32);
    }
    const uint64_t i0 = (uint64_t)blockIdx.x * chunk, i1 = dmin<uint64_t>(i0 + chunk, H);
    uint64_t run = boff[blockIdx.x];
    for (uint64_t base = i0; base < i1; base += kBlock) {                             // (uniform)
        const uint64_t i = base + threadIdx.x;
        const bool head = i < i1 && (i == 0 || key[i] != key[i - 1]);
        uint32_t total;
        const uint64_t z = run + block_scan_add_excl<uint32_t>(head ? 1u : 0u, part, total);
        run += total;
        if (i < i1 && hrank) hrank[i] = (uint32_t)z;                                  // (Z <= H < 2^32)
        if (head && z < capacity) {
            const uint64_t kx = key[i];
            uint32_t bd = 0xFFFFFFFFu, bs = 0;
            for (uint64_t x = i; x < H && key[x] == kx; x++) {
                const uint32_t h = val[x], dd = dist[h], s = sst[h];
                if (dd < bd || (dd == bd && s > bs)) {
                    bd = dd;
                    bs = s;
                }
            }
            pattern[z] = (uint32_t)(kx >> 32);
            tbegin[z] = bs;
            tend[z] = (uint32_t)kx;
            dout[z] = (uint8_t)bd;
        }
    }
}
// first[j] = the rank of the first head whose pattern is at least j (Z when there is none): the first hit of a pattern
// is a head
__global__ void __launch_bounds__(kBlock)
k_ed_first(const uint64_t* __restrict__ key, const uint32_t* __restrict__ hrank, uint64_t H, uint64_t nq, const uint32_t* __restrict__ result,
           uint64_t* __restrict__ first)
{
    const uint64_t Z = (uint64_t)result[kEdResZ + 1] << 32 | result[kEdResZ];
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j <= nq; j += stride) {
        uint64_t lo = 0, hi = H;                                                      // the first hit with pattern >= j
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if ((key[mid] >> 32) < j) lo = mid + 1; else hi = mid;
        }
        first[j] = lo < H ? hrank[lo] : Z;
    }
}

// [result 64 u32 | po pieces + 1 (u64) | start | end -> cand | off pieces + 1 (u64) | scan partials (u64) | tile counts |
//  tile offsets + total (u64) | one mask byte per thread and tile | K0 | V0 | K1 | V1 | dist | s* | radix scratch |
//  head counts | head offsets + total (u64)], the hit arrays for min(hit_limit, (2 k + 1) cand_limit) hits
struct EdWs {
    uint32_t* result;
    uint64_t* po;
    uint32_t *start, *end;
    uint64_t *off, *part;
    uint32_t* tcnt;
    uint64_t* toff;
    uint8_t* mask;
    uint64_t *K0, *K1;
    uint32_t *V0, *V1;
    uint8_t* dist;
    uint32_t *sst, *scratch, *bcnt;
    uint64_t* boff;
};
template <class A> static void ed_carve(A& a, uint64_t np, uint64_t ntiles, uint64_t hmax, EdWs* w)
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
    w->K0 = a.template take<uint64_t>(hmax);
    w->V0 = a.template take<uint32_t>(hmax);
    w->K1 = a.template take<uint64_t>(hmax);
    w->V1 = a.template take<uint32_t>(hmax);
    w->dist = a.template take<uint8_t>(hmax);
    w->sst = a.template take<uint32_t>(hmax);
    w->scratch = a.template take<uint32_t>(radix_scratch_words(hmax));
    w->bcnt = a.template take<uint32_t>(kMaxGrid);
    w->boff = a.template take<uint64_t>(kMaxGrid + 1);
}
// 0: nothing can run (no pattern, k above 31, 2^32 pieces or more)
static uint64_t ed_piece_count(uint64_t nq, uint32_t k)
{
    if (nq == 0 || k > kEdMaxK || nq > 0xFFFFFFFFull) return 0;
    const uint64_t np = nq * (k + 1);
    return np > 0xFFFFFFFFull ? 0 : np;
}
// the hits one call can hold: hit_limit of them, and no more than 2 k + 1 per candidate the limit admits
static uint64_t ed_hit_room(uint64_t np, uint32_t k, uint64_t cand_limit, uint64_t hit_limit)
{
    const uint64_t cands = dmin<uint64_t>(cand_limit, np * 0xFFFFFFFFull);            // (np < 2^32: no overflow)
    const uint64_t per = 2 * k + 1;
    return dmin<uint64_t>(dmin<uint64_t>(hit_limit, kEdMaxHits), cands > kEdMaxHits / per ? kEdMaxHits : cands * per);
}
uint64_t edit_workspace_bytes(uint64_t nq, uint32_t k, uint64_t cand_limit, uint64_t hit_limit)
{
    const uint64_t np = ed_piece_count(nq, k);
    if (np == 0 || cand_limit == 0 || hit_limit == 0) return 0;
    MemSizer z;
    EdWs w;
    ed_carve(z, np, mem_tiles(np, 0xFFFFFFFFull, cand_limit, ed_tile()), ed_hit_room(np, k, cand_limit, hit_limit), &w);
    return z.used;
}
template <class Search>
int edit_dev(const HmSource& s, Search search, const uint8_t* d_q, const uint64_t* d_qoff, uint64_t nq, uint32_t k, uint64_t cand_limit,
             uint64_t hit_limit, uint32_t* d_pattern, uint32_t* d_tbegin, uint32_t* d_tend, uint8_t* d_dist, uint64_t capacity,
             uint64_t* d_first, uint64_t* cands_out, uint64_t* hits_out, uint64_t* count_out, void* ws, uint64_t ws_bytes, hipStream_t st)
{
    if (!cands_out || !hits_out || !count_out || cand_limit == 0 || hit_limit == 0 || hit_limit > kEdMaxHits || k > kEdMaxK) return SFX_ERR_ARG;
    *cands_out = *hits_out = *count_out = 0;
    if (s.n > 0xFFFFFFFFull || (nq && ed_piece_count(nq, k) == 0)) return SFX_ERR_TOO_LARGE;
    if (capacity && (!d_pattern || !d_tbegin || !d_tend || !d_dist)) return SFX_ERR_ARG;
    if (nq == 0 || s.n == 0) {
        if (d_first) SFX_HIP(hipMemsetAsync(d_first, 0, (nq + 1) * sizeof(uint64_t), st));
        return SFX_OK;
    }
    if (!d_q || !d_qoff || !s.text || !s.sa || (s.starts && (!s.da || s.ndocs == 0))) return SFX_ERR_ARG;
    if (!ws || ws_bytes < edit_workspace_bytes(nq, k, cand_limit, hit_limit)) return SFX_ERR_WORKSPACE;
    const uint32_t kp1 = k + 1, tile = ed_tile();
    const uint64_t np = nq * kp1, ntiles = mem_tiles(np, s.n, cand_limit, tile);      // (>= 1, and no more than the sizer's)
    Arena a(ws, ws_bytes);
    EdWs w;
    ed_carve(a, np, ntiles, ed_hit_room(np, k, cand_limit, hit_limit), &w);
    if (a.overflow) return SFX_ERR_INTERNAL;
    const unsigned cap = dmin<unsigned>(kMaxGrid, grid_cap());
    const unsigned pgrid = (unsigned)dmin<uint64_t>((np + 1 + kBlock - 1) / kBlock, cap);
    const unsigned qgrid = (unsigned)dmin<uint64_t>((nq + 1 + kBlock - 1) / kBlock, cap);
    SFX_HIP(hipMemsetAsync(w.result, 0, 64 * sizeof(uint32_t), st));
    SFX_LAUNCH("hm_pieces", (double)np * 16, k_hm_pieces, pgrid, kBlock, st, d_qoff, nq, kp1, w.po, w.result);
    SFX_LAUNCH("ed_short", (double)nq * 8, k_ed_short, qgrid, kBlock, st, d_qoff, nq, k, w.result);
    SFX_LAUNCH("hm_guard", 0.0, k_hm_guard, pgrid, kBlock, st, np, w.po, (const uint32_t*)w.result);
    SFX_TRY(search(d_q, (const uint64_t*)w.po, np, w.start, w.end, st));
    SFX_LAUNCH("ed_cand", (double)np * 12, k_ed_cand, pgrid, kBlock, st, np, s.n, (const uint32_t*)w.start, w.end, (const uint32_t*)w.result);
    SFX_TRY(scan_u32_to_u64_excl_dev(w.end, np, w.off, w.part, st));
    EdIn in;
    in.e = MemIn{s.text, s.n, s.sa, s.starts, s.da, s.ndocs, d_q, np, w.off, w.start, 0u, 0u, tile, cand_limit, ntiles};
#ifdef SFX_DEV_HOOKS
    in.e.bisect = false;
#endif
    in.qoff = d_qoff;
    in.po = w.po;
    in.k = k;
    in.kp1 = kp1;
    in.hit_limit = hit_limit;
    const unsigned grid = (unsigned)dmin<uint64_t>(ntiles, cap);
    // C stays on the device, so the host has no byte estimate for the candidate kernels: they report 0 algorithmic bytes
    if (s.starts)
        SFX_LAUNCH("ed_count", 0.0, k_ed_count<true>, grid, kBlock, st, in, w.tcnt, w.mask);
    else
        SFX_LAUNCH("ed_count", 0.0, k_ed_count<false>, grid, kBlock, st, in, w.tcnt, w.mask);
    SFX_TRY(scan_u32_to_u64_excl_dev(w.tcnt, ntiles, w.toff, w.part, st));
    if (s.starts)
        SFX_LAUNCH("ed_emit", 0.0, k_ed_emit<true>, grid, kBlock, st, in, (const uint64_t*)w.toff, (const uint8_t*)w.mask, w.K0, w.V0, w.dist,
                   w.sst, w.result);
    else
        SFX_LAUNCH("ed_emit", 0.0, k_ed_emit<false>, grid, kBlock, st, in, (const uint64_t*)w.toff, (const uint8_t*)w.mask, w.K0, w.V0, w.dist,
                   w.sst, w.result);
    uint32_t back[7] = {0, 0, 0, 0, 0, 0, 0};                                         // C, H, the three flags: one read-back
    SFX_TRY(read_back(back, w.result, sizeof(back), st));
    if (back[kHmResBadOrder] || back[kEdResShort]) return SFX_ERR_ARG;
    if (back[kHmResTooLong]) return SFX_ERR_TOO_LARGE;
    const uint64_t C = (uint64_t)back[1] << 32 | back[0], H = (uint64_t)back[3] << 32 | back[2];
    *cands_out = C;
    *hits_out = H;
    if (C > cand_limit || H > hit_limit) return SFX_OK;                               // refused: nothing was written
    if (H == 0) {
        if (d_first) SFX_HIP(hipMemsetAsync(d_first, 0, (nq + 1) * sizeof(uint64_t), st));
        return SFX_OK;
    }
    // the order and the merge, queued behind the read-back and sized by it
    uint64_t *K = w.K0, *Kx = w.K1;
    uint32_t *V = w.V0, *Vx = w.V1;
    auto sorted = [&](int lo, int hi) -> int {
        int in1 = 0;
        SFX_TRY(radix_sort_kv64(K, V, Kx, Vx, H, lo, hi, w.scratch, st, &in1, nullptr, nullptr));
        if (in1) {
            uint64_t* tk = K; K = Kx; Kx = tk;
            uint32_t* tv = V; V = Vx; Vx = tv;
        }
        return SFX_OK;
    };
    SFX_TRY(sorted(0, bits_for(s.n)));                                                // tend <= n
    if (nq > 1) SFX_TRY(sorted(32, 32 + bits_for(nq - 1)));
    const uint64_t want = dmin<uint64_t>((H + kBlock - 1) / kBlock, cap);
    const uint64_t chunk = ((H + want - 1) / want + kBlock - 1) / kBlock * kBlock;
    const unsigned hgrid = (unsigned)((H + chunk - 1) / chunk);
    uint32_t* hrank = d_first ? reinterpret_cast<uint32_t*>(Kx) : nullptr;            // (the sort's spare keys: 8 H bytes)
    SFX_LAUNCH("ed_heads", (double)H * 8, k_ed_heads, hgrid, kBlock, st, (const uint64_t*)K, H, chunk, w.bcnt);
    SFX_TRY(scan_u32_to_u64_excl_dev(w.bcnt, hgrid, w.boff, w.part, st));
    SFX_LAUNCH("ed_reduce", (double)H * 21, k_ed_reduce, hgrid, kBlock, st, (const uint64_t*)K, (const uint32_t*)V, (const uint8_t*)w.dist,
               (const uint32_t*)w.sst, H, chunk, (const uint64_t*)w.boff, capacity, d_pattern, d_tbegin, d_tend, d_dist, hrank, w.result);
    if (d_first)
        SFX_LAUNCH("ed_first", (double)nq * 16, k_ed_first, qgrid, kBlock, st, (const uint64_t*)K, (const uint32_t*)hrank, H, nq,
                   (const uint32_t*)w.result, d_first);
    uint32_t zz[2] = {0, 0};                                                          // Z exists only behind the merge: a second read-back
    SFX_TRY(read_back(zz, w.result + kEdResZ, sizeof(zz), st));
    *count_out = (uint64_t)zz[1] << 32 | zz[0];
    return SFX_OK;
}

}  // namespace sfx
