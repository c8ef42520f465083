// sfx_fm.hip -- FM-index over the (bwt, samples) pair of sfx_bwt_*: backward-search count and locate
// (include/suffix_hip.h).
//
// Rows are the n + 1 sorted rotations of T$ as in section 17; i(R) = R <= primary ? R : R - 1 is the number of bwt
// entries in front of row R, so occ(c, R) counts c in bwt[0 .. i(R)).
//
// One allocation, four parts:
//   hdr     64 words: byte -> dense code (0xFF >= sigma: the byte does not occur), then C[0 .. sigma'] (bwt bytes below code c)
//   blocks  per B bwt entries [sigma' u32: occurrences of every code before the block | B bytes of bwt], and one
//           counts-only block behind the last (the totals); sigma' = sigma rounded up to a multiple of 4, so counts and
//           bytes both start on 16-byte boundaries
//   marks   a bit per row 0 .. n, 480 rows per 64-byte line: word 0 = sampled rows in front of the line, words 1 .. 15
//           the bits
//   mark_k  per sampled row, in row order: its sample number k (the row holds suffix k * sample_step)
//
// occ(c, i) with b = i / B, r = i % B scans from the nearer end: cnt[b][c] + #c in bytes[0 .. r) for r <= B / 2,
// else cnt[b + 1][c] - #c in bytes[r .. end).  Either way one count word and at most B / 2 contiguous bytes inside one
// aligned half of the block, both addresses known from (c, i) alone.
//
// A team of T lanes serves one pattern (k_fm_count) or one rank (k_fm_lookup): the half is T * L bytes, L = 16 or 32
// per lane as one or two 16-byte loads, the bytes are matched by SWAR compare + popcount, partial chunks are masked and
// the team sum goes through __shfl_xor.  Trip counts are wave-uniform (__ballot of "any team still busy"); a team that
// has run out of work keeps executing the collectives without touching memory.
//
// Not covered: collections (per-document terminators), 2-bit packing for DNA, an index built without a table first,
// bidirectional search, the multi-GPU partitioned path.
// Compiled as part of sfx_api.hip (which includes this file), so that every build of the C ABI -- the product's and the
// emulator's of tests/emu -- carries it without a source list of its own.
#pragma once
#include "sfx_host.hpp"

struct sfx_fm {
    void* mem = nullptr;            // the one allocation (nullptr: n == 0)
    uint64_t bytes = 0, n = 0, nsamples = 0, nblk = 0;
    uint32_t sigma = 0, sigp = 0, B = 0, logB = 0, step = 0, primary = 0, T = 1, nload = 1;
    const uint32_t* hdr = nullptr;
    const uint32_t* blocks = nullptr;
    const uint32_t* marks = nullptr;
    const uint32_t* mark_k = nullptr;
};

namespace sfx {

constexpr uint32_t kFmHdrMapWords = 64;                 // 256 code bytes
constexpr uint32_t kFmHdrWords = kFmHdrMapWords + 260;  // + C[0 .. 256] and padding
constexpr uint32_t kFmLineRows = 480;                   // rows per 64-byte mark line
constexpr uint32_t kFmNone = 0xFFFFFFFFu;

// what the kernels need of the handle, by value
struct FmView {
    const uint32_t* hdr;
    const uint32_t* blocks;
    const uint32_t* marks;
    const uint32_t* mark_k;
    uint32_t n, primary, sigma, sigp, stride, B, logB, nload, step, shift, limit;     // stride: words per block
};

// ---- build ------------------------------------------------------------------------------------------------------------
// One wave per block: the bytes go into the block (zeros behind the end of bwt), their counts -- dense codes, this block
// alone -- into its count words; the scan below turns those into occurrences before the block.  The counts-only block
// behind the last gets zeros, which the scan turns into the totals.
struct FmBlockLds {
    uint32_t cnt[kWavesPerBlock][kRadixDev];
    uint32_t map[kFmHdrMapWords];
};
__global__ void __launch_bounds__(kBlock)
k_fm_blocks(const uint8_t* __restrict__ bwt, uint64_t n, uint64_t nblk, uint32_t B, uint32_t sigp, uint32_t stride,
            const uint32_t* __restrict__ hdr, uint32_t* __restrict__ blocks)
{
    __shared__ FmBlockLds s;
    const unsigned w = wave_id(), lane = lane_id();
    if (threadIdx.x < kFmHdrMapWords) s.map[threadIdx.x] = hdr[threadIdx.x];
    __syncthreads();
    const uint8_t* map = reinterpret_cast<const uint8_t*>(s.map);
    const uint64_t waves = (uint64_t)gridDim.x * kWavesPerBlock;
    for (uint64_t b = (uint64_t)blockIdx.x * kWavesPerBlock + w; b <= nblk; b += waves) {
        for (unsigned d = lane; d < sigp; d += kWave) s.cnt[w][d] = 0u;
        wave_sync();
        uint32_t* const out = blocks + b * stride;
        if (b < nblk) {
            const uint64_t base = b * B;
            for (uint32_t p = lane * 4u; p < B; p += kWave * 4u) {
                uint32_t word = 0;
#pragma unroll
                for (uint32_t t = 0; t < 4; t++) {
                    const uint64_t i = base + p + t;
                    if (i < n) {
                        const uint32_t c = bwt[i];
                        word |= c << (8u * t);
                        atomicAdd(&s.cnt[w][map[c]], 1u);
                    }
                }
                out[sigp + (p >> 2)] = word;
            }
        }
        wave_sync();
        for (unsigned d = lane; d < sigp; d += kWave) out[d] = s.cnt[w][d];
        wave_sync();
    }
}
// The per-symbol exclusive scan of the count words across the nblk + 1 blocks, k_bwt_rank_scan_*'s shape restated for
// count words that lie `stride` apart: thread d owns code d, a chunk of blocks per workgroup, the chunks' sums scanned
// by one workgroup.
__global__ void __launch_bounds__(kBlock)
k_fm_scan_count(const uint32_t* __restrict__ blocks, uint32_t stride, uint32_t sigp, uint64_t nb, uint64_t chunk, uint32_t* __restrict__ part)
{
    const uint64_t b = (uint64_t)blockIdx.x * chunk, e = dmin<uint64_t>(b + chunk, nb);
    uint32_t acc = 0;
    if (threadIdx.x < sigp)
        for (uint64_t t = b; t < e; t++) acc += blocks[t * stride + threadIdx.x];
    part[(uint64_t)blockIdx.x * kRadixDev + threadIdx.x] = acc;
}
__global__ void __launch_bounds__(kBlock)
k_fm_scan_top(uint32_t* __restrict__ part, unsigned nchunks)
{
    const unsigned d = threadIdx.x;
    uint32_t run = 0;
    for (unsigned b = 0; b < nchunks; b++) {
        const uint32_t v = part[(uint64_t)b * kRadixDev + d];
        part[(uint64_t)b * kRadixDev + d] = run;
        run += v;
    }
}
__global__ void __launch_bounds__(kBlock)
k_fm_scan_apply(uint32_t* __restrict__ blocks, uint32_t stride, uint32_t sigp, uint64_t nb, uint64_t chunk, const uint32_t* __restrict__ part)
{
    const uint64_t b = (uint64_t)blockIdx.x * chunk, e = dmin<uint64_t>(b + chunk, nb);
    if (threadIdx.x >= sigp) return;
    uint32_t run = part[(uint64_t)blockIdx.x * kRadixDev + threadIdx.x];
    for (uint64_t t = b; t < e; t++) {
        const uint32_t v = blocks[t * stride + threadIdx.x];
        blocks[t * stride + threadIdx.x] = run;
        run += v;
    }
}

// Marks: the bit of every sampled row.  err[0]: a sample outside [1, n]; err[1]: two equal samples (the bit was set
// already); err[2] = samples[0], the primary.
__global__ void __launch_bounds__(kBlock)
k_fm_mark(const uint32_t* __restrict__ samples, uint64_t nsamples, uint32_t n, uint32_t* __restrict__ marks, uint32_t* __restrict__ err)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < nsamples; k += stride) {
        const uint32_t R = samples[k];
        if (k == 0) err[2] = R;
        if (R < 1u || R > n) { err[0] = 1u; continue; }
        const uint32_t line = R / kFmLineRows, bit = R % kFmLineRows, m = 1u << (bit & 31u);
        const uint32_t old = atomicOr(&marks[(uint64_t)line * 16u + 1u + (bit >> 5)], m);
        if (old & m) err[1] = 1u;
    }
}
__device__ __forceinline__ uint32_t fm_line_popc(const uint32_t* __restrict__ line)
{
    uint32_t v = 0;
#pragma unroll
    for (int j = 1; j < 16; j++) v += (uint32_t)__popc(line[j]);
    return v;
}
// the running count of every line: a chunk of lines per workgroup; APPLY false leaves the chunk's sum in part[], APPLY
// true starts from the chunk's scanned sum and writes word 0 of every line
template <bool APPLY>
__global__ void __launch_bounds__(kBlock)
k_fm_mark_scan(uint32_t* __restrict__ marks, uint64_t nlines, uint64_t chunk, uint32_t* __restrict__ part)
{
    __shared__ uint32_t sh[kWavesPerBlock];
    const uint64_t b = (uint64_t)blockIdx.x * chunk, e = dmin<uint64_t>(b + chunk, nlines);
    uint32_t carry = APPLY ? part[blockIdx.x] : 0u;
    for (uint64_t base = b; base < e; base += kBlock) {
        const uint64_t line = base + threadIdx.x;
        const bool live = line < e;
        const uint32_t v = live ? fm_line_popc(marks + line * 16u) : 0u;
        uint32_t total;
        const uint32_t excl = block_scan_add_excl<uint32_t>(v, sh, total);
        if (APPLY && live) marks[line * 16u] = carry + excl;
        carry += total;
    }
    if (!APPLY && threadIdx.x == 0) part[blockIdx.x] = carry;
}
// one workgroup: the exclusive scan of up to kMaxGrid chunk sums, eight per thread
__global__ void __launch_bounds__(kBlock)
k_fm_mark_top(uint32_t* __restrict__ part, unsigned nchunks)
{
    __shared__ uint32_t sh[kWavesPerBlock];
    constexpr unsigned per = kMaxGrid / kBlock;
    uint32_t v[per], sum = 0;
#pragma unroll
    for (unsigned j = 0; j < per; j++) {
        const unsigned idx = threadIdx.x * per + j;
        v[j] = idx < nchunks ? part[idx] : 0u;
        sum += v[j];
    }
    uint32_t total;
    uint32_t run = block_scan_add_excl<uint32_t>(sum, sh, total);
#pragma unroll
    for (unsigned j = 0; j < per; j++) {
        const unsigned idx = threadIdx.x * per + j;
        if (idx < nchunks) part[idx] = run;
        run += v[j];
    }
}
// sampled rows in front of row R (whose own bit may or may not be set); word = the line's word that holds R's bit
__device__ __forceinline__ uint32_t fm_mark_rank(const uint32_t* __restrict__ marks, uint32_t R)
{
    const uint32_t ln = R / kFmLineRows, bit = R % kFmLineRows, wi = bit >> 5;
    const uint4* const q = reinterpret_cast<const uint4*>(marks + (uint64_t)ln * 16u);
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint4 x = q[j];
        w[4 * j] = x.x; w[4 * j + 1] = x.y; w[4 * j + 2] = x.z; w[4 * j + 3] = x.w;
    }
    uint32_t rank = w[0];
#pragma unroll
    for (uint32_t j = 1; j < 16; j++) {
        const uint32_t full = j - 1u < wi ? 0xFFFFFFFFu : (j - 1u == wi ? (1u << (bit & 31u)) - 1u : 0u);
        rank += (uint32_t)__popc(w[j] & full);
    }
    return rank;
}
__global__ void __launch_bounds__(kBlock)
k_fm_scatter(const uint32_t* __restrict__ samples, uint64_t nsamples, uint32_t n, const uint32_t* __restrict__ marks,
             uint32_t* __restrict__ mark_k)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < nsamples; k += stride) {
        const uint32_t R = samples[k];
        if (R < 1u || R > n) continue;
        const uint32_t rank = fm_mark_rank(marks, R);                  // (< the number of set bits <= nsamples)
        if (rank < nsamples) mark_k[rank] = (uint32_t)k;
    }
}

// ---- occ --------------------------------------------------------------------------------------------------------------
// high bit of every byte of x that is zero; exact (no carry leaves a byte)
__device__ __forceinline__ uint32_t fm_zero_bytes(uint32_t x)
{
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}
// the bytes of the word at in-block position p that lie in [a, e), as a mask over fm_zero_bytes' flags
__device__ __forceinline__ uint32_t fm_range_mask(uint32_t p, uint32_t a, uint32_t e)
{
    const uint32_t lo = a > p ? dmin<uint32_t>(a - p, 4u) : 0u, hi = e > p ? dmin<uint32_t>(e - p, 4u) : 0u;
    return (uint32_t)((0xFFFFFFFFull << (8u * lo)) & ~(0xFFFFFFFFull << (8u * hi)));
}
// Where occ(c, i) reads: the count word's block, the half of block b the scan runs in and the byte range [a, e) of it.
struct FmProbe {
    uint32_t b, a, e;
    bool fwd;
};
__device__ __forceinline__ FmProbe fm_probe(const FmView& v, uint32_t i)
{
    FmProbe p;
    p.b = i >> v.logB;
    const uint32_t r = i & (v.B - 1u);
    const uint32_t blen = dmin<uint32_t>(v.B, v.n - (p.b << v.logB));  // (0 for the counts-only block: r == 0, nothing is read)
    p.fwd = r <= (v.B >> 1);
    p.a = p.fwd ? 0u : r;
    p.e = p.fwd ? r : blen;
    return p;
}
// this lane's chunk of a half: L = 16 * nload bytes at in-block position p0; loaded only where it meets [a, e)
struct FmChunk {
    uint4 w[2];
    uint32_t p0;
};
template <int T>
__device__ __forceinline__ void fm_load_chunk(const FmView& v, uint32_t tl, uint32_t b, bool fwd, uint32_t a, uint32_t e, bool live,
                                              FmChunk& c)
{
    const uint32_t L = 16u * v.nload;
    c.p0 = (fwd ? 0u : (v.B >> 1)) + tl * L;
    c.w[0].x = c.w[0].y = c.w[0].z = c.w[0].w = 0u;
    c.w[1] = c.w[0];
    const uint4* const q = reinterpret_cast<const uint4*>(v.blocks + (uint64_t)b * v.stride + v.sigp + (c.p0 >> 2));
    if (live && a < e && c.p0 < e && c.p0 + 16u > a) c.w[0] = q[0];
    if (live && a < e && v.nload > 1u && c.p0 + 16u < e && c.p0 + 32u > a) c.w[1] = q[1];
}
__device__ __forceinline__ uint32_t fm_chunk_count(const FmChunk& c, uint32_t nload, uint32_t cx, uint32_t a, uint32_t e)
{
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t j = 0; j < 2; j++) {
        if (j >= nload) break;
        const uint32_t p = c.p0 + 16u * j;
        cnt += (uint32_t)__popc(fm_zero_bytes(c.w[j].x ^ cx) & fm_range_mask(p, a, e));
        cnt += (uint32_t)__popc(fm_zero_bytes(c.w[j].y ^ cx) & fm_range_mask(p + 4u, a, e));
        cnt += (uint32_t)__popc(fm_zero_bytes(c.w[j].z ^ cx) & fm_range_mask(p + 8u, a, e));
        cnt += (uint32_t)__popc(fm_zero_bytes(c.w[j].w ^ cx) & fm_range_mask(p + 12u, a, e));
    }
    return cnt;
}
template <int T> __device__ __forceinline__ uint32_t fm_team_sum(uint32_t x)
{
#pragma unroll
    for (int d = 1; d < T; d <<= 1) x += __shfl_xor(x, d, T);
    return x;
}
struct FmLds {
    uint32_t map[kFmHdrMapWords];
    uint32_t C[kRadixDev + 4];
};
__device__ __forceinline__ void fm_load_lds(const FmView& v, FmLds& s)
{
    for (unsigned k = threadIdx.x; k < kFmHdrMapWords; k += kBlock) s.map[k] = v.hdr[k];
    for (unsigned k = threadIdx.x; k <= v.sigp; k += kBlock) s.C[k] = v.hdr[kFmHdrMapWords + k];
    __syncthreads();
}

// ---- count ------------------------------------------------------------------------------------------------------------
// A team per pattern, taken round-robin; one backward step per iteration of the wave's loop.  The two occs of a step are
// independent: both count words and both chunks are requested before any is used, and where both indices fall into the
// same half of the same block one chunk serves both.
template <int T>
__global__ void __launch_bounds__(kBlock)
k_fm_count(const FmView v, const uint8_t* __restrict__ qbytes, const uint64_t* __restrict__ qoff, uint64_t nq,
           uint32_t* __restrict__ start, uint32_t* __restrict__ end)
{
    __shared__ FmLds s;
    fm_load_lds(v, s);
    const uint8_t* map = reinterpret_cast<const uint8_t*>(s.map);
    const uint32_t tl = threadIdx.x & (T - 1);
    const uint64_t nteams = (uint64_t)gridDim.x * (kBlock / T);
    uint64_t j = (uint64_t)blockIdx.x * (kBlock / T) + threadIdx.x / T;
    bool have = j < nq;
    const uint8_t* q = qbytes;
    uint64_t k = 0;                                                    // pattern bytes still to go
    // rows [lo, hi) as il = i(lo), ih = i(hi) (bwt entries in front of them) and the answer so far [xl, xh) = [lo - 1,
    // hi - 1): none of them leaves [0, n], whereas hi itself reaches n + 1
    uint32_t il = 0, ih = v.n, xl = 0, xh = 0;
    if (have) {
        const uint64_t o = qoff[j];
        q = qbytes + o;
        k = qoff[j + 1] - o;
    }
    while (__ballot(have)) {
        if (have && k == 0) {                                          // this pattern is done: report, take the next
            if (tl == 0) {
                start[j] = xl < xh ? xl : 0u;
                end[j] = xl < xh ? xh : 0u;
            }
            j += nteams;
            have = j < nq;
            il = 0; ih = v.n; xl = 0; xh = 0;
            if (have) {
                const uint64_t o = qoff[j];
                q = qbytes + o;
                k = qoff[j + 1] - o;
            }
        }
        const bool stepping = have && k > 0;
        const uint32_t c = stepping ? q[k - 1] : 0u;
        const uint32_t code = map[c];
        const bool live = stepping && code < v.sigma;                   // (0xFF is a live code when all 256 bytes occur)
        const FmProbe pl = fm_probe(v, live ? il : 0u), ph = fm_probe(v, live ? ih : 0u);
        const bool same = pl.b == ph.b && pl.fwd == ph.fwd;
        // the reads of the step, all four before any use
        uint32_t cwl = 0, cwh = 0;
        if (live) {
            cwl = v.blocks[(uint64_t)(pl.b + (pl.fwd ? 0u : 1u)) * v.stride + code];
            cwh = v.blocks[(uint64_t)(ph.b + (ph.fwd ? 0u : 1u)) * v.stride + code];
        }
        FmChunk cl, ch;
        fm_load_chunk<T>(v, tl, pl.b, pl.fwd, same ? dmin(pl.a, ph.a) : pl.a, same ? dmax(pl.e, ph.e) : pl.e, live, cl);
        fm_load_chunk<T>(v, tl, ph.b, ph.fwd, ph.a, ph.e, live && !same, ch);
        const uint32_t cx = c * 0x01010101u;
        const uint32_t nl = fm_chunk_count(cl, v.nload, cx, pl.a, pl.e);
        const uint32_t nh = same ? fm_chunk_count(cl, v.nload, cx, ph.a, ph.e) : fm_chunk_count(ch, v.nload, cx, ph.a, ph.e);
        const uint32_t sum = fm_team_sum<T>(nl | (nh << 16));         // (each at most B / 2 <= 2048)
        if (live) {
            const uint32_t sl = sum & 0xFFFFu, sh = sum >> 16;
            xl = s.C[code] + (pl.fwd ? cwl + sl : cwl - sl);           // lo = 1 + xl, hi = 1 + xh
            xh = s.C[code] + (ph.fwd ? cwh + sh : cwh - sh);
            il = xl + (xl < v.primary ? 1u : 0u);
            ih = xh + (xh < v.primary ? 1u : 0u);
            k = xl < xh ? k - 1 : 0;
        } else if (stepping) {                                         // a byte the text lacks
            xl = xh = 0;
            k = 0;
        }
    }
}

// ---- lookup -----------------------------------------------------------------------------------------------------------
// A team per rank.  One iteration looks at one row: its mark word, and -- requested at the same time, used only if the
// row is not sampled -- the bwt byte of the row and the chunk of its half, then the count word of that byte.  A walk of
// `limit` steps without a sampled row is cut off (no true transform has one) and reported as UINT32_MAX, as is a rank
// >= n and a position that would lie outside the text.  For every input R stays in [1, n]: the counts are those of the
// bytes the blocks hold, and the primary row is always sampled, so it is never dereferenced.
template <int T>
__global__ void __launch_bounds__(kBlock)
k_fm_lookup(const FmView v, const uint32_t* __restrict__ ranks, uint64_t first, uint64_t count, uint32_t* __restrict__ pos)
{
    __shared__ FmLds s;
    fm_load_lds(v, s);
    const uint8_t* map = reinterpret_cast<const uint8_t*>(s.map);
    const uint32_t tl = threadIdx.x & (T - 1);
    const uint64_t nteams = (uint64_t)gridDim.x * (kBlock / T);
    uint64_t j = (uint64_t)blockIdx.x * (kBlock / T) + threadIdx.x / T;
    bool have = j < count, done = false;
    uint32_t R = 0, steps = 0, res = kFmNone;
    if (have) {
        const uint64_t r = ranks ? (uint64_t)ranks[j] : first + j;
        done = r >= v.n;
        R = done ? 0u : (uint32_t)r + 1u;
    }
    while (__ballot(have)) {
        if (have && done) {
            if (tl == 0) pos[j] = res;
            j += nteams;
            have = j < count;
            done = false;
            res = kFmNone;
            steps = 0;
            if (have) {
                const uint64_t r = ranks ? (uint64_t)ranks[j] : first + j;
                done = r >= v.n;
                R = done ? 0u : (uint32_t)r + 1u;
            }
        }
        const bool live = have && !done;
        const uint32_t Rl = live ? R : 1u;
        const uint32_t ln = Rl / kFmLineRows, bit = Rl % kFmLineRows;
        const uint32_t i = Rl < v.primary ? Rl : Rl - 1u;            // (R != primary whenever it is used: see below)
        const FmProbe p = fm_probe(v, i);
        uint32_t mw = 0, c = 0;
        if (live) {
            mw = v.marks[(uint64_t)ln * 16u + 1u + (bit >> 5)];
            c = (v.blocks[(uint64_t)p.b * v.stride + v.sigp + ((i & (v.B - 1u)) >> 2)] >> (8u * (i & 3u))) & 0xFFu;
        }
        FmChunk ck;
        fm_load_chunk<T>(v, tl, p.b, p.fwd, p.a, p.e, live, ck);
        const bool sampled = live && ((mw >> (bit & 31u)) & 1u);
        const bool walk = live && !sampled;                           // (the primary row is sampled: i < n and c is a bwt byte)
        const uint32_t code = walk ? map[c] : 0u;
        uint32_t cw = 0;
        if (walk) cw = v.blocks[(uint64_t)(p.b + (p.fwd ? 0u : 1u)) * v.stride + code];
        const uint32_t sum = fm_team_sum<T>(fm_chunk_count(ck, v.nload, c * 0x01010101u, p.a, p.e));
        if (sampled) {
            const uint32_t kk = v.mark_k[fm_mark_rank(v.marks, R)];
            const uint64_t at = ((uint64_t)kk << v.shift) * (v.step ? 1u : 0u) + steps;
            res = at < v.n ? (uint32_t)at : kFmNone;
            done = true;
        } else if (walk) {
            if (++steps >= v.limit) {
                done = true;                                           // cut off: res stays UINT32_MAX
            } else {
                R = 1u + s.C[code] + (p.fwd ? cw + sum : cw - sum);
            }
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------
struct FmLayout {
    uint64_t nblk, nlines, stride, hdr_off, blocks_off, marks_off, mark_k_off, bytes;
};
static uint64_t fm_align(uint64_t x) { return (x + kArenaAlign - 1) & ~(kArenaAlign - 1); }
static FmLayout fm_layout(uint64_t n, uint64_t nsamples, uint32_t B, uint32_t sigp)
{
    FmLayout L;
    L.nblk = (n + B - 1) / B;
    L.nlines = (n + kFmLineRows) / kFmLineRows;                         // rows 0 .. n
    L.stride = sigp + B / 4;
    L.hdr_off = 0;
    L.blocks_off = fm_align(kFmHdrWords * 4ull);
    L.marks_off = L.blocks_off + fm_align((L.nblk * L.stride + sigp) * 4ull);
    L.mark_k_off = L.marks_off + fm_align(L.nlines * 64ull);
    L.bytes = L.mark_k_off + fm_align(nsamples * 4ull);
    return L;
}
static bool fm_occ_step_ok(uint32_t B) { return B == 0 || (B >= 32u && B <= 4096u && (B & (B - 1u)) == 0); }
static uint32_t fm_auto_step(uint32_t sigp)
{
    uint32_t B = 64;
    while (B < 16u * sigp && B < 4096u) B <<= 1;
    return B;
}
static bool fm_step_ok(uint32_t step) { return (step & (step - 1u)) == 0; }
uint64_t fm_bytes(uint64_t n, uint32_t step, uint32_t occ_step)
{
    if (!fm_step_ok(step) || !fm_occ_step_ok(occ_step) || n > 0xFFFFFFFFull || n == 0) return 0;
    const uint64_t ns = bwt_sample_count(n, step);
    if (occ_step) return fm_layout(n, ns, occ_step, 256).bytes;
    // the step follows sigma': every choice keeps the count words within a quarter of the bytes, and one partial block,
    // the counts-only block and the alignment stay under 8 KiB
    const FmLayout L = fm_layout(n, ns, 4096, 256);
    return L.bytes + 8192;
}
static unsigned fm_grid(uint64_t items) { return (unsigned)dmax<uint64_t>(1, dmin<uint64_t>((items + kBlock - 1) / kBlock, dmin<unsigned>(kMaxGrid, grid_cap()))); }
static FmView fm_view(const sfx_fm* fm)
{
    FmView v;
    v.hdr = fm->hdr; v.blocks = fm->blocks; v.marks = fm->marks; v.mark_k = fm->mark_k;
    v.n = (uint32_t)fm->n; v.primary = fm->primary; v.sigma = fm->sigma; v.sigp = fm->sigp; v.stride = fm->sigp + fm->B / 4;
    v.B = fm->B; v.logB = fm->logB; v.nload = fm->nload; v.step = fm->step;
    v.shift = fm->step ? (uint32_t)bits_for(fm->step) - 1u : 0u;
    v.limit = (uint32_t)(fm->step ? dmin<uint64_t>(fm->n, fm->step) : fm->n);
    return v;
}
void fm_destroy(sfx_fm* fm)
{
    if (!fm) return;
    if (fm->mem) (void)dev_free(fm->mem);
    delete fm;
}
static int fm_build(sfx_fm* fm, const uint8_t* d_bwt, const uint32_t* d_samples, uint32_t occ_step, hipStream_t st, void** tmp_out)
{
    const uint64_t n = fm->n;
    // the alphabet: exact byte counts, read back once (creation needs sigma before it can size the blocks)
    void* tmp = nullptr;
    SFX_HIP(dev_malloc(&tmp, 4096 + (uint64_t)kMaxGrid * kRadixDev * 4));
    *tmp_out = tmp;
    uint64_t* d_bins = (uint64_t*)tmp;
    uint32_t* d_err = (uint32_t*)((char*)tmp + 2048);
    uint32_t* d_part = (uint32_t*)((char*)tmp + 4096);
    SFX_TRY(byte_histogram_dev(d_bwt, 0, n, d_bins, st));
    uint64_t bins[256];
    SFX_TRY(read_back(bins, d_bins, sizeof(bins), st));
    uint32_t hdr[kFmHdrWords];
    memset(hdr, 0, sizeof(hdr));
    uint8_t* map = reinterpret_cast<uint8_t*>(hdr);
    uint32_t* C = hdr + kFmHdrMapWords;
    uint32_t sigma = 0;
    uint64_t run = 0;
    for (int c = 0; c < 256; c++) {
        map[c] = 0xFF;
        if (bins[c]) {
            map[c] = (uint8_t)sigma;
            C[sigma++] = (uint32_t)run;
            run += bins[c];
        }
    }
    if (run != n) return SFX_ERR_INTERNAL;
    fm->sigma = sigma;
    fm->sigp = (sigma + 3u) & ~3u;
    for (uint32_t d = sigma; d <= fm->sigp; d++) C[d] = (uint32_t)n;
    fm->B = occ_step ? occ_step : fm_auto_step(fm->sigp);
    fm->logB = (uint32_t)bits_for(fm->B) - 1u;
    // the half of a block is T lanes x 16 * nload bytes
    const uint32_t half = fm->B / 2;
    fm->T = half >= 1024 ? 64 : half >= 256 ? 16 : half >= 64 ? 4 : 1;
    fm->nload = half / fm->T / 16;
    const FmLayout L = fm_layout(n, fm->nsamples, fm->B, fm->sigp);
    SFX_HIP(dev_malloc(&fm->mem, L.bytes));
    fm->bytes = L.bytes;
    char* base = (char*)fm->mem;
    uint32_t* d_hdr = (uint32_t*)(base + L.hdr_off);
    uint32_t* d_blocks = (uint32_t*)(base + L.blocks_off);
    uint32_t* d_marks = (uint32_t*)(base + L.marks_off);
    uint32_t* d_mark_k = (uint32_t*)(base + L.mark_k_off);
    fm->hdr = d_hdr; fm->blocks = d_blocks; fm->marks = d_marks; fm->mark_k = d_mark_k; fm->nblk = L.nblk;
    SFX_HIP(hipMemcpyAsync(d_hdr, hdr, sizeof(hdr), hipMemcpyHostToDevice, st));
    SFX_HIP(hipStreamSynchronize(st));                                  // (hdr is this frame's)
    SFX_HIP(hipMemsetAsync(d_marks, 0, L.nlines * 64ull, st));
    SFX_HIP(hipMemsetAsync(d_err, 0, 64 * sizeof(uint32_t), st));
    const uint32_t stride = (uint32_t)L.stride;
    const unsigned bgrid = (unsigned)dmin<uint64_t>((L.nblk + 1 + kWavesPerBlock - 1) / kWavesPerBlock, dmin<unsigned>(kMaxGrid, grid_cap()));
    SFX_LAUNCH("fm_build", (double)n * 2 + (double)L.nblk * fm->sigp * 4, k_fm_blocks, bgrid, kBlock, st, d_bwt, n, L.nblk, fm->B, fm->sigp,
               stride, (const uint32_t*)d_hdr, d_blocks);
    const uint64_t nb = L.nblk + 1;
    const unsigned nchunks = (unsigned)dmin<uint64_t>(nb, dmin<unsigned>(kMaxGrid, grid_cap()));
    const uint64_t chunk = (nb + nchunks - 1) / nchunks;
    const double cbytes = (double)nb * fm->sigp * 4;
    SFX_LAUNCH("fm_build", cbytes, k_fm_scan_count, nchunks, kBlock, st, (const uint32_t*)d_blocks, stride, fm->sigp, nb, chunk, d_part);
    SFX_LAUNCH("fm_build", (double)nchunks * kRadixDev * 8, k_fm_scan_top, 1, kBlock, st, d_part, nchunks);
    SFX_LAUNCH("fm_build", cbytes * 2, k_fm_scan_apply, nchunks, kBlock, st, d_blocks, stride, fm->sigp, nb, chunk, (const uint32_t*)d_part);
    const unsigned sgrid = fm_grid(fm->nsamples);
    SFX_LAUNCH("fm_build", (double)fm->nsamples * 68, k_fm_mark, sgrid, kBlock, st, d_samples, fm->nsamples, (uint32_t)n, d_marks, d_err);
    const unsigned mchunks = (unsigned)dmin<uint64_t>((L.nlines + kBlock - 1) / kBlock, dmin<unsigned>(kMaxGrid, grid_cap()));
    const uint64_t mchunk = (L.nlines + mchunks - 1) / mchunks;
    SFX_LAUNCH("fm_build", (double)L.nlines * 64, k_fm_mark_scan<false>, mchunks, kBlock, st, d_marks, L.nlines, mchunk, d_part);
    SFX_LAUNCH("fm_build", (double)mchunks * 8, k_fm_mark_top, 1, kBlock, st, d_part, mchunks);
    SFX_LAUNCH("fm_build", (double)L.nlines * 68, k_fm_mark_scan<true>, mchunks, kBlock, st, d_marks, L.nlines, mchunk, d_part);
    SFX_LAUNCH("fm_build", (double)fm->nsamples * 72, k_fm_scatter, sgrid, kBlock, st, d_samples, fm->nsamples, (uint32_t)n,
               (const uint32_t*)d_marks, d_mark_k);
    uint32_t err[4] = {0, 0, 0, 0};
    SFX_TRY(read_back(err, d_err, sizeof(err), st));
    if (err[0] | err[1]) return SFX_ERR_ARG;
    fm->primary = err[2];
    return SFX_OK;
}
int fm_create_dev(const uint8_t* d_bwt, uint64_t n, const uint32_t* d_samples, uint64_t nsamples, uint32_t step, uint32_t occ_step,
                  hipStream_t st, sfx_fm** out)
{
    if (!out) return SFX_ERR_ARG;
    *out = nullptr;
    if (!fm_step_ok(step) || !fm_occ_step_ok(occ_step)) return SFX_ERR_ARG;
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (nsamples != bwt_sample_count(n, step)) return SFX_ERR_ARG;
    if (n && (!d_bwt || !d_samples)) return SFX_ERR_ARG;
    sfx_fm* fm = new sfx_fm;
    fm->n = n;
    fm->nsamples = nsamples;
    fm->step = step;
    fm->B = occ_step;
    int rc = SFX_OK;
    if (n) {
        void* tmp = nullptr;
        rc = fm_build(fm, d_bwt, d_samples, occ_step, st, &tmp);
        if (tmp) {
            (void)hipStreamSynchronize(st);
            (void)dev_free(tmp);
        }
    }
    if (rc != SFX_OK) {
        fm_destroy(fm);
        return rc;
    }
    *out = fm;
    return SFX_OK;
}
int fm_info(const sfx_fm* fm, sfx_fm_info_t* info)
{
    if (!fm || !info) return SFX_ERR_ARG;
    info->n = fm->n;
    info->bytes = fm->bytes;
    info->sigma = fm->sigma;
    info->occ_step = fm->B;
    info->sample_step = fm->step;
    info->nsamples = (uint32_t)fm->nsamples;
    return SFX_OK;
}
template <template <int> class Launch, class... A> static int fm_dispatch(uint32_t T, A... a)
{
    switch (T) {
    case 1: return Launch<1>::run(a...);
    case 4: return Launch<4>::run(a...);
    case 16: return Launch<16>::run(a...);
    case 64: return Launch<64>::run(a...);
    }
    return SFX_ERR_INTERNAL;
}
template <int T> struct FmCountLaunch {
    static int run(const FmView& v, const uint8_t* q, const uint64_t* off, uint64_t nq, uint32_t* s, uint32_t* e, double bytes, hipStream_t st)
    {
        SFX_LAUNCH("fm_count", bytes, k_fm_count<T>, fm_grid(nq * T), kBlock, st, v, q, off, nq, s, e);
        return SFX_OK;
    }
};
template <int T> struct FmLookupLaunch {
    static int run(const FmView& v, const uint32_t* ranks, uint64_t first, uint64_t count, uint32_t* pos, double bytes, hipStream_t st)
    {
        SFX_LAUNCH("fm_lookup", bytes, k_fm_lookup<T>, fm_grid(count * T), kBlock, st, v, ranks, first, count, pos);
        return SFX_OK;
    }
};
int fm_count_dev(const sfx_fm* fm, const uint8_t* d_q, const uint64_t* d_qoff, uint64_t nq, uint32_t* d_start, uint32_t* d_end, hipStream_t st)
{
    if (!fm) return SFX_ERR_ARG;
    if (nq == 0) return SFX_OK;
    if (!d_qoff || !d_start || !d_end) return SFX_ERR_ARG;
    if (fm->n == 0) {                                                   // the empty index: every interval is empty
        SFX_HIP(hipMemsetAsync(d_start, 0, nq * sizeof(uint32_t), st));
        SFX_HIP(hipMemsetAsync(d_end, 0, nq * sizeof(uint32_t), st));
        return SFX_OK;
    }
    return fm_dispatch<FmCountLaunch>(fm->T, fm_view(fm), d_q, d_qoff, nq, d_start, d_end, (double)nq * 8 * 128, st);
}
int fm_lookup_dev(const sfx_fm* fm, const uint32_t* d_ranks, uint64_t first, uint64_t count, uint32_t* d_pos, hipStream_t st)
{
    if (!fm) return SFX_ERR_ARG;
    if ((fm->step ? dmin<uint64_t>(fm->n, fm->step) : fm->n) > SFX_UNBWT_MAX_CHAIN) return SFX_ERR_ARG;
    if (count == 0) return SFX_OK;
    if (!d_pos) return SFX_ERR_ARG;
    if (fm->n == 0) {                                                   // no rank is < n
        SFX_HIP(hipMemsetAsync(d_pos, 0xFF, count * sizeof(uint32_t), st));
        return SFX_OK;
    }
    return fm_dispatch<FmLookupLaunch>(fm->T, fm_view(fm), d_ranks, first, count, d_pos,
                                       (double)count * (fm->step ? fm->step / 2 + 1 : fm->n / 2 + 1) * 192, st);
}

}  // namespace sfx
