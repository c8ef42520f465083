// sfx_tree.hip -- suffix-tree topology as flat arrays, and the generalized-suffix-array lookup
// (/root/reference/suffix_tree/src/lib.rs:392-505 `to_suffix_tree`,
// /root/reference/README.md:60-74).
//
// The reference builds its suffix tree by one left-to-right sweep over (SA, LCP) with a stack of
// ancestors: every internal node is an *lcp-interval* -- a maximal range of ranks [lb, rb] whose
// suffixes share `depth` symbols, depth = min lcp[lb+1..rb] > max(lcp[lb], lcp[rb+1]).  The sweep is
// serial; the same tree falls out of two all-nearest-smaller-value problems on the LCP array:
//   for a boundary p (between ranks p-1 and p, value lcp[p]):
//     lb[p] = the nearest q < p with lcp[q] < lcp[p]          (q = 0 at the latest: lcp[0] = 0 = the root)
//     rb[p] = (the nearest q > p with lcp[q] < lcp[p]) - 1    (n - 1 at the latest)
//   -> [lb, rb] at depth lcp[p] is the node that boundary p belongs to; its id is its LEFTMOST boundary
//      with that value, node[p] = the first q > lb[p] with lcp[q] <= lcp[p];
//   parent = the node of whichever of the two delimiting boundaries lb[p] / rb[p] + 1 is deeper;
//   a leaf (rank r) hangs under the node of the deeper of its two boundaries r and r + 1.
// Boundaries with lcp 0 belong to the root (id 0, [0, n-1], depth 0).  Searches run over a pyramid of
// block minima (64-ary), so a nearest-smaller query costs O(64 log_64 n) reads in the worst case and a
// handful for the nearby answers that dominate.
#include "sfx_host.hpp"

namespace sfx {

// (kPyrFan, kPyrMaxLevels, Pyramid and range_min live in sfx_device.hpp: the LCE index's development baseline reads them too)
constexpr uint32_t kNoNode = 0xFFFFFFFFu;

__global__ void __launch_bounds__(kBlock)
k_pyr_reduce(const uint32_t* __restrict__ in, uint64_t n_in, uint32_t* __restrict__ out, uint64_t n_out, int first_is_zero)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n_out; j += stride) {
        uint32_t m = 0xFFFFFFFFu;
        const uint64_t b = j * kPyrFan, e = dmin<uint64_t>(b + kPyrFan, n_in);
        for (uint64_t i = b; i < e; i++) m = dmin(m, in[i]);
        out[j] = (j == 0 && first_is_zero) ? 0u : m;             // (boundary 0 has depth 0 whatever lcp[0] holds)
    }
}

// nearest q < p with lcp[q] < v (v > 0, so q = 0 qualifies at the latest)
__device__ __forceinline__ uint64_t prev_smaller(const Pyramid& py, uint64_t p, uint32_t v)
{
    int l = 0;
    int64_t idx = (int64_t)p - 1;
    for (;;) {                                               // climb: scan to the left inside the current block
        bool found = false;
        for (;;) {
            if ((l == 0 && idx == 0) || py.lvl[l][idx] < v) { found = true; break; }     // (boundary 0: depth 0 by definition)
            if (idx % kPyrFan == 0) break;
            idx--;
        }
        if (found) break;
        idx = idx / kPyrFan - 1;                             // the block to the left, one level up
        l++;
    }
    while (l > 0) {                                          // descend: the rightmost child below v
        l--;
        int64_t c = dmin<int64_t>(idx * kPyrFan + kPyrFan - 1, (int64_t)py.len[l] - 1);
        while (!(l == 0 && c == 0) && py.lvl[l][c] >= v) c--;
        idx = c;
    }
    return (uint64_t)idx;
}
// nearest q > p with lcp[q] < v, or n if there is none; with `or_equal`, lcp[q] <= v instead
__device__ __forceinline__ uint64_t next_smaller(const Pyramid& py, uint64_t p, uint32_t v, bool or_equal, uint64_t n)
{
    auto hit = [&](uint32_t x) { return or_equal ? x <= v : x < v; };
    int l = 0;
    uint64_t idx = p + 1;
    for (;;) {
        if (idx >= py.len[l]) return n;
        bool found = false;
        for (;;) {
            if (hit(py.lvl[l][idx])) { found = true; break; }
            if (idx % kPyrFan == kPyrFan - 1 || idx + 1 >= py.len[l]) break;
            idx++;
        }
        if (found) break;
        idx = idx / kPyrFan + 1;
        l++;
        if (l >= py.levels) return n;
    }
    while (l > 0) {
        l--;
        uint64_t c = idx * kPyrFan;
        while (!hit(py.lvl[l][c])) c++;
        idx = c;
    }
    return idx;
}

// per boundary p in [0, n): lb, rb, node id (0 for the root: p = 0 and every boundary of depth 0).
// The three nearest-smaller searches of a boundary nearly always end inside its neighbourhood: a workgroup stages
// kIvTile values in LDS under a binary min-tree (tr[1] = the tile's minimum, tr[kIvTile + i] = value i) and answers
// them there -- up the tree until a sibling holds a smaller value, down to the nearest one: <= 2 log2(kIvTile) LDS reads,
// the same for every lane (a linear scan was measured first: one lane with a distant answer holds up its wave, 170 ms
// per 10^9 boundaries against round 2's 126-133 through the global pyramid alone).  A search that leaves the tile
// continues in the global min-pyramid from the tile's edge.
constexpr int kIvTile = 2048;
// nearest position < i (tile coordinates) with a value < v, or -1
__device__ __forceinline__ int iv_prev_smaller(const uint32_t* tr, int i, uint32_t v)
{
    unsigned k = (unsigned)(kIvTile + i);
    for (;;) {
        if (k <= 1u) return -1;
        if ((k & 1u) && tr[k - 1u] < v) { k--; break; }
        k >>= 1;
    }
    while (k < (unsigned)kIvTile) {
        k = 2u * k + 1u;
        if (tr[k] >= v) k--;
    }
    return (int)k - kIvTile;
}
// nearest position > i with a value < v (or <= v with or_equal), or kIvTile
__device__ __forceinline__ int iv_next_smaller(const uint32_t* tr, int i, uint32_t v, bool or_equal)
{
    auto hit = [&](uint32_t x) { return or_equal ? x <= v : x < v; };
    unsigned k = (unsigned)(kIvTile + i);
    for (;;) {
        if (k <= 1u) return kIvTile;
        if (!(k & 1u) && hit(tr[k + 1u])) { k++; break; }
        k >>= 1;
    }
    while (k < (unsigned)kIvTile) {
        k = 2u * k;
        if (!hit(tr[k])) k++;
    }
    return (int)k - kIvTile;
}
// A search that leaves the tile goes on in the global pyramid -- dozens of dependent loads, for which the other 63
// lanes of the wave would wait.  Such boundaries (a fraction of a per cent: the shallow ones, whose intervals are huge)
// are therefore LISTED (per tile in LDS, one device-wide reservation per tile) and finished by a second, dense launch,
// one listed boundary per lane.  bit 32 / 33 of a list entry: the left / right search is open.
constexpr uint64_t kIvLeftOpen = 1ull << 32, kIvRightOpen = 1ull << 33;
__device__ __forceinline__ void iv_finish(const Pyramid& py, uint64_t n, uint64_t e, uint32_t* __restrict__ lb, uint32_t* __restrict__ rb,
                                          uint32_t* __restrict__ node)
{
    const uint64_t p = e & 0xFFFFFFFFull;
    const uint64_t base = p / kIvTile * kIvTile;
    const uint32_t v = py.lvl[0][p];
    if (e & kIvLeftOpen) {
        const uint64_t l = prev_smaller(py, base, v);                    // (everything in [base, p) is >= v)
        lb[p] = (uint32_t)l;
        node[p] = (uint32_t)next_smaller(py, l, v, true, n);             // leftmost boundary of the interval with its depth (<= p)
    }
    if (e & kIvRightOpen) rb[p] = (uint32_t)(next_smaller(py, base + kIvTile - 1, v, false, n) - 1);
}
__global__ void __launch_bounds__(kBlock)
k_lcp_intervals(Pyramid py, uint64_t n, uint64_t tiles_per_block, uint32_t* __restrict__ lb, uint32_t* __restrict__ rb,
                uint32_t* __restrict__ node, uint64_t* __restrict__ open_list, uint64_t open_cap,
                unsigned long long* __restrict__ open_count)
{
    __shared__ uint32_t tr[2 * kIvTile];
    __shared__ uint64_t esc[kIvTile];
    __shared__ uint32_t n_esc;
    __shared__ unsigned long long esc_base;
    const uint32_t* lcp = py.lvl[0];
    const uint64_t tile0 = (uint64_t)blockIdx.x * tiles_per_block;
    for (uint64_t tile = tile0; tile < tile0 + tiles_per_block; tile++) {
        const uint64_t base = tile * kIvTile;
        if (base >= n) break;
        if (threadIdx.x == 0) n_esc = 0;
        for (unsigned i = threadIdx.x; i < (unsigned)kIvTile; i += kBlock) {
            const uint64_t g = base + i;
            tr[kIvTile + i] = (g == 0 || g >= n) ? 0u : lcp[g];          // (boundary 0 and the end of the array: depth 0)
        }
        __syncthreads();
        for (unsigned w = kIvTile / 2; w >= 1; w >>= 1) {                // level by level: w nodes, ids [w, 2w)
            for (unsigned k = w + threadIdx.x; k < 2 * w; k += kBlock) tr[k] = dmin(tr[2 * k], tr[2 * k + 1]);
            __syncthreads();
        }
        for (unsigned i = threadIdx.x; i < (unsigned)kIvTile; i += kBlock) {
            const uint64_t p = base + i;
            if (p >= n) break;
            const uint32_t v = tr[kIvTile + i];
            if (p == 0 || v == 0) {                           // the root: every boundary of depth 0
                lb[p] = 0;
                rb[p] = (uint32_t)(n - 1);
                node[p] = 0;
                continue;
            }
            uint64_t open = 0;
            const int jl = iv_prev_smaller(tr, (int)i, v);
            if (jl >= 0) {
                lb[p] = (uint32_t)(base + (uint64_t)jl);
                // leftmost boundary of the interval with its depth: the first value <= v after l (everything between is >= v)
                node[p] = (uint32_t)(base + (uint64_t)iv_next_smaller(tr, jl, v, true));     // (<= i: position i qualifies)
            } else {
                open |= kIvLeftOpen;
            }
            const int jr = iv_next_smaller(tr, (int)i, v, false);
            if (jr < kIvTile) rb[p] = (uint32_t)(dmin<uint64_t>(base + (uint64_t)jr, n) - 1);
            else if (base + kIvTile >= n) rb[p] = (uint32_t)(n - 1);
            else open |= kIvRightOpen;
            if (open) esc[atomicAdd(&n_esc, 1u)] = open | p;
        }
        __syncthreads();
        const uint32_t cnt = n_esc;
        if (cnt) {
            if (threadIdx.x == 0) esc_base = atomicAdd(open_count, (unsigned long long)cnt);
            __syncthreads();
            const unsigned long long at = esc_base;
            // (what does not fit the list -- a monotone LCP array -- is finished here, slowly; every slot below the
            // capacity that was reserved is written, so the second launch reads no gap)
            for (unsigned k = threadIdx.x; k < cnt; k += kBlock) {
                if (at + k < open_cap) open_list[at + k] = esc[k];
                else iv_finish(py, n, esc[k], lb, rb, node);
            }
        }
        __syncthreads();
    }
}
// the listed boundaries, one per lane
__global__ void __launch_bounds__(kBlock)
k_lcp_intervals_open(Pyramid py, uint64_t n, const uint64_t* __restrict__ open_list, uint64_t open_cap,
                     const unsigned long long* __restrict__ open_count, uint32_t* __restrict__ lb, uint32_t* __restrict__ rb,
                     uint32_t* __restrict__ node)
{
    // (entries reserved beyond the capacity were finished by their tiles; reservations never leave gaps below it)
    unsigned long long cnt = *open_count;
    if (cnt > open_cap) cnt = open_cap;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < cnt; k += stride) iv_finish(py, n, open_list[k], lb, rb, node);
}
// parent of the node a boundary belongs to, and the parent of every leaf
__global__ void __launch_bounds__(kBlock)
k_tree_parents(const uint32_t* __restrict__ lcp, uint64_t n, const uint32_t* __restrict__ lb, const uint32_t* __restrict__ rb,
               const uint32_t* __restrict__ node, uint32_t* __restrict__ parent, uint32_t* __restrict__ leaf_parent)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += stride) {
        // leaf of rank p: under the deeper of boundaries p and p + 1.  Boundary 0 has depth 0 whatever d_lcp[0] holds
        // ("not looked at", include/suffix_hip.h: k_pyr_reduce, prev_smaller and k_lcp_intervals ignore it too)
        const uint32_t dl = p ? lcp[p] : 0u, dr = p + 1 < n ? lcp[p + 1] : 0u;
        leaf_parent[p] = dl >= dr ? node[p] : node[p + 1];
        if (node[p] == 0) { parent[p] = kNoNode; continue; }                     // (the root has no parent: every boundary of depth 0)
        const uint64_t l = lb[p], r = (uint64_t)rb[p] + 1;                        // the two delimiting boundaries
        const uint32_t vl = l ? lcp[l] : 0u, vr = r < n ? lcp[r] : 0u;
        parent[p] = vl >= vr ? node[l] : node[r];
    }
}

// generalized suffix array (README.md:60-74): documents concatenated with a separator; the document of
// a text position = the last start <= position (binary search over the sorted starts)
__global__ void __launch_bounds__(kBlock)
k_doc_lookup(const uint32_t* __restrict__ pos, uint64_t count, const uint64_t* __restrict__ starts, uint64_t ndocs,
             uint32_t* __restrict__ doc, uint32_t* __restrict__ offset)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) {
        const uint64_t p = pos[i];
        uint64_t lo = 0, hi = ndocs;                         // first start > p
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (starts[mid] <= p) lo = mid + 1; else hi = mid;
        }
        const uint64_t d = lo ? lo - 1 : 0;
        if (doc) doc[i] = (uint32_t)d;
        if (offset) offset[i] = (uint32_t)(p - starts[d]);
    }
}

static uint64_t pyramid_words(uint64_t n)
{
    uint64_t words = 0, len = n;
    for (int l = 1; l < kPyrMaxLevels && len > 1; l++) {
        len = (len + kPyrFan - 1) / kPyrFan;
        words += (len + 63) & ~uint64_t(63);
    }
    return words;
}
// the levels above an LCP array (pyramid_words(n) u32 at w); first_is_zero = 0: above any array, entry 0 as it is
static int pyramid_build(const uint32_t* d_lcp, uint64_t n, uint32_t* w, const char* name, hipStream_t st, Pyramid* out,
                         int first_is_zero = 1)
{
    Pyramid& py = *out;
    py.lvl[0] = d_lcp;
    py.len[0] = n;
    py.levels = 1;
    uint64_t len = n;
    while (py.levels < kPyrMaxLevels && len > 1) {
        const uint64_t out_len = (len + kPyrFan - 1) / kPyrFan;
        const unsigned grid = (unsigned)dmin<uint64_t>((out_len + kBlock - 1) / kBlock, kMaxGrid);
        SFX_LAUNCH(name, (double)len * 4, k_pyr_reduce, grid, kBlock, st, py.lvl[py.levels - 1], len, w, out_len, first_is_zero);
        py.lvl[py.levels] = w;
        py.len[py.levels] = out_len;
        py.levels++;
        w += (out_len + 63) & ~uint64_t(63);
        len = out_len;
    }
    for (int l = py.levels; l < kPyrMaxLevels; l++) { py.lvl[l] = nullptr; py.len[l] = 0; }
    return SFX_OK;
}
#ifdef SFX_DEV_HOOKS
// the same for the LCE index's development baseline in sfx_api.hip's translation unit: entry 0 as it is
uint64_t lcp_pyramid_words(uint64_t n) { return pyramid_words(n); }
int lcp_pyramid_build_dev(const uint32_t* d_lcp, uint64_t n, uint32_t* w, hipStream_t st, Pyramid* out)
{
    return pyramid_build(d_lcp, n, w, "lce_pyramid", st, out, 0);
}
#endif
// (+ the list of boundaries whose searches leave their tile: n / 16 entries, and its counter)
static uint64_t open_list_cap(uint64_t n) { return n / 16 + 4096; }
uint64_t lcp_intervals_workspace_bytes(uint64_t n)
{
    return ((pyramid_words(n) * sizeof(uint32_t) + 255) & ~uint64_t(255)) + 256 + open_list_cap(n) * sizeof(uint64_t) + 256;
}

// lb, rb and node alone (the document counts of sfx_docs.hip need no parents): the same workspace, the same launches
int lcp_interval_bounds_dev(const uint32_t* d_lcp, uint64_t n, uint32_t* d_lb, uint32_t* d_rb, uint32_t* d_node, void* ws,
                            uint64_t ws_bytes, hipStream_t st)
{
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!d_lcp || !d_lb || !d_rb || !d_node) return SFX_ERR_ARG;
    if (!ws || ws_bytes < lcp_intervals_workspace_bytes(n)) return SFX_ERR_WORKSPACE;
    Pyramid py;
    SFX_TRY(pyramid_build(d_lcp, n, reinterpret_cast<uint32_t*>(ws), "tree_pyramid", st, &py));
    const unsigned grid = (unsigned)dmin<uint64_t>((n + kBlock - 1) / kBlock, kMaxGrid);
    {
        char* tail = reinterpret_cast<char*>(ws) + ((pyramid_words(n) * sizeof(uint32_t) + 255) & ~uint64_t(255));
        unsigned long long* open_count = reinterpret_cast<unsigned long long*>(tail);
        uint64_t* open_list = reinterpret_cast<uint64_t*>(tail + 256);
        const uint64_t cap = open_list_cap(n);
        SFX_HIP(hipMemsetAsync(open_count, 0, sizeof(unsigned long long), st));
        Chunking ch = make_chunking(n, kIvTile, 4 * kMaxGrid);
        SFX_LAUNCH("tree_intervals", (double)n * 16, k_lcp_intervals, ch.blocks, kBlock, st, py, n, ch.tiles_per_block, d_lb, d_rb, d_node,
                   open_list, cap, open_count);
        SFX_LAUNCH("tree_intervals_open", 0.0, k_lcp_intervals_open, grid, kBlock, st, py, n, (const uint64_t*)open_list, cap,
                   (const unsigned long long*)open_count, d_lb, d_rb, d_node);
    }
    return SFX_OK;
}
int lcp_intervals_dev(const uint32_t* d_lcp, uint64_t n, uint32_t* d_lb, uint32_t* d_rb, uint32_t* d_node, uint32_t* d_parent,
                      uint32_t* d_leaf_parent, void* ws, uint64_t ws_bytes, hipStream_t st)
{
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!d_lcp || !d_lb || !d_rb || !d_node || !d_parent || !d_leaf_parent) return SFX_ERR_ARG;
    SFX_TRY(lcp_interval_bounds_dev(d_lcp, n, d_lb, d_rb, d_node, ws, ws_bytes, st));
    const unsigned grid = (unsigned)dmin<uint64_t>((n + kBlock - 1) / kBlock, kMaxGrid);
    SFX_LAUNCH("tree_parents", (double)n * 28, k_tree_parents, grid, kBlock, st, d_lcp, n, (const uint32_t*)d_lb,
               (const uint32_t*)d_rb, (const uint32_t*)d_node, d_parent, d_leaf_parent);
    return SFX_OK;
}

int doc_lookup_dev(const uint32_t* d_pos, uint64_t count, const uint64_t* d_starts, uint64_t ndocs, uint32_t* d_doc,
                   uint32_t* d_offset, hipStream_t st)
{
    if (count == 0) return SFX_OK;
    if (!d_pos || !d_starts || ndocs == 0 || (!d_doc && !d_offset)) return SFX_ERR_ARG;
    const unsigned grid = (unsigned)dmin<uint64_t>((count + kBlock - 1) / kBlock, kMaxGrid);
    SFX_LAUNCH("doc_lookup", (double)count * 12, k_doc_lookup, grid, kBlock, st, d_pos, count, d_starts, ndocs, d_doc, d_offset);
    return SFX_OK;
}

// ---- generalized suffix array over a document collection (no separators) ---------------------------------------
// Documents D_0 .. D_{m-1} are one text T plus their start offsets.  The GSA orders every (document, offset) by the
// TRUNCATED suffix D_i[o..] (a proper prefix first, equal ones by document); DA names the document of every entry,
// GLCP is the common prefix of neighbours inside their documents.  It is derived from the plain SA + LCP of T:
// for the suffix s at plain rank r with L = docend(s) - s bytes left in its document, I(s) = the nearest q <= r with
// LCP[q] < L is the first rank of the plain interval of all suffixes that start with the truncated string, and
//   GSA = the plain suffixes sorted by (I(s), L, s).
// (Distinct truncated strings: I is ordered as the strings unless one is a proper prefix of the other, in which case
// both start the same interval or the shorter one's contains the longer one's, and L decides.  Equal (I, L) = equal
// strings: the document, i.e. the position, decides -- not the plain rank, which follows the NEXT document's text.)
// A suffix with LCP[r] < L is "unaffected": I = r, it keeps its plain place relative to the other unaffected ones.
// Only the affected ones (tails of documents whose truncated string goes on in the text that follows) are sorted,
// then merged in; with one document nothing is affected and no sort runs.
constexpr uint32_t kGsaNone = 0xFFFFFFFFu;

// the document of position p: the last start <= p (empty documents share their start with the next one)
__device__ __forceinline__ uint64_t gsa_doc_of(const uint64_t* __restrict__ starts, uint64_t ndocs, uint64_t p)
{
    uint64_t lo = 0, hi = ndocs;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (starts[mid] <= p) lo = mid + 1; else hi = mid;
    }
    return lo ? lo - 1 : 0;
}
__device__ __forceinline__ uint64_t gsa_doc_end(const uint64_t* __restrict__ starts, uint64_t ndocs, uint64_t n, uint64_t d)
{
    return d + 1 < ndocs ? starts[d + 1] : n;
}

// doc_starts: [0] == 0, non-decreasing, none past n
__global__ void __launch_bounds__(kBlock)
k_gsa_check_docs(const uint64_t* __restrict__ starts, uint64_t ndocs, uint64_t n, uint32_t* __restrict__ bad)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < ndocs; i += stride) {
        const uint64_t v = starts[i];
        if (v > n || (i == 0 ? v != 0 : v < starts[i - 1])) *bad = 1u;
    }
}
// per rank: bytes left in the document, and the affected flag (LCP[r] >= L) for the scan
__global__ void __launch_bounds__(kBlock)
k_gsa_affected(const uint32_t* __restrict__ sa, const uint32_t* __restrict__ lcp, uint64_t n, const uint64_t* __restrict__ starts,
               uint64_t ndocs, uint32_t* __restrict__ rem, uint32_t* __restrict__ flag)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) {
        const uint64_t s = sa[r];
        const uint32_t L = (uint32_t)(gsa_doc_end(starts, ndocs, n, gsa_doc_of(starts, ndocs, s)) - s);
        rem[r] = L;
        flag[r] = (r > 0 && lcp[r] >= L) ? 1u : 0u;
    }
}
// exclusive scan of u32 values into T (in place when T is u32): partial sums per workgroup chunk, a one-workgroup
// scan of those, then each chunk again with its carry.  out[count] = the total.
template <class T>
__global__ void __launch_bounds__(kBlock)
k_gsa_scan_count(const uint32_t* __restrict__ in, uint64_t count, uint64_t chunk, T* __restrict__ part)
{
    __shared__ T sh[kWavesPerBlock];
    const uint64_t b = (uint64_t)blockIdx.x * chunk, e = dmin<uint64_t>(b + chunk, count);
    T acc = 0;
    for (uint64_t i = b + threadIdx.x; i < e; i += kBlock) acc += (T)in[i];
    T total;
    (void)block_scan_add_excl<T>(acc, sh, total);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}
template <class T>
__global__ void __launch_bounds__(kBlock)
k_gsa_scan_top(T* __restrict__ part, unsigned nb, T* __restrict__ out_total)
{
    __shared__ T sh[kWavesPerBlock];
    T carry = 0;
    for (unsigned base = 0; base < nb; base += kBlock) {
        const unsigned i = base + threadIdx.x;
        T total;
        const T ex = block_scan_add_excl<T>(i < nb ? part[i] : (T)0, sh, total);
        if (i < nb) part[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *out_total = carry;
}
template <class T>
__global__ void __launch_bounds__(kBlock)
k_gsa_scan_apply(const uint32_t* in, uint64_t count, uint64_t chunk, const T* __restrict__ part, T* out)
{
    __shared__ T sh[kWavesPerBlock];
    const uint64_t b = (uint64_t)blockIdx.x * chunk, e = dmin<uint64_t>(b + chunk, count);
    T run = part[blockIdx.x];
    for (uint64_t base = b; base < e; base += kBlock) {            // (uniform trip count: the block scan has barriers)
        const uint64_t i = base + threadIdx.x;
        const T v = i < e ? (T)in[i] : (T)0;
        T total;
        const T ex = block_scan_add_excl<T>(v, sh, total);
        if (i < e) out[i] = run + ex;
        run += total;
    }
}
template <class T>
static int gsa_scan(const uint32_t* in, uint64_t count, T* out, T* part, hipStream_t st)
{
    const unsigned nb = (unsigned)dmin<uint64_t>((count + kBlock - 1) / kBlock, dmin<unsigned>(kMaxGrid, grid_cap()));
    const uint64_t chunk = (count + nb - 1) / nb;
    SFX_LAUNCH("gsa_scan", (double)count * 4, k_gsa_scan_count<T>, nb, kBlock, st, in, count, chunk, part);
    SFX_LAUNCH("gsa_scan", (double)nb * sizeof(T), k_gsa_scan_top<T>, 1, kBlock, st, part, nb, out + count);
    SFX_LAUNCH("gsa_scan", (double)count * (4 + sizeof(T)), k_gsa_scan_apply<T>, nb, kBlock, st, in, count, chunk,
               (const T*)part, out);
    return SFX_OK;
}
// the same scan for other translation units (sfx_lz.hip): part is kMaxGrid + 64 elements of the output type
int scan_u32_excl_dev(const uint32_t* in, uint64_t count, uint32_t* out, uint32_t* part, hipStream_t st)
{
    return gsa_scan<uint32_t>(in, count, out, part, st);
}
int scan_u32_to_u64_excl_dev(const uint32_t* in, uint64_t count, uint64_t* out, uint64_t* part, hipStream_t st)
{
    return gsa_scan<uint64_t>(in, count, out, part, st);
}
// the affected suffixes in plain-rank order: key = L << 32 | position (sorted on the position bits first), value = rank
__global__ void __launch_bounds__(kBlock)
k_gsa_compact(const uint32_t* __restrict__ P, const uint32_t* __restrict__ sa, const uint32_t* __restrict__ rem, uint64_t n,
              uint64_t* __restrict__ K, uint32_t* __restrict__ V)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) {
        const uint32_t j = P[r];
        if (P[r + 1] == j) continue;
        K[j] = ((uint64_t)rem[r] << 32) | sa[r];
        V[j] = (uint32_t)r;
    }
}
// between the two sort stages: key = I << lbits | L (I over the pyramid), in place; the position order stays as the
// order of ties for the (stable) sort on these bits
__global__ void __launch_bounds__(kBlock)
k_gsa_fixup_keys(uint64_t* __restrict__ K, const uint32_t* __restrict__ V, uint64_t m, Pyramid py, int lbits)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += stride) {
        const uint32_t L = (uint32_t)(K[j] >> 32);
        const uint64_t I = prev_smaller(py, (uint64_t)V[j] + 1, L);      // (LCP[r] >= L: some q < r)
        K[j] = (I << lbits) | L;
    }
}
// output slot of a sorted affected suffix: its index among them + the unaffected ranks with a smaller (r, L, s)
__global__ void __launch_bounds__(kBlock)
k_gsa_merge_affected(const uint64_t* __restrict__ K, const uint32_t* __restrict__ V, uint64_t m, uint64_t n, int lbits,
                     const uint32_t* __restrict__ P, const uint32_t* __restrict__ sa, const uint32_t* __restrict__ rem,
                     uint32_t* __restrict__ gsa, uint32_t* __restrict__ R, uint32_t* __restrict__ bad)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t lmask = (1ull << lbits) - 1;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += stride) {
        const uint64_t I = K[j] >> lbits;
        const uint32_t L = (uint32_t)(K[j] & lmask);
        const uint32_t r = V[j], s = sa[r];
        uint64_t before = I - P[I];                                    // unaffected ranks < I
        if (P[I + 1] == P[I]) {                                        // rank I itself, if unaffected
            const uint32_t li = rem[I], si = sa[I];
            if (li < L || (li == L && si < s)) before++;
        }
        const uint64_t o = j + before;
        if (o >= n) { *bad = 1u; continue; }                           // (an engine bug: reported as SFX_ERR_INTERNAL, never written)
        gsa[o] = s;
        R[o] = r;
    }
}
// output slot of an unaffected rank: its index among them + the affected suffixes with a smaller key (bisection)
__global__ void __launch_bounds__(kBlock)
k_gsa_merge_unaffected(const uint32_t* __restrict__ P, const uint32_t* __restrict__ sa, const uint32_t* __restrict__ rem, uint64_t n,
                       const uint64_t* __restrict__ K, const uint32_t* __restrict__ V, uint64_t m, int lbits,
                       uint32_t* __restrict__ gsa, uint32_t* __restrict__ R, uint32_t* __restrict__ bad)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) {
        const uint32_t pr = P[r];
        if (P[r + 1] != pr) continue;
        const uint64_t key = (r << lbits) | rem[r];
        const uint32_t s = sa[r];
        uint64_t lo = 0, hi = m;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            const uint64_t km = K[mid];
            if (km < key || (km == key && sa[V[mid]] < s)) lo = mid + 1; else hi = mid;
        }
        const uint64_t o = (r - pr) + lo;
        if (o >= n) { *bad = 1u; continue; }                           // (as above)
        gsa[o] = s;
        R[o] = (uint32_t)r;
    }
}
// GLCP[o] = min(plain lcp of the two neighbours' ranks, both lengths left); R == nullptr: the identity (nothing moved)
__global__ void __launch_bounds__(kBlock)
k_gsa_lcp(const uint32_t* __restrict__ R, const uint32_t* __restrict__ rem, Pyramid py, uint64_t n, uint32_t* __restrict__ glcp)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint32_t* lcp = py.lvl[0];
    for (uint64_t o = (uint64_t)blockIdx.x * kBlock + threadIdx.x; o < n; o += stride) {
        if (o == 0) { glcp[0] = 0; continue; }
        const uint64_t ra = R ? R[o - 1] : o - 1, rb = R ? R[o] : o;
        const uint64_t lo = dmin(ra, rb) + 1, hi = dmax(ra, rb);
        const uint32_t v = lo == hi ? lcp[lo] : range_min(py, lo, hi);
        glcp[o] = dmin(v, dmin(rem[ra], rem[rb]));
    }
}

template <class A> static void gsa_phase_carve(A& a, uint64_t n, uint32_t** pyr, uint32_t** rem, uint32_t** P, uint32_t** R,
                                               uint64_t** part, uint64_t** K0, uint32_t** V0, uint64_t** K1, uint32_t** V1,
                                               uint32_t** scratch)
{
    *pyr = a.template take<uint32_t>(pyramid_words(n) + 64);
    *rem = a.template take<uint32_t>(n);
    *P = a.template take<uint32_t>(n + 1);
    *R = a.template take<uint32_t>(n);
    *part = a.template take<uint64_t>(kMaxGrid + 64);
    *K0 = a.template take<uint64_t>(n);
    *V0 = a.template take<uint32_t>(n);
    *K1 = a.template take<uint64_t>(n);
    *V1 = a.template take<uint32_t>(n);
    *scratch = a.template take<uint32_t>(radix_scratch_words(n));
}
struct GsaSizer {                                  // ArenaSizer with pointer-returning take (for gsa_phase_carve)
    uint64_t used = 0;
    template <class T> T* take(uint64_t count) { used += (count * sizeof(T) + kArenaAlign - 1) & ~(kArenaAlign - 1); return nullptr; }
};
static uint64_t gsa_phase_bytes(uint64_t n)
{
    GsaSizer z;
    uint32_t *a, *b, *c, *d, *v0, *v1, *sc;
    uint64_t *p, *k0, *k1;
    gsa_phase_carve(z, n, &a, &b, &c, &d, &p, &k0, &v0, &k1, &v1, &sc);
    return z.used;
}
// [bad flag | plain SA | plain LCP | max(plain build workspace, the GSA phase)]
uint64_t gsa_workspace_bytes(uint64_t n)
{
    GsaSizer z;
    z.take<uint32_t>(64);
    z.take<uint32_t>(n);
    z.take<uint32_t>(n);
    return z.used + dmax(sa_lcp_workspace_bytes(n), gsa_phase_bytes(n));
}

static int gsa_check_docs(const uint64_t* d_starts, uint64_t ndocs, uint64_t n, uint32_t* d_bad, hipStream_t st, bool* bad)
{
    SFX_HIP(hipMemsetAsync(d_bad, 0, sizeof(uint32_t), st));
    const unsigned grid = (unsigned)dmin<uint64_t>((ndocs + kBlock - 1) / kBlock, kMaxGrid);
    SFX_LAUNCH("gsa_check_docs", (double)ndocs * 8, k_gsa_check_docs, grid, kBlock, st, d_starts, ndocs, n, d_bad);
    uint32_t h = 0;
    SFX_TRY(read_back(&h, d_bad, sizeof(h), st));
    *bad = h != 0;
    return SFX_OK;
}

int gsa_build_dev(const uint8_t* d_text, uint64_t n, const uint64_t* d_starts, uint64_t ndocs, uint32_t* d_gsa, uint32_t* d_da,
                  uint32_t* d_glcp, void* ws, uint64_t ws_bytes, hipStream_t st)
{
    if (n > 0xFFFFFFFFull || ndocs > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!d_text || !d_starts || ndocs == 0 || !d_gsa) return SFX_ERR_ARG;
    if (!ws || ws_bytes < gsa_workspace_bytes(n)) return SFX_ERR_WORKSPACE;
    Arena a(ws, ws_bytes);
    uint32_t* d_bad = a.take<uint32_t>(64);
    uint32_t* sa = a.take<uint32_t>(n);
    uint32_t* lcp = a.take<uint32_t>(n);
    char* rest = a.base + a.used;
    const uint64_t rest_bytes = a.size - a.used;
    bool bad = false;
    SFX_TRY(gsa_check_docs(d_starts, ndocs, n, d_bad, st, &bad));
    if (bad) return SFX_ERR_ARG;
    SFX_TRY(build_sa_lcp_u32_dev(d_text, n, sa, lcp, rest, rest_bytes, st));
    // the plain build's workspace is free again: the GSA phase takes it over
    Arena b(rest, rest_bytes);
    uint32_t *pyr, *rem, *P, *R, *V0, *V1, *scratch;
    uint64_t *part, *K0, *K1;
    gsa_phase_carve(b, n, &pyr, &rem, &P, &R, &part, &K0, &V0, &K1, &V1, &scratch);
    if (b.overflow) return SFX_ERR_INTERNAL;
    Pyramid py;
    SFX_TRY(pyramid_build(lcp, n, pyr, "gsa_pyramid", st, &py));
    const unsigned grid = (unsigned)dmin<uint64_t>((n + kBlock - 1) / kBlock, kMaxGrid);
    SFX_LAUNCH("gsa_affected", (double)n * 16, k_gsa_affected, grid, kBlock, st, (const uint32_t*)sa, (const uint32_t*)lcp, n,
               d_starts, ndocs, rem, P);
    SFX_TRY(gsa_scan<uint32_t>(P, n, P, reinterpret_cast<uint32_t*>(part), st));
    uint32_t m = 0;
    SFX_TRY(read_back(&m, P + n, sizeof(m), st));
    const uint32_t* Rout = nullptr;
    if (m == 0) {
        SFX_HIP(hipMemcpyAsync(d_gsa, sa, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    } else {
        const unsigned mgrid = (unsigned)dmin<uint64_t>((m + kBlock - 1) / kBlock, kMaxGrid);
        const int pbits = bits_for(n - 1), lbits = bits_for(n);
        SFX_LAUNCH("gsa_compact", (double)n * 8 + (double)m * 12, k_gsa_compact, grid, kBlock, st, (const uint32_t*)P,
                   (const uint32_t*)sa, (const uint32_t*)rem, n, K0, V0);
        // stage 1: by position (the order of identical truncated suffixes); stage 2: stably by (I, L)
        int in1 = 0;
        SFX_TRY(radix_sort_kv64(K0, V0, K1, V1, m, 0, pbits, scratch, st, &in1, nullptr, nullptr));
        uint64_t* K = in1 ? K1 : K0;
        uint32_t* V = in1 ? V1 : V0;
        SFX_LAUNCH("gsa_fixup_sort", (double)m * 12, k_gsa_fixup_keys, mgrid, kBlock, st, K, (const uint32_t*)V, (uint64_t)m, py, lbits);
        int in1b = 0;
        SFX_TRY(radix_sort_kv64(K, V, in1 ? K0 : K1, in1 ? V0 : V1, m, 0, pbits + lbits, scratch, st, &in1b, nullptr, nullptr));
        if (in1b) { K = in1 ? K0 : K1; V = in1 ? V0 : V1; }
        SFX_LAUNCH("gsa_merge", (double)m * 24, k_gsa_merge_affected, mgrid, kBlock, st, (const uint64_t*)K, (const uint32_t*)V,
                   (uint64_t)m, n, lbits, (const uint32_t*)P, (const uint32_t*)sa, (const uint32_t*)rem, d_gsa, R, d_bad);
        SFX_LAUNCH("gsa_merge", (double)n * 20, k_gsa_merge_unaffected, grid, kBlock, st, (const uint32_t*)P, (const uint32_t*)sa,
                   (const uint32_t*)rem, n, (const uint64_t*)K, (const uint32_t*)V, (uint64_t)m, lbits, d_gsa, R, d_bad);
        // a slot outside [0, n) cannot come out of a correct merge; if one did, the flag (still 0 from the document
        // check) says so and the build fails instead of returning a table with a stale entry
        uint32_t merge_bad = 0;
        SFX_TRY(read_back(&merge_bad, d_bad, sizeof(merge_bad), st));
        if (merge_bad) return SFX_ERR_INTERNAL;
        Rout = R;
    }
    if (d_glcp)
        SFX_LAUNCH("gsa_lcp", (double)n * (Rout ? 20 : 16), k_gsa_lcp, grid, kBlock, st, Rout, (const uint32_t*)rem, py, n, d_glcp);
    if (d_da)
        SFX_LAUNCH("gsa_doc_array", (double)n * 8, k_doc_lookup, grid, kBlock, st, (const uint32_t*)d_gsa, n, d_starts, ndocs, d_da,
                   (uint32_t*)nullptr);
    return SFX_OK;
}

// ---- queries on the GSA ---------------------------------------------------------------------------------------------
// q against the truncated suffix at rank r: < 0 it sorts below q (a suffix that ends inside q included), 0 q is its
// prefix (a match), > 0 above
__device__ __forceinline__ int gsa_cmp(const uint8_t* __restrict__ text, uint64_t n, const uint64_t* __restrict__ starts, uint64_t ndocs,
                                       const uint32_t* __restrict__ sa, const uint32_t* __restrict__ da, uint64_t r,
                                       const uint8_t* __restrict__ q, uint64_t ql)
{
    const uint64_t s = sa[r];
    const uint64_t L = gsa_doc_end(starts, ndocs, n, da[r]) - s;
    const uint64_t k = dmin(L, ql);
    for (uint64_t i = 0; i < k; i++) {
        const uint8_t a = text[s + i], b = q[i];
        if (a != b) return a < b ? -1 : 1;
    }
    return L < ql ? -1 : 0;
}
__global__ void __launch_bounds__(kBlock)
k_gsa_query(const uint8_t* __restrict__ text, uint64_t n, const uint64_t* __restrict__ starts, uint64_t ndocs,
            const uint32_t* __restrict__ sa, const uint32_t* __restrict__ da, const uint8_t* __restrict__ qb,
            const uint64_t* __restrict__ qoff, uint64_t nq, uint32_t* __restrict__ d_start, uint32_t* __restrict__ d_end,
            uint8_t* __restrict__ d_found, uint32_t* __restrict__ d_any, uint32_t* __restrict__ d_len)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < nq; k += stride) {
        const uint64_t q0 = qoff[k], ql = qoff[k + 1] - q0;
        const uint8_t* q = qb + q0;
        uint64_t lo = 0, hi = 0;
        if (ql && n) {
            uint64_t a = 0, b = n;                                       // first rank >= q
            while (a < b) {
                const uint64_t mid = (a + b) >> 1;
                if (gsa_cmp(text, n, starts, ndocs, sa, da, mid, q, ql) < 0) a = mid + 1; else b = mid;
            }
            lo = a;
            b = n;                                                       // first rank > q (not prefixed by it)
            while (a < b) {
                const uint64_t mid = (a + b) >> 1;
                if (gsa_cmp(text, n, starts, ndocs, sa, da, mid, q, ql) <= 0) a = mid + 1; else b = mid;
            }
            hi = a;
            if (lo == hi) lo = hi = 0;
        }
        if (d_start) d_start[k] = (uint32_t)lo;
        if (d_end) d_end[k] = (uint32_t)hi;
        if (d_found) d_found[k] = hi > lo ? 1 : 0;
        if (d_any) d_any[k] = hi > lo ? sa[lo] : kGsaNone;
        if (d_len) d_len[k] = (uint32_t)(hi - lo);
    }
}
// matching statistics of a query text against the collection: ms_search (sfx_device.hpp) over the TRUNCATED suffixes, so
// a match stops at the end of its document as gsa_cmp's does; ranks are GSA ranks
struct MsDocSuffix {
    const uint64_t* starts;
    const uint32_t* da;
    uint64_t ndocs, n;
    __device__ __forceinline__ uint64_t len(uint64_t r, uint32_t s) const { return gsa_doc_end(starts, ndocs, n, da[r]) - s; }
};
__global__ void __launch_bounds__(kBlock)
k_ms_gsa_search(const uint8_t* __restrict__ text, uint64_t n, const uint64_t* __restrict__ starts, uint64_t ndocs,
                const uint32_t* __restrict__ sa, const uint32_t* __restrict__ da, const uint8_t* __restrict__ q, uint64_t m,
                uint32_t max_len, uint32_t* __restrict__ len_out, uint32_t* __restrict__ src_out,
                uint32_t* __restrict__ start_out, uint32_t* __restrict__ end_out)
{
    ms_positions(text, sa, n, q, m, max_len, MsDocSuffix{starts, da, ndocs, n}, MsWholeTable{}, len_out, src_out, start_out, end_out);
}
int gindex_match_stats_dev(const uint8_t* d_text, uint64_t n, const uint64_t* d_starts, uint64_t ndocs, const uint32_t* d_sa,
                           const uint32_t* d_da, const uint8_t* d_q, uint64_t m, uint32_t max_len, uint32_t* d_len,
                           uint32_t* d_src, uint32_t* d_start, uint32_t* d_end, hipStream_t st)
{
    bool run = false;
    SFX_TRY(ms_check_args(n, d_text, d_sa, d_q, m, d_len, d_start, d_end, &run));
    if (!run) return SFX_OK;
    if (n && (!d_starts || !d_da || ndocs == 0)) return SFX_ERR_ARG;
    const unsigned grid = (unsigned)dmin<uint64_t>((m + kBlock - 1) / kBlock, kMaxGrid);
    const double probes = (double)bits_for(n ? n : 1) * (d_start ? 2.0 : 1.0);
    SFX_LAUNCH("ms_gsa_search", (double)m * probes * 24.0, k_ms_gsa_search, grid, kBlock, st, d_text, n, d_starts, ndocs, d_sa, d_da,
               d_q, m, max_len, d_len, d_src, d_start, d_end);
    return SFX_OK;
}

// document frequency: the ranks r of [start, end) whose previous rank of the same document lies before start.  The work is
// the TOTAL interval length (prefix offs over the queries), 1024 consecutive ranks per wave, so one huge interval spreads
// over the whole device; a wave whose ranks all belong to one query adds its count once.
constexpr unsigned kGsaCountPerLane = 16;
__global__ void __launch_bounds__(kBlock)
k_gsa_doc_count(const uint64_t* __restrict__ offs, uint64_t nq, const uint32_t* __restrict__ start, const uint32_t* __restrict__ prev,
                uint32_t* __restrict__ ndocs)
{
    const uint64_t total = offs[nq];
    const uint64_t seg_len = (uint64_t)kWave * kGsaCountPerLane;
    const uint64_t nseg = (total + seg_len - 1) / seg_len;
    const uint64_t waves = (uint64_t)gridDim.x * kWavesPerBlock;
    const unsigned lane = lane_id();
    for (uint64_t seg = (uint64_t)blockIdx.x * kWavesPerBlock + wave_id(); seg < nseg; seg += waves) {
        const uint64_t t0 = seg * seg_len;
        const bool active = t0 + lane < total;
        unsigned long long k = 0;
        uint32_t cnt = 0;
        if (active) {
            uint64_t t = t0 + lane;
            uint64_t a = 0, b = nq + 1;                                  // first offs[] > t, minus one
            while (a < b) {
                const uint64_t mid = (a + b) >> 1;
                if (offs[mid] <= t) a = mid + 1; else b = mid;
            }
            k = a - 1;
            uint32_t sk = start[k];
            uint64_t ok = offs[k], onext = offs[k + 1];
            for (unsigned i = 0; i < kGsaCountPerLane && t < total; i++, t += kWave) {
                while (t >= onext) {                                     // the next non-empty interval
                    if (cnt) atomicAdd(&ndocs[k], cnt);
                    cnt = 0;
                    k++;
                    sk = start[k];
                    ok = onext;
                    onext = offs[k + 1];
                }
                const uint32_t p = prev[sk + (uint32_t)(t - ok)];
                cnt += (p == kGsaNone || p < sk) ? 1u : 0u;
            }
        }
        const unsigned long long k0 = __shfl(k, 0);
        if (__all(!active || k == k0)) {
            uint32_t sum = cnt;
            for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
            if (lane == 0 && sum) atomicAdd(&ndocs[k0], sum);
        } else if (cnt) {
            atomicAdd(&ndocs[k], cnt);
        }
    }
}
// index checks: doc_starts as for the build, every table entry a position of the document DA names
__global__ void __launch_bounds__(kBlock)
k_gsa_check_index(const uint32_t* __restrict__ sa, const uint32_t* __restrict__ da, uint64_t n, const uint64_t* __restrict__ starts,
                  uint64_t ndocs, uint32_t* __restrict__ bad)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) {
        const uint64_t s = sa[r], d = da[r];
        if (s >= n || d >= ndocs || starts[d] > s || gsa_doc_end(starts, ndocs, n, d) <= s) *bad = 1u;
    }
}
__global__ void __launch_bounds__(kBlock)
k_gsa_prev_keys(const uint32_t* __restrict__ da, uint64_t n, uint64_t* __restrict__ K, uint32_t* __restrict__ V)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) {
        K[r] = da[r];
        V[r] = (uint32_t)r;
    }
}
// (DA, rank) sorted stably by DA: the previous entry of the same document is the previous rank with that DA value
__global__ void __launch_bounds__(kBlock)
k_gsa_prev(const uint64_t* __restrict__ K, const uint32_t* __restrict__ V, uint64_t n, uint32_t* __restrict__ prev)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride)
        prev[V[k]] = (k > 0 && K[k - 1] == K[k]) ? V[k - 1] : kGsaNone;
}

uint64_t gindex_workspace_bytes(uint64_t n)
{
    ArenaSizer z;
    z.take<uint32_t>(64);
    z.take<uint64_t>(n);
    z.take<uint32_t>(n);
    z.take<uint64_t>(n);
    z.take<uint32_t>(n);
    z.take<uint32_t>(radix_scratch_words(n));
    return z.used;
}
int gindex_build_dev(const uint64_t* d_starts, uint64_t ndocs, uint64_t n, const uint32_t* d_sa, const uint32_t* d_da,
                     uint32_t* d_prev, void* ws, uint64_t ws_bytes, hipStream_t st, bool* bad_out)
{
    Arena a(ws, ws_bytes);
    uint32_t* d_bad = a.take<uint32_t>(64);
    uint64_t* K0 = a.take<uint64_t>(n);
    uint32_t* V0 = a.take<uint32_t>(n);
    uint64_t* K1 = a.take<uint64_t>(n);
    uint32_t* V1 = a.take<uint32_t>(n);
    uint32_t* scratch = a.take<uint32_t>(radix_scratch_words(n));
    if (a.overflow) return SFX_ERR_WORKSPACE;
    bool bad = false;
    SFX_TRY(gsa_check_docs(d_starts, ndocs, n, d_bad, st, &bad));
    if (!bad) {
        const unsigned grid = (unsigned)dmin<uint64_t>((n + kBlock - 1) / kBlock, kMaxGrid);
        SFX_LAUNCH("gsa_check_index", (double)n * 8, k_gsa_check_index, grid, kBlock, st, d_sa, d_da, n, d_starts, ndocs, d_bad);
        uint32_t h = 0;
        SFX_TRY(read_back(&h, d_bad, sizeof(h), st));
        bad = h != 0;
    }
    *bad_out = bad;
    if (bad) return SFX_OK;
    return gsa_prev_dev(d_da, n, ndocs, d_prev, K0, V0, K1, V1, scratch, st);
}
// PREV alone, for sfx_docs.hip too: (K0, V0) / (K1, V1) n entries each, scratch radix_scratch_words(n).  Only the low
// bits_for(ndocs - 1) bits of an entry are sorted on, and V holds ranks: an entry >= ndocs (the caller's check) costs nothing
int gsa_prev_dev(const uint32_t* d_da, uint64_t n, uint64_t ndocs, uint32_t* d_prev, uint64_t* K0, uint32_t* V0, uint64_t* K1, uint32_t* V1,
                 uint32_t* scratch, hipStream_t st)
{
    return gsa_prev_sorted_dev(d_da, n, ndocs, d_prev, K0, V0, K1, V1, scratch, st, nullptr, nullptr);
}
// ... and where the stable sort left (DA, rank) ordered by (DA, rank), for sfx_doclist.hip: *keys / *ranks point into
// (K0, V0) or (K1, V1) and stay valid until those are written again
int gsa_prev_sorted_dev(const uint32_t* d_da, uint64_t n, uint64_t ndocs, uint32_t* d_prev, uint64_t* K0, uint32_t* V0, uint64_t* K1,
                        uint32_t* V1, uint32_t* scratch, hipStream_t st, const uint64_t** keys, const uint32_t** ranks)
{
    const unsigned grid = (unsigned)dmin<uint64_t>((n + kBlock - 1) / kBlock, kMaxGrid);
    SFX_LAUNCH("gsa_prev", (double)n * 16, k_gsa_prev_keys, grid, kBlock, st, d_da, n, K0, V0);
    int in1 = 0;
    SFX_TRY(radix_sort_kv64(K0, V0, K1, V1, n, 0, bits_for(ndocs - 1), scratch, st, &in1, nullptr, nullptr));
    SFX_LAUNCH("gsa_prev", (double)n * 16, k_gsa_prev, grid, kBlock, st, (const uint64_t*)(in1 ? K1 : K0), (const uint32_t*)(in1 ? V1 : V0),
               n, d_prev);
    if (keys) *keys = in1 ? K1 : K0;
    if (ranks) *ranks = in1 ? V1 : V0;
    return SFX_OK;
}

// [lens nq u32 | starts nq u32 | offs nq + 1 u64 | scan partials]
uint64_t gindex_query_scratch_bytes(uint64_t nq)
{
    ArenaSizer z;
    z.take<uint32_t>(nq);
    z.take<uint32_t>(nq);
    z.take<uint64_t>(nq + 1);
    z.take<uint64_t>(kMaxGrid + 64);
    return z.used;
}
int gindex_query_dev(const uint8_t* d_text, uint64_t n, const uint64_t* d_starts, uint64_t ndocs, const uint32_t* d_sa,
                     const uint32_t* d_da, const uint32_t* d_prev, const uint8_t* d_q, const uint64_t* d_qoff, uint64_t nq,
                     uint32_t* d_start, uint32_t* d_end, uint8_t* d_found, uint32_t* d_any, uint32_t* d_ndocs, void* scratch,
                     uint64_t scratch_bytes, hipStream_t st)
{
    if (nq == 0) return SFX_OK;
    if (!d_qoff || nq > 0xFFFFFFFFull) return SFX_ERR_ARG;
    uint32_t *lens = nullptr, *qstart = d_start;
    uint64_t *offs = nullptr, *part = nullptr;
    if (d_ndocs) {
        Arena a(scratch, scratch_bytes);
        lens = a.take<uint32_t>(nq);
        uint32_t* own_start = a.take<uint32_t>(nq);
        offs = a.take<uint64_t>(nq + 1);
        part = a.take<uint64_t>(kMaxGrid + 64);
        if (!scratch || a.overflow) return SFX_ERR_WORKSPACE;
        if (!qstart) qstart = own_start;
    }
    const unsigned qgrid = (unsigned)dmin<uint64_t>((nq + kBlock - 1) / kBlock, kMaxGrid);
    SFX_LAUNCH("gsa_query", (double)nq * 32, k_gsa_query, qgrid, kBlock, st, d_text, n, d_starts, ndocs, d_sa, d_da, d_q, d_qoff, nq,
               qstart, d_end, d_found, d_any, lens);
    if (!d_ndocs) return SFX_OK;
    SFX_HIP(hipMemsetAsync(d_ndocs, 0, nq * sizeof(uint32_t), st));
    SFX_TRY(gsa_scan<uint64_t>(lens, nq, offs, part, st));
    // (the total is on the device: the grid is sized by its bound nq x n, the kernel reads the real one)
    const double bound = (double)nq * (double)n;
    const double per_block = (double)kWave * kGsaCountPerLane * kWavesPerBlock;
    const unsigned cgrid = (unsigned)dmax(1.0, dmin((double)dmin<unsigned>(kMaxGrid, grid_cap()), bound / per_block + 1.0));
    SFX_LAUNCH("gsa_doc_count", 0.0, k_gsa_doc_count, cgrid, kBlock, st, (const uint64_t*)offs, nq, (const uint32_t*)qstart, d_prev, d_ndocs);
    return SFX_OK;
}

// ---- repeat lengths and repeated spans from SA + LCP (include/suffix_hip.h) ----------------------------------------
// rep[p] = the longest common prefix of the suffix at text position p (truncated at its document's end in a collection)
// with any suffix the scope allows; no text access: the common prefix of two ranks is the minimum of the LCP values
// between them, and the best partner on either side of a rank is the NEAREST allowed one.
//   ANY        the two neighbours;
//   EARLIER    the nearest ranks on either side that hold a smaller position (LPF): all-nearest-smaller-values on the
//              SA VALUES, over a second min-pyramid, then two range minima on the LCP pyramid;
//   OTHER_DOC  the ranks just outside the run of equal DA values the rank stands in.
// Every kernel that scatters by position refuses a table entry >= n (flag, read back once; never written).
constexpr uint32_t kRepNone = 0xFFFFFFFFu;

__device__ __forceinline__ void rep_store(uint32_t* __restrict__ rep, uint32_t* __restrict__ src, uint64_t p, uint32_t left, uint32_t right,
                                          uint32_t wl, uint32_t wr)
{
    const uint32_t m = dmax(left, right);
    rep[p] = m;
    if (src) src[p] = m == 0 ? kRepNone : (left >= right ? wl : wr);
}
__global__ void __launch_bounds__(kBlock)
k_rep_any(const uint32_t* __restrict__ sa, const uint32_t* __restrict__ lcp, uint64_t n, uint32_t* __restrict__ rep,
          uint32_t* __restrict__ src, uint32_t* __restrict__ bad)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) {
        const uint64_t p = sa[r];
        if (p >= n) { *bad = 1u; continue; }
        const uint32_t left = r ? lcp[r] : 0u, right = r + 1 < n ? lcp[r + 1] : 0u;       // (lcp[0] and lcp[n] count as 0)
        rep_store(rep, src, p, left, right, left ? sa[r - 1] : kRepNone, right ? sa[r + 1] : kRepNone);
    }
}

// nearest q < from with lvl[0][q] < v, or -1: "none" is an answer here (prev_smaller's boundary 0 is an LCP convention, and
// this pyramid stands on suffix-array values)
__device__ __forceinline__ int64_t rep_prev_smaller(const Pyramid& py, uint64_t from, uint32_t v)
{
    int l = 0;
    int64_t idx = (int64_t)from - 1;
    for (;;) {
        if (idx < 0) return -1;
        bool found = false;
        for (;;) {
            if (py.lvl[l][idx] < v) { found = true; break; }
            if (idx % kPyrFan == 0) break;
            idx--;
        }
        if (found) break;
        idx = idx / kPyrFan - 1;                             // (the top level is one block: -1 there)
        l++;
    }
    while (l > 0) {
        l--;
        int64_t c = dmin<int64_t>(idx * kPyrFan + kPyrFan - 1, (int64_t)py.len[l] - 1);
        while (py.lvl[l][c] >= v) c--;
        idx = c;
    }
    return idx;
}
// min of tile values [lo, hi] (tile coordinates, lo <= hi) under the binary min-tree of k_lcp_intervals
__device__ __forceinline__ uint32_t iv_range_min(const uint32_t* tr, int lo, int hi)
{
    uint32_t m = 0xFFFFFFFFu;
    unsigned l = (unsigned)(kIvTile + lo), r = (unsigned)(kIvTile + hi + 1);
    while (l < r) {
        if (l & 1u) m = dmin(m, tr[l++]);
        if (r & 1u) m = dmin(m, tr[--r]);
        l >>= 1;
        r >>= 1;
    }
    return m;
}
// rank r (position v = sa[r] < n) through the two global pyramids
__device__ __forceinline__ void rep_earlier_finish(const Pyramid& ps, const Pyramid& pl, uint64_t n, uint64_t r, uint32_t* __restrict__ rep,
                                                   uint32_t* __restrict__ src)
{
    const uint32_t v = ps.lvl[0][r];
    const int64_t a = rep_prev_smaller(ps, r, v);
    const uint64_t b = next_smaller(ps, r, v, false, n);
    const uint32_t left = a < 0 ? 0u : range_min(pl, (uint64_t)a + 1, r);
    const uint32_t right = b >= n ? 0u : range_min(pl, r + 1, b);
    rep_store(rep, src, v, left, right, a < 0 ? kRepNone : ps.lvl[0][a], b >= n ? kRepNone : ps.lvl[0][b]);
}
// The shape of k_lcp_intervals: a workgroup stages kIvTile SA values and their LCP values in LDS, each under a binary
// min-tree; a rank whose two nearest smaller positions lie inside the tile is answered there (two tree searches, two tree
// range minima, the same few LDS reads for every lane).  A rank whose search leaves the tile is LISTED and finished by a
// dense second launch over the global pyramids (what does not fit the list is finished in place).
__global__ void __launch_bounds__(kBlock)
k_rep_earlier(Pyramid ps, Pyramid pl, uint64_t n, uint64_t tiles_per_block, uint32_t* __restrict__ rep, uint32_t* __restrict__ src,
              uint32_t* __restrict__ open_list, uint64_t open_cap, unsigned long long* __restrict__ open_count, uint32_t* __restrict__ bad)
{
    __shared__ uint32_t ts[2 * kIvTile];
    __shared__ uint32_t tl[2 * kIvTile];
    __shared__ uint32_t esc[kIvTile];
    __shared__ uint32_t n_esc;
    __shared__ unsigned long long esc_base;
    const uint32_t* sa = ps.lvl[0];
    const uint32_t* lcp = pl.lvl[0];
    const uint64_t tile0 = (uint64_t)blockIdx.x * tiles_per_block;
    for (uint64_t tile = tile0; tile < tile0 + tiles_per_block; tile++) {
        const uint64_t base = tile * kIvTile;
        if (base >= n) break;
        if (threadIdx.x == 0) n_esc = 0;
        for (unsigned i = threadIdx.x; i < (unsigned)kIvTile; i += kBlock) {
            const uint64_t g = base + i;
            ts[kIvTile + i] = g < n ? sa[g] : 0xFFFFFFFFu;               // (past the end: smaller than nothing)
            tl[kIvTile + i] = (g == 0 || g >= n) ? 0u : lcp[g];
        }
        __syncthreads();
        for (unsigned w = kIvTile / 2; w >= 1; w >>= 1) {
            for (unsigned k = w + threadIdx.x; k < 2 * w; k += kBlock) {
                ts[k] = dmin(ts[2 * k], ts[2 * k + 1]);
                tl[k] = dmin(tl[2 * k], tl[2 * k + 1]);
            }
            __syncthreads();
        }
        for (unsigned i = threadIdx.x; i < (unsigned)kIvTile; i += kBlock) {
            const uint64_t r = base + i;
            if (r >= n) break;
            const uint32_t v = ts[kIvTile + i];
            if (v >= n) { *bad = 1u; continue; }
            if (v == 0) { rep_store(rep, src, 0, 0u, 0u, kRepNone, kRepNone); continue; }     // nothing is earlier
            const int jl = iv_prev_smaller(ts, (int)i, v);
            const int jr = iv_next_smaller(ts, (int)i, v, false);
            if ((jl < 0 && base > 0) || (jr >= kIvTile && base + kIvTile < n)) {
                esc[atomicAdd(&n_esc, 1u)] = (uint32_t)r;
                continue;
            }
            const uint32_t left = jl < 0 ? 0u : iv_range_min(tl, jl + 1, (int)i);
            const uint32_t right = jr >= kIvTile ? 0u : iv_range_min(tl, (int)i + 1, jr);
            rep_store(rep, src, v, left, right, jl < 0 ? kRepNone : ts[kIvTile + jl], jr >= kIvTile ? kRepNone : ts[kIvTile + jr]);
        }
        __syncthreads();
        const uint32_t cnt = n_esc;
        if (cnt) {
            if (threadIdx.x == 0) esc_base = atomicAdd(open_count, (unsigned long long)cnt);
            __syncthreads();
            const unsigned long long at = esc_base;
            for (unsigned k = threadIdx.x; k < cnt; k += kBlock) {
                if (at + k < open_cap) open_list[at + k] = esc[k];
                else rep_earlier_finish(ps, pl, n, esc[k], rep, src);
            }
        }
        __syncthreads();
    }
}
__global__ void __launch_bounds__(kBlock)
k_rep_earlier_open(Pyramid ps, Pyramid pl, uint64_t n, const uint32_t* __restrict__ open_list, uint64_t open_cap,
                   const unsigned long long* __restrict__ open_count, uint32_t* __restrict__ rep, uint32_t* __restrict__ src)
{
    unsigned long long cnt = *open_count;
    if (cnt > open_cap) cnt = open_cap;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < cnt; k += stride) rep_earlier_finish(ps, pl, n, open_list[k], rep, src);
}

// OTHER_DOC: head flags of the runs of equal DA values (scanned into run ids), the first rank of every run, then per rank
// the two range minima to just outside its run
__global__ void __launch_bounds__(kBlock)
k_rep_doc_heads(const uint32_t* __restrict__ sa, const uint32_t* __restrict__ da, uint64_t n, uint32_t* __restrict__ flag,
                uint32_t* __restrict__ bad)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) {
        if (sa[r] >= n) *bad = 1u;
        flag[r] = (r == 0 || da[r] != da[r - 1]) ? 1u : 0u;
    }
}
// P = the exclusive scan of the head flags (P[n] = the number of runs): run_start[k] = first rank of run k, [runs] = n
__global__ void __launch_bounds__(kBlock)
k_rep_run_starts(const uint32_t* __restrict__ P, uint64_t n, uint32_t* __restrict__ run_start)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) {
        if (P[r + 1] != P[r]) run_start[P[r]] = (uint32_t)r;
        if (r == 0) run_start[P[n]] = (uint32_t)n;
    }
}
__global__ void __launch_bounds__(kBlock)
k_rep_other_doc(const uint32_t* __restrict__ sa, Pyramid pl, uint64_t n, const uint32_t* __restrict__ P,
                const uint32_t* __restrict__ run_start, uint32_t* __restrict__ rep, uint32_t* __restrict__ src)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint32_t* lcp = pl.lvl[0];
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) {
        const uint64_t p = sa[r];
        if (p >= n) continue;                                            // (flagged by k_rep_doc_heads)
        const uint32_t k = P[r + 1] - 1;
        const uint64_t s = run_start[k], e = run_start[k + 1];           // a = s - 1, b = e
        const uint32_t left = s == 0 ? 0u : (s == r ? lcp[r] : range_min(pl, s, r));
        const uint32_t right = e >= n ? 0u : (e == r + 1 ? lcp[e] : range_min(pl, r + 1, e));
        rep_store(rep, src, p, left, right, s == 0 ? kRepNone : sa[s - 1], e >= n ? kRepNone : sa[e]);
    }
}

// [bad flag | LCP pyramid | EARLIER: SA pyramid, counter, list | OTHER_DOC: P (n + 1), run starts (n + 1), scan partials]
struct RepLensWs {
    uint32_t *bad, *pyr_lcp, *pyr_sa, *open_list, *P, *run_start, *part;
    unsigned long long* open_count;
};
template <class A> static void rep_lens_carve(A& a, uint64_t n, int scope, RepLensWs* w)
{
    *w = RepLensWs();
    w->bad = a.template take<uint32_t>(64);
    if (scope == SFX_REP_ANY) return;
    w->pyr_lcp = a.template take<uint32_t>(pyramid_words(n) + 64);
    if (scope == SFX_REP_EARLIER) {
        w->pyr_sa = a.template take<uint32_t>(pyramid_words(n) + 64);
        w->open_count = a.template take<unsigned long long>(32);
        w->open_list = a.template take<uint32_t>(open_list_cap(n));
    } else {
        w->P = a.template take<uint32_t>(n + 1);
        w->run_start = a.template take<uint32_t>(n + 1);
        w->part = a.template take<uint32_t>(kMaxGrid + 64);
    }
}
uint64_t repeat_lens_workspace_bytes(uint64_t n, int scope)
{
    if (scope != SFX_REP_ANY && scope != SFX_REP_EARLIER && scope != SFX_REP_OTHER_DOC) return 0;
    GsaSizer z;
    RepLensWs w;
    rep_lens_carve(z, n, scope, &w);
    return z.used;
}
int repeat_lens_dev(const uint32_t* d_sa, const uint32_t* d_lcp, const uint32_t* d_da, uint64_t n, int scope, uint32_t* d_rep,
                    uint32_t* d_src, void* ws, uint64_t ws_bytes, hipStream_t st)
{
    if (scope != SFX_REP_ANY && scope != SFX_REP_EARLIER && scope != SFX_REP_OTHER_DOC) return SFX_ERR_ARG;
    if (scope == SFX_REP_OTHER_DOC && !d_da && n) return SFX_ERR_ARG;
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!d_sa || !d_lcp || !d_rep) return SFX_ERR_ARG;
    if (!ws || ws_bytes < repeat_lens_workspace_bytes(n, scope)) return SFX_ERR_WORKSPACE;
    Arena a(ws, ws_bytes);
    RepLensWs w;
    rep_lens_carve(a, n, scope, &w);
    if (a.overflow) return SFX_ERR_INTERNAL;
    SFX_HIP(hipMemsetAsync(w.bad, 0, sizeof(uint32_t), st));
    const unsigned grid = (unsigned)dmin<uint64_t>((n + kBlock - 1) / kBlock, kMaxGrid);
    if (scope == SFX_REP_ANY) {
        SFX_LAUNCH("rep_any", (double)n * (d_src ? 20 : 12), k_rep_any, grid, kBlock, st, d_sa, d_lcp, n, d_rep, d_src, w.bad);
    } else if (scope == SFX_REP_EARLIER) {
        Pyramid pl, ps;
        SFX_TRY(pyramid_build(d_lcp, n, w.pyr_lcp, "rep_pyramid", st, &pl));
        SFX_TRY(pyramid_build(d_sa, n, w.pyr_sa, "rep_pyramid", st, &ps, 0));
        const uint64_t cap = open_list_cap(n);
        SFX_HIP(hipMemsetAsync(w.open_count, 0, sizeof(unsigned long long), st));
        Chunking ch = make_chunking(n, kIvTile, 4 * kMaxGrid);
        SFX_LAUNCH("rep_earlier", (double)n * (d_src ? 16 : 12), k_rep_earlier, ch.blocks, kBlock, st, ps, pl, n, ch.tiles_per_block, d_rep,
                   d_src, w.open_list, cap, w.open_count, w.bad);
        SFX_LAUNCH("rep_earlier_open", 0.0, k_rep_earlier_open, grid, kBlock, st, ps, pl, n, (const uint32_t*)w.open_list, cap,
                   (const unsigned long long*)w.open_count, d_rep, d_src);
    } else {
        SFX_LAUNCH("rep_doc_runs", (double)n * 12, k_rep_doc_heads, grid, kBlock, st, d_sa, d_da, n, w.P, w.bad);
        SFX_TRY(gsa_scan<uint32_t>(w.P, n, w.P, w.part, st));
        uint32_t runs = 0;
        SFX_TRY(read_back(&runs, w.P + n, sizeof(runs), st));
        if (runs <= 1) {                                     // one document: nothing is in another one, no search
            SFX_HIP(hipMemsetAsync(d_rep, 0, n * sizeof(uint32_t), st));
            if (d_src) SFX_HIP(hipMemsetAsync(d_src, 0xFF, n * sizeof(uint32_t), st));
        } else {
            Pyramid pl;
            SFX_TRY(pyramid_build(d_lcp, n, w.pyr_lcp, "rep_pyramid", st, &pl));
            SFX_LAUNCH("rep_doc_runs", (double)n * 8 + (double)runs * 4, k_rep_run_starts, grid, kBlock, st, (const uint32_t*)w.P, n,
                       w.run_start);
            SFX_LAUNCH("rep_other_doc", (double)n * (d_src ? 24 : 16), k_rep_other_doc, grid, kBlock, st, d_sa, pl, n,
                       (const uint32_t*)w.P, (const uint32_t*)w.run_start, d_rep, d_src);
        }
    }
    uint32_t bad = 0;
    SFX_TRY(read_back(&bad, w.bad, sizeof(bad), st));
    return bad ? SFX_ERR_ARG : SFX_OK;
}

// Spans: byte i is covered iff some qualifying p <= i (rep[p] >= min_len) reaches past it, i.e. iff the prefix MAXIMUM of
// p + rep[p] over the qualifying p <= i exceeds i.  The scan has the three phases of gsa_scan with max in place of add;
// a run begins at a covered byte whose predecessor is not covered or that starts a document; the k-th end belongs to
// the k-th begin, so one sum scan of the begin flags places both.
__device__ __forceinline__ uint32_t rep_span_reach(const uint32_t* __restrict__ rep, uint64_t p, uint32_t min_len, uint64_t n)
{
    const uint32_t v = rep[p];
    return v >= min_len ? (uint32_t)dmin<uint64_t>(p + v, n) : 0u;       // (<= n: fits, whatever the caller's array holds)
}
__global__ void __launch_bounds__(kBlock)
k_rep_spans_max_count(const uint32_t* __restrict__ rep, uint64_t n, uint32_t min_len, uint64_t chunk, uint32_t* __restrict__ part)
{
    __shared__ uint32_t sh[kWavesPerBlock];
    const uint64_t b = (uint64_t)blockIdx.x * chunk, e = dmin<uint64_t>(b + chunk, n);
    uint32_t acc = 0;
    for (uint64_t i = b + threadIdx.x; i < e; i += kBlock) acc = dmax(acc, rep_span_reach(rep, i, min_len, n));
    uint32_t total;
    (void)block_scan_max_excl<uint32_t>(acc, sh, total);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}
__global__ void __launch_bounds__(kBlock)
k_rep_spans_max_top(uint32_t* __restrict__ part, unsigned nb)
{
    __shared__ uint32_t sh[kWavesPerBlock];
    uint32_t carry = 0;
    for (unsigned base = 0; base < nb; base += kBlock) {
        const unsigned i = base + threadIdx.x;
        uint32_t total;
        const uint32_t ex = block_scan_max_excl<uint32_t>(i < nb ? part[i] : 0u, sh, total);
        if (i < nb) part[i] = dmax(carry, ex);
        carry = dmax(carry, total);
    }
}
__global__ void __launch_bounds__(kBlock)
k_rep_spans_max_apply(const uint32_t* __restrict__ rep, uint64_t n, uint32_t min_len, uint64_t chunk, const uint32_t* __restrict__ part,
                      uint32_t* __restrict__ M)
{
    __shared__ uint32_t sh[kWavesPerBlock];
    const uint64_t b = (uint64_t)blockIdx.x * chunk, e = dmin<uint64_t>(b + chunk, n);
    uint32_t run = part[blockIdx.x];
    for (uint64_t base = b; base < e; base += kBlock) {                // (uniform trip count: the block scan has barriers)
        const uint64_t i = base + threadIdx.x;
        const uint32_t v = i < e ? rep_span_reach(rep, i, min_len, n) : 0u;
        uint32_t total;
        const uint32_t ex = block_scan_max_excl<uint32_t>(v, sh, total);
        if (i < e) M[i] = dmax(run, dmax(ex, v));
        run = dmax(run, total);
    }
}
// document starts: ndocs writes into a zeroed byte per position (empty documents write the same byte again)
__global__ void __launch_bounds__(kBlock)
k_rep_spans_mark(const uint64_t* __restrict__ starts, uint64_t ndocs, uint64_t n, uint8_t* __restrict__ mark)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < ndocs; i += stride) {
        const uint64_t s = starts[i];
        if (s < n) mark[s] = 1;
    }
}
__global__ void __launch_bounds__(kBlock)
k_rep_spans_flag(const uint32_t* __restrict__ M, const uint8_t* __restrict__ mark, uint64_t n, uint32_t* __restrict__ flag)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const bool cov = M[i] > i, prev = i > 0 && M[i - 1] > i - 1;
        flag[i] = (cov && (!prev || (mark && mark[i]))) ? 1u : 0u;
    }
}
// P = the exclusive scan of the begin flags: a begin at i is span P[i]; a covered byte that ends a run ends span P[i + 1] - 1
__global__ void __launch_bounds__(kBlock)
k_rep_spans_emit(const uint32_t* __restrict__ M, const uint8_t* __restrict__ mark, const uint32_t* __restrict__ P, uint64_t n,
                 uint32_t* __restrict__ begin, uint32_t* __restrict__ end, uint64_t capacity)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        if (!(M[i] > i)) continue;
        const uint32_t k0 = P[i], k1 = P[i + 1];
        if (k1 != k0 && k0 < capacity) begin[k0] = (uint32_t)i;
        const bool last = i + 1 == n || !(M[i + 1] > i + 1) || (mark && mark[i + 1]);
        if (last && (uint64_t)(k1 - 1) < capacity) end[k1 - 1] = (uint32_t)(i + 1);
    }
}

// [bad flag | prefix maxima n | flags / their scan n + 1 | scan partials | document-start marks n + 1 bytes]
struct RepSpansWs {
    uint32_t *bad, *M, *P, *part;
    uint8_t* mark;
};
template <class A> static void rep_spans_carve(A& a, uint64_t n, RepSpansWs* w)
{
    w->bad = a.template take<uint32_t>(64);
    w->M = a.template take<uint32_t>(n);
    w->P = a.template take<uint32_t>(n + 1);
    w->part = a.template take<uint32_t>(kMaxGrid + 64);
    w->mark = a.template take<uint8_t>(n + 1);
}
uint64_t repeat_spans_workspace_bytes(uint64_t n)
{
    GsaSizer z;
    RepSpansWs w;
    rep_spans_carve(z, n, &w);
    return z.used;
}
int repeat_spans_dev(const uint32_t* d_rep, uint64_t n, uint32_t min_len, const uint64_t* d_starts, uint64_t ndocs, uint32_t* d_begin,
                     uint32_t* d_end, uint64_t capacity, uint64_t* count_out, void* ws, uint64_t ws_bytes, hipStream_t st)
{
    if (!count_out || min_len == 0) return SFX_ERR_ARG;
    *count_out = 0;
    if (n > 0xFFFFFFFFull || ndocs > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!d_rep || (capacity && (!d_begin || !d_end)) || (d_starts && ndocs == 0)) return SFX_ERR_ARG;
    if (!ws || ws_bytes < repeat_spans_workspace_bytes(n)) return SFX_ERR_WORKSPACE;
    Arena a(ws, ws_bytes);
    RepSpansWs w;
    rep_spans_carve(a, n, &w);
    if (a.overflow) return SFX_ERR_INTERNAL;
    const uint8_t* mark = nullptr;
    if (d_starts) {
        bool bad = false;
        SFX_TRY(gsa_check_docs(d_starts, ndocs, n, w.bad, st, &bad));
        if (bad) return SFX_ERR_ARG;
        SFX_HIP(hipMemsetAsync(w.mark, 0, n + 1, st));
        const unsigned dgrid = (unsigned)dmin<uint64_t>((ndocs + kBlock - 1) / kBlock, kMaxGrid);
        SFX_LAUNCH("rep_spans_mark", (double)ndocs * 9, k_rep_spans_mark, dgrid, kBlock, st, d_starts, ndocs, n, w.mark);
        mark = w.mark;
    }
    const unsigned nb = (unsigned)dmin<uint64_t>((n + kBlock - 1) / kBlock, dmin<unsigned>(kMaxGrid, grid_cap()));
    const uint64_t chunk = (n + nb - 1) / nb;
    SFX_LAUNCH("rep_spans_max", (double)n * 4, k_rep_spans_max_count, nb, kBlock, st, d_rep, n, min_len, chunk, w.part);
    SFX_LAUNCH("rep_spans_max", (double)nb * 8, k_rep_spans_max_top, 1, kBlock, st, w.part, nb);
    SFX_LAUNCH("rep_spans_max", (double)n * 8, k_rep_spans_max_apply, nb, kBlock, st, d_rep, n, min_len, chunk, (const uint32_t*)w.part, w.M);
    const unsigned grid = (unsigned)dmin<uint64_t>((n + kBlock - 1) / kBlock, kMaxGrid);
    SFX_LAUNCH("rep_spans_flag", (double)n * (mark ? 9 : 8), k_rep_spans_flag, grid, kBlock, st, (const uint32_t*)w.M, mark, n, w.P);
    SFX_TRY(gsa_scan<uint32_t>(w.P, n, w.P, w.part, st));
    SFX_LAUNCH("rep_spans", (double)n * (mark ? 9 : 8), k_rep_spans_emit, grid, kBlock, st, (const uint32_t*)w.M, mark, (const uint32_t*)w.P,
               n, d_begin, d_end, capacity);
    uint32_t count = 0;
    SFX_TRY(read_back(&count, w.P + n, sizeof(count), st));
    *count_out = count;
    return SFX_OK;
}

// ---- suffix-tree node table with ordered children (include/suffix_hip.h: sfx_suffix_tree_dev) ------------------
// The topology above looks upwards and names nodes by boundary numbers.  The table looks down: the heads (boundary 0
// and every p with node[p] == p) get dense ids by a scan of their flags, which is the order the reference's sweep
// creates them in; every child item -- a non-root head under its parent, a rank under its leaf parent unless its
// suffix ends exactly at that node (the node's TERMINAL, lib.rs:127-131) -- counts itself at its parent, a 64-bit
// scan of the counts gives the segments, a second pass over the same items hands out the slots of a segment in
// arrival order (the counter counted down again), and every segment is then ordered by its first ranks: the result
// does not depend on the order the atomics ran in.  A node of a text has at most 256 children (distinct first
// bytes), so no counter receives more than 256 adds however large n is.
constexpr int kTreeLaneSeg = 8;                  // segments of up to 8 children are ordered by one lane, in registers
constexpr int kTreeWaveSeg = 256;                // longer ones by a wave in LDS (a longer one is no text's: left as it is)

// head flags for the scan, and the table check
__global__ void __launch_bounds__(kBlock)
k_tree_heads(const uint32_t* __restrict__ sa, const uint32_t* __restrict__ node, uint64_t n, uint32_t* __restrict__ flag,
             uint32_t* __restrict__ bad)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += stride) {
        if (sa[p] >= n) *bad = 1u;
        flag[p] = (p == 0 || node[p] == p) ? 1u : 0u;
    }
}
// is the leaf of rank r, hanging under the node of boundary v, a child of it (true) or its terminal (false)?
__device__ __forceinline__ bool tree_leaf_is_child(const uint32_t* __restrict__ sa, const uint32_t* __restrict__ lcp, uint64_t n,
                                                   uint64_t r, uint32_t v)
{
    const uint64_t s = sa[r];
    const uint32_t depth = v ? lcp[v] : 0u;
    return !(s < n && n - s == depth);
}
// P = the exclusive scan of the head flags (P[boundary of a head] = its dense id, P[n] = the number of nodes).
// Every child item adds one to its parent's counter (cnt: n + 1 zeroed words; an id is <= n whatever lcp holds).
__global__ void __launch_bounds__(kBlock)
k_tree_count(const uint32_t* __restrict__ sa, const uint32_t* __restrict__ lcp, uint64_t n, const uint32_t* __restrict__ node,
             const uint32_t* __restrict__ parent, const uint32_t* __restrict__ leaf_parent, const uint32_t* __restrict__ P,
             uint32_t* __restrict__ cnt)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += stride) {
        if (p && node[p] == p) {
            const uint32_t up = parent[p];
            if (up < n) atomicAdd(&cnt[P[up]], 1u);
        }
        const uint32_t v = leaf_parent[p];
        if (v < n && tree_leaf_is_child(sa, lcp, n, p, v)) atomicAdd(&cnt[P[v]], 1u);
    }
}
// the three words the host waits for: nodes, children, the table check
__global__ void __launch_bounds__(64)
k_tree_totals(const uint32_t* __restrict__ P, const uint64_t* __restrict__ off, const uint32_t* __restrict__ bad, uint64_t n,
              uint64_t* __restrict__ res)
{
    if (threadIdx.x == 0) {
        res[0] = P[n];
        res[1] = off[n];
        res[2] = *bad;
    }
}
__device__ __forceinline__ void tree_place(uint32_t* __restrict__ cnt, const uint64_t* __restrict__ off, uint64_t total, uint32_t k,
                                           uint32_t first, uint32_t id, uint32_t* __restrict__ child_lb, uint32_t* __restrict__ child_node)
{
    const uint32_t slot = atomicSub(&cnt[k], 1u) - 1u;               // (the count of k_tree_count, handed back one by one)
    const uint64_t at = off[k] + slot;
    if (at < total) {                                                // (always, for the items that were counted)
        child_lb[at] = first;
        child_node[at] = id;
    }
}
// one lane per boundary / rank p: the five per-node arrays of a head, its slot under its parent, the slot of leaf p
__global__ void __launch_bounds__(kBlock)
k_tree_fill(const uint32_t* __restrict__ sa, const uint32_t* __restrict__ lcp, uint64_t n, const uint32_t* __restrict__ lb,
            const uint32_t* __restrict__ rb, const uint32_t* __restrict__ node, const uint32_t* __restrict__ parent,
            const uint32_t* __restrict__ leaf_parent, const uint32_t* __restrict__ P, uint32_t* __restrict__ cnt,
            const uint64_t* __restrict__ off, uint64_t nodes, uint64_t total, uint32_t* __restrict__ node_lb,
            uint32_t* __restrict__ node_rb, uint32_t* __restrict__ node_depth, uint32_t* __restrict__ node_parent,
            uint32_t* __restrict__ node_terminal, uint32_t* __restrict__ child_lb, uint32_t* __restrict__ child_node,
            uint32_t* __restrict__ leaf_parent_out)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += stride) {
        if (p == 0 || node[p] == p) {
            const uint32_t k = P[p];
            const uint32_t l = p ? lb[p] : 0u, depth = p ? lcp[p] : 0u;
            const uint32_t up = p ? parent[p] : kNoNode;
            const uint32_t upk = up < n ? P[up] : kNoNode;
            if (k < nodes) {
                const uint64_t s = l < n ? sa[l] : n;
                node_lb[k] = l;
                node_rb[k] = p ? rb[p] : (uint32_t)(n - 1);
                node_depth[k] = depth;
                node_parent[k] = upk;
                node_terminal[k] = (s < n && n - s == depth) ? (uint32_t)s : kNoNode;
            }
            if (upk != kNoNode) tree_place(cnt, off, total, upk, l, k, child_lb, child_node);
        }
        const uint32_t v = leaf_parent[p];
        if (v < n) {
            const uint32_t k = P[v];
            if (leaf_parent_out) leaf_parent_out[p] = k;
            if (tree_leaf_is_child(sa, lcp, n, p, v)) tree_place(cnt, off, total, k, (uint32_t)p, kNoNode, child_lb, child_node);
        }
    }
}
// first byte of the edge to the child that starts at rank `first`, under a node of string depth `depth`
__device__ __forceinline__ uint8_t tree_edge_byte(const uint8_t* __restrict__ text, const uint32_t* __restrict__ sa, uint64_t n,
                                                  uint32_t first, uint32_t depth)
{
    if (first >= n) return 0;
    const uint64_t at = (uint64_t)sa[first] + depth;
    return at < n ? text[at] : (uint8_t)0;
}
#define SFX_TREE_CSWAP(a, b) do { const uint64_t lo_ = dmin(a, b), hi_ = dmax(a, b); a = lo_; b = hi_; } while (0)
// Orders every segment by (first rank << 32 | child id) -- first ranks are distinct inside a node -- and writes the edge bytes.
// A wave takes 64 nodes at a time: each lane orders its node's segment if that is short (an 8-input network on
// registers), then the wave goes through the longer ones among the 64 together, ranking every entry against the others in LDS.
__global__ void __launch_bounds__(kBlock)
k_tree_order(const uint8_t* __restrict__ text, const uint32_t* __restrict__ sa, uint64_t n, uint64_t nodes,
             const uint64_t* __restrict__ off, const uint32_t* __restrict__ node_depth, uint32_t* __restrict__ child_lb,
             uint32_t* __restrict__ child_node, uint8_t* __restrict__ child_byte)
{
    __shared__ uint64_t seg[kWavesPerBlock][kTreeWaveSeg];
    const unsigned lane = lane_id(), wave = wave_id();
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock + wave * kWave; base < nodes; base += stride) {
        const uint64_t k = base + lane;
        const bool valid = k < nodes;
        const uint64_t b = valid ? off[k] : 0, e = valid ? off[k + 1] : 0;
        const uint64_t len = e >= b ? e - b : 0;
        if (valid && len >= 1 && len <= (uint64_t)kTreeLaneSeg) {
            const uint32_t depth = node_depth[k];
            const uint64_t none = ~0ull;
            uint64_t a0 = ((uint64_t)child_lb[b] << 32) | child_node[b], a1 = none, a2 = none, a3 = none, a4 = none, a5 = none,
                     a6 = none, a7 = none;
            if (len > 1) a1 = ((uint64_t)child_lb[b + 1] << 32) | child_node[b + 1];
            if (len > 2) a2 = ((uint64_t)child_lb[b + 2] << 32) | child_node[b + 2];
            if (len > 3) a3 = ((uint64_t)child_lb[b + 3] << 32) | child_node[b + 3];
            if (len > 4) a4 = ((uint64_t)child_lb[b + 4] << 32) | child_node[b + 4];
            if (len > 5) a5 = ((uint64_t)child_lb[b + 5] << 32) | child_node[b + 5];
            if (len > 6) a6 = ((uint64_t)child_lb[b + 6] << 32) | child_node[b + 6];
            if (len > 7) a7 = ((uint64_t)child_lb[b + 7] << 32) | child_node[b + 7];
            if (len > 1) {
                SFX_TREE_CSWAP(a0, a1); SFX_TREE_CSWAP(a2, a3);
                SFX_TREE_CSWAP(a0, a2); SFX_TREE_CSWAP(a1, a3);
                SFX_TREE_CSWAP(a1, a2);
            }
            if (len > 4) {                                           // (19 exchanges in all: the 8-input network)
                SFX_TREE_CSWAP(a4, a5); SFX_TREE_CSWAP(a6, a7);
                SFX_TREE_CSWAP(a4, a6); SFX_TREE_CSWAP(a5, a7);
                SFX_TREE_CSWAP(a5, a6);
                SFX_TREE_CSWAP(a0, a4); SFX_TREE_CSWAP(a1, a5); SFX_TREE_CSWAP(a2, a6); SFX_TREE_CSWAP(a3, a7);
                SFX_TREE_CSWAP(a2, a4); SFX_TREE_CSWAP(a3, a5);
                SFX_TREE_CSWAP(a1, a2); SFX_TREE_CSWAP(a3, a4); SFX_TREE_CSWAP(a5, a6);
            }
#define SFX_TREE_PUT(i, a)                                                                              \
    if (len > i) {                                                                                      \
        child_lb[b + i] = (uint32_t)(a >> 32);                                                          \
        child_node[b + i] = (uint32_t)a;                                                                \
        if (child_byte) child_byte[b + i] = tree_edge_byte(text, sa, n, (uint32_t)(a >> 32), depth);    \
    }
            SFX_TREE_PUT(0, a0) SFX_TREE_PUT(1, a1) SFX_TREE_PUT(2, a2) SFX_TREE_PUT(3, a3)
            SFX_TREE_PUT(4, a4) SFX_TREE_PUT(5, a5) SFX_TREE_PUT(6, a6) SFX_TREE_PUT(7, a7)
#undef SFX_TREE_PUT
        }
        unsigned long long todo = __ballot(valid && len > (uint64_t)kTreeLaneSeg);
        while (todo) {
            const unsigned src = (unsigned)__ffsll(todo) - 1u;
            todo &= todo - 1ull;
            const uint64_t kk = base + src;
            const uint64_t sb = off[kk], sl = off[kk + 1] - sb;
            const uint32_t depth = node_depth[kk];
            uint64_t* sh = seg[wave];
            if (sl <= (uint64_t)kTreeWaveSeg) {
                for (uint64_t i = lane; i < sl; i += kWave) sh[i] = ((uint64_t)child_lb[sb + i] << 32) | child_node[sb + i];
                wave_sync();
                for (uint64_t i = lane; i < sl; i += kWave) {
                    const uint64_t mine = sh[i];
                    uint32_t r = 0;
                    for (uint32_t j = 0; j < (uint32_t)sl; j++) r += sh[j] < mine ? 1u : 0u;
                    child_lb[sb + r] = (uint32_t)(mine >> 32);
                    child_node[sb + r] = (uint32_t)mine;
                    if (child_byte) child_byte[sb + r] = tree_edge_byte(text, sa, n, (uint32_t)(mine >> 32), depth);
                }
                wave_sync();
            } else if (child_byte) {                                 // (no text has such a node: the bytes only, in place)
                for (uint64_t i = lane; i < sl; i += kWave) child_byte[sb + i] = tree_edge_byte(text, sa, n, child_lb[sb + i], depth);
            }
        }
    }
}
#undef SFX_TREE_CSWAP

// [results | bad flag | lb, rb, node, parent, leaf_parent: n each | P: n + 1 | counters: n + 1 | offsets: n + 1 u64 |
//  scan partials | the topology's own workspace]
struct TreeWs {
    uint64_t *res, *off, *part;
    uint32_t *bad, *lb, *rb, *node, *parent, *leaf_parent, *P, *cnt;
    uint8_t* topo;
};
template <class A> static void tree_carve(A& a, uint64_t n, TreeWs* w)
{
    w->res = a.template take<uint64_t>(32);
    w->bad = a.template take<uint32_t>(64);
    w->lb = a.template take<uint32_t>(n);
    w->rb = a.template take<uint32_t>(n);
    w->node = a.template take<uint32_t>(n);
    w->parent = a.template take<uint32_t>(n);
    w->leaf_parent = a.template take<uint32_t>(n);
    w->P = a.template take<uint32_t>(n + 1);
    w->cnt = a.template take<uint32_t>(n + 1);
    w->off = a.template take<uint64_t>(n + 1);
    w->part = a.template take<uint64_t>(kMaxGrid + 64);
    w->topo = a.template take<uint8_t>(lcp_intervals_workspace_bytes(n));
}
uint64_t suffix_tree_workspace_bytes(uint64_t n)
{
    if (n == 0 || n > 0xFFFFFFFFull) return 0;
    GsaSizer z;
    TreeWs w;
    tree_carve(z, n, &w);
    return z.used;
}
int suffix_tree_dev(const uint8_t* d_text, const uint32_t* d_sa, const uint32_t* d_lcp, uint64_t n, uint64_t node_capacity,
                    uint64_t child_capacity, uint32_t* d_node_lb, uint32_t* d_node_rb, uint32_t* d_node_depth,
                    uint32_t* d_node_parent, uint32_t* d_node_terminal, uint64_t* d_child_off, uint32_t* d_child_lb,
                    uint32_t* d_child_node, uint8_t* d_child_byte, uint32_t* d_leaf_parent, uint64_t* nodes_out,
                    uint64_t* children_out, void* ws, uint64_t ws_bytes, hipStream_t st)
{
    if (!nodes_out || !children_out) return SFX_ERR_ARG;
    *nodes_out = 0;
    *children_out = 0;
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if ((d_text == nullptr) != (d_child_byte == nullptr)) return SFX_ERR_ARG;
    if (n == 0) return SFX_OK;
    if (!d_sa || !d_lcp) return SFX_ERR_ARG;
    if (!ws || ws_bytes < suffix_tree_workspace_bytes(n)) return SFX_ERR_WORKSPACE;
    Arena a(ws, ws_bytes);
    TreeWs w;
    tree_carve(a, n, &w);
    if (a.overflow) return SFX_ERR_INTERNAL;
    SFX_TRY(lcp_intervals_dev(d_lcp, n, w.lb, w.rb, w.node, w.parent, w.leaf_parent, w.topo, lcp_intervals_workspace_bytes(n), st));
    SFX_HIP(hipMemsetAsync(w.bad, 0, sizeof(uint32_t), st));
    SFX_HIP(hipMemsetAsync(w.cnt, 0, (n + 1) * sizeof(uint32_t), st));
    const unsigned grid = (unsigned)dmin<uint64_t>((n + kBlock - 1) / kBlock, kMaxGrid);
    SFX_LAUNCH("tree_heads", (double)n * 12, k_tree_heads, grid, kBlock, st, d_sa, (const uint32_t*)w.node, n, w.P, w.bad);
    SFX_TRY(gsa_scan<uint32_t>(w.P, n, w.P, reinterpret_cast<uint32_t*>(w.part), st));
    SFX_LAUNCH("tree_count", (double)n * 28, k_tree_count, grid, kBlock, st, d_sa, d_lcp, n, (const uint32_t*)w.node,
               (const uint32_t*)w.parent, (const uint32_t*)w.leaf_parent, (const uint32_t*)w.P, w.cnt);
    SFX_TRY(gsa_scan<uint64_t>(w.cnt, n, w.off, w.part, st));
    SFX_LAUNCH("tree_totals", 0.0, k_tree_totals, 1, 64, st, (const uint32_t*)w.P, (const uint64_t*)w.off, (const uint32_t*)w.bad, n,
               w.res);
    uint64_t res[3] = {0, 0, 0};
    SFX_TRY(read_back(res, w.res, sizeof(res), st));
    if (res[2]) return SFX_ERR_ARG;
    const uint64_t nodes = res[0], total = res[1];
    *nodes_out = nodes;
    *children_out = total;
    if (nodes > node_capacity || total > child_capacity) return SFX_OK;
    if (!d_node_lb || !d_node_rb || !d_node_depth || !d_node_parent || !d_node_terminal || !d_child_off ||
        (total && (!d_child_lb || !d_child_node)))
        return SFX_ERR_ARG;
    SFX_HIP(hipMemcpyAsync(d_child_off, w.off, (nodes + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    SFX_LAUNCH("tree_fill", (double)n * 44 + (double)nodes * 20, k_tree_fill, grid, kBlock, st, d_sa, d_lcp, n, (const uint32_t*)w.lb,
               (const uint32_t*)w.rb, (const uint32_t*)w.node, (const uint32_t*)w.parent, (const uint32_t*)w.leaf_parent,
               (const uint32_t*)w.P, w.cnt, (const uint64_t*)w.off, nodes, total, d_node_lb, d_node_rb, d_node_depth, d_node_parent,
               d_node_terminal, d_child_lb, d_child_node, d_leaf_parent);
    const unsigned ogrid = (unsigned)dmin<uint64_t>((nodes + kBlock - 1) / kBlock, kMaxGrid);
    SFX_LAUNCH("tree_order", (double)nodes * 12 + (double)total * (d_child_byte ? 22 : 16), k_tree_order, ogrid, kBlock, st, d_text, d_sa,
               n, nodes, (const uint64_t*)w.off, (const uint32_t*)d_node_depth, d_child_lb, d_child_node, d_child_byte);
    return SFX_OK;
}

// ---- Burrows-Wheeler transform with sampled ranks, and its inverse (include/suffix_hip.h) ----
// Rows are the n + 1 sorted rotations of T$: row 0 begins with $, row R >= 1 with suffix sa[R-1]; the primary is the row
// of suffix 0, and row R != primary sits at bwt[R < primary ? R : R - 1].
// Forward: a pass over the table finds the primary (samples[0]), then one rank per lane gathers T[sa - 1].
// Not covered: collections (per-document terminators), inversion without samples at scale (list ranking), the transform
// without a table.  (Occurrence tables and backward search: sfx_fm.hip.)
__global__ void __launch_bounds__(kBlock)
k_bwt_primary(const uint32_t* __restrict__ sa, uint64_t n, uint32_t* __restrict__ samples)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride)
        if (sa[r] == 0u) atomicMax(&samples[0], (uint32_t)(r + 1));       // (the largest of several zeros; none: stays 0)
}
// the index of row R in bwt, for a primary in [1, n] and R in [0, n], R != primary: always in [0, n-1]
__device__ __forceinline__ uint64_t bwt_index(uint64_t R, uint64_t primary) { return R < primary ? R : R - 1; }
// One row per lane: a coalesced read of the table, one random byte, a coalesced byte store at the shifted index, and the
// sample scatter where sa % step == 0 (samples[0] is k_bwt_primary's and only read here).  The table is unchecked: a
// primary of 0 (no zero entry) is clamped into [1, n], a second zero entry wraps to T[n-1], and with every entry < n
// each index stays inside its array.
__global__ void __launch_bounds__(kBlock)
k_bwt_gather(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ sa, uint32_t step, int shift,
             uint8_t* __restrict__ bwt, uint32_t* __restrict__ samples)
{
    const uint64_t primary = dmin<uint64_t>(dmax<uint64_t>(samples[0], 1), n);
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t R = (uint64_t)blockIdx.x * kBlock + threadIdx.x; R <= n; R += stride) {
        if (R == 0) { bwt[0] = text[n - 1]; continue; }
        const uint64_t s = sa[R - 1];
        const uint8_t c = text[s ? s - 1 : n - 1];
        if (R != primary) bwt[bwt_index(R, primary)] = c;
        if (step && s && (s & (uint64_t)(step - 1u)) == 0) samples[s >> shift] = (uint32_t)R;
    }
}
__host__ __device__ inline bool bwt_step_ok(uint32_t step) { return (step & (step - 1u)) == 0; }
uint64_t bwt_sample_count(uint64_t n, uint32_t step)
{
    if (n == 0 || !bwt_step_ok(step)) return 0;
    return step ? (n + step - 1) / step : 1;
}
int bwt_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, uint32_t step, uint8_t* d_bwt, uint32_t* d_samples, hipStream_t st)
{
    if (!bwt_step_ok(step)) return SFX_ERR_ARG;
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!d_text || !d_sa || !d_bwt || !d_samples) return SFX_ERR_ARG;
    SFX_HIP(hipMemsetAsync(d_samples, 0, sizeof(uint32_t), st));
    const unsigned pgrid = (unsigned)dmin<uint64_t>((n + kBlock - 1) / kBlock, kMaxGrid);
    SFX_LAUNCH("bwt_primary", (double)n * 4, k_bwt_primary, pgrid, kBlock, st, d_sa, n, d_samples);
    const unsigned grid = (unsigned)dmin<uint64_t>((n + kBlock) / kBlock, kMaxGrid);
    SFX_LAUNCH("bwt_gather", (double)n * 5 + (double)n * 64, k_bwt_gather, grid, kBlock, st, d_text, n, d_sa, step,
               step ? bits_for(step) - 1 : 0, d_bwt, d_samples);
    return SFX_OK;
}

// lf from bwt: a stable 256-way counting rank.  A tile is `tile` bytes (a multiple of kBlock), one workgroup, a quarter per
// wave.  k_bwt_rank_count: per tile the count of every symbol, counts[tile][256].  k_bwt_rank_scan_*: per symbol the
// exclusive scan of its column over the tiles -- thread d owns symbol d, a chunk of tiles per workgroup, the chunks' sums
// scanned by one workgroup, which also lays down C[0..256] -- leaving 1 + C[d] + (occurrences in earlier tiles) in place.
// k_bwt_rank: the tile's bases, split over its waves by their own counts, then the match-mask ranking of the radix
// passes (rank_round's scheme) 64 bytes at a time.
constexpr uint64_t kBwtTile = 16384;
static uint64_t bwt_tile()
{
    static const uint64_t tile = [] {                   // test hook: SFX_BWT_TILE=<bytes>, so that small inputs span several tiles
        const char* e = dev_env("SFX_BWT_TILE");
        const long long v = e ? atoll(e) : 0;
        return (v >= kBlock && v <= (long long)kBwtTile && v % kBlock == 0) ? (uint64_t)v : kBwtTile;
    }();
    return tile;
}
struct BwtRankLds {
    unsigned long long flags[kWavesPerBlock][kRadixDev];
    uint32_t cnt[kWavesPerBlock][kRadixDev];
};
// the counts of the calling wave's quarter of tile t into s.cnt[wave] (which the caller has zeroed)
__device__ __forceinline__ void bwt_wave_count(const uint8_t* __restrict__ bwt, uint64_t n, uint64_t b, uint64_t e, uint32_t* cnt_w)
{
    for (uint64_t i = b + lane_id(); i < e; i += kWave) atomicAdd(&cnt_w[bwt[i]], 1u);
    (void)n;
}
__global__ void __launch_bounds__(kBlock)
k_bwt_rank_count(const uint8_t* __restrict__ bwt, uint64_t n, uint64_t tile, uint64_t ntiles, uint32_t* __restrict__ counts)
{
    __shared__ BwtRankLds s;
    const unsigned tid = threadIdx.x, w = wave_id();
    const uint64_t quarter = tile / kWavesPerBlock;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
#pragma unroll
        for (int k = 0; k < kWavesPerBlock; k++) s.cnt[k][tid] = 0u;
        __syncthreads();
        const uint64_t b = dmin<uint64_t>(t * tile + w * quarter, n), e = dmin<uint64_t>(b + quarter, n);
        bwt_wave_count(bwt, n, b, e, s.cnt[w]);
        __syncthreads();
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < kWavesPerBlock; k++) sum += s.cnt[k][tid];
        counts[t * kRadixDev + tid] = sum;
        __syncthreads();
    }
}
__global__ void __launch_bounds__(kBlock)
k_bwt_rank_scan_count(const uint32_t* __restrict__ counts, uint64_t ntiles, uint64_t chunk, uint32_t* __restrict__ part)
{
    const uint64_t b = (uint64_t)blockIdx.x * chunk, e = dmin<uint64_t>(b + chunk, ntiles);
    uint32_t acc = 0;
    for (uint64_t t = b; t < e; t++) acc += counts[t * kRadixDev + threadIdx.x];
    part[(uint64_t)blockIdx.x * kRadixDev + threadIdx.x] = acc;
}
// one workgroup: thread d scans the chunks' sums of symbol d, the symbols' totals are scanned into C, and every chunk's
// carry becomes 1 + C[d] + (occurrences of d in earlier chunks): the lf value of the chunk's first d
__global__ void __launch_bounds__(kBlock)
k_bwt_rank_scan_top(uint32_t* __restrict__ part, unsigned nb, uint32_t* __restrict__ ctab)
{
    __shared__ uint32_t sh[kWavesPerBlock];
    const unsigned d = threadIdx.x;
    uint32_t run = 0;
    for (unsigned b = 0; b < nb; b++) run += part[(uint64_t)b * kRadixDev + d];
    uint32_t total;
    const uint32_t C = block_scan_add_excl<uint32_t>(run, sh, total);
    ctab[d] = C;
    if (d == 0) ctab[kRadixDev] = total;
    run = 1u + C;
    for (unsigned b = 0; b < nb; b++) {
        const uint32_t v = part[(uint64_t)b * kRadixDev + d];
        part[(uint64_t)b * kRadixDev + d] = run;
        run += v;
    }
}
__global__ void __launch_bounds__(kBlock)
k_bwt_rank_scan_apply(uint32_t* __restrict__ counts, uint64_t ntiles, uint64_t chunk, const uint32_t* __restrict__ part)
{
    const uint64_t b = (uint64_t)blockIdx.x * chunk, e = dmin<uint64_t>(b + chunk, ntiles);
    uint32_t run = part[(uint64_t)blockIdx.x * kRadixDev + threadIdx.x];
    for (uint64_t t = b; t < e; t++) {
        const uint32_t v = counts[t * kRadixDev + threadIdx.x];
        counts[t * kRadixDev + threadIdx.x] = run;
        run += v;
    }
}
__global__ void __launch_bounds__(kBlock)
k_bwt_rank(const uint8_t* __restrict__ bwt, uint64_t n, uint64_t tile, uint64_t ntiles, const uint32_t* __restrict__ counts,
           uint32_t* __restrict__ lf)
{
    __shared__ BwtRankLds s;
    const unsigned tid = threadIdx.x, w = wave_id(), lane = lane_id();
    const unsigned long long mybit = 1ull << lane;
    const uint64_t quarter = tile / kWavesPerBlock;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
#pragma unroll
        for (int k = 0; k < kWavesPerBlock; k++) {
            s.cnt[k][tid] = 0u;
            s.flags[k][tid] = 0ull;
        }
        __syncthreads();
        const uint64_t b = dmin<uint64_t>(t * tile + w * quarter, n), e = dmin<uint64_t>(b + quarter, n);
        bwt_wave_count(bwt, n, b, e, s.cnt[w]);
        __syncthreads();
        {                                                             // thread d: the waves' bases of symbol d
            uint32_t run = counts[t * kRadixDev + tid];
#pragma unroll
            for (int k = 0; k < kWavesPerBlock; k++) {
                const uint32_t c = s.cnt[k][tid];
                s.cnt[k][tid] = run;
                run += c;
            }
        }
        __syncthreads();
        // (a uniform trip count per wave: the ranking round has wave-level rendezvous; lanes past the end take no part)
        for (uint64_t base = b; base < e; base += kWave) {
            const uint64_t i = base + lane;
            const bool live = i < e;
            const unsigned d = live ? bwt[i] : 0u;
            if (live) atomicOr(&s.flags[w][d], mybit);
            wave_sync();
            const unsigned long long peers = live ? s.flags[w][d] : 0ull;
            const uint32_t pre = live ? s.cnt[w][d] : 0u;
            wave_sync();
            const unsigned below = lanes_below(peers);
            if (live && below == 0) {
                s.flags[w][d] = 0ull;
                s.cnt[w][d] = pre + (uint32_t)__popcll(peers);
            }
            wave_sync();
            if (live) lf[i] = pre + below;
        }
        __syncthreads();
    }
}

// One lane per segment: `len` dependent steps, one random 4-byte read each.  The byte is recovered from lf[i] by a search
// of C[0..256] in LDS: lf[i] - 1 lies in [C[c], C[c+1]) for exactly the c = bwt[i].  Bytes leave four at a time where
// the address allows.  err[0]: a sample outside [1, n]; err[1]: a walk that met the primary row early or did not end at
// samples[k].  No input can take an index out of [0, n-1]: R <= n always (lf values and checked samples), and the
// primary row is never dereferenced.
constexpr int kUnbwtBlock = 64;
__global__ void __launch_bounds__(kUnbwtBlock)
k_unbwt_walk(const uint32_t* __restrict__ lf, uint64_t n, const uint32_t* __restrict__ samples, uint64_t cnt, uint32_t step,
             const uint32_t* __restrict__ ctab, uint8_t* __restrict__ out, uint32_t* __restrict__ err)
{
    __shared__ uint32_t C[kRadixDev + 1];
    for (unsigned k = threadIdx.x; k <= (unsigned)kRadixDev; k += kUnbwtBlock) C[k] = ctab[k];
    __syncthreads();
    const uint64_t k = (uint64_t)blockIdx.x * kUnbwtBlock + threadIdx.x;
    if (k >= cnt) return;
    const uint64_t primary = samples[0], want = samples[k];
    const uint64_t begin = step ? k * step : 0, end = (step && k + 1 < cnt) ? begin + step : n;
    uint64_t R = k + 1 < cnt ? samples[k + 1] : 0;
    if (primary < 1 || primary > n || want < 1 || want > n || R > n || (k + 1 < cnt && R < 1)) {
        err[0] = 1u;
        return;
    }
    uint32_t acc = 0;
    int held = 0;                                                     // acc = the bytes of [pos, pos + held), lowest first
    uint64_t pos = end;
    while (pos > begin) {
        if (R == primary) break;                                      // the $ row: this is no transform
        const uint32_t v = lf[bwt_index(R, primary)];
        unsigned lo = 0, hi = kRadixDev;                              // the c with C[c] <= v - 1 < C[c + 1]
        while (hi - lo > 1) {
            const unsigned mid = (lo + hi) >> 1;
            if (C[mid] <= v - 1u) lo = mid; else hi = mid;
        }
        pos--;
        acc = (acc << 8) | lo;
        if (++held == 4) {
            if (((uintptr_t)(out + pos) & 3u) == 0) {
                *reinterpret_cast<uint32_t*>(out + pos) = acc;
                held = 0;
            } else {
                out[pos + 3] = (uint8_t)(acc >> 24);
                held = 3;
            }
        }
        R = v;
    }
    for (int j = 0; j < held; j++) out[pos + j] = (uint8_t)(acc >> (8 * j));
    if (pos != begin || R != want) err[1] = 1u;
}

// [err 64 words | C 257 words | lf n | counts ntiles x 256 | the scan's chunk sums]
struct UnbwtWs {
    uint32_t *err, *ctab, *lf, *counts, *part;
};
static unsigned bwt_scan_blocks(uint64_t ntiles) { return (unsigned)dmin<uint64_t>(ntiles, dmin<unsigned>(kMaxGrid, grid_cap())); }
template <class A> static void unbwt_carve(A& a, uint64_t n, UnbwtWs* w)
{
    const uint64_t ntiles = (n + bwt_tile() - 1) / bwt_tile();
    w->err = a.template take<uint32_t>(64);
    w->ctab = a.template take<uint32_t>(kRadixDev + 1);
    w->lf = a.template take<uint32_t>(n);
    w->counts = a.template take<uint32_t>(ntiles * kRadixDev);
    w->part = a.template take<uint32_t>((uint64_t)bwt_scan_blocks(ntiles) * kRadixDev);
}
uint64_t unbwt_workspace_bytes(uint64_t n)
{
    if (n == 0) return 0;
    GsaSizer z;
    UnbwtWs w;
    unbwt_carve(z, n, &w);
    return z.used;
}
int unbwt_dev(const uint8_t* d_bwt, uint64_t n, const uint32_t* d_samples, uint64_t nsamples, uint32_t step, uint8_t* d_out, void* ws,
              uint64_t ws_bytes, hipStream_t st)
{
    if (!bwt_step_ok(step)) return SFX_ERR_ARG;
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (nsamples != bwt_sample_count(n, step)) return SFX_ERR_ARG;
    if (n == 0) return SFX_OK;
    if ((step ? dmin<uint64_t>(n, step) : n) > SFX_UNBWT_MAX_CHAIN) return SFX_ERR_ARG;
    if (!d_bwt || !d_samples || !d_out) return SFX_ERR_ARG;
    {
        const uintptr_t a = reinterpret_cast<uintptr_t>(d_bwt), b = reinterpret_cast<uintptr_t>(d_out);
        if (a < b + n && b < a + n) return SFX_ERR_ARG;
    }
    if (!ws || ws_bytes < unbwt_workspace_bytes(n)) return SFX_ERR_WORKSPACE;
    Arena a(ws, ws_bytes);
    UnbwtWs w;
    unbwt_carve(a, n, &w);
    if (a.overflow) return SFX_ERR_INTERNAL;
    const uint64_t tile = bwt_tile(), ntiles = (n + tile - 1) / tile;
    SFX_HIP(hipMemsetAsync(w.err, 0, 64 * sizeof(uint32_t), st));
    const unsigned tgrid = (unsigned)dmin<uint64_t>(ntiles, dmin<unsigned>(kMaxGrid, grid_cap()));
    SFX_LAUNCH("bwt_rank", (double)n, k_bwt_rank_count, tgrid, kBlock, st, d_bwt, n, tile, ntiles, w.counts);
    const unsigned nb = bwt_scan_blocks(ntiles);
    const uint64_t chunk = (ntiles + nb - 1) / nb;
    const double cbytes = (double)ntiles * kRadixDev * 4;
    SFX_LAUNCH("bwt_rank", cbytes, k_bwt_rank_scan_count, nb, kBlock, st, (const uint32_t*)w.counts, ntiles, chunk, w.part);
    SFX_LAUNCH("bwt_rank", (double)nb * kRadixDev * 8, k_bwt_rank_scan_top, 1, kBlock, st, w.part, nb, w.ctab);
    SFX_LAUNCH("bwt_rank", cbytes * 2, k_bwt_rank_scan_apply, nb, kBlock, st, w.counts, ntiles, chunk, (const uint32_t*)w.part);
    SFX_LAUNCH("bwt_rank", (double)n * 5 + cbytes, k_bwt_rank, tgrid, kBlock, st, d_bwt, n, tile, ntiles, (const uint32_t*)w.counts,
               w.lf);
    const uint64_t wgrid = (nsamples + kUnbwtBlock - 1) / kUnbwtBlock;           // (<= 2^32 / 64)
    SFX_LAUNCH("unbwt_walk", (double)n * 65, k_unbwt_walk, (unsigned)wgrid, kUnbwtBlock, st, (const uint32_t*)w.lf, n, d_samples,
               nsamples, step, (const uint32_t*)w.ctab, d_out, w.err);
    uint32_t err[2] = {0, 0};
    SFX_TRY(read_back(err, w.err, sizeof(err), st));
    return (err[0] | err[1]) ? SFX_ERR_ARG : SFX_OK;
}

}  // namespace sfx
