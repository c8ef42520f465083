/* include/suffix_hip.h -- C ABI of libsuffix_hip.so, the MI355X (gfx950) engine
 * that replaces the suffix-array hot path of BurntSushi/suffix v1.3.0.
 *
 * The reference is pure Rust with no FFI of its own; these entry points are
 * what a Rust `extern "C"` block binds at the private seams listed below
 * (citations are /root/reference/src/table.rs; the Rust side a maintainer
 * would add is shown in INTEGRATION.md and rust/suffix-hip/src/lib.rs).
 *
 * Conventions
 *  - caller allocates, callee fills (mirrors `vec![0u32; n]` at :381);
 *  - every function returns an `int` status, 0 == SFX_OK (the reference panics,
 *    :380 / :117; the shim turns non-zero into panic!);
 *  - plain pointers and sizes only; `void* stream` is a hipStream_t (NULL = the
 *    default stream);
 *  - "*_dev" entry points take DEVICE pointers (inputs already resident in HBM,
 *    outputs left in HBM) plus a caller-provided device workspace; the others
 *    take HOST pointers and stage through HBM themselves;
 *  - re-entrant: no global mutable state except the optional profiler.
 *
 * Alignment of the DEVICE pointers of the "*_dev" entry points (checked on the host before anything is
 * launched; a pointer that does not meet it is SFX_ERR_ARG and nothing is read or written):
 *  - text and query bytes (const uint8_t*), d_found, the 256 scratch bytes of sfx_pack_text_dev: ANY address.
 *    The kernels take their 16-byte loads only from a 16-byte boundary on and read the bytes in front one by one;
 *  - uint32_t arrays (suffix array, LCP, DA, rep / src, lb / rb / node / parent / leaf_parent, begin / end, the
 *    query outputs, the packed words, slices of any of them): 4 bytes, the element's own alignment, is enough.
 *    An array that also sits on a 16-byte boundary is read and written 16 bytes at a time where that pays;
 *  - uint64_t arrays (d_qoff, d_doc_starts, d_bins*, d_global_byte_bins256, the widened table): 8 bytes;
 *  - workspaces: SFX_WORKSPACE_ALIGN bytes.  The engine carves a workspace at 256-byte steps FROM ITS BASE and
 *    uses the pieces with loads and stores of up to 16 bytes and with 64-bit atomics, so the base's alignment
 *    is every piece's.  hipMalloc, malloc and every tensor allocator meet it.  A workspace that is long
 *    enough but misaligned is SFX_ERR_ARG; one that is too short (or NULL) is SFX_ERR_WORKSPACE wherever it
 *    lies.  A workspace may hold anything on entry: the engine clears what it needs cleared.
 * Everything a call queues goes to the caller's `stream` and to no other; outputs are complete when the work
 * queued on it is (entry points that read a result back -- documented at each -- synchronise that stream).
 */
#define SFX_WORKSPACE_ALIGN 16
#ifndef SUFFIX_HIP_H
#define SUFFIX_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum {
    SFX_OK = 0,
    SFX_ERR_ARG = 1,          /* null pointer / inconsistent sizes            */
    SFX_ERR_TOO_LARGE = 2,    /* n > u32::MAX on a u32 entry point (:380)     */
    SFX_ERR_NO_DEVICE = 3,    /* no HIP device visible                        */
    SFX_ERR_HIP = 4,          /* a HIP runtime call or kernel failed          */
    SFX_ERR_WORKSPACE = 5,    /* caller workspace smaller than *_workspace_bytes */
    SFX_ERR_INTERNAL = 6,     /* engine invariant violated (bug)              */
    SFX_ERR_NEEDS_RANKS = 7   /* range build only: the slice holds repeats too long for text-symbol
                                 refinement; build the whole suffix array instead (suffix_amd/dist.py does) */
};

const char* sfx_strerror(int status);
int sfx_device_count(void);
/* text of the last HIP error seen by this thread ("" if none) */
const char* sfx_last_hip_error(void);
/* Process-wide switches (additive; the defaults are what every number in DESIGN.md is quoted with; the library reads no
 * environment).  SFX_OPT_TINY_MAX: texts of up to this many bytes are built by ONE workgroup in ONE launch (sfx_tiny.hip:
 * alphabet, LSD radix sort of the suffixes' first key bits and the ordering of tied suffixes all inside one CU's LDS) --
 * default and largest value 16384, 0 = never (the tests use it to run small inputs through the general build as well).
 * sfx_set_option returns SFX_ERR_ARG for an unknown option or a value out of range. */
#define SFX_OPT_TINY_MAX 1
int      sfx_set_option(int option, uint64_t value);
uint64_t sfx_get_option(int option);

/* ---- SuffixTable::new -> sais_table (:378-386): suffix array, u32 indices ---- */
/* Host buffers.  Replaces the body of sais_table after `vec![0u32; n]` (:381-385).
 * n == 0 and n == 1 succeed (:395-402).  sa_out[r] = start of the r-th smallest
 * byte suffix, "shorter prefix sorts first" (naive_table :367-376). */
int sfx_build_sa_u32(const uint8_t* text, uint64_t n, uint32_t* sa_out);
/* Device-resident variant: d_text (n bytes) -> d_sa (n u32), all in HBM. */
uint64_t sfx_sa_workspace_bytes(uint64_t n);
int sfx_build_sa_u32_dev(const uint8_t* d_text, uint64_t n, uint32_t* d_sa,
                         void* d_workspace, uint64_t workspace_bytes, void* stream);

/* u64 index array (BASELINE config 4: "u64 indices").  SuffixTable itself is u32-only
 * (`Cow<[u32]>` :57, assert :380), so positions fit 32 bits: the u32 engine runs and the
 * array is widened on the device.  n > u32::MAX is SFX_ERR_TOO_LARGE as on the u32 entry. */
int sfx_build_sa_u64(const uint8_t* text, uint64_t n, uint64_t* sa_out);
int sfx_widen_u32_to_u64_dev(const uint32_t* d_in, uint64_t count, uint64_t* d_out, void* stream);

/* The host-pointer entry points keep a few released device buffers (at most 8) in a mutex-guarded pool
 * so that repeated calls on similar sizes skip hipMalloc/hipFree -- a loop at one size allocates once; this
 * returns them, and with them the CALLING thread's query scratch (sfx_index_query_dev), after waiting for the
 * last batch that used it.  What else a thread holds between calls -- one non-blocking stream per device and one
 * pinned page of 4608 bytes for the small read-backs -- stays until the thread ends: everything a thread holds is
 * given back when it returns (not at process exit: the library never calls into HIP from exit()). */
void sfx_release_cached_buffers(void);

/* What the library holds at this moment, process-wide: every device allocation, pinned page, stream and event it
 * makes is counted where it is made and where it is given back.  Pure host code: works without a device.
 * device_* / pinned_*: live allocations and their requested sizes (the pool's idle buffers included, reported
 * again as pooled_*); device_allocs_total only grows: a *_dev call over a caller workspace leaves it unchanged.
 * The counters are read one by one, not as a snapshot: read them while no other thread is inside the library. */
typedef struct {
    uint64_t device_bytes, device_allocs;
    uint64_t pinned_bytes, pinned_allocs;
    uint64_t streams, events;
    uint64_t pooled_bytes, pooled_buffers;   /* the idle part of the pool */
    uint64_t device_allocs_total;            /* device allocations ever made */
    uint64_t reserved[7];                    /* zero */
} sfx_resource_stats_t;
int sfx_resource_stats(sfx_resource_stats_t* out);

/* ---- lcp_lens (:130-138 -> lcp_lens_quadratic :348-361): LCP array ---------- */
/* lcp_out[0] = 0, lcp_out[r] = |lcp(text[sa[r-1]..], text[sa[r]..])| in bytes.
 * The array is the same whichever route computes it: from 1 MiB of text up a sample of
 * adjacent pairs picks the reference's direct comparison (one window gather per suffix, capped;
 * the right choice for low-LCP text) or the linear Phi/PLCP form; a pair that reaches the cap
 * of the direct route sends the whole array through Phi/PLCP, so the cost stays linear in n.
 * The _dev entry synchronises the stream once or twice to read that choice back. */
int sfx_build_lcp_u32(const uint8_t* text, uint64_t n, const uint32_t* sa, uint32_t* lcp_out);
uint64_t sfx_lcp_workspace_bytes(uint64_t n);
int sfx_build_lcp_u32_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa,
                          uint32_t* d_lcp, void* d_workspace, uint64_t workspace_bytes,
                          void* stream);

/* ---- SuffixTable::new + lcp_lens in one call (:78-85 + :130-138; the pair suffix_tree/src/lib.rs:71,
 * :413 makes) -------------------------------------------------------------------
 * The same two arrays as sfx_build_sa_u32 followed by sfx_build_lcp_u32.  Where the initial key sort
 * already tells two neighbours apart (98 % of the pairs of uniform DNA) their LCP is read off the sorted
 * keys inside the build; only the remaining pairs are compared on the text. */
int sfx_build_sa_lcp_u32(const uint8_t* text, uint64_t n, uint32_t* sa_out, uint32_t* lcp_out);
uint64_t sfx_sa_lcp_workspace_bytes(uint64_t n);
int sfx_build_sa_lcp_u32_dev(const uint8_t* d_text, uint64_t n, uint32_t* d_sa, uint32_t* d_lcp,
                             void* d_workspace, uint64_t workspace_bytes, void* stream);

/* ---- positions / contains / any_position (:223-293), batched ---------------- */
/* Device-resident index = text + suffix array kept in HBM across calls. */
typedef struct sfx_index sfx_index;
/* sa == NULL => build it on the device.  Host pointers.  A caller-supplied table is checked for
 * entries >= n (SFX_ERR_ARG; the reference's from_parts is unchecked and "fails in weird ways", :105-107 --
 * a memory-safe panic there, so the engine must not read out of bounds either).  The index also holds a
 * BUCKET DIRECTORY: for every prefix of dbits bits of dense symbol codes (dbits = log2 n - 2, at most 28:
 * about one bucket per four suffixes, n bytes of HBM) the first rank whose suffix is not smaller -- a query
 * looks its own first dbits bits up and searches only inside that bucket -- and, memory permitting (17 n
 * bytes), a static 16-ary B+TREE over the first 16 bytes of every suffix in table order: a query of <= 16
 * bytes is answered from its nodes alone, a longer one bisects the ranks that share its first 16 bytes.
 * Batches of >= 4096 queries keep a per-thread scratch list (256 + 12 bytes per query of the thread's largest batch,
 * and one event) between calls: sfx_index_query_dev makes or grows it on the calling thread, and it is given back when
 * that thread ends or calls sfx_release_cached_buffers() -- the next large batch then allocates it again. */
int sfx_index_create(const uint8_t* text, uint64_t n, const uint32_t* sa, sfx_index** out);
/* the same over text and suffix array that already live in HBM (borrowed, not copied: keep them alive and
 * unchanged while the index exists); only the directory and the tree are built.  Queries with device buffers: */
int sfx_index_create_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, void* stream, sfx_index** out);
int sfx_index_query_dev(const sfx_index* ix, const uint8_t* d_qbytes, const uint64_t* d_qoff, uint64_t nq,
                        uint32_t* d_start, uint32_t* d_end, uint8_t* d_found, uint32_t* d_any, void* stream);
void sfx_index_destroy(sfx_index* ix);
uint64_t sfx_index_len(const sfx_index* ix);
/* copy the index's suffix array back to the host (n u32) */
int sfx_index_table(const sfx_index* ix, uint32_t* sa_out);
/* Queries are concatenated in `qbytes`; query k is qbytes[qoff[k] .. qoff[k+1]).
 * positions(q) == table[start_out[k] .. end_out[k]) exactly as :244-258; an empty
 * result is reported as start == end == 0.  found_out[k] = contains(q) (:197-199);
 * any_out[k] = any_position(q) or UINT32_MAX for None (:279-293; which occurrence
 * is "arbitrary" by contract, :261-262).  Output arrays may be NULL to skip. */
int sfx_positions_batch(const sfx_index* ix, const uint8_t* qbytes, const uint64_t* qoff,
                        uint64_t nq, uint32_t* start_out, uint32_t* end_out);
int sfx_contains_batch(const sfx_index* ix, const uint8_t* qbytes, const uint64_t* qoff,
                       uint64_t nq, uint8_t* found_out, uint32_t* any_out);
/* all-device variant of the above (d_qbytes, d_qoff, outputs in HBM) */
int sfx_query_batch_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa,
                        const uint8_t* d_qbytes, const uint64_t* d_qoff, uint64_t nq,
                        uint32_t* d_start, uint32_t* d_end, uint8_t* d_found,
                        uint32_t* d_any, void* stream);

/* ---- suffix-tree topology from SA + LCP (suffix_tree/src/lib.rs:392-505 `to_suffix_tree`), flat ------
 * The internal nodes of the suffix tree are the lcp-intervals of the LCP array; the reference finds them
 * with a serial stack sweep, the engine with nearest-smaller-value searches over a min-pyramid.  For every
 * BOUNDARY p in [0, n) (between ranks p - 1 and p; value lcp[p]) the call writes
 *   lb[p], rb[p]   the rank range of the node the boundary belongs to (its string depth is lcp[p]);
 *   node[p]        that node's id = its leftmost boundary with that depth (0 = the root: [0, n-1], depth 0,
 *                  to which every boundary with lcp[p] == 0 belongs);
 *   parent[p]      the id of that node's parent (UINT32_MAX for every boundary of the root: p = 0 and every p with
 *                  lcp[p] == 0 -- the root is nobody's child, its own included);
 * and for every RANK r:  leaf_parent[r] = id of the node the leaf of suffix sa[r] hangs under.
 * Node k's edge label is text[sa[lb[k]] + depth(parent) .. sa[lb[k]] + depth(k)); children are the nodes /
 * leaves whose parent is k -- the same tree as `to_suffix_tree`, as arrays.  All device pointers, n u32 each.
 * Boundary 0 (in front of the first suffix) has depth 0 by definition: d_lcp[0] is not looked at. */
uint64_t sfx_lcp_intervals_workspace_bytes(uint64_t n);
int sfx_lcp_intervals_dev(const uint32_t* d_lcp, uint64_t n, uint32_t* d_lb, uint32_t* d_rb, uint32_t* d_node,
                          uint32_t* d_parent, uint32_t* d_leaf_parent, void* d_workspace, uint64_t workspace_bytes,
                          void* stream);
/* ---- suffix-tree node table with ordered children (suffix_tree/src/lib.rs:107-160, the `Node` interface) ------
 * The same tree looking DOWN, for a plain table (sa, lcp of a text of n bytes; lcp[0] is not looked at).
 *   Internal nodes  the lcp-intervals, the root [0, n-1] at depth 0 among them: m of them, with dense ids 0 .. m-1 in
 *                   ascending order of their sfx_lcp_intervals_dev id (the order the reference's sweep creates them in;
 *                   not preorder).  The root is node 0.
 *   Terminals       the leaf of rank r under node v has the edge label text[sa[r] + depth(v) ..].  Where that is empty
 *                   (n - sa[r] == depth(v)) the reference makes no child: the suffix is a TERMINAL of v itself
 *                   (lib.rs:127-131).  A node has at most one, the suffix at its first rank; the root has none.
 *                   T = the number of nodes that have one.
 *   Children        of v, in rank order: its child intervals and the ranks directly under it whose label is not empty.
 *                   Rank order is the order of the first bytes of their edge labels (distinct inside a node: at most 256
 *                   children), the reference's BTreeMap<u8, _> order.  C = n - 1 + m - T children in all, C <= 2n - 1.
 * Arrays (device pointers; NONE = UINT32_MAX):
 *   node_lb, node_rb   m u32        rank range of node k
 *   node_depth         m u32        its string depth (the reference's path_len)
 *   node_parent        m u32        dense id of its parent, NONE for the root
 *   node_terminal      m u32        text position of its terminal suffix, NONE if it has none
 *   child_off          m + 1 u64    the children of node k are entries child_off[k] .. child_off[k + 1]; child_off[m] == C
 *   child_lb           C u32        first rank of the child, strictly ascending inside a node; the child ends where the
 *                                   next one begins, or at node_rb
 *   child_node         C u32        dense id of the child if it is an internal node, NONE if it is the leaf of rank child_lb
 *   child_byte         C u8         first byte of the child's edge label (any address); d_text and d_child_byte are both
 *                                   given or both NULL
 *   leaf_parent        n u32        dense id of the node the leaf of rank r is a child or the terminal of; may be NULL
 * Every array is determined by (text, sa, lcp) alone: two calls give the same bytes.
 * *nodes_out = m and *children_out = C (HOST pointers) are written on every SFX_OK.  If m > node_capacity or
 * C > child_capacity no array is written and the call still returns SFX_OK: the caller compares and calls again with
 * more room (capacities of 0 with NULL arrays is the sizing call; node_capacity = n and child_capacity = 2n always
 * suffice).  The call SYNCHRONISES the stream once, to read m, C and the table check back, as sfx_repeat_lens_dev does;
 * everything is queued on the caller's stream, and the workspace may hold anything on entry.
 * n == 0 succeeds with m = C = 0; n == 1 is the root with one leaf child.
 * SFX_ERR_ARG: a table entry >= n (checked on the device), exactly one of d_text / d_child_byte NULL, a NULL among the
 * other arrays (leaf_parent excepted) when the capacities suffice; SFX_ERR_TOO_LARGE: n > u32::MAX.
 * For ANY lcp contents and any table with entries < n nothing is read or written out of bounds; what the arrays hold
 * for an lcp array that is not the table's is unspecified.
 * Suffix links of the internal nodes: sfx_suffix_links_dev below (over an sfx_lce handle).
 * Not covered: generalized tables (truncated suffixes give a node several terminals), preorder numbers. */
uint64_t sfx_suffix_tree_workspace_bytes(uint64_t n);
int sfx_suffix_tree_dev(const uint8_t* d_text /* may be NULL */, const uint32_t* d_sa, const uint32_t* d_lcp, uint64_t n,
                        uint64_t node_capacity, uint64_t child_capacity,
                        uint32_t* d_node_lb, uint32_t* d_node_rb, uint32_t* d_node_depth, uint32_t* d_node_parent,
                        uint32_t* d_node_terminal, uint64_t* d_child_off /* node_capacity + 1 */,
                        uint32_t* d_child_lb, uint32_t* d_child_node, uint8_t* d_child_byte /* may be NULL */,
                        uint32_t* d_leaf_parent /* may be NULL */,
                        uint64_t* nodes_out /* host */, uint64_t* children_out /* host */,
                        void* d_workspace, uint64_t workspace_bytes, void* stream);
/* the same with host buffers, staged through HBM */
int sfx_suffix_tree_u32(const uint8_t* text /* may be NULL */, const uint32_t* sa, const uint32_t* lcp, uint64_t n,
                        uint64_t node_capacity, uint64_t child_capacity,
                        uint32_t* node_lb, uint32_t* node_rb, uint32_t* node_depth, uint32_t* node_parent,
                        uint32_t* node_terminal, uint64_t* child_off, uint32_t* child_lb, uint32_t* child_node,
                        uint8_t* child_byte /* may be NULL */, uint32_t* leaf_parent /* may be NULL */,
                        uint64_t* nodes_out, uint64_t* children_out);
/* ---- generalized suffix array (README.md:60-74): documents concatenated with a separator byte into one
 * text, one SuffixTable over it; a match position is mapped back to (document, offset) by a binary search
 * over the sorted document start offsets.  doc / offset may be NULL to skip. */
int sfx_doc_lookup_dev(const uint32_t* d_positions, uint64_t count, const uint64_t* d_doc_starts, uint64_t ndocs,
                       uint32_t* d_doc, uint32_t* d_offset, void* stream);

/* ---- generalized suffix array over a document collection (README.md:60-74, without the separator) ------
 * Documents D_0 .. D_{m-1} (any bytes, NUL and 0xFF included; empty ones allowed) are given as ONE buffer of
 * n = sum |D_i| bytes plus doc_starts[0..ndocs) (non-decreasing, doc_starts[0] == 0, none past n; document i =
 * text[doc_starts[i] .. doc_starts[i + 1]), the last one ending at n).  No separator byte is involved.
 *   sa_out   all n positions doc_starts[i] + o, ordered by the TRUNCATED suffix D_i[o..] (bytes, a proper prefix
 *            first), equal truncated suffixes by document index -- the suffix array of D_0 $_0 D_1 $_1 ... with
 *            distinct terminators $_0 < $_1 < ... < every byte, terminator suffixes left out;
 *   da_out   da_out[r] = the document of sa_out[r];
 *   lcp_out  lcp_out[0] = 0, lcp_out[r] = common prefix of the truncated suffixes at ranks r - 1 and r (never past
 *            either one's document end).
 * With one document, sa_out / lcp_out are exactly sfx_build_sa_u32 / sfx_build_lcp_u32 of it.  da / lcp may be NULL.
 * SFX_ERR_ARG: ndocs == 0 with n > 0, or doc_starts not as above (checked on the device, read back once);
 * SFX_ERR_TOO_LARGE: n > u32::MAX.  n == 0 succeeds. */
uint64_t sfx_gsa_workspace_bytes(uint64_t n, uint64_t ndocs);
int sfx_build_gsa_u32_dev(const uint8_t* d_text, uint64_t n, const uint64_t* d_doc_starts, uint64_t ndocs,
                          uint32_t* d_sa, uint32_t* d_da, uint32_t* d_lcp,
                          void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_build_gsa_u32(const uint8_t* text, uint64_t n, const uint64_t* doc_starts, uint64_t ndocs,
                      uint32_t* sa_out, uint32_t* da_out, uint32_t* lcp_out);
/* ---- merge of two generalized suffix arrays: add documents without a rebuild ------
 * A = the first ndocs_a documents (n_a bytes), B = the documents behind them (n_b bytes).  sa_a / da_a / lcp_a and
 * sa_b / da_b / lcp_b are exactly what sfx_build_gsa_u32 returns for A alone and for B alone, so B's positions and
 * document numbers are relative to B.  text[0 .. n_a + n_b) and doc_starts[0 .. ndocs) describe the whole collection;
 * doc_starts[ndocs_a] == n_a (ndocs_a == ndocs: B is empty; ndocs_a == 0: A is).  Equal truncated suffixes are ordered
 * by position, so an added document never moves an old suffix relative to another and sorts behind every old suffix
 * equal to it: the arrays of the whole collection are the STABLE MERGE of the two sets, the old entry first on equal
 * strings.  For the new suffix x_j at B-rank j, p[j] = the number of old truncated suffixes <= x_j (an equal one
 * counts), left[j] / right[j] = its common prefix with the old suffix at rank p[j] - 1 / p[j], never past a document
 * end, 0 where there is no such rank.  x_j goes to slot p[j] + j and writes sa_b[j] + n_a, da_b[j] + ndocs_a and the
 * lcp lcp_b[j] when the slot in front holds a new suffix too, else left[j]; old rank r goes to slot
 * r + #{j : p[j] <= r} and writes sa_a[r], da_a[r] and right[j] of the new suffix in the slot in front, lcp_a[r] when
 * that slot is old.  Cost: one bisection over the old table per NEW suffix (O(log n_a + match length) compared bytes)
 * and one streaming pass; no sort.
 *   match_limit   adding a near-copy of a long document compares a number of bytes quadratic in its length.  0: no
 *                 limit.  Otherwise a comparison stops once a common prefix exceeds match_limit.
 *   *longest_out  the largest left / right, capped at match_limit + 1 when a comparison stopped.  *longest_out >
 *                 match_limit (match_limit > 0): SFX_OK, NOTHING is written to d_sa / d_da / d_lcp -- the refusal is
 *                 recognised by that inequality, as sfx_mems_dev's pair_limit is; build the whole collection instead.
 *   d_da_a / d_da_b may be NULL (the documents are then found from doc_starts); d_da / d_lcp may be NULL to skip them,
 *   and d_lcp_a / d_lcp_b are read only when d_lcp is given.
 * SFX_ERR_ARG, found on the device and read back before anything indexes by it: doc_starts not as sfx_build_gsa_u32
 * wants it or with doc_starts[ndocs_a] != n_a, an sa_a entry >= n_a, an sa_b entry >= n_b, a da_a entry >= ndocs_a, a
 * da_b entry >= ndocs - ndocs_a; after the rank search: p not non-decreasing (sa_b is no GSA of B).  Arrays that pass
 * these checks without being GSAs give some answer; nothing is read or written out of bounds.  SFX_ERR_ARG on the host:
 * ndocs_a > ndocs, bytes without documents on either side, a NULL among the needed arrays, longest_out NULL, an output
 * that overlaps an input or the workspace, a pointer off its alignment.  n_a + n_b > u32::MAX: SFX_ERR_TOO_LARGE.
 * n_a + n_b == 0: SFX_OK.  n_b == 0 or n_a == 0 copies the other side (offset as above).
 * sfx_gsa_merge_workspace_bytes(n_a, n_b) <= 12 n_b + 34 KiB (p, left, right; one word per wave of the rank search); a
 * shorter one is SFX_ERR_WORKSPACE.  The device entry borrows everything, keeps nothing, allocates nothing, and may run
 * from several threads and streams at once.  It synchronises `stream` twice (the check, the rank search) and returns with
 * its last kernel queued.
 * sfx_gsa_merge_u32: the same over host pointers.  sfx_gsa_extend_u32: the whole collection's text and doc_starts plus
 * A's arrays; builds B = documents ndocs_a .. with sfx_build_gsa_u32_dev and merges.  *route_out says what produced the
 * outputs: SFX_GSA_ROUTE_MERGE, SFX_GSA_ROUTE_REBUILD (refused and rebuild_on_limit != 0: one build of the whole
 * collection) or SFX_GSA_ROUTE_NONE (refused, rebuild_on_limit == 0: nothing written). */
enum { SFX_GSA_ROUTE_NONE = 0, SFX_GSA_ROUTE_MERGE = 1, SFX_GSA_ROUTE_REBUILD = 2 };
uint64_t sfx_gsa_merge_workspace_bytes(uint64_t n_a, uint64_t n_b);
int sfx_gsa_merge_dev(const uint8_t* d_text, const uint64_t* d_doc_starts, uint64_t ndocs, uint64_t ndocs_a,
                      const uint32_t* d_sa_a, const uint32_t* d_da_a /* may be NULL */, const uint32_t* d_lcp_a, uint64_t n_a,
                      const uint32_t* d_sa_b, const uint32_t* d_da_b /* may be NULL */, const uint32_t* d_lcp_b, uint64_t n_b,
                      uint32_t match_limit, uint32_t* d_sa, uint32_t* d_da, uint32_t* d_lcp, uint64_t* longest_out,
                      void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_gsa_merge_u32(const uint8_t* text, const uint64_t* doc_starts, uint64_t ndocs, uint64_t ndocs_a,
                      const uint32_t* sa_a, const uint32_t* da_a /* may be NULL */, const uint32_t* lcp_a, uint64_t n_a,
                      const uint32_t* sa_b, const uint32_t* da_b /* may be NULL */, const uint32_t* lcp_b, uint64_t n_b,
                      uint32_t match_limit, uint32_t* sa_out, uint32_t* da_out, uint32_t* lcp_out, uint64_t* longest_out);
int sfx_gsa_extend_u32(const uint8_t* text, uint64_t n, const uint64_t* doc_starts, uint64_t ndocs, uint64_t ndocs_a,
                       const uint32_t* sa_a, const uint32_t* da_a /* may be NULL */, const uint32_t* lcp_a,
                       uint32_t match_limit, int rebuild_on_limit, uint32_t* sa_out, uint32_t* da_out, uint32_t* lcp_out,
                       uint64_t* longest_out, uint32_t* route_out);
/* Resident generalized index over (text, doc_starts, GSA, DA).  q matches at (i, o) iff |q| <= |D_i| - o and
 * D_i[o .. o + |q|) == q: matches never span documents and form one GSA interval.  Per query: start / end (0 / 0
 * when empty; the empty query is empty), found, any (a position, UINT32_MAX for none) and ndocs = the number of
 * DISTINCT documents containing q.  Outputs may be NULL to skip.  The _dev create borrows its four arrays (keep them
 * alive and unchanged); it checks doc_starts and every (table, DA) entry (SFX_ERR_ARG) and builds the previous-rank-
 * of-the-same-document array (4 n bytes).  sfx_gindex_create copies host arrays. */
typedef struct sfx_gindex sfx_gindex;
int  sfx_gindex_create_dev(const uint8_t* d_text, uint64_t n, const uint64_t* d_doc_starts, uint64_t ndocs,
                           const uint32_t* d_sa, const uint32_t* d_da, void* stream, sfx_gindex** out);
int  sfx_gindex_create(const uint8_t* text, uint64_t n, const uint64_t* doc_starts, uint64_t ndocs,
                       const uint32_t* sa, const uint32_t* da, sfx_gindex** out);
int  sfx_gindex_query_dev(const sfx_gindex* gx, const uint8_t* d_qbytes, const uint64_t* d_qoff, uint64_t nq,
                          uint32_t* d_start, uint32_t* d_end, uint8_t* d_found, uint32_t* d_any,
                          uint32_t* d_ndocs, void* stream);
/* the same with host buffers (queries concatenated as for sfx_positions_batch) */
int  sfx_gindex_query(const sfx_gindex* gx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t nq,
                      uint32_t* start_out, uint32_t* end_out, uint8_t* found_out, uint32_t* any_out,
                      uint32_t* ndocs_out);
void sfx_gindex_destroy(sfx_gindex* gx);

/* ---- what is repeated: repeat lengths and repeated spans from SA + LCP (no text access) -----------------
 * S_p = the suffix at text position p: to the end of the text for a plain table, to the end of p's document for a
 * collection (the truncated suffix of sfx_build_gsa_u32, whose sa / lcp / da are what is passed here).
 *   rep[p]  the longest common prefix of S_p with any S_q the scope allows, 0 if it allows none:
 *             SFX_REP_ANY        q != p                          = max(lcp[r], lcp[r + 1]), r = the rank of p
 *             SFX_REP_EARLIER    q < p as text positions         the longest-previous-factor (LPF) array
 *             SFX_REP_OTHER_DOC  q in another document (needs d_da; one document: all zeros)
 *           lcp[0] counts as 0 whatever it holds (as for sfx_lcp_intervals_dev), and so does lcp[n].
 *   src[p]  (d_src may be NULL) a position q that attains rep[p]: allowed by the scope, S_p and S_q share rep[p] bytes;
 *           UINT32_MAX where rep[p] == 0.  WHICH witness is arbitrary by contract, as for any_position.
 * All device pointers, n u32 each.  SFX_ERR_ARG: an unknown scope, OTHER_DOC without d_da, or a table entry >= n
 * (checked on the device, read back once; nothing is written out of bounds even for a table that is no permutation).
 * The call synchronises the stream for that read-back.  n == 0 succeeds. */
enum { SFX_REP_ANY = 0, SFX_REP_EARLIER = 1, SFX_REP_OTHER_DOC = 2 };
uint64_t sfx_repeat_lens_workspace_bytes(uint64_t n, int scope);
int sfx_repeat_lens_dev(const uint32_t* d_sa, const uint32_t* d_lcp, const uint32_t* d_da /* OTHER_DOC only, else NULL */,
                        uint64_t n, int scope, uint32_t* d_rep, uint32_t* d_src /* may be NULL */,
                        void* d_workspace, uint64_t workspace_bytes, void* stream);
/* Spans: byte i is COVERED iff some p <= i < p + rep[p] has rep[p] >= min_len (min_len >= 1).  The report lists the
 * maximal runs of covered bytes as [begin[k], end[k]) in ascending order; with d_doc_starts (as for sfx_build_gsa_u32)
 * a run also ends at every document start.  Every run is at least min_len long: n / min_len + 1 entries always suffice.
 * *count_out (a HOST pointer) = the total number of spans; only the first `capacity` are written and nothing past them --
 * a caller that sees count > capacity calls again with more room.  Keeping the first copy of every span of >= L bytes
 * is EARLIER at min_len = L.  SFX_ERR_ARG: min_len == 0, doc_starts not as sfx_build_gsa_u32 wants them. */
uint64_t sfx_repeat_spans_workspace_bytes(uint64_t n);
int sfx_repeat_spans_dev(const uint32_t* d_rep, uint64_t n, uint32_t min_len,
                         const uint64_t* d_doc_starts /* may be NULL */, uint64_t ndocs,
                         uint32_t* d_begin, uint32_t* d_end, uint64_t capacity, uint64_t* count_out /* host */,
                         void* d_workspace, uint64_t workspace_bytes, void* stream);
/* the same with host buffers, staged through HBM */
int sfx_repeat_lens_u32(const uint32_t* sa, const uint32_t* lcp, const uint32_t* da, uint64_t n, int scope,
                        uint32_t* rep_out, uint32_t* src_out);
int sfx_repeat_spans_u32(const uint32_t* rep, uint64_t n, uint32_t min_len, const uint64_t* doc_starts, uint64_t ndocs,
                         uint32_t* begin_out, uint32_t* end_out, uint64_t capacity, uint64_t* count_out);

/* ---- matching statistics: which parts of a NEW text Q already stand in the indexed text T ----------------
 * T = the indexed text of n bytes with suffix array sa; Q = a query text of m bytes; max_len = the caller's cap on a
 * match, 0 = none.  For every i in [0, m), with lim = m - i (max_len == 0) or min(max_len, m - i):
 *   len[i]            the largest l <= lim such that Q[i .. i + l) occurs in T;
 *   start[i], end[i]  the rank range of the suffixes that begin with Q[i .. i + len[i]) -- what positions() of that
 *                     pattern returns; 0 / 0 where len[i] == 0 (the empty query is empty);
 *   src[i]            one text position where those len[i] bytes stand, UINT32_MAX where len[i] == 0.  WHICH
 *                     occurrence is arbitrary by contract, as for any_position.
 * For a collection (sfx_gindex) an occurrence lies inside ONE document (the truncated suffixes of sfx_build_gsa_u32);
 * ranks are GSA ranks.  len, start and end are determined by (T, sa, Q, max_len) alone: two calls, two entry points or
 * two streams give the same bytes; a capped len is min(uncapped len, max_len).  The arrays are rep-shaped:
 * sfx_repeat_spans_dev(len, m, L, ...) lists the spans of Q that occur in T with at least L bytes, and for that report
 * max_len = L is enough (the covered bytes are the same for every cap >= L).
 * Arguments: d_len is required; d_src may be NULL; d_start and d_end are both given or both NULL (exactly one NULL is
 * SFX_ERR_ARG).  m == 0 is SFX_OK and writes nothing.  n == 0 gives len = 0, src = UINT32_MAX and 0 / 0 everywhere.
 * m > u32::MAX (or n > u32::MAX) is SFX_ERR_TOO_LARGE, whatever the pointers are.  d_query may have any alignment;
 * the u32 arrays need 4 bytes.
 * The _dev calls queue everything on the caller's stream, allocate nothing, keep no state in the index, read nothing
 * back and DO NOT SYNCHRONISE: any number of threads may call on one index at once.  Nothing is read outside
 * [d_query, d_query + m), [d_text, d_text + n) and d_sa[0 .. n) (for a collection also its doc_starts and DA); nothing
 * is written outside the m entries of each output.
 * sfx_match_stats_dev takes text and table as they are, like sfx_query_batch_dev: a table entry >= n reaches the
 * kernel unchecked and is read out of bounds (the reference's from_parts "fails in weird ways", :105-107) -- hand it
 * a table the engine built, or go through an index: the two index entries rely on the check made at index creation.
 * Cost: one bisection per position, O(log n + len[i]) compared bytes (each probe starts at the bytes its two bounds
 * already share), plus O(len[i] log(end - start)) for the interval.  An UNCAPPED call with Q = T is therefore quadratic
 * on a repetitive text: max_len is the caller's bound. */
int sfx_match_stats_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa,
                        const uint8_t* d_query, uint64_t m, uint32_t max_len,
                        uint32_t* d_len, uint32_t* d_src /* may be NULL */, uint32_t* d_start, uint32_t* d_end /* both or neither */,
                        void* stream);
int sfx_index_match_stats_dev(const sfx_index* ix, const uint8_t* d_query, uint64_t m, uint32_t max_len,
                              uint32_t* d_len, uint32_t* d_src, uint32_t* d_start, uint32_t* d_end, void* stream);
int sfx_gindex_match_stats_dev(const sfx_gindex* gx, const uint8_t* d_query, uint64_t m, uint32_t max_len,
                               uint32_t* d_len, uint32_t* d_src, uint32_t* d_start, uint32_t* d_end, void* stream);
/* the same with host buffers, staged through HBM (these synchronise their own stream) */
int sfx_index_match_stats(const sfx_index* ix, const uint8_t* query, uint64_t m, uint32_t max_len,
                          uint32_t* len_out, uint32_t* src_out, uint32_t* start_out, uint32_t* end_out);
int sfx_gindex_match_stats(const sfx_gindex* gx, const uint8_t* query, uint64_t m, uint32_t max_len,
                           uint32_t* len_out, uint32_t* src_out, uint32_t* start_out, uint32_t* end_out);

/* ---- Burrows-Wheeler transform with sampled ranks, and its inverse ------------------
 * T = a text of n bytes with suffix array sa.  The n + 1 sorted rotations of T$ ($ smaller than every byte) are the
 * ROWS: row 0 begins with $, row j (1 <= j <= n) with suffix sa[j-1].  Last column: L[0] = T[n-1];
 * L[j] = T[sa[j-1]-1] if sa[j-1] > 0, else $.
 *   primary       the row whose L is $ = 1 + the rank of suffix 0; 1 <= primary <= n
 *   bwt           n bytes: L without its $ entry; row R != primary sits at bwt[R < primary ? R : R - 1]
 *   sample_step   s = 0 or a power of two
 *   samples[k]    the row of the suffix that starts at text position k*s, k in [0, cnt), cnt = ceil(n / s);
 *                 samples[0] == primary always.  s == 0: the primary only (cnt = 1 for n > 0); n == 0: cnt = 0.
 * Inverse: lf[i] = 1 + C[bwt[i]] + #{j < i : bwt[j] == bwt[i]} with C[c] = the number of bytes of bwt below c.
 * Segment k = the text positions [k*s, min(n, (k+1)*s)) (s == 0: one segment, the whole text).  Its walk starts at row
 * samples[k+1] (row 0 for the last segment); each step writes bwt[i(R)] at the current position, going down, and sets
 * R = lf[i(R)]; it must end at row samples[k].  One lane walks one segment, so the samples are what makes the inverse
 * parallel: n / s chains of s dependent steps.
 *
 * sfx_bwt_sample_count: cnt above; 0 for a step that is neither 0 nor a power of two.
 * sfx_bwt_dev: no workspace, no read-back, no synchronisation: three launches on the caller's stream (the primary is
 *   found on the device).  d_text and d_bwt may have any alignment, d_sa and d_samples need 4 bytes; d_samples holds
 *   sfx_bwt_sample_count(n, sample_step) entries.  The table is taken as it is, like sfx_match_stats_dev's: for any
 *   table whose entries are all < n nothing is read or written out of bounds -- without a zero entry or with several
 *   too; what the outputs hold for a table that is no permutation is unspecified.  A step that is neither 0 nor a power
 *   of two is SFX_ERR_ARG, n > u32::MAX is SFX_ERR_TOO_LARGE, n == 0 is SFX_OK and writes nothing.
 * sfx_bwt_u32: the same with host buffers; sa == NULL builds the table first.
 * sfx_unbwt_dev: queues everything on the caller's stream and synchronises it ONCE, at the end, to read two device-side
 *   checks back: (a) every sample lies in [1, n]; (b) every segment's walk ended at row samples[k] (and met the primary
 *   row nowhere before).  (b) is a complete integrity check: lf is injective, the walks chain into n steps from row 0
 *   that end at the primary, so they visit every row once -- SFX_OK means that (d_bwt, d_samples) IS the transform of
 *   the text returned; anything else is SFX_ERR_ARG, and d_text_out then holds unspecified bytes.  Whatever the input
 *   bytes are, nothing is read or written out of bounds: rows stay in [0, n], indices in [0, n-1].
 *   SFX_ERR_ARG also, before anything is launched: a bad step; nsamples != sfx_bwt_sample_count(n, sample_step);
 *   d_text_out overlapping d_bwt; a chain -- min(n, s), n for s == 0 -- longer than SFX_UNBWT_MAX_CHAIN; a workspace off
 *   SFX_WORKSPACE_ALIGN.  A workspace below sfx_unbwt_workspace_bytes(n) is SFX_ERR_WORKSPACE, n > u32::MAX
 *   SFX_ERR_TOO_LARGE.  d_bwt and d_text_out may have any alignment.
 *   SFX_UNBWT_MAX_CHAIN is a contract, not a tuning knob: one lane walking 10^9 dependent misses would hold a shared
 *   GPU for minutes; 2^20 steps of one idle-latency HBM miss each (about 900 cycles) stay well under a few seconds.
 * sfx_unbwt: the same with host buffers.
 * Not covered: the transform of a collection (per-document terminators); inversion without samples at scale (list
 * ranking); the transform without a table.
 * (The LZ77 calls further down have a per-launch bound of their own, SFX_LZ_MAX_STEPS = 4096 dependent loads per lane.) */
#define SFX_UNBWT_MAX_CHAIN (1u << 20)
uint64_t sfx_bwt_sample_count(uint64_t n, uint32_t sample_step);
int sfx_bwt_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, uint32_t sample_step,
                uint8_t* d_bwt, uint32_t* d_samples, void* stream);
int sfx_bwt_u32(const uint8_t* text, uint64_t n, const uint32_t* sa /* NULL: build it */, uint32_t sample_step,
                uint8_t* bwt_out, uint32_t* samples_out);
uint64_t sfx_unbwt_workspace_bytes(uint64_t n);
int sfx_unbwt_dev(const uint8_t* d_bwt, uint64_t n, const uint32_t* d_samples, uint64_t nsamples, uint32_t sample_step,
                  uint8_t* d_text_out, void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_unbwt(const uint8_t* bwt, uint64_t n, const uint32_t* samples, uint64_t nsamples, uint32_t sample_step,
              uint8_t* text_out);

/* ---- FM-index: backward-search count and locate over the (bwt, samples) pair -----------
 * Rows, primary, bwt, samples and sample_step s as above.  The index answers positions() / contains() from the pair
 * alone -- neither the text nor the table -- in about 1.4-1.5 n bytes of HBM; a pattern of m bytes costs m steps
 * whatever n is.
 *   C[c]        the number of bytes of bwt below c
 *   i(R)        R <= primary ? R : R - 1 for a row R in [0, n + 1]: the bwt entries in front of row R, in [0, n]
 *   occ(c, R)   the number of c in bwt[0 .. i(R))
 *   count       a non-empty pattern P starts from the rows [0, n + 1); for c = P[m-1] down to P[0]:
 *               lo = 1 + C[c] + occ(c, lo), hi = 1 + C[c] + occ(c, hi); empty as soon as lo >= hi or c does not occur.
 *               (start, end) = (lo - 1, hi - 1) are table ranks: exactly the interval sfx_positions_batch reports.
 *               Every empty result is (0, 0): no match, the empty pattern, n == 0.
 *   lookup      the table entry of rank r: R = r + 1, steps = 0; while R is no sampled row: c = bwt[i(R)],
 *               R = 1 + C[c] + occ(c, R), steps++; at the row of sample k the answer is k * s + steps.  samples[0] =
 *               primary is always sampled, so the $ row is never dereferenced; a true transform needs at most s - 1
 *               steps (n - 1 for s == 0).
 * The structure (one device allocation the handle owns; the caller may free the pair after creation): the live bytes
 * get dense codes (sigma of them, sigma' = sigma rounded up to a multiple of 4); bwt is cut into blocks of occ_step = B
 * entries laid out as [sigma' u32: occurrences of every code before the block | B bytes], one counts-only block behind
 * the last; a bit per row marks the sampled rows, 480 rows and a running count per 64-byte line; one u32 per sample
 * gives, in row order, its number k.  occ_step is a power of two in [32, 4096]; 0 picks the smallest power of two
 * >= 16 sigma' within [64, 4096], which keeps the count words at or below n / 4 bytes.
 *
 * sfx_fm_bytes: an upper bound on the HBM a handle over such a pair holds, whatever its alphabet; 0 for n == 0 or
 *   arguments creation would refuse.
 * sfx_fm_create_dev: builds on the caller's stream and synchronises it (the alphabet is read back before the blocks
 *   can be sized, one flag word at the end).  d_bwt may have any alignment, d_samples needs 4 bytes.  SFX_ERR_ARG:
 *   a step that is neither 0 nor a power of two; nsamples != sfx_bwt_sample_count(n, sample_step); an occ_step that
 *   is neither 0 nor a power of two in [32, 4096]; a sample outside [1, n]; two equal samples.  n > u32::MAX is
 *   SFX_ERR_TOO_LARGE.  n == 0 gives a valid empty index.  Creation does NOT prove that the pair is a transform
 *   (sfx_unbwt is the complete check); what holds for every pair it accepts is that no later call reads or writes out
 *   of bounds: rows stay in [0, n], and a lookup walk is cut off after min(n, s) steps (n for s == 0).
 * sfx_fm_count_dev / sfx_fm_lookup_dev: one launch on the caller's stream, no workspace, no synchronisation.
 *   d_qbytes may have any alignment, d_qoff (nq + 1 offsets) needs 8 bytes, the u32 arrays 4.  d_ranks == NULL means the
 *   ranks first + j, j in [0, count): first = 0, count = n regenerates the whole suffix array.  A rank >= n, a walk
 *   that was cut off and a position that would lie outside the text (either only for a pair that is no transform) are
 *   written as UINT32_MAX.  sfx_fm_lookup* is SFX_ERR_ARG on an index whose chain -- min(n, s), n for s == 0 -- exceeds
 *   SFX_UNBWT_MAX_CHAIN; sfx_fm_count* works on such an index.
 * sfx_fm_create / sfx_fm_count / sfx_fm_lookup: the same with host buffers.
 * Not covered: collections (per-document terminators); 2-bit packing for DNA; building the index without first having
 * a table; bidirectional search; the multi-GPU partitioned path. */
typedef struct sfx_fm sfx_fm;
typedef struct { uint64_t n, bytes; uint32_t sigma, occ_step, sample_step, nsamples; } sfx_fm_info_t;
uint64_t sfx_fm_bytes(uint64_t n, uint32_t sample_step, uint32_t occ_step);
int sfx_fm_create_dev(const uint8_t* d_bwt, uint64_t n, const uint32_t* d_samples, uint64_t nsamples,
                      uint32_t sample_step, uint32_t occ_step, void* stream, sfx_fm** out);
int sfx_fm_create(const uint8_t* bwt, uint64_t n, const uint32_t* samples, uint64_t nsamples,
                  uint32_t sample_step, uint32_t occ_step, sfx_fm** out);
void sfx_fm_destroy(sfx_fm* fm);
int sfx_fm_info(const sfx_fm* fm, sfx_fm_info_t* info_out);
int sfx_fm_count_dev(const sfx_fm* fm, const uint8_t* d_qbytes, const uint64_t* d_qoff, uint64_t nq,
                     uint32_t* d_start, uint32_t* d_end, void* stream);
int sfx_fm_count(const sfx_fm* fm, const uint8_t* qbytes, const uint64_t* qoff, uint64_t nq,
                 uint32_t* start_out, uint32_t* end_out);
int sfx_fm_lookup_dev(const sfx_fm* fm, const uint32_t* d_ranks /* NULL: first + j */, uint64_t first, uint64_t count,
                      uint32_t* d_pos, void* stream);
int sfx_fm_lookup(const sfx_fm* fm, const uint32_t* ranks /* NULL: first + j */, uint64_t first, uint64_t count,
                  uint32_t* pos_out);

/* ---- LZ77 factorization from the longest-previous-factor array, and its decoder ----------
 * rep, src: n u32 values as sfx_repeat_lens_dev(..., SFX_REP_EARLIER, d_rep, d_src) writes them.  min_len >= 1.
 *   r(p)      min(rep[p], n - p)
 *   step(p)   r(p) if r(p) >= min_len, else 1;  next(p) = p + step(p)
 *   phrases   the chain b_0 = 0, b_(k+1) = next(b_k) while b_k < n; z is their number
 *   copy      phrase k with r(b_k) >= min_len: len = r, src = src[b_k], lit = 0
 *   literal   every other phrase: len = 1, src = UINT32_MAX, lit = text[b_k]
 * min_len = 1 is the classical self-referential LZ77 parse.  (begin, len) are unique; which src is reported is
 * arbitrary, as everywhere in this library.  With the rep / src of a generalized table (truncated suffixes) phrases
 * end at document ends by themselves.  next() is non-decreasing only for a true LPF array at min_len = 1; the
 * kernels do not rely on it.
 * Decoding z phrases (len, src, lit) into n bytes: begin = the exclusive sum of len; byte i of a literal is lit[k];
 * byte i of a copy equals byte src[k] + (i - begin[k]); src[k] < begin[k] is required and overlap with the phrase
 * itself is allowed ("a" * n is a literal and one copy of n - 1 bytes from position 0).
 *
 * sfx_lz_parse_dev: on the caller's stream, synchronised once at the end (z and two flags come back in one read).
 *   *count_out is the total z; only the first `capacity` phrases are written and nothing past them; n always
 *   suffices as capacity.  d_begin may be NULL; d_text == NULL writes no d_lit.  rep[p] is clipped to n - p before
 *   it is used and no src is used as an address, so unchecked arrays stay in bounds and every loop ends; an entry
 *   rep[p] > n - p anywhere, or a copy phrase with src >= begin, is SFX_ERR_ARG.  SFX_OK means the phrases tile [0, n)
 *   and every copy points backwards -- not that the copied bytes are equal (decode and compare for that).
 *   min_len == 0 is SFX_ERR_ARG, n > u32::MAX SFX_ERR_TOO_LARGE, n == 0 succeeds with z = 0, a workspace off
 *   SFX_WORKSPACE_ALIGN is SFX_ERR_ARG and a short one SFX_ERR_WORKSPACE.  Workspace <= 9 n + 64 KiB bytes.
 * sfx_lz_decode_dev: checks the whole list first (a zero len, a literal whose len is not 1, a copy with
 *   src >= begin, lengths that do not sum to n: SFX_ERR_ARG with d_text_out untouched), then writes the text; it
 *   synchronises for that check and once every few pointer-jumping rounds.  d_text_out overlapping an input is
 *   SFX_ERR_ARG.  Workspace <= 5 n + 8 z + 64 KiB bytes.
 * No lane of either call follows more than SFX_LZ_MAX_STEPS dependent global loads, for any input of n < 2^32:
 *   a tile is SFX_LZ_MAX_STEPS positions, a group 2^8 tiles, and a text has at most 2^12 groups of 2^20 positions.
 * sfx_lz77_u32 / sfx_unlz: the same with host buffers; sa / lcp == NULL are built.
 * Not covered: LZ-End, LZ78, non-overlapping variants, entropy coding, an LZ index, the multi-GPU path, n >= 2^32. */
#define SFX_LZ_MAX_STEPS (1u << 12)
uint64_t sfx_lz_parse_workspace_bytes(uint64_t n);
int sfx_lz_parse_dev(const uint32_t* d_rep, const uint32_t* d_src, const uint8_t* d_text /* NULL: no d_lit */,
                     uint64_t n, uint32_t min_len,
                     uint32_t* d_begin /* may be NULL */, uint32_t* d_len, uint32_t* d_psrc, uint8_t* d_lit,
                     uint64_t capacity, uint64_t* count_out /* host */,
                     void* d_workspace, uint64_t workspace_bytes, void* stream);
uint64_t sfx_lz_decode_workspace_bytes(uint64_t n, uint64_t z);
int sfx_lz_decode_dev(const uint32_t* d_len, const uint32_t* d_psrc, const uint8_t* d_lit, uint64_t z,
                      uint64_t n, uint8_t* d_text_out, void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_lz77_u32(const uint8_t* text, uint64_t n, const uint32_t* sa /* NULL: build */, const uint32_t* lcp /* NULL: build */,
                 uint32_t min_len, uint32_t* begin_out, uint32_t* len_out, uint32_t* src_out, uint8_t* lit_out,
                 uint64_t capacity, uint64_t* count_out);
int sfx_unlz(const uint32_t* len, const uint32_t* src, const uint8_t* lit, uint64_t z, uint64_t n, uint8_t* text_out);

/* ---- maximal exact matches of a query text against the table ------------------------------
 * T = the indexed text of n bytes with table sa, Q = a query text of m bytes, L = min_len >= 1.
 * A maximal exact match (MEM) is a triple (i, p, l) with l >= L and Q[i .. i+l) == T[p .. p+l) that can be extended
 * in neither direction:
 *   left    i == 0, or p == 0, or Q[i-1] != T[p-1]
 *   right   i + l == m, or p + l == n, or Q[i+l] != T[p+l]
 * For a collection (sfx_gindex) a match lies inside ONE document: the start of p's document plays the part of p == 0
 * and its end the part of n (the truncated-suffix model of sfx_build_gsa_u32); p is a text position
 * doc_starts[d] + offset.  With SFX_MEM_UNIQUE only those MEMs are kept whose l bytes occur exactly once in T (once
 * among all truncated suffixes of a collection).
 * Order: ascending by i, for equal i by the table rank of p -- the output is determined bit for bit by
 * (T, sa, Q, L, flags), and the unique list is the full list filtered, in the same order.
 * Two counts: P = the number of candidate pairs (i, r), r a rank whose suffix shares at least L bytes with Q[i..]
 * = the sum of end - start over the positions whose capped (max_len = L) matching statistic reaches L; Z = the number
 * of MEMs reported.  Work is proportional to P plus the bytes of the matches, not to Z: a shared stretch of M bytes
 * is M - L + 1 pairs and one MEM, and Q = T = a^n has about n^2 / 2 pairs.  The caller therefore gives a pair_limit,
 * the same duty as max_len on an uncapped sfx_match_stats_dev.  With P_k = P at min_len = k:
 *   Z(L) = P_L - P_(L+1)                     (a pair is not left-maximal iff the pair one byte earlier is an (L+1)-pair)
 *   the sum of (l - L + 1) over the MEMs = P_L   (every L-pair lies on exactly one MEM's diagonal)
 *
 * sfx_mems_dev / sfx_index_mems_dev / sfx_gindex_mems_dev: everything is queued on the caller's stream, which is
 *   synchronised ONCE, at the end, to read (P, Z) back.  The calls keep no state in the index and allocate nothing:
 *   any number of threads may call on one index at once, each with its own workspace.
 *   *pairs_out = P always.  P <= pair_limit: *count_out = Z, the first min(Z, capacity) triples are written and
 *   nothing past them; a caller that sees count > capacity calls again with more room.  P > pair_limit: SFX_OK,
 *   no triple is written and *count_out = 0 -- the refusal is recognised by *pairs_out > pair_limit.
 *   SFX_ERR_ARG: min_len == 0, pair_limit == 0, unknown flag bits, pairs_out / count_out NULL, an output array NULL
 *   while capacity > 0, a NULL input of a non-empty call, a workspace off SFX_WORKSPACE_ALIGN.  m or n > u32::MAX is
 *   SFX_ERR_TOO_LARGE, a workspace below sfx_mems_workspace_bytes(m, pair_limit) SFX_ERR_WORKSPACE.
 *   m == 0, n == 0 or L > min(m, n): SFX_OK with P = Z = 0.
 *   Workspace <= 24 m + pair_limit / 4 + 64 KiB bytes (a pair_limit above m * u32::MAX counts as that).
 *   d_text and d_query may have any alignment, the u32 arrays need 4 bytes.  Outside the caller's buffers nothing is
 *   written; outside Q, T, sa (da and doc_starts of a collection) and the workspace nothing is read.
 *   sfx_mems_dev takes text and table as they are, like sfx_match_stats_dev: for any table whose entries are all < n
 *   nothing is read or written out of bounds and every loop ends; what is reported for a table that is not the
 *   text's suffix array is unspecified.  The index entries rely on the check made when the index was created;
 *   sfx_index_mems_dev starts the search in the bucket directory, sfx_gindex_mems_dev uses the collection's search.
 * sfx_index_mems / sfx_gindex_mems: the same with host buffers, staged through HBM.
 * Not covered: matches unique in the query too (MUMmer's -mum), MEMs over the FM-index, chaining of seeds, the
 * multi-GPU path.  (Approximate matches of whole patterns: the k-mismatch search below.) */
enum { SFX_MEM_UNIQUE = 1 };
uint64_t sfx_mems_workspace_bytes(uint64_t m, uint64_t pair_limit);
int sfx_mems_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint8_t* d_query, uint64_t m,
                 uint32_t min_len, uint32_t flags, uint64_t pair_limit,
                 uint32_t* d_qpos, uint32_t* d_tpos, uint32_t* d_len, uint64_t capacity,
                 uint64_t* pairs_out /* host */, uint64_t* count_out /* host */,
                 void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_index_mems_dev(const sfx_index* ix, const uint8_t* d_query, uint64_t m,
                       uint32_t min_len, uint32_t flags, uint64_t pair_limit,
                       uint32_t* d_qpos, uint32_t* d_tpos, uint32_t* d_len, uint64_t capacity,
                       uint64_t* pairs_out /* host */, uint64_t* count_out /* host */,
                       void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_gindex_mems_dev(const sfx_gindex* gx, const uint8_t* d_query, uint64_t m,
                        uint32_t min_len, uint32_t flags, uint64_t pair_limit,
                        uint32_t* d_qpos, uint32_t* d_tpos, uint32_t* d_len, uint64_t capacity,
                        uint64_t* pairs_out /* host */, uint64_t* count_out /* host */,
                        void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_index_mems(const sfx_index* ix, const uint8_t* query, uint64_t m, uint32_t min_len, uint32_t flags,
                   uint64_t pair_limit, uint32_t* qpos_out, uint32_t* tpos_out, uint32_t* len_out, uint64_t capacity,
                   uint64_t* pairs_out, uint64_t* count_out);
int sfx_gindex_mems(const sfx_gindex* gx, const uint8_t* query, uint64_t m, uint32_t min_len, uint32_t flags,
                    uint64_t pair_limit, uint32_t* qpos_out, uint32_t* tpos_out, uint32_t* len_out, uint64_t capacity,
                    uint64_t* pairs_out, uint64_t* count_out);

/* ---- k-mismatch pattern search against the table -------------------------------------------
 * Where does a pattern occur if up to k bytes may differ (Hamming distance; no insertions or deletions)?
 * T = the indexed text of n bytes with table sa.  Patterns P_0 .. P_(nq-1) arrive as qbytes / qoff, exactly as for
 * sfx_index_query_dev; m_j = the length of pattern j, k = max_mismatches <= 255.
 *   occurrence   of pattern j: a position p with m_j >= 1 and p + m_j <= end(p) such that fewer than k + 1 indices
 *                i < m_j have P_j[i] != T[p+i].  end(p) = n for a plain index, the end of p's document for a
 *                collection (the truncated-suffix model): a window never leaves the document in which it starts.
 *                mism = the number of differing bytes, 0 <= mism <= k.  An empty pattern has no occurrence; a pattern
 *                with 0 < m_j <= k occurs at every window that has room.
 *   pieces       pattern j is cut at b_t = floor(t * m_j / (k + 1)), t = 0 .. k + 1; piece t = P_j[b_t .. b_(t+1)), empty
 *                now and then when m_j < k + 1.  By the pigeonhole principle every occurrence has a piece that matches
 *                exactly at p + b_t (an empty piece matches everywhere); the first such t is its OWNING piece -- a
 *                property of (T, P_j, k, p), not of the implementation.
 *   candidates   triples (j, t, r), r a rank in the exact interval of piece t (the interval of the collection's search
 *                for a collection; all of [0, n) for an empty piece of a non-empty pattern; none for an empty pattern),
 *                numbered ascending by j, then t, then r; C of them.  With q = sa[r] and p = q - b_t a candidate yields
 *                an occurrence iff q >= b_t, p is not before the start of q's document, p + m_j <= end(q), every earlier
 *                piece has at least one mismatch at p, and the whole window has at most k.  Every occurrence is thus
 *                produced by exactly one candidate, that of its owning piece.
 *   output       the triples (pattern, tpos, mism) of the surviving candidates, in candidate order: ascending by
 *                pattern, then by owning piece, then by the table rank of tpos + b_owner.  first[0 .. nq] (u64): the
 *                occurrences of pattern j are out[first[j] .. first[j+1]); first[nq] = Z even when Z exceeds
 *                `capacity` (first counts occurrences, not written triples).  The whole result is determined bit for
 *                bit by (T, sa, doc_starts, patterns, k).  At k = 0 the triples of pattern j are exactly
 *                sa[start_j .. end_j) of the exact search, in that order, with mism = 0.
 * Work is proportional to C plus the bytes compared (a window is abandoned at mismatch k + 1): short pieces of a
 * repetitive text have wide intervals, so the caller gives a cand_limit, the same duty as pair_limit above.
 *
 * sfx_hamming_dev / sfx_index_hamming_dev / sfx_gindex_hamming_dev: everything is queued on the caller's stream, which
 *   is synchronised ONCE, at the end, to read (C, Z) back.  The calls keep no state in the index and take their memory
 *   from the workspace (the piece search of sfx_index_hamming_dev is sfx_index_query_dev, whose large batches use that
 *   call's scratch, kept per calling thread): any number of threads may call on one index at once, each with its own
 *   workspace.
 *   *cands_out = C always.  C <= cand_limit: *count_out = Z, the first min(Z, capacity) triples are written and nothing
 *   past them, and first (when given) is complete whatever capacity is.  C > cand_limit: SFX_OK, nothing is written to
 *   the triple arrays or to first, and *count_out = 0 -- the refusal is recognised by *cands_out > cand_limit.
 *   SFX_ERR_ARG: cand_limit == 0, max_mismatches > 255, cands_out / count_out NULL, a triple array NULL while
 *   capacity > 0, a NULL input of a non-empty call, a qoff that is not monotone (found on the device, reported
 *   through the same single read-back), a workspace off SFX_WORKSPACE_ALIGN.  SFX_ERR_TOO_LARGE: n > u32::MAX, a
 *   pattern longer than u32::MAX (found on the device likewise), nq * (k + 1) >= 2^32.  A workspace below
 *   sfx_hamming_workspace_bytes(nq, max_mismatches, cand_limit) is SFX_ERR_WORKSPACE.
 *   nq == 0 or n == 0: SFX_OK with C = Z = 0, first all zero if given.
 *   Workspace <= 32 (nq (k + 1) + 1) + cand_limit / 4 + 64 KiB bytes (a cand_limit above nq (k + 1) * u32::MAX counts
 *   as that).
 *   d_text and d_qbytes may have any alignment, d_pattern / d_tpos need 4 bytes, d_qoff / d_first 8.  Outside the
 *   caller's buffers nothing is written; outside T, sa (da and doc_starts of a collection), the patterns and the
 *   workspace nothing is read; no load of the compare touches a byte outside the window [p, p + m_j).
 *   sfx_hamming_dev takes text and table as they are, like sfx_mems_dev: for any table whose entries are all < n
 *   nothing is read or written out of bounds and every loop ends; what is reported for a table that is not the
 *   text's suffix array is unspecified.  sfx_index_hamming_dev searches the pieces through the bucket directory and
 *   the key tree, sfx_gindex_hamming_dev with the collection's search.
 * sfx_index_hamming / sfx_gindex_hamming: the same with host buffers, staged through HBM.
 * Not covered: search over the FM-index, wildcards, per-pattern k, the multi-GPU path.  (Insertions and deletions:
 * the k-error search further down.) */
uint64_t sfx_hamming_workspace_bytes(uint64_t nq, uint32_t max_mismatches, uint64_t cand_limit);
int sfx_hamming_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa,
                    const uint8_t* d_qbytes, const uint64_t* d_qoff, uint64_t nq, uint32_t max_mismatches, uint64_t cand_limit,
                    uint32_t* d_pattern, uint32_t* d_tpos, uint8_t* d_mism, uint64_t capacity, uint64_t* d_first /* nq + 1, may be NULL */,
                    uint64_t* cands_out /* host */, uint64_t* count_out /* host */,
                    void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_index_hamming_dev(const sfx_index* ix,
                          const uint8_t* d_qbytes, const uint64_t* d_qoff, uint64_t nq, uint32_t max_mismatches, uint64_t cand_limit,
                          uint32_t* d_pattern, uint32_t* d_tpos, uint8_t* d_mism, uint64_t capacity, uint64_t* d_first,
                          uint64_t* cands_out /* host */, uint64_t* count_out /* host */,
                          void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_gindex_hamming_dev(const sfx_gindex* gx,
                           const uint8_t* d_qbytes, const uint64_t* d_qoff, uint64_t nq, uint32_t max_mismatches, uint64_t cand_limit,
                           uint32_t* d_pattern, uint32_t* d_tpos, uint8_t* d_mism, uint64_t capacity, uint64_t* d_first,
                           uint64_t* cands_out /* host */, uint64_t* count_out /* host */,
                           void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_index_hamming(const sfx_index* ix, const uint8_t* qbytes, const uint64_t* qoff, uint64_t nq, uint32_t max_mismatches,
                      uint64_t cand_limit, uint32_t* pattern_out, uint32_t* tpos_out, uint8_t* mism_out, uint64_t capacity,
                      uint64_t* first_out, uint64_t* cands_out, uint64_t* count_out);
int sfx_gindex_hamming(const sfx_gindex* gx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t nq, uint32_t max_mismatches,
                       uint64_t cand_limit, uint32_t* pattern_out, uint32_t* tpos_out, uint8_t* mism_out, uint64_t capacity,
                       uint64_t* first_out, uint64_t* cands_out, uint64_t* count_out);

/* ---- k-error pattern search against the table ----------------------------------------------
 * Where does a pattern occur if up to k bytes may be substituted, inserted or deleted (unit-cost Levenshtein distance)?
 * T = the indexed text of n bytes with table sa.  Patterns arrive as qbytes / qoff, exactly as for
 * sfx_index_hamming_dev; m_j = the length of pattern j, k = max_errors, 0 <= k <= 31.  Every pattern needs
 * m_j >= k + 1 (a shorter one would occur at every position).
 *   occurrence   of pattern j: an end position e for which some s <= e has ed(P_j, T[s..e)) <= k, T[s..e) inside one
 *                document for a collection (the truncated-suffix model).  dist = the least such distance over s,
 *                tbegin = the LARGEST s that attains it (the shortest best alignment), tend = e.  The triple is a
 *                property of (T, doc_starts, P_j, k) alone.
 *   pieces       as for the k-mismatch search: pattern j is cut at b_t = floor(t * m_j / (k + 1)); no piece is empty.
 *   candidates   triples (j, t, r), r a rank in the exact interval of piece t, numbered ascending by j, t, r; C of
 *                them.  q = sa[r], qe = q + |piece t|; lo / hi = the bounds of the text, or of q's document.
 *                left value   L = min over s in [max(lo, q - b_t - k), q] of ed(P_j[0..b_t), T[s..q)), s* = the largest
 *                             s that attains L
 *                right values R(e) = ed(P_j[b_(t+1)..m_j), T[qe..e)) for e in [qe, min(hi, qe + m_j - b_(t+1) + k)]
 *   hits         a candidate yields a hit (j, e, L + R(e), s*) for every e with L + R(e) <= k; H hits in all.  An
 *                alignment with at most k edits leaves one piece untouched, so it passes through a candidate, and its
 *                two parts cost at least L and R(e), while L + R(e) is itself the cost of an alignment: the occurrence
 *                at (j, e) has dist = the least L + R(e) over its hits and tbegin = the largest s* among the hits that
 *                attain it.  Expect several hits per occurrence.
 *   output       the quadruples (pattern, tbegin, tend, dist), ascending by pattern, then by tend; Z = the number of
 *                distinct (j, e).  first[0 .. nq] (u64) in CSR form, complete whatever `capacity` is; first[nq] = Z.
 *                Determined bit for bit by the inputs.  At k = 0 the quadruples of pattern j are (p, p + m_j, 0) for
 *                the positions p of the exact search, ascending by p.
 * Work is proportional to C times the pattern length in the worst case (an extension is abandoned once every cell of
 * its band is above the budget) plus a sort of the H hits: the caller gives cand_limit and hit_limit.
 *
 * sfx_edit_dev / sfx_index_edit_dev / sfx_gindex_edit_dev: everything is queued on the caller's stream, which is
 *   synchronised once to read (C, H, flags) back and, when there are hits, a second time behind the sort and the
 *   merge, for Z.  The calls keep no state in the index and take their memory from the workspace (the piece search of
 *   sfx_index_edit_dev is sfx_index_query_dev, as for sfx_index_hamming_dev): any number of threads may call on one
 *   index at once, each with its own workspace.
 *   *cands_out = C and *hits_out = H always (H = 0 when C is refused).  C <= cand_limit and H <= hit_limit:
 *   *count_out = Z, the first min(Z, capacity) quadruples are written and nothing past them, and first (when given)
 *   is complete.  C > cand_limit or H > hit_limit: SFX_OK, nothing is written to the quadruple arrays or to first, and
 *   *count_out = 0 -- the refusal is recognised by *cands_out > cand_limit or *hits_out > hit_limit.
 *   SFX_ERR_ARG: cand_limit == 0, hit_limit == 0 or hit_limit >= 2^32 (hits are numbered in 32 bits), max_errors > 31,
 *   cands_out / hits_out / count_out NULL, a quadruple array NULL while capacity > 0, a NULL input of a non-empty
 *   call, a qoff that is not monotone or a pattern with m_j <= k (both found on the device, reported through the same
 *   read-back), a workspace off SFX_WORKSPACE_ALIGN.  SFX_ERR_TOO_LARGE: n > u32::MAX, a pattern longer than u32::MAX
 *   (found on the device likewise), nq * (k + 1) >= 2^32.  A workspace below
 *   sfx_edit_workspace_bytes(nq, max_errors, cand_limit, hit_limit) is SFX_ERR_WORKSPACE.
 *   nq == 0 or n == 0: SFX_OK with C = H = Z = 0, first all zero if given.
 *   Workspace <= 24 (P + 1) + cand_limit / 7 + 30 hit_limit + 9 MiB bytes with P = nq (k + 1) (a cand_limit above
 *   P * u32::MAX counts as that, a hit_limit above (2 k + 1) cand_limit as that).
 *   d_text and d_qbytes may have any alignment, d_pattern / d_tbegin / d_tend need 4 bytes, d_qoff / d_first 8.
 *   Outside the caller's buffers nothing is written; outside T, sa (da and doc_starts of a collection), the patterns
 *   and the workspace nothing is read; no load of an extension touches a byte outside the candidate's two windows
 *   [max(lo, q - b_t - k), q) and [qe, min(hi, qe + m_j - b_(t+1) + k)) or outside the pattern.
 *   sfx_edit_dev takes text and table as they are: for any table whose entries are all < n nothing is read or written
 *   out of bounds and every loop ends; what is reported for a table that is not the text's suffix array is
 *   unspecified.
 * sfx_index_edit / sfx_gindex_edit: the same with host buffers, staged through HBM; they find a short pattern on the
 *   host.
 * Not covered: local-minima-only reporting, the alignment script (CIGAR), per-pattern k, k > 31, search over the
 * FM-index, the multi-GPU path. */
uint64_t sfx_edit_workspace_bytes(uint64_t nq, uint32_t max_errors, uint64_t cand_limit, uint64_t hit_limit);
int sfx_edit_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa,
                 const uint8_t* d_qbytes, const uint64_t* d_qoff, uint64_t nq, uint32_t max_errors, uint64_t cand_limit, uint64_t hit_limit,
                 uint32_t* d_pattern, uint32_t* d_tbegin, uint32_t* d_tend, uint8_t* d_dist, uint64_t capacity,
                 uint64_t* d_first /* nq + 1, may be NULL */,
                 uint64_t* cands_out /* host */, uint64_t* hits_out /* host */, uint64_t* count_out /* host */,
                 void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_index_edit_dev(const sfx_index* ix,
                       const uint8_t* d_qbytes, const uint64_t* d_qoff, uint64_t nq, uint32_t max_errors, uint64_t cand_limit, uint64_t hit_limit,
                       uint32_t* d_pattern, uint32_t* d_tbegin, uint32_t* d_tend, uint8_t* d_dist, uint64_t capacity, uint64_t* d_first,
                       uint64_t* cands_out /* host */, uint64_t* hits_out /* host */, uint64_t* count_out /* host */,
                       void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_gindex_edit_dev(const sfx_gindex* gx,
                        const uint8_t* d_qbytes, const uint64_t* d_qoff, uint64_t nq, uint32_t max_errors, uint64_t cand_limit, uint64_t hit_limit,
                        uint32_t* d_pattern, uint32_t* d_tbegin, uint32_t* d_tend, uint8_t* d_dist, uint64_t capacity, uint64_t* d_first,
                        uint64_t* cands_out /* host */, uint64_t* hits_out /* host */, uint64_t* count_out /* host */,
                        void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_index_edit(const sfx_index* ix, const uint8_t* qbytes, const uint64_t* qoff, uint64_t nq, uint32_t max_errors,
                   uint64_t cand_limit, uint64_t hit_limit, uint32_t* pattern_out, uint32_t* tbegin_out, uint32_t* tend_out,
                   uint8_t* dist_out, uint64_t capacity, uint64_t* first_out, uint64_t* cands_out, uint64_t* hits_out,
                   uint64_t* count_out);
int sfx_gindex_edit(const sfx_gindex* gx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t nq, uint32_t max_errors,
                    uint64_t cand_limit, uint64_t hit_limit, uint32_t* pattern_out, uint32_t* tbegin_out, uint32_t* tend_out,
                    uint8_t* dist_out, uint64_t capacity, uint64_t* first_out, uint64_t* cands_out, uint64_t* hits_out,
                    uint64_t* count_out);

/* ---- LCE index: inverse table, LCP range minima, k-mismatch extension -------- */
/* How far do the suffixes at two positions of the indexed text agree?  T has n bytes, with table sa and lcp as
 * sfx_build_sa_lcp_u32* write them; a collection uses the sa / in-document lcp of sfx_build_gsa_u32* plus doc_starts.
 * end(p) = n for a plain table, the end of p's document for a collection (the truncated-suffix model).
 *
 *   inverse table    isa[sa[r]] = r for r in [0, n).
 *   range_min(lo,hi) the minimum of lcp[lo .. hi) for 0 <= lo < hi <= n; UINT32_MAX for an empty range (lo >= hi) or
 *                    hi > n.  lcp[0] is taken as stored.
 *   LCE(i, j)        for i, j in [0, n): the largest l with T[i..i+l) = T[j..j+l), i + l <= end(i), j + l <= end(j)
 *                    = min(range_min(lo + 1, hi + 1), end(i) - i, end(j) - j), lo < hi the ranks of i and j.
 *                    i == j: end(i) - i.  A position equal to n gives 0, a position above n UINT32_MAX.
 *   LCE_k(i, j)      max_mismatches = k: the largest l within the same bounds such that T[i..i+l) and T[j..j+l) differ
 *                    in at most k places: l = LCE(i, j); while mismatches remain and both i + l and j + l are below
 *                    their ends, one mismatch is counted and stepped over (l += 1) and LCE(i + l, j + l) is added --
 *                    at most k + 1 rounds.  k is the same for the whole batch.  i == j gives end(i) - i for every k.
 *   The results are determined bit for bit by (T, sa, lcp, doc_starts, i, j, k).
 *
 * Structure: isa (4n bytes) and a 32-ary min-tree over lcp whose level 0 is the LCP array itself; every level above
 * starts on a 128-byte boundary, so a node is one line, and a range touches at most two lines per level.  The levels
 * above 0 take 4n/31 bytes plus padding: sfx_lce_bytes(n) <= 4n + n/7 + 64 KiB bounds what a handle from
 * sfx_lce_create_dev holds; the host route adds 4n for its copy of lcp (and 8 ndocs for doc_starts).  The index needs
 * neither T nor sa after creation.
 *
 * sfx_lce_create_dev borrows d_lcp and d_doc_starts (keep them alive until sfx_lce_destroy, like the arrays of
 * sfx_index_create_dev); d_sa is free again when it returns.  sfx_lce_create copies.  n == 0 gives a valid empty
 * handle, n > u32::MAX SFX_ERR_TOO_LARGE.  d_doc_starts == NULL (then ndocs == 0): a plain table.  The alignment rules
 * are those of the first comment: a 4-byte-aligned lcp works, 16-byte alignment lets level 0 be read 16 bytes at a time.
 *
 * What creation proves: every sa entry is < n and every one of the n slots of isa was written, hence sa is a
 * permutation of [0, n); doc_starts starts with 0, never decreases and stays <= n.  Otherwise SFX_ERR_ARG, with
 * nothing read or written out of bounds on any input.  What it does not prove: that lcp belongs to sa.  No address
 * depends on a value read from lcp and every result is clamped to min(end(i) - i, end(j) - j), so with a foreign lcp
 * the values are unspecified and nothing else.  Creation synchronises the stream once (the two flags);
 * sfx_inverse_table_dev likewise.  Creation allocates the handle's memory, and takes its scratch -- 256 bytes, from
 * 2^27 entries on 16 n bytes + the radix scratch of the partitioned scatter -- from the buffer pool of the host-pointer
 * entry points: a loop of creates at one size allocates it once, sfx_release_cached_buffers() returns it.  The query calls queue on the caller's stream, take no workspace and do not
 * synchronise; a handle may be queried from several threads at once.
 *
 * sfx_inverse_table_dev: isa alone, with the same proof (SFX_ERR_ARG for a table that is no permutation); a workspace
 * below sfx_inverse_table_workspace_bytes(n) is SFX_ERR_WORKSPACE.  sfx_lce_ranks*: rank[q] = isa[pos[q]], UINT32_MAX
 * for pos >= n.  sfx_lce_u32: create, query, destroy over host buffers.
 *
 * The argmin of a range and the suffix-tree LCA on top of it are the navigation calls below (sfx_lce_range_argmin*,
 * sfx_lce_lca*).  Not covered: LCE between a query text and the index (that is sfx_match_stats), positions >= 2^32, the
 * multi-GPU path. */
uint64_t sfx_inverse_table_workspace_bytes(uint64_t n);
int sfx_inverse_table_dev(const uint32_t* d_sa, uint64_t n, uint32_t* d_isa, void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_inverse_table_u32(const uint32_t* sa, uint64_t n, uint32_t* isa_out);

typedef struct sfx_lce sfx_lce;
uint64_t sfx_lce_bytes(uint64_t n);
int sfx_lce_create_dev(const uint32_t* d_sa, const uint32_t* d_lcp, uint64_t n, const uint64_t* d_doc_starts /* NULL: plain */,
                       uint64_t ndocs, void* stream, sfx_lce** out);
int sfx_lce_create(const uint32_t* sa, const uint32_t* lcp, uint64_t n, const uint64_t* doc_starts, uint64_t ndocs, sfx_lce** out);
void sfx_lce_destroy(sfx_lce* lx);
int sfx_lce_query_dev(const sfx_lce* lx, const uint32_t* d_a, const uint32_t* d_b, uint64_t nq, uint32_t max_mismatches,
                      uint32_t* d_len, void* stream);
int sfx_lce_query(const sfx_lce* lx, const uint32_t* a, const uint32_t* b, uint64_t nq, uint32_t max_mismatches, uint32_t* len_out);
int sfx_lce_range_min_dev(const sfx_lce* lx, const uint32_t* d_lo, const uint32_t* d_hi, uint64_t nq, uint32_t* d_min, void* stream);
int sfx_lce_range_min(const sfx_lce* lx, const uint32_t* lo, const uint32_t* hi, uint64_t nq, uint32_t* min_out);
int sfx_lce_ranks_dev(const sfx_lce* lx, const uint32_t* d_pos, uint64_t nq, uint32_t* d_rank, void* stream);
int sfx_lce_ranks(const sfx_lce* lx, const uint32_t* pos, uint64_t nq, uint32_t* rank_out);
int sfx_lce_u32(const uint32_t* sa, const uint32_t* lcp, uint64_t n, const uint64_t* doc_starts, uint64_t ndocs,
                const uint32_t* a, const uint32_t* b, uint64_t nq, uint32_t max_mismatches, uint32_t* len_out);

/* ---- suffix-tree navigation over the LCE handle: substring loci, LCA, argmin, suffix links ----
 * How often does T[pos .. pos+len) occur and where, what is the lowest common ancestor of two suffixes, where does a
 * node's suffix link point?  All from the handle above: no new index, no memory added to it.  end(p) as above;
 * B[p] = the LCP value of boundary p with B[0] = 0 whatever lcp[0] holds (the convention of sfx_lcp_intervals_dev);
 * NONE = UINT32_MAX.
 *
 *   bounds(r, d)     for a rank r < n and d >= 1: lo = the largest p <= r with B[p] < d (boundary 0 always qualifies),
 *                    hi = the smallest p > r with B[p] < d, or n.  bounds(r, 0) = [0, n).  Always lo <= r < hi.
 *   substr(pos,len)  len == 0 and pos <= n: [0, n), depth 0.  pos < n and 1 <= len <= end(pos) - pos:
 *                    [lo, hi) = bounds(isa[pos], len), exactly the ranks whose (truncated) suffix starts with
 *                    T[pos..pos+len): hi - lo occurrences, at sa[lo..hi).  depth = the string depth of the lowest
 *                    node at or below the locus: end(pos) - pos if hi - lo == 1, else min lcp[lo+1 .. hi).
 *                    Anything else: lo = hi = depth = NONE.
 *   lca(i, j)        i, j < n.  i == j: [isa[i], isa[i] + 1), depth end(i) - i.  Otherwise with a < b the two ranks
 *                    and d = min lcp[a+1 .. b+1): bounds(a, d), depth d (d == 0: the root [0, n)).  A position >= n:
 *                    all three NONE.
 *   argmin(lo, hi)   the smallest index that attains min lcp[lo .. hi), lcp[0] as stored (like range_min); NONE for
 *                    an empty range or hi > n.
 *   slink[k]         for node k of sfx_suffix_tree_dev's table (plain tables only) with string depth d: the dense id
 *                    of the node that spells k's string without its first byte.  It always exists and has depth d - 1.
 *                    slink[root] = NONE; every node of depth 1 links to the root, id 0.
 * An interval does not identify a node: in a unary text the root and the depth-1 node share [0, n).  A node is
 * (interval, depth), or its home boundary: the leftmost p in (lb, rb] with lcp[p] == depth, which is its
 * sfx_lcp_intervals_dev id and the leftmost argmin of lcp[lb+1 .. rb+1).  The root is decided by depth == 0.
 *
 * The three query calls work on collection handles too (intervals of the generalized table), queue on the caller's
 * stream, take no workspace, allocate nothing and do not synchronise; d_depth may be NULL.  Each query reads one
 * inverse-table entry and, per side of the search, at most 2 levels - 1 lines of the min-tree, whatever len is.
 * sfx_suffix_links_dev: d_sa is the table the handle was made from; SFX_ERR_ARG for a collection handle, a workspace
 * below sfx_suffix_links_workspace_bytes(n) (<= 4 n + 64 KiB; may hold anything on entry) is SFX_ERR_WORKSPACE.  It
 * queues two kernels and does not synchronise.  nq == 0, nodes == 0 and n == 0 succeed.  The node table is not
 * verified: node_lb >= node_rb or node_rb >= n gives slink = NONE for that node (a node spans two ranks or more), and
 * for a table that is not this lcp's every entry written is < nodes or NONE and nothing is accessed out of bounds.
 * If the caller changes the borrowed lcp after creation the intervals are unspecified, within lo <= rank < hi <= n.
 * Results are determined bit for bit by the inputs.  sfx_suffix_links_u32: create, link, destroy over host buffers.
 *
 * Not covered: suffix links of leaves and of collection trees, Weiner links, a walk of the matching statistics over
 * suffix links, positions >= 2^32, the multi-GPU path. */
int sfx_lce_substr_dev(const sfx_lce* lx, const uint32_t* d_pos, const uint32_t* d_len, uint64_t nq,
                       uint32_t* d_lo, uint32_t* d_hi, uint32_t* d_depth /* may be NULL */, void* stream);
int sfx_lce_substr(const sfx_lce* lx, const uint32_t* pos, const uint32_t* len, uint64_t nq,
                   uint32_t* lo_out, uint32_t* hi_out, uint32_t* depth_out /* may be NULL */);
int sfx_lce_lca_dev(const sfx_lce* lx, const uint32_t* d_a, const uint32_t* d_b, uint64_t nq,
                    uint32_t* d_lo, uint32_t* d_hi, uint32_t* d_depth /* may be NULL */, void* stream);
int sfx_lce_lca(const sfx_lce* lx, const uint32_t* a, const uint32_t* b, uint64_t nq,
                uint32_t* lo_out, uint32_t* hi_out, uint32_t* depth_out /* may be NULL */);
int sfx_lce_range_argmin_dev(const sfx_lce* lx, const uint32_t* d_lo, const uint32_t* d_hi, uint64_t nq, uint32_t* d_arg, void* stream);
int sfx_lce_range_argmin(const sfx_lce* lx, const uint32_t* lo, const uint32_t* hi, uint64_t nq, uint32_t* arg_out);
uint64_t sfx_suffix_links_workspace_bytes(uint64_t n);
int sfx_suffix_links_dev(const sfx_lce* lx, const uint32_t* d_sa, uint64_t nodes, const uint32_t* d_node_lb,
                         const uint32_t* d_node_rb, const uint32_t* d_node_depth, uint32_t* d_slink,
                         void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_suffix_links_u32(const uint32_t* sa, const uint32_t* lcp, uint64_t n, uint64_t nodes, const uint32_t* node_lb,
                         const uint32_t* node_rb, const uint32_t* node_depth, uint32_t* slink_out);

/* ---- document counts of every lcp-interval, k-common substrings of a collection ----------
 * Which strings are shared by many documents?  da, lcp, n, ndocs are a collection's arrays as sfx_build_gsa_u32* writes
 * them (lcp the in-document one; lcp[0] counts as 0 whatever it holds).  One document is a valid collection.
 *
 *   PREV[r]        the largest rank q < r with da[q] == da[r], or none.
 *   p(r)           for a rank with a PREV: the LARGEST boundary p in (PREV[r], r] with lcp[p] = min lcp(PREV[r], r].
 *   dup_prefix[x]  the number of ranks r with p(r) <= x (an inclusive prefix sum; it fits 32 bits: at most n - 1).
 *   For a rank interval [lb, rb] whose inner boundaries (lb, rb] all have lcp >= h while lcp[lb] < h and lcp[rb + 1] < h
 *   (boundary 0 and boundary n count as below) -- every lcp-interval, and the interval [start, end - 1] of every pattern
 *   that sfx_gindex_query* reports -- the number of distinct documents among da[lb .. rb] is
 *       (rb - lb + 1) - (dup_prefix[rb] - dup_prefix[lb]).
 *   df[p]          that number for the interval boundary p belongs to, [lb[p], rb[p]] of sfx_lcp_intervals_dev; boundary 0
 *                  and every boundary with lcp[p] == 0 belong to the root: df = the number of non-empty documents.
 *
 * sfx_doc_counts_dev writes d_dup_prefix and d_df, n entries each; either may be NULL.  Both are determined bit for bit
 * by (da, lcp).  It queues on the caller's stream and synchronises it once at the end, for one flag: a da entry >= ndocs
 * is SFX_ERR_ARG (nothing is read or written out of bounds on the way).  n == 0 succeeds; ndocs == 0 with n > 0 is
 * SFX_ERR_ARG; n > u32::MAX SFX_ERR_TOO_LARGE.  lcp is not verified: no address depends on a value read from it, so a
 * foreign lcp gives unspecified values and nothing else.  The workspace may hold anything on entry;
 * sfx_doc_counts_workspace_bytes(n) <= 34 n + 9 MiB bytes (PREV 4n, two (u64 key, u32 value) arrays 24n, the counts 4n,
 * the levels of the min-tree n/7, the interval search n/2 + n/15, the radix sort's scratch of 8 MiB + about n/2 and
 * the scan's partials); a shorter one is SFX_ERR_WORKSPACE.
 *
 * k-common substrings: for d in 1 .. ndocs,
 *   len[d - 1]  the length of the longest string that occurs in at least d distinct documents, 0 if there is none; it
 *               does not increase with d.  For d >= 2 the maximum of lcp[p] over the boundaries p >= 1 with df[p] >= d;
 *               for d == 1 the whole documents count too, so it is the longest document's length.
 *   pos[d - 1]  a text position where that string stands, UINT32_MAX where len is 0: sa[p*] for the smallest boundary
 *               p* with df[p*] >= d and lcp[p*] == len[d - 1]; for d == 1, if no boundary attains the length, the start
 *               of the first longest document.
 * sfx_common_substrings_dev reads sa, lcp, df (n entries, df as sfx_doc_counts_dev writes it; an entry of 0 or above
 * ndocs is passed over) and doc_starts, and writes ndocs entries of d_len and d_pos.  It synchronises the stream once,
 * for the check of doc_starts (first 0, never decreasing, none past n: else SFX_ERR_ARG), and returns with its last
 * kernel queued.  ndocs == 0 is SFX_ERR_ARG unless n == 0; n or ndocs above u32::MAX is SFX_ERR_TOO_LARGE.  The workspace
 * is sfx_common_substrings_workspace_bytes(ndocs) = 8 ndocs + 1 KiB at most.
 *
 * sfx_doc_counts_u32 / sfx_common_substrings_u32: the same over host buffers.
 *
 * Not covered: sfx_gindex_query* still counts documents by its linear pass over PREV; the node table of
 * sfx_suffix_tree_dev for collections; the multi-GPU path. */
uint64_t sfx_doc_counts_workspace_bytes(uint64_t n);
int sfx_doc_counts_dev(const uint32_t* d_da, const uint32_t* d_lcp, uint64_t n, uint64_t ndocs, uint32_t* d_dup_prefix /* may be NULL */,
                       uint32_t* d_df /* may be NULL */, void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_doc_counts_u32(const uint32_t* da, const uint32_t* lcp, uint64_t n, uint64_t ndocs, uint32_t* dup_prefix_out, uint32_t* df_out);
uint64_t sfx_common_substrings_workspace_bytes(uint64_t ndocs);
int sfx_common_substrings_dev(const uint32_t* d_sa, const uint32_t* d_lcp, const uint32_t* d_df, uint64_t n, const uint64_t* d_doc_starts,
                              uint64_t ndocs, uint32_t* d_len, uint32_t* d_pos, void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_common_substrings_u32(const uint32_t* sa, const uint32_t* lcp, const uint32_t* df, uint64_t n, const uint64_t* doc_starts,
                              uint64_t ndocs, uint32_t* len_out, uint32_t* pos_out);

/* ---- document listing with term frequencies and top-k per interval -------------------------
 * Which documents hold a pattern, and how often each?  da[0..n) and doc_starts[0..ndocs) are a collection's arrays as
 * sfx_build_gsa_u32* takes and writes them; the nq rank intervals [s_j, e_j) with s_j <= e_j <= n are as
 * sfx_gindex_query* returns them (all occurrences of one string under the truncated-suffix model).  Any rank interval
 * is legal: a tree node's lb .. rb + 1, or [0, n).
 *
 *   tf_j(d)   the number of ranks r in [s_j, e_j) with da[r] == d.
 *   D_j       the set of documents d with tf_j(d) > 0.  Empty documents never appear.
 *   order     SFX_DOCLIST_BY_DOC (0): list j holds D_j ascending by document id.
 *             SFX_DOCLIST_BY_TF (1): descending tf, ties ascending by id.
 *   top_k     0: the whole list; otherwise the first min(top_k, |D_j|) entries of the list in the chosen order.
 *   output    CSR: doc[] and tf[] (u32), first[0 .. nq] (u64); list j is [first[j], first[j+1]); first[nq] = Z counts
 *             entries, not written ones.  The output is determined bit for bit by (da, intervals, order, top_k).
 *
 * The index (sfx_doclist): PREV[r] = the previous rank of r's document (or none) and R = the ranks ordered by (document,
 * rank), both from one stable sort of (da, rank).  Every text position contributes one suffix, so document d's ranks are
 * R[doc_starts[d] .. doc_end(d)) and tf_j(d) is the difference of two bisections inside that slice.  The object holds
 * sfx_doclist_bytes(n) = 8n bytes (+ at most 512 of padding); sfx_doclist_create_dev borrows d_da and d_doc_starts (keep
 * them alive until sfx_doclist_destroy), sfx_doclist_create copies them (4n + 8 ndocs more).
 * What creation proves: every da entry is < ndocs; doc_starts starts with 0, never decreases and stays <= n; slot k of
 * the sorted (da, rank) pairs names the document that owns text position k -- hence document d has exactly its length in
 * ranks.  Otherwise SFX_ERR_ARG, found through the one read-back of a create, with nothing read or written out of bounds.
 * n == 0 gives a valid empty handle; ndocs == 0 with n > 0 is SFX_ERR_ARG; n or ndocs > u32::MAX SFX_ERR_TOO_LARGE.
 * Creation scratch: sfx_doclist_create_workspace_bytes(n) <= 24.5 n + 9 MiB bytes of the caller's (any contents), or, with
 * d_workspace == NULL, of the buffer pool of the host-pointer entry points (sfx_release_cached_buffers() returns it).
 * occ_cut: intervals longer than occ_cut are listed by document (lanes bisect every document's slice: 2 ndocs log random
 * lines whatever e - s is), the others by occurrence (PREV is streamed; the first occurrence of a document in the
 * interval bisects).  0 = automatic, 32 ndocs (measured: DESIGN.md section 24).  Both routes give the same bytes.
 *
 * sfx_doclist_list_dev queues on the caller's stream and synchronises it ONCE, to read (Z_full, Z, flags) back; the
 * ordering of the entries and their copy into d_doc / d_tf are queued behind that read-back, so those two arrays are
 * complete in stream order (d_first is complete when the call returns).  That queued work reads the workspace: unlike the
 * other `_dev` calls, keep the workspace alive and unwritten until the stream has passed it (a later call on the SAME
 * stream may reuse it; freeing it, or using it on another stream, needs a synchronisation or an event first).  A call keeps no state in the object and takes
 * its memory from the workspace: any number of threads may call on one object, each with its own workspace.
 *   *listed_out = Z_full = the sum of |D_j|, always.
 *   Z_full <= list_limit: *count_out = Z, the first min(Z, capacity) entries are written and nothing past them, and
 *   first (when given) is complete whatever capacity is.
 *   Z_full > list_limit: SFX_OK, nothing is written to doc, tf or first, and *count_out = 0.  A list_limit above
 *   u32::MAX counts as u32::MAX.
 *   SFX_ERR_ARG: order > 1, listed_out / count_out NULL, d_doc or d_tf NULL while capacity > 0, a NULL interval array
 *   of a non-empty call, an interval with s > e or e > n (found on the device, reported through the same read-back,
 *   nothing written), a workspace off SFX_WORKSPACE_ALIGN.  nq >= 2^32: SFX_ERR_TOO_LARGE.  A workspace below
 *   sfx_doclist_workspace_bytes(nq, list_limit) is SFX_ERR_WORKSPACE.  nq == 0 or n == 0: SFX_OK, first all zeros.
 *   Workspace <= 36 nq + 25 L + 9 MiB bytes, L = min(list_limit, u32::MAX): per interval its item count, three offsets
 *   and the cut length; per entry two (u64 key, u32 value) pairs for the sort, whose scratch is 8 MiB + L / 2.
 *   d_start / d_end / d_doc / d_tf need 4-byte alignment, d_first 8.
 * sfx_doclist_list: the same with host buffers, staged through HBM; it lowers list_limit to the sum of
 * min(e_j - s_j, ndocs), which Z_full cannot exceed.
 * Not covered: listing straight from pattern bytes in one call (sfx_gindex_query* gives the intervals), weights other
 * than tf, the multi-GPU path. */
#define SFX_DOCLIST_BY_DOC 0u
#define SFX_DOCLIST_BY_TF 1u
typedef struct sfx_doclist sfx_doclist;
uint64_t sfx_doclist_bytes(uint64_t n);
uint64_t sfx_doclist_create_workspace_bytes(uint64_t n);
int sfx_doclist_create_dev(const uint32_t* d_da, uint64_t n, const uint64_t* d_doc_starts, uint64_t ndocs, uint64_t occ_cut,
                           void* d_workspace /* NULL: pooled */, uint64_t workspace_bytes, void* stream, sfx_doclist** out);
int sfx_doclist_create(const uint32_t* da, uint64_t n, const uint64_t* doc_starts, uint64_t ndocs, uint64_t occ_cut, sfx_doclist** out);
void sfx_doclist_destroy(sfx_doclist* dx);
uint64_t sfx_doclist_workspace_bytes(uint64_t nq, uint64_t list_limit);
int sfx_doclist_list_dev(const sfx_doclist* dx, const uint32_t* d_start, const uint32_t* d_end, uint64_t nq, uint32_t order, uint32_t top_k,
                         uint64_t list_limit, uint32_t* d_doc, uint32_t* d_tf, uint64_t capacity, uint64_t* d_first /* nq + 1, may be NULL */,
                         uint64_t* listed_out /* host */, uint64_t* count_out /* host */,
                         void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_doclist_list(const sfx_doclist* dx, const uint32_t* start, const uint32_t* end, uint64_t nq, uint32_t order, uint32_t top_k,
                     uint64_t list_limit, uint32_t* doc_out, uint32_t* tf_out, uint64_t capacity, uint64_t* first_out,
                     uint64_t* listed_out, uint64_t* count_out);

/* ---- maximal repetitions (runs), the Lyndon array, tandem repeats --------------------------
 * T is a plain text of n bytes, 0 <= n < 2^32 - 1 (larger: SFX_ERR_TOO_LARGE).  Collections are out of scope.
 *
 *   run       a triple (b, e, p), 0 <= b < e <= n, p >= 1, such that p is the smallest period of T[b..e), e - b >= 2p,
 *             b == 0 or T[b-1] != T[b-1+p], and e == n or T[e] != T[e-p].  (b, p) determines e; there are fewer than n runs.
 *             T[b..e) is its first p bytes written (e - b) / p times in a row: the tandem repeats of T.
 *   lyn_o[i]  the Lyndon array under order o: o = 0 byte order, o = 1 reversed byte order; in both a proper prefix is smaller
 *             than its extension.  lyn_o[i] = nss_o(i) - i, nss_o(i) = the least j > i whose suffix is smaller than the suffix
 *             at i under o, or n.  Over the inverse table of order o: the next j > i with isa_o[j] < isa_o[i].  The table of
 *             order 1 is the table of the complemented text (byte -> 255 - byte).  T[i .. i + lyn_o[i]) is the longest Lyndon
 *             word of order o that starts at i.
 *   Lyndon factorization: the factors start at i_0 = 0, i_{k+1} = i_k + lyn_0[i_k].
 *
 * sfx_lyndon_array_dev: d_lyn[0..n) from an inverse table (sfx_inverse_table_dev), queued on the stream: no read-back, no
 * synchronisation.  d_isa is not verified -- its values are only compared, no address is formed from them.  Workspace
 * sfx_lyndon_array_workspace_bytes(n) <= 4n + n / 7 + 2 KiB bytes.  sfx_lyndon_array_u32: host buffers; sa == NULL builds the
 * table of `text` under `order` (0 | 1, anything else SFX_ERR_ARG); a given sa is taken as the table of that order (text may
 * then be NULL) and must be a permutation of [0, n), else SFX_ERR_ARG.
 *
 * sfx_runs_dev: every run that passes the filter (min_period <= p <= max_period, e - b >= min_len; max_period 0 = n; filter
 * NULL = all), ascending by (begin, period), unique, determined bit for bit by T and the filter.  *count_out is always the
 * full count; the first min(count, capacity) triples in that order are written and nothing past them; capacity n always
 * suffices.  d_sa / d_lcp are the tables of T as sfx_build_sa_lcp_u32_dev writes them.  A d_sa that is not a permutation of
 * [0, n) is SFX_ERR_ARG (proven while its inverse table is made, nothing read or written out of bounds).  d_lcp is not
 * verified: no address is formed from it, and every reported triple satisfies 0 <= b < e <= n and 2p <= e - b whatever it
 * holds (with a foreign d_lcp the triples are otherwise unspecified, and at most n are counted).
 * The call builds the table of the complemented text (sfx_build_sa_u32_dev: its read-backs), then synchronises the stream
 * ONCE, to read (count, flags) back; the ordering of the triples and their copy into d_begin / d_end / d_period are queued
 * behind that read-back, so the three arrays are complete in stream order, and the workspace must stay alive and unwritten
 * until the stream has passed that work (as sfx_doclist_list_dev).  The `_dev` route allocates nothing.
 *   Workspace: with up(x) = x rounded up to 256 and tw(n) = the words of the 32-ary levels above n words
 *   (sum of ceil(n / 32^k) rounded up to 32, while the level below has more than 32 words; <= n / 31 + 32 per level),
 *     sfx_runs_workspace_bytes(n) = up(256) + 2 up(8 * 2048) + 2 up(8 * 2049) + up(n) + 5 up(4n) + up(4 tw(n))
 *                                   + max(up(sfx_sa_workspace_bytes(n)), late(n)),
 *     late(n) = up(4 tw(n)) + 3 up(4n) + 2 up(8n) + up(4 s(n)),   s(n) = the words of the radix sort's scratch, <= 2 Mi + n / 8
 *   hence <= 21.13 n + 80 KiB + max(sfx_sa_workspace_bytes(n) + 256, 28.63 n + 8.1 MiB).
 *   SFX_ERR_ARG: count_out NULL, a NULL text or table of a non-empty call, an output array NULL while capacity > 0, a
 *   workspace off SFX_WORKSPACE_ALIGN.  A workspace below sfx_runs_workspace_bytes(n) is SFX_ERR_WORKSPACE.  n == 0: SFX_OK,
 *   count 0.  d_sa, d_lcp and the three outputs need 4-byte alignment.
 * sfx_runs_u32: the same with host buffers, staged through the buffer pool; sa == NULL builds both tables, lcp == NULL with
 * a given sa builds the LCP array (lcp without sa is SFX_ERR_ARG).
 * Not built: collections, the multi-GPU path, the Rust binding, a direct comparison of the first text bytes in front of the
 * first extension, the partitioned scatter for the inverse tables of more than 2^27 entries. */
typedef struct { uint32_t min_period, max_period, min_len, reserved; } sfx_runs_filter_t;
uint64_t sfx_lyndon_array_workspace_bytes(uint64_t n);
int sfx_lyndon_array_dev(const uint32_t* d_isa, uint64_t n, uint32_t* d_lyn, void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_lyndon_array_u32(const uint8_t* text, uint64_t n, const uint32_t* sa /* NULL: built */, int order, uint32_t* lyn_out);
uint64_t sfx_runs_workspace_bytes(uint64_t n);
int sfx_runs_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint32_t* d_lcp, const sfx_runs_filter_t* filter /* NULL: all */,
                 uint32_t* d_begin, uint32_t* d_end, uint32_t* d_period, uint64_t capacity, uint64_t* count_out /* host */,
                 void* d_workspace, uint64_t workspace_bytes, void* stream);
int sfx_runs_u32(const uint8_t* text, uint64_t n, const uint32_t* sa /* NULL: built */, const uint32_t* lcp /* NULL: built */,
                 const sfx_runs_filter_t* filter, uint32_t* begin, uint32_t* end, uint32_t* period, uint64_t capacity, uint64_t* count_out);

/* ---- range-partitioned construction (multi-GPU, one rank per GPU) ----------- */
/* Every rank holds the whole text in HBM (all-gathered over RCCL) and owns the
 * text shard [shard_begin, shard_end).
 * Step 1  sfx_byte_histogram_dev: 256 u64 byte counts of the rank's shard
 *         (cf. Bins::find_sizes :686-704).  Ranks all-reduce(sum) them; the
 *         result defines the dense symbol codes, identically on every rank.
 * Step 2  sfx_key_histogram_dev: every suffix has a key = its first k symbols
 *         packed big-endian (k fixed by the global byte COUNTS and n -- an alphabet of
 *         more than 16 symbols that is used unevenly gets the wider key: the rule looks
 *         at the order-0 entropy -- so steps 2 and 4 must be given the same all-reduced
 *         counts, not presence flags); this counts,
 *         for the suffixes starting in the rank's shard, the top `top_bits`
 *         (<= 14) bits of that key into 2^top_bits u64 bins.  Ranks all-reduce
 *         them = the bucket-boundary histogram exchange.
 * Step 3  the host splits the bins into contiguous, balanced ranges, one per rank.
 * Step 4  sfx_build_sa_range_u32_dev: sort ONLY the suffixes whose bin lies in
 *         [bin_lo, bin_hi).  Writes them, fully sorted, to d_sa_part (capacity
 *         entries available) and their number to *count_out (host pointer):
 *         d_sa_part is this rank's contiguous slice of the global suffix array. */
int sfx_byte_histogram_dev(const uint8_t* d_text, uint64_t shard_begin, uint64_t shard_end,
                           uint64_t* d_bins256, void* stream);
int sfx_key_histogram_dev(const uint8_t* d_text, uint64_t n, uint64_t shard_begin,
                          uint64_t shard_end, const uint64_t* d_global_byte_bins256,
                          int top_bits, uint64_t* d_bins, void* stream);
uint64_t sfx_sa_range_workspace_bytes(uint64_t n, uint64_t capacity);
int sfx_build_sa_range_u32_dev(const uint8_t* d_text, uint64_t n,
                               const uint64_t* d_global_byte_bins256, int top_bits,
                               uint32_t bin_lo, uint32_t bin_hi, uint64_t capacity,
                               uint32_t* d_sa_part, uint64_t* count_out, void* d_workspace,
                               uint64_t workspace_bytes, void* stream);

/* Packed-text variant of steps 1 and 4 (saves xGMI volume: the all-gather moves
 * bits/8 of the raw bytes, and no rank packs the whole text):
 *   sfx_pack_text_dev   symbols of d_text[0..count) re-coded with the GLOBAL alphabet
 *         (d_global_byte_bins256) and packed big-endian, floor(32/bits) per u32 word,
 *         bits = ceil(log2 sigma); writes exactly n_words words (zeros past the text).
 *         A shard whose length is a multiple of floor(32/bits) packs into count /
 *         floor(32/bits) words that can be concatenated across ranks; the concatenation
 *         must end in >= 3 zero words.  d_scratch256: 256 bytes of device scratch.
 *   sfx_build_sa_range_packed_u32_dev   step 4 on that packed text (n = symbols). */
int sfx_pack_text_dev(const uint8_t* d_text, uint64_t count, const uint64_t* d_global_byte_bins256,
                      uint8_t* d_scratch256, uint32_t* d_words, uint64_t n_words, void* stream);
int sfx_build_sa_range_packed_u32_dev(const uint32_t* d_packed, uint64_t n,
                                      const uint64_t* d_global_byte_bins256, int top_bits,
                                      uint32_t bin_lo, uint32_t bin_hi, uint64_t capacity,
                                      uint32_t* d_sa_part, uint64_t* count_out, void* d_workspace,
                                      uint64_t workspace_bytes, void* stream);

/* Per-rank pieces of the partitioned index (every rank holds the text and ONE contiguous
 * slice d_sa_part[0..count) of the suffix array):
 *  - LCP of the slice: lcp_part[r] = |lcp(text[sa_part[r-1]..], text[sa_part[r]..])|, with
 *    prev_suffix = the last suffix of the previous rank's slice for r == 0 (UINT32_MAX for
 *    the first slice, giving 0 as :352 does).  Direct comparison, exactly :348-361.
 *  - queries against the slice: start/end are positions INSIDE the slice (0/0 if the
 *    slice holds no match); the global interval is the concatenation over ranks.        */
int sfx_build_lcp_range_u32_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa_part,
                                uint64_t count, uint32_t prev_suffix, uint32_t* d_lcp_part,
                                void* stream);
int sfx_query_batch_range_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa_part,
                              uint64_t count, const uint8_t* d_qbytes, const uint64_t* d_qoff,
                              uint64_t nq, uint32_t* d_start, uint32_t* d_end, uint8_t* d_found,
                              uint32_t* d_any, void* stream);

/* ---- memory-system micro-benchmarks (the scatter/gather roofline
 * must be measured) -------------------------------------------------------------
 * Allocates its own device buffers of about `bytes`, runs `reps` timed launches
 * (after one warm-up) and reports algorithmic GB/s (10^9 B/s) in *gbps_out.
 *   SFX_MB_COPY        streaming 16-byte copy (read + write counted)
 *   SFX_MB_SCATTER4    random 4-byte writes into a `bytes`-sized array
 *                      (head_insert/tail_insert :723-736, ISA[suffix] = rank)
 *   SFX_MB_GATHER1     random 1-byte reads (T[s-1] in induce, :429)
 *   SFX_MB_GATHER4     random 4-byte reads (ISA[suffix + h])
 *   SFX_MB_RUNSCATTER  runs of `param` bytes (power of two >= 8) copied to
 *                      pseudo-random places, run-aligned if param2 != 0, else
 *                      offset by 8 bytes: the write side of a radix pass        */
enum { SFX_MB_COPY = 0, SFX_MB_SCATTER4 = 1, SFX_MB_GATHER1 = 2, SFX_MB_GATHER4 = 3, SFX_MB_RUNSCATTER = 4 };
int sfx_microbench(int kind, uint64_t bytes, int param, int param2, int reps, double* gbps_out);

/* ---- profiling (per-kernel HIP-event timing; off by default) ---------------- */
/* When enabled every kernel launch is bracketed by hipEvents on its stream.
 * sfx_profile_report writes up to `cap` records and returns how many exist. */
typedef struct {
    char     name[48];
    uint64_t launches;
    double   total_ms;
    double   algo_bytes;      /* algorithmic bytes summed over launches */
} sfx_kernel_stat;
void sfx_profile_enable(int on);
void sfx_profile_reset(void);
int  sfx_profile_report(sfx_kernel_stat* out, int cap);
/* per-build statistics of the most recent SA construction on this thread */
typedef struct {
    uint64_t n;
    uint32_t sigma;           /* distinct byte values                          */
    uint32_t bits_per_symbol;
    uint32_t key_bits;        /* width of the initial k-mer key (32 or 64)     */
    uint32_t symbols_per_key; /* k (compressed 64-bit keys: the average, 64 / mean code length) */
    uint32_t rounds;          /* refinement rounds after the initial sort      */
    uint32_t reserved;        /* bit 0: sfx_build_sa_lcp_u32 stopped reading LCP values off the sort (most suffixes tied on the initial key);
                                 bit 1: the initial keys are context codes (a code per class of the preceding symbol) */
    uint64_t active_after_initial;
    uint64_t radix_passes;
    uint64_t elements_sorted; /* sum over passes of elements moved             */
    uint64_t small_bucket_resolved; /* suffixes placed by direct comparison of small buckets */
    uint64_t tile_sorted;     /* elements ordered by the in-LDS bucket sort, summed over rounds   */
    uint64_t large_sorted;    /* elements of buckets too large for LDS, summed over rounds        */
    uint32_t text_rounds;     /* refinement rounds keyed by text symbols                          */
    uint32_t rank_rounds;     /* refinement rounds keyed by ranks (prefix doubling)               */
    uint64_t deep_gathers;    /* 64-bit key gathers of the deep text rounds (one random line each) */
} sfx_build_stats;
/* Writes sizeof(sfx_build_stats) bytes AS OF THE LIBRARY'S header.  The struct has grown (round 3 appended deep_gathers:
 * 104 -> 112 bytes) and may grow again, always at its end: a consumer compiled against an older header must use
 * sfx_build_stats_read instead, or it is written past its struct. */
void sfx_last_build_stats(sfx_build_stats* out);
/* The size-aware form: copies the first min(out_bytes, sizeof(sfx_build_stats)) bytes and returns the library's
 * sizeof(sfx_build_stats) (so a caller can tell which trailing fields it got).  out == NULL: only the size. */
uint64_t sfx_build_stats_read(void* out, uint64_t out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SUFFIX_HIP_H */
