//! suffix-hip -- the Rust side of the drop-in boundary of the MI355X suffix-array engine.
//!
//! A cargo crate: `rust/suffix-hip/{Cargo.toml, build.rs, src/lib.rs}` plus two patches for a checkout
//! of BurntSushi/suffix v1.3.0 (`table.rs.patch`, `Cargo.toml.patch`).  With them applied,
//!
//!     SUFFIX_HIP_LIB_DIR=<dir of libsuffix_hip.so> cargo test --features hip
//!
//! runs the upstream `tests/tests.rs` (31 tests, 5 QuickCheck properties) with `SuffixTable::new`,
//! `lcp_lens` and the additive `positions_batch` going through `libsuffix_hip.so`.
//! NOT COMPILED IN THIS REPOSITORY'S CI: the build image has no rustc/cargo; what is
//! checked here, on the CPU, is that the patches apply to the reference sources and that every
//! signature in the `extern "C"` block below equals its declaration in `include/suffix_hip.h`
//! (tests/test_rust_crate.py).  The ctypes binding in `suffix_amd/_lib.py` and the C++ mirror
//! exercise the same symbols with the same argument meaning on the GPU box.
//!
//! What changes in the crate (nothing in `:140-312` or `lib.rs` changes):
//!   * `sais_table`  (src/table.rs:378-386)  body after `vec![0u32; n]`
//!   * `lcp_lens`    (src/table.rs:130-138)  body
//!   * new additive  `SuffixTable::device_index()` (the resident index, kept by the caller across batches),
//!     `positions_batch_on(&index, queries)` and the one-shot `positions_batch(queries)`
//!   * texts below `min_device_len()` bytes keep the crate's own CPU path.  The default is `MIN_DEVICE_LEN` = 64 KiB (a trip
//!     to the device costs ~100 us whatever the length): right for production, but every string of the upstream tests --
//!     QuickCheck's (< 100 bytes) and the literals of `tests/tests.rs` -- is far below it.  A TEST RUN THEREFORE SETS
//!     `SUFFIX_HIP_MIN_LEN=0` (read once per process) or builds with `--features hip-always`: then all 31 upstream tests
//!     cross the FFI, the empty text and the one-byte text included (tests/tests.rs:42-65).
//! `sais()`, `Bins`, `SuffixTypes` stay in the crate as the reference CPU path (feature `hip` off).

use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct SfxIndex {
    _private: [u8; 0],
}

extern "C" {
    fn sfx_strerror(status: c_int) -> *const c_char;
    fn sfx_last_hip_error() -> *const c_char;
    fn sfx_device_count() -> c_int;
    // SuffixTable::new -> sais_table
    fn sfx_build_sa_u32(text: *const u8, n: u64, sa_out: *mut u32) -> c_int;
    // lcp_lens
    fn sfx_build_lcp_u32(text: *const u8, n: u64, sa: *const u32, lcp_out: *mut u32) -> c_int;
    // SuffixTable::new + lcp_lens in one engine call (what suffix_tree's to_suffix_tree needs)
    fn sfx_build_sa_lcp_u32(text: *const u8, n: u64, sa_out: *mut u32, lcp_out: *mut u32) -> c_int;
    // device-resident index for batched queries
    fn sfx_index_create(text: *const u8, n: u64, sa: *const u32, out: *mut *mut SfxIndex) -> c_int;
    fn sfx_index_destroy(ix: *mut SfxIndex);
    fn sfx_index_len(ix: *const SfxIndex) -> u64;
    fn sfx_positions_batch(ix: *const SfxIndex, qbytes: *const u8, qoff: *const u64, nq: u64,
                           start_out: *mut u32, end_out: *mut u32) -> c_int;
    fn sfx_contains_batch(ix: *const SfxIndex, qbytes: *const u8, qoff: *const u64, nq: u64,
                          found_out: *mut u8, any_out: *mut u32) -> c_int;
    // matching statistics of a second text against the resident index (host buffers; src / start+end may be null)
    fn sfx_index_match_stats(ix: *const SfxIndex, query: *const u8, m: u64, max_len: u32, len_out: *mut u32,
                             src_out: *mut u32, start_out: *mut u32, end_out: *mut u32) -> c_int;
    #[allow(dead_code)]
    fn sfx_index_match_stats_dev(ix: *const SfxIndex, d_query: *const u8, m: u64, max_len: u32, d_len: *mut u32,
                                 d_src: *mut u32, d_start: *mut u32, d_end: *mut u32, stream: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn sfx_match_stats_dev(d_text: *const u8, n: u64, d_sa: *const u32, d_query: *const u8, m: u64, max_len: u32,
                           d_len: *mut u32, d_src: *mut u32, d_start: *mut u32, d_end: *mut u32,
                           stream: *mut c_void) -> c_int;
    // maximal exact matches of a second text against the resident index (host buffers; the outputs may be null at capacity 0)
    fn sfx_index_mems(ix: *const SfxIndex, query: *const u8, m: u64, min_len: u32, flags: u32, pair_limit: u64,
                      qpos_out: *mut u32, tpos_out: *mut u32, len_out: *mut u32, capacity: u64, pairs_out: *mut u64,
                      count_out: *mut u64) -> c_int;
    #[allow(dead_code)]
    fn sfx_index_mems_dev(ix: *const SfxIndex, d_query: *const u8, m: u64, min_len: u32, flags: u32, pair_limit: u64,
                          d_qpos: *mut u32, d_tpos: *mut u32, d_len: *mut u32, capacity: u64, pairs_out: *mut u64,
                          count_out: *mut u64, d_workspace: *mut c_void, workspace_bytes: u64, stream: *mut c_void) -> c_int;
    // Burrows-Wheeler transform with sampled ranks and its inverse (host buffers; sa may be null: the table is built)
    fn sfx_bwt_sample_count(n: u64, sample_step: u32) -> u64;
    fn sfx_bwt_u32(text: *const u8, n: u64, sa: *const u32, sample_step: u32, bwt_out: *mut u8,
                   samples_out: *mut u32) -> c_int;
    fn sfx_unbwt(bwt: *const u8, n: u64, samples: *const u32, nsamples: u64, sample_step: u32,
                 text_out: *mut u8) -> c_int;
    #[allow(dead_code)]
    fn sfx_bwt_dev(d_text: *const u8, n: u64, d_sa: *const u32, sample_step: u32, d_bwt: *mut u8,
                   d_samples: *mut u32, stream: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn sfx_unbwt_workspace_bytes(n: u64) -> u64;
    #[allow(dead_code)]
    fn sfx_unbwt_dev(d_bwt: *const u8, n: u64, d_samples: *const u32, nsamples: u64, sample_step: u32,
                     d_text_out: *mut u8, d_workspace: *mut c_void, workspace_bytes: u64,
                     stream: *mut c_void) -> c_int;
    // LZ77 factorization from the EARLIER repeat lengths and its decoder (lz77 / unlz below; the *_dev forms for callers that
    // keep their arrays in device memory)
    #[allow(dead_code)]
    fn sfx_lz_parse_workspace_bytes(n: u64) -> u64;
    #[allow(dead_code)]
    fn sfx_lz_parse_dev(d_rep: *const u32, d_src: *const u32, d_text: *const u8, n: u64, min_len: u32, d_begin: *mut u32,
                        d_len: *mut u32, d_psrc: *mut u32, d_lit: *mut u8, capacity: u64, count_out: *mut u64,
                        d_workspace: *mut c_void, workspace_bytes: u64, stream: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn sfx_lz_decode_workspace_bytes(n: u64, z: u64) -> u64;
    #[allow(dead_code)]
    fn sfx_lz_decode_dev(d_len: *const u32, d_psrc: *const u32, d_lit: *const u8, z: u64, n: u64, d_text_out: *mut u8,
                         d_workspace: *mut c_void, workspace_bytes: u64, stream: *mut c_void) -> c_int;
    fn sfx_lz77_u32(text: *const u8, n: u64, sa: *const u32, lcp: *const u32, min_len: u32, begin_out: *mut u32,
                    len_out: *mut u32, src_out: *mut u32, lit_out: *mut u8, capacity: u64, count_out: *mut u64) -> c_int;
    fn sfx_unlz(len: *const u32, src: *const u32, lit: *const u8, z: u64, n: u64, text_out: *mut u8) -> c_int;
    // maximal exact matches of a query text (sfx_mems_dev: text and table in device memory; DeviceIndex::mems below goes
    // through the same kernels with host buffers)
    #[allow(dead_code)]
    fn sfx_mems_workspace_bytes(m: u64, pair_limit: u64) -> u64;
    #[allow(dead_code)]
    fn sfx_mems_dev(d_text: *const u8, n: u64, d_sa: *const u32, d_query: *const u8, m: u64, min_len: u32, flags: u32,
                    pair_limit: u64, d_qpos: *mut u32, d_tpos: *mut u32, d_len: *mut u32, capacity: u64, pairs_out: *mut u64,
                    count_out: *mut u64, d_workspace: *mut c_void, workspace_bytes: u64, stream: *mut c_void) -> c_int;
    // k-mismatch pattern search (Hamming distance) of a batch of patterns; DeviceIndex::approx_positions below goes through
    // sfx_index_hamming (host buffers; the outputs may be null at capacity 0, first_out may be null)
    fn sfx_index_hamming(ix: *const SfxIndex, qbytes: *const u8, qoff: *const u64, nq: u64, max_mismatches: u32,
                         cand_limit: u64, pattern_out: *mut u32, tpos_out: *mut u32, mism_out: *mut u8, capacity: u64,
                         first_out: *mut u64, cands_out: *mut u64, count_out: *mut u64) -> c_int;
    #[allow(dead_code)]
    fn sfx_hamming_workspace_bytes(nq: u64, max_mismatches: u32, cand_limit: u64) -> u64;
    #[allow(dead_code)]
    fn sfx_hamming_dev(d_text: *const u8, n: u64, d_sa: *const u32, d_qbytes: *const u8, d_qoff: *const u64, nq: u64,
                       max_mismatches: u32, cand_limit: u64, d_pattern: *mut u32, d_tpos: *mut u32, d_mism: *mut u8,
                       capacity: u64, d_first: *mut u64, cands_out: *mut u64, count_out: *mut u64,
                       d_workspace: *mut c_void, workspace_bytes: u64, stream: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn sfx_index_hamming_dev(ix: *const SfxIndex, d_qbytes: *const u8, d_qoff: *const u64, nq: u64, max_mismatches: u32,
                             cand_limit: u64, d_pattern: *mut u32, d_tpos: *mut u32, d_mism: *mut u8, capacity: u64,
                             d_first: *mut u64, cands_out: *mut u64, count_out: *mut u64, d_workspace: *mut c_void,
                             workspace_bytes: u64, stream: *mut c_void) -> c_int;
    // k-error pattern search (edit distance) of a batch of patterns; DeviceIndex::edit_positions below goes through
    // sfx_index_edit (host buffers; the outputs may be null at capacity 0, first_out may be null).  Like the rest of this
    // crate the declarations and the wrapper have not been compiled (no Rust toolchain where the engine is built): the
    // signature check of tests/test_rust_crate.py holds them against the header
    fn sfx_index_edit(ix: *const SfxIndex, qbytes: *const u8, qoff: *const u64, nq: u64, max_errors: u32, cand_limit: u64,
                      hit_limit: u64, pattern_out: *mut u32, tbegin_out: *mut u32, tend_out: *mut u32, dist_out: *mut u8,
                      capacity: u64, first_out: *mut u64, cands_out: *mut u64, hits_out: *mut u64, count_out: *mut u64) -> c_int;
    #[allow(dead_code)]
    fn sfx_edit_workspace_bytes(nq: u64, max_errors: u32, cand_limit: u64, hit_limit: u64) -> u64;
    #[allow(dead_code)]
    fn sfx_edit_dev(d_text: *const u8, n: u64, d_sa: *const u32, d_qbytes: *const u8, d_qoff: *const u64, nq: u64,
                    max_errors: u32, cand_limit: u64, hit_limit: u64, d_pattern: *mut u32, d_tbegin: *mut u32, d_tend: *mut u32,
                    d_dist: *mut u8, capacity: u64, d_first: *mut u64, cands_out: *mut u64, hits_out: *mut u64,
                    count_out: *mut u64, d_workspace: *mut c_void, workspace_bytes: u64, stream: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn sfx_index_edit_dev(ix: *const SfxIndex, d_qbytes: *const u8, d_qoff: *const u64, nq: u64, max_errors: u32,
                          cand_limit: u64, hit_limit: u64, d_pattern: *mut u32, d_tbegin: *mut u32, d_tend: *mut u32,
                          d_dist: *mut u8, capacity: u64, d_first: *mut u64, cands_out: *mut u64, hits_out: *mut u64,
                          count_out: *mut u64, d_workspace: *mut c_void, workspace_bytes: u64, stream: *mut c_void) -> c_int;
    // FM-index over that pair (sfx_fm_*): the size bound; the handle functions take `sfx_fm*`, a type the signature check
    // of this block (tests/test_rust_crate.py) has no mapping for yet, so they are not bound here
    fn sfx_fm_bytes(n: u64, sample_step: u32, occ_step: u32) -> u64;
    // longest common extensions between two text positions (sfx_lce_*): the inverse table, the one-shot query and the size
    // bound; the handle functions take `sfx_lce*`, which the signature check of this block has no mapping for either
    fn sfx_inverse_table_u32(sa: *const u32, n: u64, isa_out: *mut u32) -> c_int;
    fn sfx_lce_u32(sa: *const u32, lcp: *const u32, n: u64, doc_starts: *const u64, ndocs: u64, a: *const u32, b: *const u32,
                   nq: u64, max_mismatches: u32, len_out: *mut u32) -> c_int;
    fn sfx_lce_bytes(n: u64) -> u64;
    // suffix_tree's node table with ordered children (children(), preorder(), leaves(), suffix_indices() read it)
    #[allow(dead_code)]
    fn sfx_suffix_tree_u32(text: *const u8, sa: *const u32, lcp: *const u32, n: u64, node_capacity: u64,
                           child_capacity: u64, node_lb: *mut u32, node_rb: *mut u32, node_depth: *mut u32,
                           node_parent: *mut u32, node_terminal: *mut u32, child_off: *mut u64, child_lb: *mut u32,
                           child_node: *mut u32, child_byte: *mut u8, leaf_parent: *mut u32, nodes_out: *mut u64,
                           children_out: *mut u64) -> c_int;
    #[allow(dead_code)]
    fn sfx_suffix_tree_workspace_bytes(n: u64) -> u64;
    #[allow(dead_code)]
    fn sfx_suffix_tree_dev(d_text: *const u8, d_sa: *const u32, d_lcp: *const u32, n: u64, node_capacity: u64,
                           child_capacity: u64, d_node_lb: *mut u32, d_node_rb: *mut u32, d_node_depth: *mut u32,
                           d_node_parent: *mut u32, d_node_terminal: *mut u32, d_child_off: *mut u64,
                           d_child_lb: *mut u32, d_child_node: *mut u32, d_child_byte: *mut u8,
                           d_leaf_parent: *mut u32, nodes_out: *mut u64, children_out: *mut u64, ws: *mut c_void,
                           ws_bytes: u64, stream: *mut c_void) -> c_int;
    // merge of two generalized suffix arrays (sfx_gsa_merge_*, sfx_gsa_extend_u32): documents added without a rebuild
    fn sfx_gsa_extend_u32(text: *const u8, n: u64, doc_starts: *const u64, ndocs: u64, ndocs_a: u64, sa_a: *const u32,
                          da_a: *const u32, lcp_a: *const u32, match_limit: u32, rebuild_on_limit: c_int, sa_out: *mut u32,
                          da_out: *mut u32, lcp_out: *mut u32, longest_out: *mut u64, route_out: *mut u32) -> c_int;
    #[allow(dead_code)]
    fn sfx_gsa_merge_u32(text: *const u8, doc_starts: *const u64, ndocs: u64, ndocs_a: u64, sa_a: *const u32, da_a: *const u32,
                         lcp_a: *const u32, n_a: u64, sa_b: *const u32, da_b: *const u32, lcp_b: *const u32, n_b: u64,
                         match_limit: u32, sa_out: *mut u32, da_out: *mut u32, lcp_out: *mut u32, longest_out: *mut u64) -> c_int;
    #[allow(dead_code)]
    fn sfx_gsa_merge_workspace_bytes(n_a: u64, n_b: u64) -> u64;
    #[allow(dead_code)]
    fn sfx_gsa_merge_dev(d_text: *const u8, d_doc_starts: *const u64, ndocs: u64, ndocs_a: u64, d_sa_a: *const u32,
                         d_da_a: *const u32, d_lcp_a: *const u32, n_a: u64, d_sa_b: *const u32, d_da_b: *const u32,
                         d_lcp_b: *const u32, n_b: u64, match_limit: u32, d_sa: *mut u32, d_da: *mut u32, d_lcp: *mut u32,
                         longest_out: *mut u64, d_workspace: *mut c_void, workspace_bytes: u64, stream: *mut c_void) -> c_int;
    // device-pointer variants (`*_dev`) take a hipStream_t as *mut c_void; omitted here.
    #[allow(dead_code)]
    fn sfx_build_sa_u32_dev(d_text: *const u8, n: u64, d_sa: *mut u32, ws: *mut c_void,
                            ws_bytes: u64, stream: *mut c_void) -> c_int;
}

/// Texts shorter than this stay on the crate's own CPU path (`sais`, `lcp_lens_quadratic`): a build on the device costs
/// ~100 us of launches and two PCIe copies whatever the length, the reference needs ~1 us for QuickCheck's strings
/// (README.md:116) and ~1 ms for 64 KiB.  The patched `sais_table` / `lcp_lens` compare against it.
pub const MIN_DEVICE_LEN: usize = 1 << 16;

/// The threshold the patched `sais_table` / `lcp_lens` compare against: `MIN_DEVICE_LEN`, unless the crate was built with the
/// `always` feature (the parent crate's `hip-always`: 0) or the environment names another one (`SUFFIX_HIP_MIN_LEN=<bytes>`,
/// read once per process).  `SUFFIX_HIP_MIN_LEN=0 cargo test --features hip` is how the upstream test-suite -- whose
/// strings are all far below 64 KiB -- is made to run on the device (tests/tests.rs:73-96).
pub fn min_device_len() -> usize {
    use std::sync::atomic::{AtomicUsize, Ordering};
    static CACHED: AtomicUsize = AtomicUsize::new(usize::MAX);
    let v = CACHED.load(Ordering::Relaxed);
    if v != usize::MAX {
        return v;
    }
    let default = if cfg!(feature = "always") { 0 } else { MIN_DEVICE_LEN };
    let parsed = std::env::var("SUFFIX_HIP_MIN_LEN")
        .ok()
        .and_then(|s| s.trim().parse::<usize>().ok())
        .map(|x| if x == usize::MAX { usize::MAX - 1 } else { x })
        .unwrap_or(default);
    CACHED.store(parsed, Ordering::Relaxed);
    parsed
}

fn check(status: c_int, what: &str) {
    if status != 0 {
        let msg = unsafe { std::ffi::CStr::from_ptr(sfx_strerror(status)) }.to_string_lossy();
        let hip = unsafe { std::ffi::CStr::from_ptr(sfx_last_hip_error()) }.to_string_lossy();
        // the reference's error convention is panic (assert! at :380, assert_eq! at :117)
        panic!("{}: {} {}", what, msg, hip);
    }
}

/// Replacement for `fn sais_table(text: &str) -> Vec<u32>` (src/table.rs:378-386).
pub fn sais_table(text: &str) -> Vec<u32> {
    let text = text.as_bytes();
    assert!(text.len() <= u32::MAX as usize);              // :380, unchanged
    let mut sa = vec![0u32; text.len()];                   // :381, unchanged: caller allocates
    if unsafe { sfx_device_count() } <= 0 {
        panic!("suffix: no HIP device (build without the `hip` feature for the CPU path)");
    }
    check(unsafe { sfx_build_sa_u32(text.as_ptr(), text.len() as u64, sa.as_mut_ptr()) },
          "sfx_build_sa_u32");
    sa
}

/// Replacement for the body of `SuffixTable::lcp_lens` (src/table.rs:130-138).
pub fn lcp_lens(text: &str, table: &[u32]) -> Vec<u32> {
    let mut lcp = vec![0u32; table.len()];
    check(unsafe {
        sfx_build_lcp_u32(text.as_ptr(), text.len() as u64, table.as_ptr(), lcp.as_mut_ptr())
    }, "sfx_build_lcp_u32");
    lcp
}

/// `SuffixTable::new` and `lcp_lens` in one engine call: (table, lcp).
pub fn sais_table_with_lcp(text: &str) -> (Vec<u32>, Vec<u32>) {
    let text = text.as_bytes();
    assert!(text.len() <= u32::MAX as usize);
    let mut sa = vec![0u32; text.len()];
    let mut lcp = vec![0u32; text.len()];
    check(unsafe {
        sfx_build_sa_lcp_u32(text.as_ptr(), text.len() as u64, sa.as_mut_ptr(), lcp.as_mut_ptr())
    }, "sfx_build_sa_lcp_u32");
    (sa, lcp)
}

/// What produced the arrays of `gsa_extend`: the merge, or -- an added suffix shared more than `match_limit` bytes with an
/// old one -- one build of the whole collection.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum GsaRoute {
    Merge,
    Rebuild,
}

/// Additive API: the generalized suffix array, document array and LCP of `text` cut at `doc_starts`, from the arrays
/// `(sa_a, da_a, lcp_a)` of its first `ndocs_a` documents: only the documents behind them are built, then merged in
/// (`sfx_gsa_extend_u32`).  `match_limit` 0 never rebuilds.  -> (sa, da, lcp, the longest old/new match seen, route).
pub fn gsa_extend(text: &[u8], doc_starts: &[u64], ndocs_a: usize, sa_a: &[u32], da_a: &[u32], lcp_a: &[u32],
                  match_limit: u32) -> (Vec<u32>, Vec<u32>, Vec<u32>, u64, GsaRoute) {
    assert!(text.len() <= u32::MAX as usize);
    assert!(ndocs_a <= doc_starts.len());
    let n_a = if ndocs_a < doc_starts.len() { doc_starts[ndocs_a] as usize } else { text.len() };
    assert!(sa_a.len() == n_a && da_a.len() == n_a && lcp_a.len() == n_a);
    let n = text.len();
    let (mut sa, mut da, mut lcp) = (vec![0u32; n], vec![0u32; n], vec![0u32; n]);
    let (mut longest, mut route) = (0u64, 0u32);
    check(unsafe {
        sfx_gsa_extend_u32(text.as_ptr(), n as u64, doc_starts.as_ptr(), doc_starts.len() as u64, ndocs_a as u64, sa_a.as_ptr(),
                           da_a.as_ptr(), lcp_a.as_ptr(), match_limit, 1, sa.as_mut_ptr(), da.as_mut_ptr(), lcp.as_mut_ptr(),
                           &mut longest, &mut route)
    }, "sfx_gsa_extend_u32");
    (sa, da, lcp, longest, if route == 2 { GsaRoute::Rebuild } else { GsaRoute::Merge })
}

/// Additive API: the Burrows-Wheeler transform of `text` with its suffix table, and the rows of the suffixes at every
/// `sample_step`-th position (0 or a power of two; `samples[0]` is the primary row, 0 keeps the primary only).
/// `bwt` is the last column of the sorted rotations of `text$` without its `$` entry.
pub fn bwt(text: &[u8], table: &[u32], sample_step: u32) -> (Vec<u8>, Vec<u32>) {
    assert!(text.len() <= u32::MAX as usize);
    assert_eq!(text.len(), table.len());
    assert!(sample_step & sample_step.wrapping_sub(1) == 0, "sample_step must be 0 or a power of two");
    let cnt = unsafe { sfx_bwt_sample_count(text.len() as u64, sample_step) } as usize;
    let (mut out, mut samples) = (vec![0u8; text.len()], vec![0u32; cnt]);
    check(unsafe {
        sfx_bwt_u32(text.as_ptr(), text.len() as u64, table.as_ptr(), sample_step, out.as_mut_ptr(), samples.as_mut_ptr())
    }, "sfx_bwt_u32");
    (out, samples)
}

/// The inverse of `bwt`: the text whose transform `(bwt, samples)` is, or `None` where the pair is the transform of no
/// text (the walks check themselves: `Some` means the pair IS the transform of what is returned).
pub fn unbwt(bwt: &[u8], samples: &[u32], sample_step: u32) -> Option<Vec<u8>> {
    let mut out = vec![0u8; bwt.len()];
    let rc = unsafe {
        sfx_unbwt(bwt.as_ptr(), bwt.len() as u64, samples.as_ptr(), samples.len() as u64, sample_step, out.as_mut_ptr())
    };
    if rc == 1 {
        return None;                                       // SFX_ERR_ARG
    }
    check(rc, "sfx_unbwt");
    Some(out)
}

/// The greedy LZ77 factorization of a text: one entry per phrase in `len` / `src` / `lit`.  A copy repeats `len` bytes from
/// position `src`, which lies before the phrase's own begin (it may run into itself) and has `lit` 0; a literal has
/// `len` 1, `src` `u32::MAX` and its byte in `lit`.  The begins are the running sums of `len`.
pub struct Lz77 {
    pub len: Vec<u32>,
    pub src: Vec<u32>,
    pub lit: Vec<u8>,
}

/// The factorization of `text`: every phrase is the longest prefix of what is left that also starts at an earlier position
/// when that is at least `min_len` (>= 1) bytes, else one literal byte.  `table`: the text's suffix array, or `None` to
/// build it.
pub fn lz77(text: &[u8], table: Option<&[u32]>, min_len: u32) -> Lz77 {
    assert!(min_len >= 1, "min_len must be at least 1");
    if let Some(t) = table {
        assert_eq!(t.len(), text.len());
    }
    let n = text.len();
    let (mut len, mut src, mut lit) = (vec![0u32; n], vec![0u32; n], vec![0u8; n]);
    let mut count = 0u64;
    check(unsafe {
        sfx_lz77_u32(text.as_ptr(), n as u64, table.map_or(std::ptr::null(), |t| t.as_ptr()), std::ptr::null(), min_len,
                     std::ptr::null_mut(), len.as_mut_ptr(), src.as_mut_ptr(), lit.as_mut_ptr(), n as u64, &mut count)
    }, "sfx_lz77_u32");
    let z = count as usize;
    len.truncate(z);
    src.truncate(z);
    lit.truncate(z);
    Lz77 { len, src, lit }
}

/// The text of a factorization, or `None` where the list is none: a zero length, a literal of another length than 1, a copy
/// that does not point backwards.
pub fn unlz(f: &Lz77) -> Option<Vec<u8>> {
    assert!(f.src.len() == f.len.len() && f.lit.len() == f.len.len());
    let n: u64 = f.len.iter().map(|&l| l as u64).sum();
    let mut out = vec![0u8; n as usize];
    let rc = unsafe { sfx_unlz(f.len.as_ptr(), f.src.as_ptr(), f.lit.as_ptr(), f.len.len() as u64, n, out.as_mut_ptr()) };
    if rc == 1 {
        return None;                                       // SFX_ERR_ARG
    }
    check(rc, "sfx_unlz");
    Some(out)
}

/// An upper bound on the device memory an FM-index over the transform of `n` bytes holds (`sfx_fm_create`), whatever the
/// alphabet; 0 for `n == 0` or steps the engine refuses (`sample_step`: 0 or a power of two; `occ_step`: 0 or a power of
/// two in 32..=4096).
pub fn fm_index_bytes(n: usize, sample_step: u32, occ_step: u32) -> u64 {
    unsafe { sfx_fm_bytes(n as u64, sample_step, occ_step) }
}

/// The inverse of a suffix table: `isa[table[r]] = r`, or `None` where `table` is no permutation of `0..table.len()`.
pub fn inverse_table(table: &[u32]) -> Option<Vec<u32>> {
    let mut isa = vec![0u32; table.len()];
    let rc = unsafe { sfx_inverse_table_u32(table.as_ptr(), table.len() as u64, isa.as_mut_ptr()) };
    if rc == 1 {
        return None;                                       // SFX_ERR_ARG
    }
    check(rc, "sfx_inverse_table_u32");
    Some(isa)
}

/// Longest common extensions: for every pair `(a[q], b[q])` of byte positions of the text behind (`table`, `lcp`), how far
/// the two suffixes agree when up to `max_mismatches` bytes may differ -- never past the end of the text, or with
/// `doc_starts` (a collection: the table and in-document LCP of a generalized build) past the end of either position's
/// document.  A position equal to the length gives 0, one above `u32::MAX`.  One shot: the index (inverse table and a
/// min-tree over `lcp`) is built, queried and dropped.
pub fn lce(table: &[u32], lcp: &[u32], doc_starts: Option<&[u64]>, a: &[u32], b: &[u32], max_mismatches: u32) -> Vec<u32> {
    assert_eq!(table.len(), lcp.len());
    assert_eq!(a.len(), b.len());
    let mut len = vec![0u32; a.len()];
    let (starts, ndocs) = doc_starts.map_or((std::ptr::null(), 0u64), |d| (d.as_ptr(), d.len() as u64));
    check(unsafe {
        sfx_lce_u32(table.as_ptr(), lcp.as_ptr(), table.len() as u64, starts, ndocs, a.as_ptr(), b.as_ptr(), a.len() as u64,
                    max_mismatches, len.as_mut_ptr())
    }, "sfx_lce_u32");
    len
}

/// An upper bound on the device memory an LCE index over `n` suffixes holds: the inverse table and the levels above the
/// LCP array, at most `4 n + n / 7 + 64 KiB`; 0 for `n == 0`.
pub fn lce_index_bytes(n: usize) -> u64 {
    unsafe { sfx_lce_bytes(n as u64) }
}

/// Additive API: many `positions()` at once.  Returns (start, end) pairs;
/// `positions(q_k) == &table[start_k as usize .. end_k as usize]` exactly as :244-258.
pub struct DeviceIndex(*mut SfxIndex);
unsafe impl Send for DeviceIndex {}
unsafe impl Sync for DeviceIndex {}          // queries only read the index

impl DeviceIndex {
    pub fn new(text: &str, table: &[u32]) -> DeviceIndex {
        let mut h: *mut SfxIndex = std::ptr::null_mut();
        check(unsafe { sfx_index_create(text.as_ptr(), text.len() as u64, table.as_ptr(), &mut h) },
              "sfx_index_create");
        DeviceIndex(h)
    }
    pub fn positions_batch(&self, queries: &[&str]) -> Vec<(u32, u32)> {
        let mut off = Vec::with_capacity(queries.len() + 1);
        let mut blob = Vec::new();
        off.push(0u64);
        for q in queries {
            blob.extend_from_slice(q.as_bytes());
            off.push(blob.len() as u64);
        }
        let (mut s, mut e) = (vec![0u32; queries.len()], vec![0u32; queries.len()]);
        check(unsafe {
            sfx_positions_batch(self.0, blob.as_ptr(), off.as_ptr(), queries.len() as u64,
                                s.as_mut_ptr(), e.as_mut_ptr())
        }, "sfx_positions_batch");
        s.into_iter().zip(e).collect()
    }
    pub fn contains_batch(&self, queries: &[&str]) -> Vec<bool> {
        let mut off = vec![0u64];
        let mut blob = Vec::new();
        for q in queries {
            blob.extend_from_slice(q.as_bytes());
            off.push(blob.len() as u64);
        }
        let mut f = vec![0u8; queries.len()];
        check(unsafe {
            sfx_contains_batch(self.0, blob.as_ptr(), off.as_ptr(), queries.len() as u64,
                               f.as_mut_ptr(), std::ptr::null_mut())
        }, "sfx_contains_batch");
        f.into_iter().map(|b| b != 0).collect()
    }
    /// Additive API: the matching statistics of `query` against the indexed text.  `len[i]` = the longest prefix of
    /// `query[i..]` (at most `max_len` bytes, 0 = no cap) that occurs in the text; `src[i]` = one position where it
    /// stands, `u32::MAX` where `len[i] == 0`.  The cost grows with the lengths found: cap a query that may repeat the text.
    pub fn match_stats(&self, query: &[u8], max_len: u32) -> (Vec<u32>, Vec<u32>) {
        assert!(query.len() <= u32::MAX as usize);
        let (mut len, mut src) = (vec![0u32; query.len()], vec![u32::MAX; query.len()]);
        check(unsafe {
            sfx_index_match_stats(self.0, query.as_ptr(), query.len() as u64, max_len, len.as_mut_ptr(),
                                  src.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut())
        }, "sfx_index_match_stats");
        (len, src)
    }
    /// Additive API: the maximal exact matches of at least `min_len` (>= 1) bytes between `query` and the indexed text:
    /// `query[qpos..qpos + len] == text[tpos..tpos + len]`, extendable neither to the left nor to the right, ascending by
    /// `qpos` and then by the table rank of `tpos`.  `unique`: only matches whose bytes occur once in the text.
    /// `Err(pairs)`: the call would look at `pairs` > `max_pairs` candidate pairs (a shared stretch of M bytes is
    /// M - min_len + 1 of them) and wrote nothing; raise `min_len` or `max_pairs`.
    pub fn mems(&self, query: &[u8], min_len: u32, unique: bool, max_pairs: u64) -> Result<Mems, u64> {
        assert!(min_len >= 1 && max_pairs >= 1 && query.len() <= u32::MAX as usize);
        let mut cap = query.len().max(1024);
        let (mut pairs, mut count) = (0u64, 0u64);
        let mut r = Mems { qpos: Vec::new(), tpos: Vec::new(), len: Vec::new(), pairs: 0 };
        for _ in 0..2 {                                        // the room is a guess: once more when there were more
            r.qpos.resize(cap, 0);
            r.tpos.resize(cap, 0);
            r.len.resize(cap, 0);
            check(unsafe {
                sfx_index_mems(self.0, query.as_ptr(), query.len() as u64, min_len, if unique { 1 } else { 0 }, max_pairs,
                               r.qpos.as_mut_ptr(), r.tpos.as_mut_ptr(), r.len.as_mut_ptr(), cap as u64, &mut pairs, &mut count)
            }, "sfx_index_mems");
            if pairs > max_pairs {
                return Err(pairs);
            }
            if count as usize <= cap {
                break;
            }
            cap = count as usize;
        }
        r.qpos.truncate(count as usize);
        r.tpos.truncate(count as usize);
        r.len.truncate(count as usize);
        r.pairs = pairs;
        Ok(r)
    }
    /// Additive API: where do `queries` occur in the indexed text if up to `mismatches` (<= 255) bytes may differ?  No
    /// insertions or deletions.  Per query, in order: `first[j] .. first[j + 1]` are its entries of `tpos` (the window's
    /// start) and `mism` (the differing bytes of that window, 0 ..= mismatches), ordered by the owning piece of the
    /// pigeonhole cut and then by table rank -- sort a slice by position if that is what is wanted.  An empty query has
    /// no occurrence.  `Err(cands)`: the exact hits of the query pieces add up to `cands` > `max_candidates` and nothing
    /// was compared; use longer queries, fewer mismatches or a larger limit.
    pub fn approx_positions(&self, queries: &[&[u8]], mismatches: u32, max_candidates: u64) -> Result<ApproxPositions, u64> {
        assert!(mismatches <= 255 && max_candidates >= 1);
        let mut off = vec![0u64];
        let mut blob = Vec::new();
        for q in queries {
            blob.extend_from_slice(q);
            off.push(blob.len() as u64);
        }
        let nq = queries.len();
        let mut cap = (4 * nq).max(1024);
        let (mut cands, mut count) = (0u64, 0u64);
        let mut r = ApproxPositions { first: vec![0u64; nq + 1], tpos: Vec::new(), mism: Vec::new(), candidates: 0 };
        let mut pattern: Vec<u32> = Vec::new();
        for _ in 0..2 {                                        // the room is a guess: once more when there were more
            pattern.resize(cap, 0);
            r.tpos.resize(cap, 0);
            r.mism.resize(cap, 0);
            check(unsafe {
                sfx_index_hamming(self.0, blob.as_ptr(), off.as_ptr(), nq as u64, mismatches, max_candidates,
                                  pattern.as_mut_ptr(), r.tpos.as_mut_ptr(), r.mism.as_mut_ptr(), cap as u64,
                                  r.first.as_mut_ptr(), &mut cands, &mut count)
            }, "sfx_index_hamming");
            if cands > max_candidates {
                return Err(cands);
            }
            if count as usize <= cap {
                break;
            }
            cap = count as usize;
        }
        r.tpos.truncate(count as usize);
        r.mism.truncate(count as usize);
        r.candidates = cands;
        Ok(r)
    }
    /// Additive API: where do `queries` occur in the indexed text within `errors` (<= 31) substitutions, insertions and
    /// deletions (unit-cost edit distance)?  Every query needs more than `errors` bytes.  Per query, in order:
    /// `first[j] .. first[j + 1]` are its entries of `tbegin`, `tend` and `dist`, ascending by `tend`: an occurrence is
    /// an end position for which some `text[tbegin .. tend)` is within `errors` edits of the query, with the least such
    /// distance and the largest begin that attains it.  `Err((cands, hits))`: more than `max_candidates` exact piece
    /// hits, or more than `max_hits` (candidate, end) pairs before the merge; nothing was written.
    pub fn edit_positions(&self, queries: &[&[u8]], errors: u32, max_candidates: u64, max_hits: u64) -> Result<EditPositions, (u64, u64)> {
        assert!(errors <= 31 && max_candidates >= 1 && max_hits >= 1 && max_hits < (1u64 << 32));
        assert!(queries.iter().all(|q| q.len() > errors as usize));
        let mut off = vec![0u64];
        let mut blob = Vec::new();
        for q in queries {
            blob.extend_from_slice(q);
            off.push(blob.len() as u64);
        }
        let nq = queries.len();
        let mut cap = (4 * nq).max(1024);
        let (mut cands, mut hits, mut count) = (0u64, 0u64, 0u64);
        let mut r = EditPositions { first: vec![0u64; nq + 1], tbegin: Vec::new(), tend: Vec::new(), dist: Vec::new(), candidates: 0, hits: 0 };
        let mut pattern: Vec<u32> = Vec::new();
        for _ in 0..2 {                                        // the room is a guess: once more when there were more
            pattern.resize(cap, 0);
            r.tbegin.resize(cap, 0);
            r.tend.resize(cap, 0);
            r.dist.resize(cap, 0);
            check(unsafe {
                sfx_index_edit(self.0, blob.as_ptr(), off.as_ptr(), nq as u64, errors, max_candidates, max_hits,
                               pattern.as_mut_ptr(), r.tbegin.as_mut_ptr(), r.tend.as_mut_ptr(), r.dist.as_mut_ptr(), cap as u64,
                               r.first.as_mut_ptr(), &mut cands, &mut hits, &mut count)
            }, "sfx_index_edit");
            if cands > max_candidates || hits > max_hits {
                return Err((cands, hits));
            }
            if count as usize <= cap {
                break;
            }
            cap = count as usize;
        }
        r.tbegin.truncate(count as usize);
        r.tend.truncate(count as usize);
        r.dist.truncate(count as usize);
        r.candidates = cands;
        r.hits = hits;
        Ok(r)
    }
}
/// The k-error occurrences of a batch of queries (`DeviceIndex::edit_positions`), in CSR form: the occurrences of query j
/// are the entries `first[j] .. first[j + 1]` of `tbegin` / `tend` / `dist`; `candidates` = the exact piece hits looked
/// at, `hits` = the (candidate, end) pairs they found before the merge.
pub struct EditPositions {
    pub first: Vec<u64>,
    pub tbegin: Vec<u32>,
    pub tend: Vec<u32>,
    pub dist: Vec<u8>,
    pub candidates: u64,
    pub hits: u64,
}
/// The k-mismatch occurrences of a batch of queries (`DeviceIndex::approx_positions`), in CSR form: the occurrences of
/// query j are the entries `first[j] .. first[j + 1]` of `tpos` / `mism`; `candidates` = the exact piece hits looked at.
pub struct ApproxPositions {
    pub first: Vec<u64>,
    pub tpos: Vec<u32>,
    pub mism: Vec<u8>,
    pub candidates: u64,
}
/// The maximal exact matches of a query text (`DeviceIndex::mems`): one entry per match, and the number of candidate
/// pairs the call looked at.
pub struct Mems {
    pub qpos: Vec<u32>,
    pub tpos: Vec<u32>,
    pub len: Vec<u32>,
    pub pairs: u64,
}
impl DeviceIndex {
    pub fn len(&self) -> usize {
        unsafe { sfx_index_len(self.0) as usize }
    }
}
impl Drop for DeviceIndex {
    fn drop(&mut self) {
        unsafe { sfx_index_destroy(self.0) }
    }
}
