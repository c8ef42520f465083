// sfx_api.hip -- the extern "C" boundary (include/suffix_hip.h): argument
// checking, host<->HBM staging for the host-pointer entry points, the
// device-resident index handle, error text and the event profiler.
#include <stdio.h>
#include <string.h>

#include <pthread.h>

#include <atomic>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "sfx_host.hpp"
#include "sfx_fm.hip"   // the FM-index: kernels and host side, one translation unit with its entry points below
#include "sfx_lz.hip"   // LZ77 factorization and its decoder, likewise
#include "sfx_mem.hip"  // maximal exact matches, likewise
#include "sfx_hamming.hip"  // k-mismatch pattern search, likewise (over sfx_mem.hip's expansion)
#include "sfx_edit.hip"  // k-error (edit distance) pattern search, likewise (over sfx_hamming.hip's pieces)
#include "sfx_lce.hip"  // longest common extensions (inverse table + LCP min-tree), likewise
#include "sfx_nav.hip"  // suffix-tree navigation: substring loci, LCA, argmin, suffix links, likewise (over sfx_lce.hip's handle)
#include "sfx_runs.hip"  // Lyndon arrays and maximal repetitions (runs) of a plain text, likewise (over sfx_lce.hip's tables)
#include "sfx_docs.hip"  // document counts per lcp-interval and k-common substrings, likewise (over sfx_lce.hip's levels)
#include "sfx_doclist.hip"  // document listing with term frequencies and top-k, likewise
#include "sfx_gsamerge.hip"  // merge of two generalized suffix arrays, likewise

namespace sfx {

// ---- error capture ---------------------------------------------------------------
static thread_local char tls_hip_error[512] = "";

void note_hip_error(hipError_t e, const char* what, const char* file, int line)
{
    snprintf(tls_hip_error, sizeof(tls_hip_error), "%s (%d) at %s:%d in `%s`", hipGetErrorString(e),
             (int)e, file, line, what);
}

sfx_build_stats& tls_build_stats()
{
    static thread_local sfx_build_stats s;
    return s;
}

// ---- profiler ---------------------------------------------------------------------
struct ProfRecord {
    const char* name;
    double bytes;
    hipEvent_t a, b;
};
static bool g_profile = false;
static std::mutex g_prof_mu;
static std::vector<ProfRecord> g_prof_open;      // recorded, not yet folded
struct ProfStat { std::string name; uint64_t launches; double ms, bytes; };
static std::vector<ProfStat> g_prof_stats;

bool profile_on() { return g_profile; }

void profile_begin(const char* name, hipStream_t st, double algo_bytes)
{
    ProfRecord r;
    r.name = name;
    r.bytes = algo_bytes;
    if (event_create(&r.a) != hipSuccess || event_create(&r.b) != hipSuccess) return;
    (void)hipEventRecord(r.a, st);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_open.push_back(r);
}
void profile_end(hipStream_t st)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (!g_prof_open.empty()) (void)hipEventRecord(g_prof_open.back().b, st);
}
static void profile_fold()
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (ProfRecord& r : g_prof_open) {
        float ms = 0.f;
        (void)hipEventSynchronize(r.b);
        (void)hipEventElapsedTime(&ms, r.a, r.b);
        (void)event_destroy(r.a);
        (void)event_destroy(r.b);
        ProfStat* s = nullptr;
        for (ProfStat& t : g_prof_stats) if (t.name == r.name) { s = &t; break; }
        if (!s) { g_prof_stats.push_back(ProfStat{r.name, 0, 0.0, 0.0}); s = &g_prof_stats.back(); }
        s->launches++;
        s->ms += ms;
        s->bytes += r.bytes;
    }
    g_prof_open.clear();
}

// ---- resource ledger (sfx_host.hpp's wrappers; sfx_resource_stats) ---------------------------------
struct ResCounters {
    std::atomic<uint64_t> device_bytes{0}, device_allocs{0}, pinned_bytes{0}, pinned_allocs{0}, streams{0}, events{0}, device_allocs_total{0};
};
static ResCounters g_res;
// pointer -> bytes of what is live (device and pinned alike: their addresses never coincide).  Never destroyed: a thread
// that ends while the process exits may still return its buffers.
static std::mutex& res_mu() { static std::mutex* m = new std::mutex; return *m; }
static std::unordered_map<void*, uint64_t>& res_sizes() { static auto* t = new std::unordered_map<void*, uint64_t>; return *t; }
namespace res {
void note_alloc(void* p, uint64_t bytes, bool pinned)
{
    { std::lock_guard<std::mutex> lk(res_mu()); res_sizes()[p] = bytes; }
    (pinned ? g_res.pinned_bytes : g_res.device_bytes).fetch_add(bytes, std::memory_order_relaxed);
    (pinned ? g_res.pinned_allocs : g_res.device_allocs).fetch_add(1, std::memory_order_relaxed);
    if (!pinned) g_res.device_allocs_total.fetch_add(1, std::memory_order_relaxed);
}
void note_free(void* p, bool pinned)
{
    uint64_t bytes = 0;
    {
        std::lock_guard<std::mutex> lk(res_mu());
        auto it = res_sizes().find(p);
        if (it == res_sizes().end()) return;          // (not ours: nothing to take off)
        bytes = it->second;
        res_sizes().erase(it);
    }
    (pinned ? g_res.pinned_bytes : g_res.device_bytes).fetch_sub(bytes, std::memory_order_relaxed);
    (pinned ? g_res.pinned_allocs : g_res.device_allocs).fetch_sub(1, std::memory_order_relaxed);
}
void note_stream(int delta) { g_res.streams.fetch_add((uint64_t)(int64_t)delta, std::memory_order_relaxed); }
void note_event(int delta) { g_res.events.fetch_add((uint64_t)(int64_t)delta, std::memory_order_relaxed); }
}  // namespace res

// ---- per-thread state (sfx_host.hpp: ThreadRes) -----------------------------------------------------
void ThreadRes::release_scratch()
{
    for (QueryScratch& sc : scratch) {
        if (sc.p) {
            if (sc.used) (void)hipEventSynchronize(sc.done);
            (void)dev_free(sc.p);
        }
        if (sc.done) (void)event_destroy(sc.done);
        sc = QueryScratch();
    }
}
ThreadRes::~ThreadRes()
{
    release_scratch();
    // (every host-pointer call drains its stream before it returns: nothing is queued on these)
    for (hipStream_t st : stream) if (st) (void)stream_destroy(st);
    if (stage) (void)pinned_free(stage);
}
static pthread_key_t g_thread_res_key;
static std::once_flag g_thread_res_once;
ThreadRes& thread_res()
{
    thread_local ThreadRes* t = nullptr;             // (a plain pointer: no destructor of its own, the key's gives the record back)
    if (!t) {
        std::call_once(g_thread_res_once, [] { (void)pthread_key_create(&g_thread_res_key, [](void* v) { delete static_cast<ThreadRes*>(v); }); });
        t = new ThreadRes();
        (void)pthread_setspecific(g_thread_res_key, t);
    }
    return *t;
}

// ---- device buffers of the host-pointer entry points ----------------------------------
// A small mutex-guarded pool ("workspace from a mutex-guarded pool"): a buffer
// released by one call is handed to the next call on the same device that asks for at most
// that size and at least half of it, so a loop of SuffixTable::new over similar texts does
// not pay hipMalloc/hipFree of ~50 n bytes every time.  At most kPoolMaxBuffers buffers
// are kept; sfx_release_cached_buffers() returns them to the driver.
struct PooledBuf { void* p; uint64_t bytes; int device; };
static std::mutex g_pool_mu;
static std::vector<PooledBuf> g_pool;
constexpr size_t kPoolMaxBuffers = 8;

static void* pool_take(uint64_t bytes, int device, uint64_t* got_bytes)
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    size_t best = g_pool.size();
    for (size_t i = 0; i < g_pool.size(); i++) {
        const PooledBuf& b = g_pool[i];
        if (b.device == device && b.bytes >= bytes && b.bytes / 2 <= bytes &&
            (best == g_pool.size() || b.bytes < g_pool[best].bytes))
            best = i;
    }
    if (best == g_pool.size()) return nullptr;
    void* p = g_pool[best].p;
    *got_bytes = g_pool[best].bytes;
    g_pool.erase(g_pool.begin() + (long)best);
    return p;
}
static void pool_give(void* p, uint64_t bytes, int device)
{
    void* evict = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        g_pool.push_back(PooledBuf{p, bytes, device});
        if (g_pool.size() > kPoolMaxBuffers) {                 // drop the oldest
            evict = g_pool.front().p;
            g_pool.erase(g_pool.begin());
        }
    }
    if (evict) (void)dev_free(evict);
}

struct DevBuf {
    void* p = nullptr;
    uint64_t bytes = 0;
    int device = 0;
    ~DevBuf() { release(); }
    int alloc(uint64_t want)
    {
        if (want == 0) want = 1;
        (void)hipGetDevice(&device);
        p = pool_take(want, device, &bytes);
        if (p) return SFX_OK;
        hipError_t e = dev_malloc(&p, want);
        if (e != hipSuccess) {
            // the pool may be what is in the way: give everything back and retry once
            sfx_release_cached_buffers();
            e = dev_malloc(&p, want);
        }
        if (e != hipSuccess) { note_hip_error(e, "hipMalloc", __FILE__, __LINE__); p = nullptr; return SFX_ERR_HIP; }
        bytes = want;
        return SFX_OK;
    }
    void release()
    {
        if (p) pool_give(p, bytes, device);
        p = nullptr;
    }
};

// Stream of the host-pointer entry points: one non-blocking stream per calling thread, created on first
// use, so that SuffixTable::new from several threads runs concurrently on the device instead of
// serialising on the NULL stream ("per-call stream").  nullptr if creation fails.
// A stream belongs to the device that was current when it was made: one per (thread, device), looked up by the
// device current NOW (suffix_amd/device.py switches devices per call).
// -1: the ordinal does not fit the per-device tables (or cannot be told): such a call runs on the NULL stream and without
// cached scratch -- never on a stream, event or buffer that was made on another device
static int current_device()
{
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return (d >= 0 && d < kMaxDevices) ? d : -1;
}
static hipStream_t call_stream()
{
    const int d = current_device();
    if (d < 0) return nullptr;
    ThreadRes& t = thread_res();
    if (!t.stream_tried[d]) {
        t.stream_tried[d] = true;
        if (stream_create(&t.stream[d], hipStreamNonBlocking) != hipSuccess) {
            t.stream[d] = nullptr;
            (void)hipGetLastError();
        }
    }
    return t.stream[d];
}
// pooled device buffers must not go back to the pool while work that uses them may still be queued
struct StreamDrain {
    hipStream_t st;
    ~StreamDrain() { (void)hipStreamSynchronize(st); }
};

static int check_device()
{
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return SFX_ERR_NO_DEVICE;
    return SFX_OK;
}

// ---- the alignment contract of the *_dev entry points (include/suffix_hip.h) --------------------
// Checked on the host before anything is launched.  NULL passes: what NULL means is each entry point's own business.
// What the kernels do on caller pointers beyond element-wide accesses, and why the contract covers it:
//  - text / query bytes: 16-byte loads only behind a test of the address (k_byte_hist's head / vector / tail split,
//    k_byte_presence, k_bigram_hist, k_key_hist_raw's vec_ok, k_tiny_sa's LDS fill; prepare_text picks k_pack_text_pow2 only
//    for a 16-byte aligned text) -- and the 8-byte loads at byte addresses of extend_match and the query comparisons, plain
//    global loads that the hardware serves from any address and that every GPU run has always relied on;
//  - uint32_t arrays: the fused LCP moves d_lcp 16 bytes at a time (k_groups_reduce writes it, k_lcp_pending reads it), so
//    build_sa_lcp_u32_dev fuses only into an array on a 16-byte boundary and otherwise runs the separate LCP routine, which
//    goes entry by entry; k_groups_apply reads the table 16 bytes at a time behind a test of its address;
//  - uint64_t arrays and workspaces see 64-bit atomics: 8 / SFX_WORKSPACE_ALIGN bytes are required, never assumed.
template <class... P> static bool aligned_to(uintptr_t a, P... p)
{
    return ((... | reinterpret_cast<uintptr_t>(static_cast<const void*>(p))) & (a - 1)) == 0;
}
#define SFX_NEED_U32(...) do { if (!::sfx::aligned_to(4, __VA_ARGS__)) return SFX_ERR_ARG; } while (0)
#define SFX_NEED_U64(...) do { if (!::sfx::aligned_to(8, __VA_ARGS__)) return SFX_ERR_ARG; } while (0)
// a workspace that is large enough but off the boundary is an argument error; a short or missing one stays
// SFX_ERR_WORKSPACE wherever it lies (the entry point's own check)
#define SFX_NEED_WS(p, have, need) \
    do { if ((p) && (have) >= (need) && !::sfx::aligned_to(SFX_WORKSPACE_ALIGN, p)) return SFX_ERR_ARG; } while (0)

}  // namespace sfx

using namespace sfx;

struct sfx_index {
    uint8_t* d_text = nullptr;
    uint32_t* d_sa = nullptr;
    uint64_t n = 0;
    bool owns_arrays = true;        // false: created over the caller's device arrays (sfx_index_create_dev)
    // bucket directory (sfx_query.hip): first k symbols of a query -> its stretch of the suffix array
    uint32_t* d_dir = nullptr;
    uint16_t* d_lut = nullptr;      // 256 entries: byte -> symbol code + 1, 0 = byte absent from the text
    int bits = 0, k = 0, dbits = 0;
    uint64_t entries = 0;
    // prefix-key B+tree (sfx_query.hip): 8.6 n bytes; when it cannot be allocated the directory alone serves
    uint64_t* d_tree = nullptr;
    uint64_t tree_off[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int tree_levels = 0;
};

struct sfx_gindex {
    const uint8_t* d_text = nullptr;
    const uint64_t* d_starts = nullptr;
    const uint32_t* d_sa = nullptr;
    const uint32_t* d_da = nullptr;
    uint64_t n = 0, ndocs = 0;
    uint32_t* d_prev = nullptr;     // previous rank of the same document (owned)
    void* own[4] = {nullptr, nullptr, nullptr, nullptr};   // sfx_gindex_create: the copies of text, starts, sa, da
    // per-batch scratch of the document counts, reused across calls: the stream of a batch waits for the previous one
    std::mutex mu;
    void* scratch = nullptr;
    uint64_t scratch_bytes = 0;
    hipEvent_t done = nullptr;
    bool used = false;
};

namespace sfx {
// alphabet -> dense codes, directory shape, device build; SFX_ERR_ARG if the table holds an entry >= n
static int index_build_directory(sfx_index* ix, hipStream_t st)
{
    if (ix->n == 0) return SFX_OK;
    void* small = nullptr;
    SFX_HIP(dev_malloc(&small, 4096));
    unsigned long long bins[256];
    int rc = byte_presence_host(ix->d_text, ix->n, small, bins, st);
    (void)dev_free(small);
    if (rc != SFX_OK) return rc;
    uint16_t lut[256];
    unsigned sigma = 0;
    for (int c = 0; c < 256; c++) lut[c] = bins[c] ? (uint16_t)(++sigma) : (uint16_t)0;
    ix->bits = bits_for(sigma > 1 ? sigma - 1 : 1);
    SFX_TRY(dir_shape(ix->n, ix->bits, &ix->k, &ix->dbits, &ix->entries));
    SFX_HIP(dev_malloc((void**)&ix->d_dir, ix->entries * sizeof(uint32_t)));
    SFX_HIP(dev_malloc((void**)&ix->d_lut, 256 * sizeof(uint16_t)));
    uint32_t* scratch = nullptr;
    SFX_HIP(dev_malloc((void**)&scratch, (dir_scratch_words(ix->entries) + 2) * sizeof(uint32_t)));
    uint64_t bad = 0;
    rc = dir_build_dev(ix->d_text, ix->n, ix->d_sa, lut, ix->bits, ix->k, ix->dbits, ix->entries, ix->d_lut, ix->d_dir, scratch, st, &bad);
    (void)dev_free(scratch);
    if (rc != SFX_OK) return rc;
    if (bad) return SFX_ERR_ARG;
    // SFX_INDEX_TREE=0 (development): directory only
    static const bool want_tree = [] { const char* e = dev_env("SFX_INDEX_TREE"); return !e || atoi(e) != 0; }();
    if (want_tree && dev_malloc((void**)&ix->d_tree, key_tree_words(ix->n) * sizeof(uint64_t)) == hipSuccess) {
        rc = key_tree_build_dev(ix->d_text, ix->n, ix->d_sa, ix->d_tree, ix->tree_off, &ix->tree_levels, st);
        if (rc != SFX_OK) return rc;
        // the index is handed to callers who will query it on OTHER streams: the tree must be complete, not queued
        SFX_HIP(hipStreamSynchronize(st));
    } else {
        ix->d_tree = nullptr;
        (void)hipGetLastError();
    }
    return SFX_OK;
}
}  // namespace sfx

extern "C" {

const char* sfx_strerror(int status)
{
    switch (status) {
    case SFX_OK: return "ok";
    case SFX_ERR_ARG: return "invalid argument";
    case SFX_ERR_TOO_LARGE: return "text longer than u32::MAX bytes";
    case SFX_ERR_NO_DEVICE: return "no HIP device available";
    case SFX_ERR_HIP: return "HIP runtime error (see sfx_last_hip_error)";
    case SFX_ERR_WORKSPACE: return "device workspace too small";
    case SFX_ERR_INTERNAL: return "internal invariant violated";
    case SFX_ERR_NEEDS_RANKS: return "slice needs rank refinement: build the whole suffix array";
    default: return "unknown status";
    }
}

int sfx_device_count(void)
{
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
    return cnt;
}

const char* sfx_last_hip_error(void) { return tls_hip_error; }

// ---- suffix array --------------------------------------------------------------------
uint64_t sfx_sa_workspace_bytes(uint64_t n) { return sa_workspace_bytes(n); }

int sfx_build_sa_u32_dev(const uint8_t* d_text, uint64_t n, uint32_t* d_sa, void* d_workspace,
                         uint64_t workspace_bytes, void* stream)
{
    SFX_NEED_U32(d_sa);
    SFX_NEED_WS(d_workspace, workspace_bytes, sa_workspace_bytes(n));
    return build_sa_u32_dev(d_text, n, d_sa, d_workspace, workspace_bytes, (hipStream_t)stream);
}

int sfx_build_sa_u32(const uint8_t* text, uint64_t n, uint32_t* sa_out)
{
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!text || !sa_out) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    DevBuf dt, ds, dw;
    uint64_t wsb = sa_workspace_bytes(n);
    SFX_TRY(dt.alloc(n));
    SFX_TRY(ds.alloc(n * sizeof(uint32_t)));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    SFX_HIP(hipMemcpyAsync(dt.p, text, n, hipMemcpyHostToDevice, st));
    SFX_TRY(build_sa_u32_dev((const uint8_t*)dt.p, n, (uint32_t*)ds.p, dw.p, wsb, st));
    SFX_HIP(hipMemcpyAsync(sa_out, ds.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}

// u64 index array (BASELINE config 4).  Positions fit u32 (n <= u32::MAX, :380), so the u32
// engine runs and the result is widened on the device before the copy back.
int sfx_build_sa_u64(const uint8_t* text, uint64_t n, uint64_t* sa_out)
{
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!text || !sa_out) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    DevBuf dt, ds, dw, d64;
    uint64_t wsb = sa_workspace_bytes(n);
    SFX_TRY(dt.alloc(n));
    SFX_TRY(ds.alloc(n * sizeof(uint32_t)));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    SFX_HIP(hipMemcpyAsync(dt.p, text, n, hipMemcpyHostToDevice, st));
    SFX_TRY(build_sa_u32_dev((const uint8_t*)dt.p, n, (uint32_t*)ds.p, dw.p, wsb, st));
    SFX_HIP(hipStreamSynchronize(st));
    dw.release();                                      // the workspace is larger than the u64 array
    SFX_TRY(d64.alloc(n * sizeof(uint64_t)));
    SFX_TRY(widen_u32_to_u64_dev((const uint32_t*)ds.p, n, (uint64_t*)d64.p, st));
    SFX_HIP(hipMemcpyAsync(sa_out, d64.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}

// ---- LCP ---------------------------------------------------------------------------------
uint64_t sfx_lcp_workspace_bytes(uint64_t n) { return lcp_workspace_bytes(n); }

int sfx_build_lcp_u32_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, uint32_t* d_lcp,
                          void* d_workspace, uint64_t workspace_bytes, void* stream)
{
    SFX_NEED_U32(d_sa, d_lcp);
    SFX_NEED_WS(d_workspace, workspace_bytes, lcp_workspace_bytes(n));
    return build_lcp_u32_dev(d_text, n, d_sa, d_lcp, d_workspace, workspace_bytes, (hipStream_t)stream);
}

int sfx_build_lcp_u32(const uint8_t* text, uint64_t n, const uint32_t* sa, uint32_t* lcp_out)
{
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!text || !sa || !lcp_out) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    DevBuf dt, ds, dl, dw;
    uint64_t wsb = lcp_workspace_bytes(n);
    SFX_TRY(dt.alloc(n));
    SFX_TRY(ds.alloc(n * sizeof(uint32_t)));
    SFX_TRY(dl.alloc(n * sizeof(uint32_t)));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    SFX_HIP(hipMemcpyAsync(dt.p, text, n, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(ds.p, sa, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    SFX_TRY(build_lcp_u32_dev((const uint8_t*)dt.p, n, (const uint32_t*)ds.p, (uint32_t*)dl.p, dw.p,
                              wsb, st));
    SFX_HIP(hipMemcpyAsync(lcp_out, dl.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}

// ---- SA + LCP in one call --------------------------------------------------------------------
uint64_t sfx_sa_lcp_workspace_bytes(uint64_t n) { return sa_lcp_workspace_bytes(n); }

int sfx_build_sa_lcp_u32_dev(const uint8_t* d_text, uint64_t n, uint32_t* d_sa, uint32_t* d_lcp, void* d_workspace,
                             uint64_t workspace_bytes, void* stream)
{
    SFX_NEED_U32(d_sa, d_lcp);
    SFX_NEED_WS(d_workspace, workspace_bytes, sa_lcp_workspace_bytes(n));
    return build_sa_lcp_u32_dev(d_text, n, d_sa, d_lcp, d_workspace, workspace_bytes, (hipStream_t)stream);
}

int sfx_build_sa_lcp_u32(const uint8_t* text, uint64_t n, uint32_t* sa_out, uint32_t* lcp_out)
{
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!text || !sa_out || !lcp_out) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    DevBuf dt, ds, dl, dw;
    uint64_t wsb = sa_lcp_workspace_bytes(n);
    SFX_TRY(dt.alloc(n));
    SFX_TRY(ds.alloc(n * sizeof(uint32_t)));
    SFX_TRY(dl.alloc(n * sizeof(uint32_t)));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    SFX_HIP(hipMemcpyAsync(dt.p, text, n, hipMemcpyHostToDevice, st));
    SFX_TRY(build_sa_lcp_u32_dev((const uint8_t*)dt.p, n, (uint32_t*)ds.p, (uint32_t*)dl.p, dw.p, wsb, st));
    SFX_HIP(hipMemcpyAsync(sa_out, ds.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SFX_HIP(hipMemcpyAsync(lcp_out, dl.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}

// ---- index + queries ---------------------------------------------------------------------
int sfx_index_create(const uint8_t* text, uint64_t n, const uint32_t* sa, sfx_index** out)
{
    if (!out) return SFX_ERR_ARG;
    *out = nullptr;
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n && !text) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    sfx_index* ix = new sfx_index();
    ix->n = n;
    int rc = SFX_OK;
    if (n) {
        DevBuf dw;
        hipStream_t st = call_stream();
        StreamDrain drain{st};        // (declared after the buffer: runs before it returns to the pool)
        auto hip_ok = [&](hipError_t e, const char* what) {
            if (e == hipSuccess) return true;
            note_hip_error(e, what, __FILE__, __LINE__);
            rc = SFX_ERR_HIP;
            return false;
        };
        do {
            if (!hip_ok(dev_malloc((void**)&ix->d_text, n), "text buffer") ||
                !hip_ok(dev_malloc((void**)&ix->d_sa, n * sizeof(uint32_t)), "table buffer")) break;
            if (!hip_ok(hipMemcpyAsync(ix->d_text, text, n, hipMemcpyHostToDevice, st), "H2D text")) break;
            if (sa) {
                if (!hip_ok(hipMemcpyAsync(ix->d_sa, sa, n * sizeof(uint32_t), hipMemcpyHostToDevice, st), "H2D sa")) break;
            } else {
                uint64_t wsb = sa_workspace_bytes(n);
                rc = dw.alloc(wsb);
                if (rc != SFX_OK) break;
                rc = build_sa_u32_dev(ix->d_text, n, ix->d_sa, dw.p, wsb, st);
                if (rc != SFX_OK) break;
            }
            // the directory build also checks every table entry against n (an unchecked from_parts table
            // must not make the kernels read out of bounds: SFX_ERR_ARG instead of the reference's panic)
            rc = index_build_directory(ix, st);
            if (rc != SFX_OK) break;
            if (!hip_ok(hipStreamSynchronize(st), "sync")) break;
        } while (0);
        if (rc != SFX_OK) (void)hipStreamSynchronize(st);          // nothing may still use the buffers we release
    }
    if (rc != SFX_OK) { sfx_index_destroy(ix); return rc; }
    *out = ix;
    return SFX_OK;
}

// The same over arrays that already live in HBM (not copied: the caller keeps d_text / d_sa alive and
// unchanged for the life of the index); builds only the bucket directory.
int sfx_index_create_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, void* stream, sfx_index** out)
{
    SFX_NEED_U32(d_sa);
    if (!out) return SFX_ERR_ARG;
    *out = nullptr;
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n && (!d_text || !d_sa)) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    sfx_index* ix = new sfx_index();
    ix->n = n;
    ix->owns_arrays = false;
    ix->d_text = const_cast<uint8_t*>(d_text);
    ix->d_sa = const_cast<uint32_t*>(d_sa);
    int rc = index_build_directory(ix, (hipStream_t)stream);
    if (rc != SFX_OK) { (void)hipStreamSynchronize((hipStream_t)stream); sfx_index_destroy(ix); return rc; }
    *out = ix;
    return SFX_OK;
}

int sfx_index_query_dev(const sfx_index* ix, const uint8_t* d_qbytes, const uint64_t* d_qoff, uint64_t nq,
                        uint32_t* d_start, uint32_t* d_end, uint8_t* d_found, uint32_t* d_any, void* stream)
{
    SFX_NEED_U64(d_qoff);
    SFX_NEED_U32(d_start, d_end, d_any);
    if (!ix) return SFX_ERR_ARG;
    if (ix->n == 0 || !ix->d_dir)
        return query_batch_dev(ix->d_text, ix->n, ix->d_sa, ix->n, d_qbytes, d_qoff, nq, d_start, d_end, d_found, d_any,
                               (hipStream_t)stream);
    if (ix->d_tree) {
        // (Answering large batches in the order of their first 8 bytes, so that neighbouring lanes share tree nodes and probes,
        // was measured on config 5's 10^6 queries: the search kernel 1.39 -> 1.23 ms, the 8-pass sort of the (key, query) pairs
        // 0.24 ms -- not worth it.)
        // scratch of phase 2 (the list of queries that go on), kept across calls per (thread, device) in the thread's
        // ThreadRes -- given back when the thread ends or calls sfx_release_cached_buffers(): no
        // allocation and no host synchronisation on the hot path.  The previous batch may still be using it on another
        // stream (whose handle may be gone by now): it left an EVENT behind, and this batch's stream waits on that -- on
        // the device.  Without scratch the batch is answered in one phase.
        const int dev = current_device();
        QueryScratch none;
        QueryScratch& sc = dev >= 0 ? thread_res().scratch[dev] : none;
        void* os = nullptr;
        if (dev >= 0 && nq >= query_two_phase_min()) {
            const uint64_t need = query_scratch_bytes(nq);
            if (!sc.done && event_create(&sc.done, hipEventDisableTiming) != hipSuccess) { sc.done = nullptr; (void)hipGetLastError(); }
            if (sc.done) {
                if (sc.bytes < need) {
                    if (sc.p) { if (sc.used) (void)hipEventSynchronize(sc.done); (void)dev_free(sc.p); sc.p = nullptr; sc.bytes = 0; sc.used = false; }
                    if (dev_malloc(&sc.p, need) == hipSuccess) sc.bytes = need; else { sc.p = nullptr; (void)hipGetLastError(); }
                }
                if (sc.p) {
                    if (sc.used) (void)hipStreamWaitEvent((hipStream_t)stream, sc.done, 0);
                    os = sc.p;
                }
            }
        }
        const int qrc = query_batch_tree_dev(ix->d_text, ix->n, ix->d_sa, ix->d_tree, ix->tree_off, ix->tree_levels, d_qbytes, d_qoff, nq,
                                             d_start, d_end, d_found, d_any, (hipStream_t)stream, os, ix->d_dir, ix->d_lut,
                                             ix->bits, ix->k, ix->dbits);
        if (os) { (void)hipEventRecord(sc.done, (hipStream_t)stream); sc.used = true; }
        return qrc;
    }
    return query_batch_dir_dev(ix->d_text, ix->n, ix->d_sa, ix->d_dir, ix->d_lut, ix->bits, ix->k, ix->dbits, d_qbytes, d_qoff, nq,
                               d_start, d_end, d_found, d_any, (hipStream_t)stream);
}

void sfx_index_destroy(sfx_index* ix)
{
    if (!ix) return;
    if (ix->owns_arrays) {
        if (ix->d_text) (void)dev_free(ix->d_text);
        if (ix->d_sa) (void)dev_free(ix->d_sa);
    }
    if (ix->d_dir) (void)dev_free(ix->d_dir);
    if (ix->d_tree) (void)dev_free(ix->d_tree);
    if (ix->d_lut) (void)dev_free(ix->d_lut);
    delete ix;
}

uint64_t sfx_index_len(const sfx_index* ix) { return ix ? ix->n : 0; }

int sfx_index_table(const sfx_index* ix, uint32_t* sa_out)
{
    if (!ix || (ix->n && !sa_out)) return SFX_ERR_ARG;
    if (ix->n == 0) return SFX_OK;
    SFX_HIP(hipMemcpy(sa_out, ix->d_sa, ix->n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SFX_OK;
}

int sfx_query_batch_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa,
                        const uint8_t* d_qbytes, const uint64_t* d_qoff, uint64_t nq,
                        uint32_t* d_start, uint32_t* d_end, uint8_t* d_found, uint32_t* d_any,
                        void* stream)
{
    SFX_NEED_U64(d_qoff);
    SFX_NEED_U32(d_sa, d_start, d_end, d_any);
    return query_batch_dev(d_text, n, d_sa, n, d_qbytes, d_qoff, nq, d_start, d_end, d_found, d_any,
                           (hipStream_t)stream);
}
int sfx_query_batch_range_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa_part, uint64_t count,
                              const uint8_t* d_qbytes, const uint64_t* d_qoff, uint64_t nq,
                              uint32_t* d_start, uint32_t* d_end, uint8_t* d_found, uint32_t* d_any,
                              void* stream)
{
    SFX_NEED_U64(d_qoff);
    SFX_NEED_U32(d_sa_part, d_start, d_end, d_any);
    return query_batch_dev(d_text, n, d_sa_part, count, d_qbytes, d_qoff, nq, d_start, d_end, d_found, d_any,
                           (hipStream_t)stream);
}
int sfx_build_lcp_range_u32_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa_part, uint64_t count,
                                uint32_t prev_suffix, uint32_t* d_lcp_part, void* stream)
{
    SFX_NEED_U32(d_sa_part, d_lcp_part);
    return build_lcp_range_u32_dev(d_text, n, d_sa_part, count, prev_suffix, d_lcp_part, (hipStream_t)stream);
}
int sfx_widen_u32_to_u64_dev(const uint32_t* d_in, uint64_t count, uint64_t* d_out, void* stream)
{
    SFX_NEED_U32(d_in);
    SFX_NEED_U64(d_out);
    return widen_u32_to_u64_dev(d_in, count, d_out, (hipStream_t)stream);
}

static int query_host(const sfx_index* ix, const uint8_t* qbytes, const uint64_t* qoff, uint64_t nq,
                      uint32_t* start_out, uint32_t* end_out, uint8_t* found_out, uint32_t* any_out)
{
    if (!ix || (nq && !qoff)) return SFX_ERR_ARG;
    if (nq == 0) return SFX_OK;
    uint64_t qtotal = qoff[nq];
    if (qtotal && !qbytes) return SFX_ERR_ARG;
    for (uint64_t k = 0; k < nq; k++) if (qoff[k + 1] < qoff[k]) return SFX_ERR_ARG;
    DevBuf dq, doff, ds, de, df, da;
    SFX_TRY(dq.alloc(qtotal));
    SFX_TRY(doff.alloc((nq + 1) * sizeof(uint64_t)));
    if (start_out) SFX_TRY(ds.alloc(nq * 4));
    if (end_out) SFX_TRY(de.alloc(nq * 4));
    if (found_out) SFX_TRY(df.alloc(nq));
    if (any_out) SFX_TRY(da.alloc(nq * 4));
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    if (qtotal) SFX_HIP(hipMemcpyAsync(dq.p, qbytes, qtotal, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(doff.p, qoff, (nq + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    SFX_TRY(sfx_index_query_dev(ix, (const uint8_t*)dq.p, (const uint64_t*)doff.p, nq, (uint32_t*)ds.p, (uint32_t*)de.p,
                                (uint8_t*)df.p, (uint32_t*)da.p, st));
    if (start_out) SFX_HIP(hipMemcpyAsync(start_out, ds.p, nq * 4, hipMemcpyDeviceToHost, st));
    if (end_out) SFX_HIP(hipMemcpyAsync(end_out, de.p, nq * 4, hipMemcpyDeviceToHost, st));
    if (found_out) SFX_HIP(hipMemcpyAsync(found_out, df.p, nq, hipMemcpyDeviceToHost, st));
    if (any_out) SFX_HIP(hipMemcpyAsync(any_out, da.p, nq * 4, hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}

int sfx_positions_batch(const sfx_index* ix, const uint8_t* qbytes, const uint64_t* qoff,
                        uint64_t nq, uint32_t* start_out, uint32_t* end_out)
{
    return query_host(ix, qbytes, qoff, nq, start_out, end_out, nullptr, nullptr);
}

int sfx_contains_batch(const sfx_index* ix, const uint8_t* qbytes, const uint64_t* qoff,
                       uint64_t nq, uint8_t* found_out, uint32_t* any_out)
{
    return query_host(ix, qbytes, qoff, nq, nullptr, nullptr, found_out, any_out);
}

// ---- matching statistics of a query text (include/suffix_hip.h) -------------------------------
// Pure launches on the caller's stream: nothing is allocated, read back or kept in the index.  The index entry starts
// every bisection inside the bucket directory's stretch (DESIGN.md section 16 says why the key tree stays out of it) and
// relies on the table check made when the index was created.
int sfx_match_stats_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint8_t* d_query, uint64_t m,
                        uint32_t max_len, uint32_t* d_len, uint32_t* d_src, uint32_t* d_start, uint32_t* d_end, void* stream)
{
    SFX_NEED_U32(d_sa, d_len, d_src, d_start, d_end);
    return match_stats_dev(d_text, n, d_sa, d_query, m, max_len, d_len, d_src, d_start, d_end, (hipStream_t)stream);
}
int sfx_index_match_stats_dev(const sfx_index* ix, const uint8_t* d_query, uint64_t m, uint32_t max_len, uint32_t* d_len,
                              uint32_t* d_src, uint32_t* d_start, uint32_t* d_end, void* stream)
{
    SFX_NEED_U32(d_len, d_src, d_start, d_end);
    if (!ix) return SFX_ERR_ARG;
    return match_stats_dir_dev(ix->d_text, ix->n, ix->d_sa, ix->d_dir, ix->d_lut, ix->bits, ix->k, ix->dbits, d_query, m, max_len,
                               d_len, d_src, d_start, d_end, (hipStream_t)stream);
}
int sfx_gindex_match_stats_dev(const sfx_gindex* gx, const uint8_t* d_query, uint64_t m, uint32_t max_len, uint32_t* d_len,
                               uint32_t* d_src, uint32_t* d_start, uint32_t* d_end, void* stream)
{
    SFX_NEED_U32(d_len, d_src, d_start, d_end);
    if (!gx) return SFX_ERR_ARG;
    return gindex_match_stats_dev(gx->d_text, gx->n, gx->d_starts, gx->ndocs, gx->d_sa, gx->d_da, d_query, m, max_len, d_len,
                                  d_src, d_start, d_end, (hipStream_t)stream);
}
// host buffers staged through HBM on the calling thread's stream; exactly one of ix / gx is given
static int match_stats_host(const sfx_index* ix, const sfx_gindex* gx, const uint8_t* query, uint64_t m, uint32_t max_len,
                            uint32_t* len_out, uint32_t* src_out, uint32_t* start_out, uint32_t* end_out)
{
    if (!ix && !gx) return SFX_ERR_ARG;
    if (m > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if ((start_out == nullptr) != (end_out == nullptr)) return SFX_ERR_ARG;
    if (m == 0) return SFX_OK;
    if (!query || !len_out) return SFX_ERR_ARG;
    DevBuf dq, dl, ds, da, de;
    SFX_TRY(dq.alloc(m));
    SFX_TRY(dl.alloc(m * 4));
    if (src_out) SFX_TRY(ds.alloc(m * 4));
    if (start_out) { SFX_TRY(da.alloc(m * 4)); SFX_TRY(de.alloc(m * 4)); }
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    SFX_HIP(hipMemcpyAsync(dq.p, query, m, hipMemcpyHostToDevice, st));
    if (ix)
        SFX_TRY(sfx_index_match_stats_dev(ix, (const uint8_t*)dq.p, m, max_len, (uint32_t*)dl.p, (uint32_t*)ds.p, (uint32_t*)da.p,
                                          (uint32_t*)de.p, st));
    else
        SFX_TRY(sfx_gindex_match_stats_dev(gx, (const uint8_t*)dq.p, m, max_len, (uint32_t*)dl.p, (uint32_t*)ds.p, (uint32_t*)da.p,
                                           (uint32_t*)de.p, st));
    SFX_HIP(hipMemcpyAsync(len_out, dl.p, m * 4, hipMemcpyDeviceToHost, st));
    if (src_out) SFX_HIP(hipMemcpyAsync(src_out, ds.p, m * 4, hipMemcpyDeviceToHost, st));
    if (start_out) SFX_HIP(hipMemcpyAsync(start_out, da.p, m * 4, hipMemcpyDeviceToHost, st));
    if (end_out) SFX_HIP(hipMemcpyAsync(end_out, de.p, m * 4, hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}
int sfx_index_match_stats(const sfx_index* ix, const uint8_t* query, uint64_t m, uint32_t max_len, uint32_t* len_out,
                          uint32_t* src_out, uint32_t* start_out, uint32_t* end_out)
{
    return match_stats_host(ix, nullptr, query, m, max_len, len_out, src_out, start_out, end_out);
}
int sfx_gindex_match_stats(const sfx_gindex* gx, const uint8_t* query, uint64_t m, uint32_t max_len, uint32_t* len_out,
                           uint32_t* src_out, uint32_t* start_out, uint32_t* end_out)
{
    return match_stats_host(nullptr, gx, query, m, max_len, len_out, src_out, start_out, end_out);
}

// ---- Burrows-Wheeler transform with sampled ranks, and its inverse (include/suffix_hip.h) ------
uint64_t sfx_bwt_sample_count(uint64_t n, uint32_t sample_step) { return bwt_sample_count(n, sample_step); }
int sfx_bwt_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, uint32_t sample_step, uint8_t* d_bwt, uint32_t* d_samples,
                void* stream)
{
    SFX_NEED_U32(d_sa, d_samples);
    return bwt_dev(d_text, n, d_sa, sample_step, d_bwt, d_samples, (hipStream_t)stream);
}
int sfx_bwt_u32(const uint8_t* text, uint64_t n, const uint32_t* sa, uint32_t sample_step, uint8_t* bwt_out, uint32_t* samples_out)
{
    if (sample_step & (sample_step - 1u)) return SFX_ERR_ARG;
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!text || !bwt_out || !samples_out) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    const uint64_t cnt = bwt_sample_count(n, sample_step), wsb = sa ? 0 : sa_workspace_bytes(n);
    DevBuf dt, ds, db, dm, dw;
    SFX_TRY(dt.alloc(n));
    SFX_TRY(ds.alloc(n * sizeof(uint32_t)));
    SFX_TRY(db.alloc(n));
    SFX_TRY(dm.alloc(cnt * sizeof(uint32_t)));
    if (!sa) SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    SFX_HIP(hipMemcpyAsync(dt.p, text, n, hipMemcpyHostToDevice, st));
    if (sa)
        SFX_HIP(hipMemcpyAsync(ds.p, sa, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    else
        SFX_TRY(build_sa_u32_dev((const uint8_t*)dt.p, n, (uint32_t*)ds.p, dw.p, wsb, st));
    SFX_TRY(bwt_dev((const uint8_t*)dt.p, n, (const uint32_t*)ds.p, sample_step, (uint8_t*)db.p, (uint32_t*)dm.p, st));
    SFX_HIP(hipMemcpyAsync(bwt_out, db.p, n, hipMemcpyDeviceToHost, st));
    SFX_HIP(hipMemcpyAsync(samples_out, dm.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}
uint64_t sfx_unbwt_workspace_bytes(uint64_t n) { return unbwt_workspace_bytes(n); }
int sfx_unbwt_dev(const uint8_t* d_bwt, uint64_t n, const uint32_t* d_samples, uint64_t nsamples, uint32_t sample_step,
                  uint8_t* d_text_out, void* d_workspace, uint64_t workspace_bytes, void* stream)
{
    SFX_NEED_U32(d_samples);
    SFX_NEED_WS(d_workspace, workspace_bytes, unbwt_workspace_bytes(n));
    return unbwt_dev(d_bwt, n, d_samples, nsamples, sample_step, d_text_out, d_workspace, workspace_bytes, (hipStream_t)stream);
}
int sfx_unbwt(const uint8_t* bwt, uint64_t n, const uint32_t* samples, uint64_t nsamples, uint32_t sample_step, uint8_t* text_out)
{
    if (sample_step & (sample_step - 1u)) return SFX_ERR_ARG;
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (nsamples != bwt_sample_count(n, sample_step)) return SFX_ERR_ARG;
    if (n == 0) return SFX_OK;
    if ((sample_step ? dmin<uint64_t>(n, sample_step) : n) > SFX_UNBWT_MAX_CHAIN) return SFX_ERR_ARG;
    if (!bwt || !samples || !text_out) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    const uint64_t wsb = unbwt_workspace_bytes(n);
    DevBuf db, dm, dt, dw;
    SFX_TRY(db.alloc(n));
    SFX_TRY(dm.alloc(nsamples * sizeof(uint32_t)));
    SFX_TRY(dt.alloc(n));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};
    SFX_HIP(hipMemcpyAsync(db.p, bwt, n, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(dm.p, samples, nsamples * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    SFX_TRY(unbwt_dev((const uint8_t*)db.p, n, (const uint32_t*)dm.p, nsamples, sample_step, (uint8_t*)dt.p, dw.p, wsb, st));
    SFX_HIP(hipMemcpyAsync(text_out, dt.p, n, hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}

// ---- FM-index over the (bwt, samples) pair (include/suffix_hip.h) -------------------------------
uint64_t sfx_fm_bytes(uint64_t n, uint32_t sample_step, uint32_t occ_step) { return fm_bytes(n, sample_step, occ_step); }
int sfx_fm_create_dev(const uint8_t* d_bwt, uint64_t n, const uint32_t* d_samples, uint64_t nsamples, uint32_t sample_step,
                      uint32_t occ_step, void* stream, sfx_fm** out)
{
    SFX_NEED_U32(d_samples);
    return fm_create_dev(d_bwt, n, d_samples, nsamples, sample_step, occ_step, (hipStream_t)stream, out);
}
int sfx_fm_create(const uint8_t* bwt, uint64_t n, const uint32_t* samples, uint64_t nsamples, uint32_t sample_step, uint32_t occ_step,
                  sfx_fm** out)
{
    if (n == 0 || n > 0xFFFFFFFFull || nsamples != bwt_sample_count(n, sample_step) || !bwt || !samples)
        return fm_create_dev(nullptr, n, nullptr, nsamples, sample_step, occ_step, nullptr, out);       // (decided on the host)
    SFX_TRY(check_device());
    DevBuf db, dm;
    SFX_TRY(db.alloc(n));
    SFX_TRY(dm.alloc(nsamples * sizeof(uint32_t)));
    hipStream_t st = call_stream();
    StreamDrain drain{st};
    SFX_HIP(hipMemcpyAsync(db.p, bwt, n, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(dm.p, samples, nsamples * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    return fm_create_dev((const uint8_t*)db.p, n, (const uint32_t*)dm.p, nsamples, sample_step, occ_step, st, out);
}
void sfx_fm_destroy(sfx_fm* fm) { fm_destroy(fm); }
int sfx_fm_info(const sfx_fm* fm, sfx_fm_info_t* info_out) { return fm_info(fm, info_out); }
int sfx_fm_count_dev(const sfx_fm* fm, const uint8_t* d_qbytes, const uint64_t* d_qoff, uint64_t nq, uint32_t* d_start, uint32_t* d_end,
                     void* stream)
{
    SFX_NEED_U64(d_qoff);
    SFX_NEED_U32(d_start, d_end);
    return fm_count_dev(fm, d_qbytes, d_qoff, nq, d_start, d_end, (hipStream_t)stream);
}
int sfx_fm_count(const sfx_fm* fm, const uint8_t* qbytes, const uint64_t* qoff, uint64_t nq, uint32_t* start_out, uint32_t* end_out)
{
    if (!fm) return SFX_ERR_ARG;
    if (nq == 0) return SFX_OK;
    if (!qoff || !start_out || !end_out) return SFX_ERR_ARG;
    const uint64_t qb = qoff[nq];
    if (qb && !qbytes) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    DevBuf dq, dof, ds, de;
    SFX_TRY(dq.alloc(qb));
    SFX_TRY(dof.alloc((nq + 1) * sizeof(uint64_t)));
    SFX_TRY(ds.alloc(nq * sizeof(uint32_t)));
    SFX_TRY(de.alloc(nq * sizeof(uint32_t)));
    hipStream_t st = call_stream();
    StreamDrain drain{st};
    if (qb) SFX_HIP(hipMemcpyAsync(dq.p, qbytes, qb, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(dof.p, qoff, (nq + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    SFX_TRY(fm_count_dev(fm, (const uint8_t*)dq.p, (const uint64_t*)dof.p, nq, (uint32_t*)ds.p, (uint32_t*)de.p, st));
    SFX_HIP(hipMemcpyAsync(start_out, ds.p, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SFX_HIP(hipMemcpyAsync(end_out, de.p, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}
int sfx_fm_lookup_dev(const sfx_fm* fm, const uint32_t* d_ranks, uint64_t first, uint64_t count, uint32_t* d_pos, void* stream)
{
    SFX_NEED_U32(d_ranks, d_pos);
    return fm_lookup_dev(fm, d_ranks, first, count, d_pos, (hipStream_t)stream);
}
int sfx_fm_lookup(const sfx_fm* fm, const uint32_t* ranks, uint64_t first, uint64_t count, uint32_t* pos_out)
{
    if (!fm) return SFX_ERR_ARG;
    if (count && !pos_out) return SFX_ERR_ARG;
    if (count) SFX_TRY(check_device());
    DevBuf dr, dp;
    if (ranks) SFX_TRY(dr.alloc(count * sizeof(uint32_t)));
    SFX_TRY(dp.alloc(count * sizeof(uint32_t)));
    hipStream_t st = call_stream();
    StreamDrain drain{st};
    if (ranks && count) SFX_HIP(hipMemcpyAsync(dr.p, ranks, count * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    SFX_TRY(fm_lookup_dev(fm, ranks ? (const uint32_t*)dr.p : nullptr, first, count, (uint32_t*)dp.p, st));
    if (count) SFX_HIP(hipMemcpyAsync(pos_out, dp.p, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}

// ---- LCE index: inverse table, LCP range minima, k-mismatch extension (include/suffix_hip.h) ---------------------
uint64_t sfx_inverse_table_workspace_bytes(uint64_t n) { return inverse_table_workspace_bytes(n); }
int sfx_inverse_table_dev(const uint32_t* d_sa, uint64_t n, uint32_t* d_isa, void* d_workspace, uint64_t workspace_bytes, void* stream)
{
    SFX_NEED_U32(d_sa, d_isa);
    SFX_NEED_WS(d_workspace, workspace_bytes, inverse_table_workspace_bytes(n));
    return inverse_table_dev(d_sa, n, d_isa, d_workspace, workspace_bytes, (hipStream_t)stream);
}
int sfx_inverse_table_u32(const uint32_t* sa, uint64_t n, uint32_t* isa_out)
{
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!sa || !isa_out) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    const uint64_t wsb = inverse_table_workspace_bytes(n);
    DevBuf ds, di, dw;
    SFX_TRY(ds.alloc(n * sizeof(uint32_t)));
    SFX_TRY(di.alloc(n * sizeof(uint32_t)));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};
    SFX_HIP(hipMemcpyAsync(ds.p, sa, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    SFX_TRY(inverse_table_dev((const uint32_t*)ds.p, n, (uint32_t*)di.p, dw.p, wsb, st));
    SFX_HIP(hipMemcpyAsync(isa_out, di.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}
uint64_t sfx_lce_bytes(uint64_t n) { return lce_bytes(n); }
// A create's scratch (the two flags; from 2^27 entries on the 16 n bytes + radix scratch of the partitioned scatter) comes
// from the pool of the host-pointer entry points: a loop of creates at one size allocates it once, and
// sfx_release_cached_buffers() returns it.  It goes back to the pool when the create's work is done: after SFX_OK the
// read-back of the flags was the last thing queued; after an error the stream is drained first.
static int lce_create_pooled(const uint32_t* d_sa, const uint32_t* d_lcp, uint64_t n, const uint64_t* d_starts, uint64_t ndocs,
                             hipStream_t st, bool own, sfx_lce** out)
{
    if (!out || n == 0 || n > 0xFFFFFFFFull || !d_sa || !d_lcp || (d_starts ? ndocs == 0 : ndocs != 0))
        return lce_create_dev(d_sa, d_lcp, n, d_starts, ndocs, st, own, nullptr, 0, out);                   // (decided on the host)
    const uint64_t need = inverse_table_workspace_bytes(n);
    DevBuf scratch;
    SFX_TRY(scratch.alloc(need));
    const int rc = lce_create_dev(d_sa, d_lcp, n, d_starts, ndocs, st, own, scratch.p, need, out);
    if (rc != SFX_OK) (void)hipStreamSynchronize(st);
    return rc;
}
int sfx_lce_create_dev(const uint32_t* d_sa, const uint32_t* d_lcp, uint64_t n, const uint64_t* d_doc_starts, uint64_t ndocs, void* stream,
                       sfx_lce** out)
{
    SFX_NEED_U32(d_sa, d_lcp);
    SFX_NEED_U64(d_doc_starts);
    return lce_create_pooled(d_sa, d_lcp, n, d_doc_starts, ndocs, (hipStream_t)stream, false, out);
}
int sfx_lce_create(const uint32_t* sa, const uint32_t* lcp, uint64_t n, const uint64_t* doc_starts, uint64_t ndocs, sfx_lce** out)
{
    if (n == 0 || n > 0xFFFFFFFFull || !sa || !lcp || !out || (doc_starts ? ndocs == 0 : ndocs != 0))
        return lce_create_dev(nullptr, nullptr, n, doc_starts, ndocs, nullptr, false, nullptr, 0, out);  // (decided on the host)
    SFX_TRY(check_device());
    DevBuf ds;
    SFX_TRY(ds.alloc(n * sizeof(uint32_t)));
    void* d_lcp = nullptr;
    void* d_starts = nullptr;
    hipStream_t st = call_stream();
    int rc = SFX_OK;
    {
        StreamDrain drain{st};
        rc = [&]() -> int {
            SFX_HIP(dev_malloc(&d_lcp, n * sizeof(uint32_t)));                                               // the handle's own level 0
            if (doc_starts) SFX_HIP(dev_malloc(&d_starts, ndocs * sizeof(uint64_t)));
            SFX_HIP(hipMemcpyAsync(ds.p, sa, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            SFX_HIP(hipMemcpyAsync(d_lcp, lcp, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            if (doc_starts) SFX_HIP(hipMemcpyAsync(d_starts, doc_starts, ndocs * sizeof(uint64_t), hipMemcpyHostToDevice, st));
            return lce_create_pooled((const uint32_t*)ds.p, (const uint32_t*)d_lcp, n, (const uint64_t*)d_starts, ndocs, st, true, out);
        }();
    }
    if (rc != SFX_OK) {
        if (d_lcp) (void)dev_free(d_lcp);
        if (d_starts) (void)dev_free(d_starts);
    }
    return rc;
}
void sfx_lce_destroy(sfx_lce* lx) { lce_destroy(lx); }
int sfx_lce_query_dev(const sfx_lce* lx, const uint32_t* d_a, const uint32_t* d_b, uint64_t nq, uint32_t max_mismatches, uint32_t* d_len,
                      void* stream)
{
    SFX_NEED_U32(d_a, d_b, d_len);
    return lce_query_dev(lx, d_a, d_b, nq, max_mismatches, d_len, (hipStream_t)stream);
}
int sfx_lce_range_min_dev(const sfx_lce* lx, const uint32_t* d_lo, const uint32_t* d_hi, uint64_t nq, uint32_t* d_min, void* stream)
{
    SFX_NEED_U32(d_lo, d_hi, d_min);
    return lce_range_min_dev(lx, d_lo, d_hi, nq, d_min, (hipStream_t)stream);
}
int sfx_lce_ranks_dev(const sfx_lce* lx, const uint32_t* d_pos, uint64_t nq, uint32_t* d_rank, void* stream)
{
    SFX_NEED_U32(d_pos, d_rank);
    return lce_ranks_dev(lx, d_pos, nq, d_rank, (hipStream_t)stream);
}
// the host forms of the three queries: in0 / in1 (nullptr: one input) up, one launch, the answers down
extern "C++" {
template <class Run> static int lce_host_call(const sfx_lce* lx, const uint32_t* in0, const uint32_t* in1, bool two, uint64_t nq, uint32_t* out,
                                              Run run)
{
    if (!lx) return SFX_ERR_ARG;
    if (nq == 0) return SFX_OK;
    if (!in0 || (two && !in1) || !out) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    DevBuf d0, d1, dout;
    SFX_TRY(d0.alloc(nq * sizeof(uint32_t)));
    if (two) SFX_TRY(d1.alloc(nq * sizeof(uint32_t)));
    SFX_TRY(dout.alloc(nq * sizeof(uint32_t)));
    hipStream_t st = call_stream();
    StreamDrain drain{st};
    SFX_HIP(hipMemcpyAsync(d0.p, in0, nq * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (two) SFX_HIP(hipMemcpyAsync(d1.p, in1, nq * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    SFX_TRY(run((const uint32_t*)d0.p, (const uint32_t*)d1.p, (uint32_t*)dout.p, st));
    SFX_HIP(hipMemcpyAsync(out, dout.p, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}
}  // extern "C++"
int sfx_lce_query(const sfx_lce* lx, const uint32_t* a, const uint32_t* b, uint64_t nq, uint32_t max_mismatches, uint32_t* len_out)
{
    return lce_host_call(lx, a, b, true, nq, len_out, [&](const uint32_t* da, const uint32_t* db, uint32_t* dl, hipStream_t st) {
        return lce_query_dev(lx, da, db, nq, max_mismatches, dl, st);
    });
}
int sfx_lce_range_min(const sfx_lce* lx, const uint32_t* lo, const uint32_t* hi, uint64_t nq, uint32_t* min_out)
{
    return lce_host_call(lx, lo, hi, true, nq, min_out, [&](const uint32_t* dl, const uint32_t* dh, uint32_t* dm, hipStream_t st) {
        return lce_range_min_dev(lx, dl, dh, nq, dm, st);
    });
}
int sfx_lce_ranks(const sfx_lce* lx, const uint32_t* pos, uint64_t nq, uint32_t* rank_out)
{
    return lce_host_call(lx, pos, nullptr, false, nq, rank_out, [&](const uint32_t* dp, const uint32_t*, uint32_t* dr, hipStream_t st) {
        return lce_ranks_dev(lx, dp, nq, dr, st);
    });
}
int sfx_lce_u32(const uint32_t* sa, const uint32_t* lcp, uint64_t n, const uint64_t* doc_starts, uint64_t ndocs, const uint32_t* a,
                const uint32_t* b, uint64_t nq, uint32_t max_mismatches, uint32_t* len_out)
{
    sfx_lce* lx = nullptr;
    SFX_TRY(sfx_lce_create(sa, lcp, n, doc_starts, ndocs, &lx));
    const int rc = sfx_lce_query(lx, a, b, nq, max_mismatches, len_out);
    sfx_lce_destroy(lx);
    return rc;
}

// ---- suffix-tree navigation over the LCE handle: substring loci, LCA, argmin, suffix links (include/suffix_hip.h) ---
int sfx_lce_substr_dev(const sfx_lce* lx, const uint32_t* d_pos, const uint32_t* d_len, uint64_t nq, uint32_t* d_lo, uint32_t* d_hi,
                       uint32_t* d_depth, void* stream)
{
    SFX_NEED_U32(d_pos, d_len, d_lo, d_hi, d_depth);
    return nav_substr_dev(lx, d_pos, d_len, nq, d_lo, d_hi, d_depth, (hipStream_t)stream);
}
int sfx_lce_lca_dev(const sfx_lce* lx, const uint32_t* d_a, const uint32_t* d_b, uint64_t nq, uint32_t* d_lo, uint32_t* d_hi,
                    uint32_t* d_depth, void* stream)
{
    SFX_NEED_U32(d_a, d_b, d_lo, d_hi, d_depth);
    return nav_lca_dev(lx, d_a, d_b, nq, d_lo, d_hi, d_depth, (hipStream_t)stream);
}
int sfx_lce_range_argmin_dev(const sfx_lce* lx, const uint32_t* d_lo, const uint32_t* d_hi, uint64_t nq, uint32_t* d_arg, void* stream)
{
    SFX_NEED_U32(d_lo, d_hi, d_arg);
    return nav_argmin_dev(lx, d_lo, d_hi, nq, d_arg, (hipStream_t)stream);
}
// the host forms of the two interval queries: two inputs up, one launch, lo / hi / depth (nullptr: not wanted) down
extern "C++" {
template <class Run> static int nav_host_call(const sfx_lce* lx, const uint32_t* in0, const uint32_t* in1, uint64_t nq, uint32_t* lo, uint32_t* hi,
                                              uint32_t* depth, Run run)
{
    if (!lx) return SFX_ERR_ARG;
    if (nq == 0) return SFX_OK;
    if (!in0 || !in1 || !lo || !hi) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    const uint64_t bytes = nq * sizeof(uint32_t);
    DevBuf d0, d1, dl, dh, dd;
    SFX_TRY(d0.alloc(bytes));
    SFX_TRY(d1.alloc(bytes));
    SFX_TRY(dl.alloc(bytes));
    SFX_TRY(dh.alloc(bytes));
    if (depth) SFX_TRY(dd.alloc(bytes));
    hipStream_t st = call_stream();
    StreamDrain drain{st};
    SFX_HIP(hipMemcpyAsync(d0.p, in0, bytes, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(d1.p, in1, bytes, hipMemcpyHostToDevice, st));
    SFX_TRY(run((const uint32_t*)d0.p, (const uint32_t*)d1.p, (uint32_t*)dl.p, (uint32_t*)dh.p, depth ? (uint32_t*)dd.p : nullptr, st));
    SFX_HIP(hipMemcpyAsync(lo, dl.p, bytes, hipMemcpyDeviceToHost, st));
    SFX_HIP(hipMemcpyAsync(hi, dh.p, bytes, hipMemcpyDeviceToHost, st));
    if (depth) SFX_HIP(hipMemcpyAsync(depth, dd.p, bytes, hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}
}  // extern "C++"
int sfx_lce_substr(const sfx_lce* lx, const uint32_t* pos, const uint32_t* len, uint64_t nq, uint32_t* lo_out, uint32_t* hi_out,
                   uint32_t* depth_out)
{
    return nav_host_call(lx, pos, len, nq, lo_out, hi_out, depth_out,
                         [&](const uint32_t* dp, const uint32_t* dn, uint32_t* dl, uint32_t* dh, uint32_t* dd, hipStream_t st) {
                             return nav_substr_dev(lx, dp, dn, nq, dl, dh, dd, st);
                         });
}
int sfx_lce_lca(const sfx_lce* lx, const uint32_t* a, const uint32_t* b, uint64_t nq, uint32_t* lo_out, uint32_t* hi_out, uint32_t* depth_out)
{
    return nav_host_call(lx, a, b, nq, lo_out, hi_out, depth_out,
                         [&](const uint32_t* da, const uint32_t* db, uint32_t* dl, uint32_t* dh, uint32_t* dd, hipStream_t st) {
                             return nav_lca_dev(lx, da, db, nq, dl, dh, dd, st);
                         });
}
int sfx_lce_range_argmin(const sfx_lce* lx, const uint32_t* lo, const uint32_t* hi, uint64_t nq, uint32_t* arg_out)
{
    return lce_host_call(lx, lo, hi, true, nq, arg_out, [&](const uint32_t* dl, const uint32_t* dh, uint32_t* da, hipStream_t st) {
        return nav_argmin_dev(lx, dl, dh, nq, da, st);
    });
}
uint64_t sfx_suffix_links_workspace_bytes(uint64_t n) { return suffix_links_workspace_bytes(n); }
int sfx_suffix_links_dev(const sfx_lce* lx, const uint32_t* d_sa, uint64_t nodes, const uint32_t* d_node_lb, const uint32_t* d_node_rb,
                         const uint32_t* d_node_depth, uint32_t* d_slink, void* d_workspace, uint64_t workspace_bytes, void* stream)
{
    SFX_NEED_U32(d_sa, d_node_lb, d_node_rb, d_node_depth, d_slink);
    SFX_NEED_WS(d_workspace, workspace_bytes, lx ? suffix_links_workspace_bytes(lx->n) : 0);
    return suffix_links_dev(lx, d_sa, nodes, d_node_lb, d_node_rb, d_node_depth, d_slink, d_workspace, workspace_bytes, (hipStream_t)stream);
}
int sfx_suffix_links_u32(const uint32_t* sa, const uint32_t* lcp, uint64_t n, uint64_t nodes, const uint32_t* node_lb, const uint32_t* node_rb,
                         const uint32_t* node_depth, uint32_t* slink_out)
{
    if (n > 0xFFFFFFFFull || nodes > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0 || nodes == 0) return SFX_OK;
    if (!sa || !lcp || !node_lb || !node_rb || !node_depth || !slink_out) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    const uint64_t bytes = n * sizeof(uint32_t), nbytes = nodes * sizeof(uint32_t), wsb = suffix_links_workspace_bytes(n);
    DevBuf ds, dl, dlb, drb, ddp, dout, dw;
    SFX_TRY(ds.alloc(bytes));
    SFX_TRY(dl.alloc(bytes));
    SFX_TRY(dlb.alloc(nbytes));
    SFX_TRY(drb.alloc(nbytes));
    SFX_TRY(ddp.alloc(nbytes));
    SFX_TRY(dout.alloc(nbytes));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    struct Handle {                    // (declared after the buffers: the handle borrows dl and goes first)
        sfx_lce* lx = nullptr;
        hipStream_t st;
        ~Handle() { (void)hipStreamSynchronize(st); lce_destroy(lx); }
    } h;
    h.st = st;
    SFX_HIP(hipMemcpyAsync(ds.p, sa, bytes, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(dl.p, lcp, bytes, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(dlb.p, node_lb, nbytes, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(drb.p, node_rb, nbytes, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(ddp.p, node_depth, nbytes, hipMemcpyHostToDevice, st));
    SFX_TRY(lce_create_pooled((const uint32_t*)ds.p, (const uint32_t*)dl.p, n, nullptr, 0, st, false, &h.lx));
    SFX_TRY(suffix_links_dev(h.lx, (const uint32_t*)ds.p, nodes, (const uint32_t*)dlb.p, (const uint32_t*)drb.p, (const uint32_t*)ddp.p,
                             (uint32_t*)dout.p, dw.p, wsb, st));
    SFX_HIP(hipMemcpyAsync(slink_out, dout.p, nbytes, hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}

// ---- document counts of every lcp-interval, k-common substrings of a collection (include/suffix_hip.h) -------------
uint64_t sfx_doc_counts_workspace_bytes(uint64_t n) { return doc_counts_workspace_bytes(n); }
int sfx_doc_counts_dev(const uint32_t* d_da, const uint32_t* d_lcp, uint64_t n, uint64_t ndocs, uint32_t* d_dup_prefix, uint32_t* d_df,
                       void* d_workspace, uint64_t workspace_bytes, void* stream)
{
    SFX_NEED_U32(d_da, d_lcp, d_dup_prefix, d_df);
    SFX_NEED_WS(d_workspace, workspace_bytes, doc_counts_workspace_bytes(n));
    return doc_counts_dev(d_da, d_lcp, n, ndocs, d_dup_prefix, d_df, d_workspace, workspace_bytes, (hipStream_t)stream);
}
int sfx_doc_counts_u32(const uint32_t* da, const uint32_t* lcp, uint64_t n, uint64_t ndocs, uint32_t* dup_prefix_out, uint32_t* df_out)
{
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (ndocs == 0 || !da || !lcp) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    const uint64_t wsb = doc_counts_workspace_bytes(n), bytes = n * sizeof(uint32_t);
    DevBuf dd, dl, dp, df, dw;
    SFX_TRY(dd.alloc(bytes));
    SFX_TRY(dl.alloc(bytes));
    if (dup_prefix_out) SFX_TRY(dp.alloc(bytes));
    if (df_out) SFX_TRY(df.alloc(bytes));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};
    SFX_HIP(hipMemcpyAsync(dd.p, da, bytes, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(dl.p, lcp, bytes, hipMemcpyHostToDevice, st));
    SFX_TRY(doc_counts_dev((const uint32_t*)dd.p, (const uint32_t*)dl.p, n, ndocs, (uint32_t*)dp.p, (uint32_t*)df.p, dw.p, wsb, st));
    if (dup_prefix_out) SFX_HIP(hipMemcpyAsync(dup_prefix_out, dp.p, bytes, hipMemcpyDeviceToHost, st));
    if (df_out) SFX_HIP(hipMemcpyAsync(df_out, df.p, bytes, hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}
uint64_t sfx_common_substrings_workspace_bytes(uint64_t ndocs) { return common_substrings_workspace_bytes(ndocs); }
int sfx_common_substrings_dev(const uint32_t* d_sa, const uint32_t* d_lcp, const uint32_t* d_df, uint64_t n, const uint64_t* d_doc_starts,
                              uint64_t ndocs, uint32_t* d_len, uint32_t* d_pos, void* d_workspace, uint64_t workspace_bytes, void* stream)
{
    SFX_NEED_U32(d_sa, d_lcp, d_df, d_len, d_pos);
    SFX_NEED_U64(d_doc_starts);
    SFX_NEED_WS(d_workspace, workspace_bytes, common_substrings_workspace_bytes(ndocs));
    return common_substrings_dev(d_sa, d_lcp, d_df, n, d_doc_starts, ndocs, d_len, d_pos, d_workspace, workspace_bytes, (hipStream_t)stream);
}
int sfx_common_substrings_u32(const uint32_t* sa, const uint32_t* lcp, const uint32_t* df, uint64_t n, const uint64_t* doc_starts,
                              uint64_t ndocs, uint32_t* len_out, uint32_t* pos_out)
{
    if (n > 0xFFFFFFFFull || ndocs > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (ndocs == 0) return n ? SFX_ERR_ARG : SFX_OK;
    if (!doc_starts || !len_out || !pos_out || (n && (!sa || !lcp || !df))) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    const uint64_t wsb = common_substrings_workspace_bytes(ndocs), bytes = n * sizeof(uint32_t);
    DevBuf ds, dl, dd, dt, dn, dp, dw;
    SFX_TRY(ds.alloc(bytes));
    SFX_TRY(dl.alloc(bytes));
    SFX_TRY(dd.alloc(bytes));
    SFX_TRY(dt.alloc(ndocs * sizeof(uint64_t)));
    SFX_TRY(dn.alloc(ndocs * sizeof(uint32_t)));
    SFX_TRY(dp.alloc(ndocs * sizeof(uint32_t)));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};
    if (n) {
        SFX_HIP(hipMemcpyAsync(ds.p, sa, bytes, hipMemcpyHostToDevice, st));
        SFX_HIP(hipMemcpyAsync(dl.p, lcp, bytes, hipMemcpyHostToDevice, st));
        SFX_HIP(hipMemcpyAsync(dd.p, df, bytes, hipMemcpyHostToDevice, st));
    }
    SFX_HIP(hipMemcpyAsync(dt.p, doc_starts, ndocs * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    SFX_TRY(common_substrings_dev((const uint32_t*)ds.p, (const uint32_t*)dl.p, (const uint32_t*)dd.p, n, (const uint64_t*)dt.p, ndocs,
                                  (uint32_t*)dn.p, (uint32_t*)dp.p, dw.p, wsb, st));
    SFX_HIP(hipMemcpyAsync(len_out, dn.p, ndocs * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SFX_HIP(hipMemcpyAsync(pos_out, dp.p, ndocs * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}

// ---- document listing with term frequencies and top-k (include/suffix_hip.h) ----------------
uint64_t sfx_doclist_bytes(uint64_t n) { return doclist_bytes(n); }
uint64_t sfx_doclist_create_workspace_bytes(uint64_t n) { return doclist_create_workspace_bytes(n); }
uint64_t sfx_doclist_workspace_bytes(uint64_t nq, uint64_t list_limit) { return doclist_workspace_bytes(nq, list_limit); }
// d_workspace == NULL: the scratch comes from the pool of the host-pointer entry points, as sfx_lce_create_dev's does
static int doclist_create_pooled(const uint32_t* d_da, uint64_t n, const uint64_t* d_starts, uint64_t ndocs, uint64_t occ_cut, void* ws,
                                 uint64_t ws_bytes, hipStream_t st, bool own, sfx_doclist** out)
{
    if (ws || !out || n == 0 || n > 0xFFFFFFFFull || ndocs == 0 || ndocs > 0xFFFFFFFFull || !d_da || !d_starts)
        return doclist_create_dev(d_da, n, d_starts, ndocs, occ_cut, ws, ws_bytes, st, own, out);
    const uint64_t need = doclist_create_workspace_bytes(n);
    DevBuf scratch;
    SFX_TRY(scratch.alloc(need));
    const int rc = doclist_create_dev(d_da, n, d_starts, ndocs, occ_cut, scratch.p, need, st, own, out);
    if (rc != SFX_OK) (void)hipStreamSynchronize(st);
    return rc;
}
int sfx_doclist_create_dev(const uint32_t* d_da, uint64_t n, const uint64_t* d_doc_starts, uint64_t ndocs, uint64_t occ_cut, void* d_workspace,
                           uint64_t workspace_bytes, void* stream, sfx_doclist** out)
{
    SFX_NEED_U32(d_da);
    SFX_NEED_U64(d_doc_starts);
    SFX_NEED_WS(d_workspace, workspace_bytes, doclist_create_workspace_bytes(n));
    return doclist_create_pooled(d_da, n, d_doc_starts, ndocs, occ_cut, d_workspace, workspace_bytes, (hipStream_t)stream, false, out);
}
int sfx_doclist_create(const uint32_t* da, uint64_t n, const uint64_t* doc_starts, uint64_t ndocs, uint64_t occ_cut, sfx_doclist** out)
{
    if (n == 0 || n > 0xFFFFFFFFull || ndocs == 0 || ndocs > 0xFFFFFFFFull || !da || !doc_starts || !out)
        return doclist_create_dev(nullptr, n, nullptr, ndocs, occ_cut, nullptr, 0, nullptr, false, out);      // (decided on the host)
    SFX_TRY(check_device());
    void* d_da = nullptr;
    void* d_starts = nullptr;
    hipStream_t st = call_stream();
    int rc = SFX_OK;
    {
        StreamDrain drain{st};
        rc = [&]() -> int {
            SFX_HIP(dev_malloc(&d_da, n * sizeof(uint32_t)));                                                // the handle's own copies
            SFX_HIP(dev_malloc(&d_starts, ndocs * sizeof(uint64_t)));
            SFX_HIP(hipMemcpyAsync(d_da, da, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            SFX_HIP(hipMemcpyAsync(d_starts, doc_starts, ndocs * sizeof(uint64_t), hipMemcpyHostToDevice, st));
            return doclist_create_pooled((const uint32_t*)d_da, n, (const uint64_t*)d_starts, ndocs, occ_cut, nullptr, 0, st, true, out);
        }();
    }
    if (rc != SFX_OK) {
        if (d_da) (void)dev_free(d_da);
        if (d_starts) (void)dev_free(d_starts);
    }
    return rc;
}
void sfx_doclist_destroy(sfx_doclist* dx) { doclist_destroy(dx); }
int sfx_doclist_list_dev(const sfx_doclist* dx, const uint32_t* d_start, const uint32_t* d_end, uint64_t nq, uint32_t order, uint32_t top_k,
                         uint64_t list_limit, uint32_t* d_doc, uint32_t* d_tf, uint64_t capacity, uint64_t* d_first, uint64_t* listed_out,
                         uint64_t* count_out, void* d_workspace, uint64_t workspace_bytes, void* stream)
{
    SFX_NEED_U32(d_start, d_end, d_doc, d_tf);
    SFX_NEED_U64(d_first);
    SFX_NEED_WS(d_workspace, workspace_bytes, doclist_workspace_bytes(nq, list_limit));
    return doclist_list_dev(dx, d_start, d_end, nq, order, top_k, list_limit, d_doc, d_tf, capacity, d_first, listed_out, count_out,
                            d_workspace, workspace_bytes, (hipStream_t)stream);
}
int sfx_doclist_list(const sfx_doclist* dx, const uint32_t* start, const uint32_t* end, uint64_t nq, uint32_t order, uint32_t top_k,
                     uint64_t list_limit, uint32_t* doc_out, uint32_t* tf_out, uint64_t capacity, uint64_t* first_out, uint64_t* listed_out,
                     uint64_t* count_out)
{
    if (!dx || !listed_out || !count_out || order > SFX_DOCLIST_BY_TF) return SFX_ERR_ARG;
    *listed_out = *count_out = 0;
    if (nq > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (capacity && (!doc_out || !tf_out)) return SFX_ERR_ARG;
    if (nq == 0 || dx->n == 0) {
        if (first_out) memset(first_out, 0, (nq + 1) * sizeof(uint64_t));
        return SFX_OK;
    }
    if (!start || !end) return SFX_ERR_ARG;
    uint64_t bound = 0;                                                    // (Z_full cannot be larger: the workspace need not be either)
    for (uint64_t j = 0; j < nq; j++) {
        if (start[j] > end[j] || end[j] > dx->n) return SFX_ERR_ARG;
        bound += dmin<uint64_t>(end[j] - start[j], dx->ndocs);
    }
    SFX_TRY(check_device());
    list_limit = dmin(list_limit, dmax<uint64_t>(bound, 1));
    capacity = dmin(capacity, list_limit);
    const uint64_t wsb = doclist_workspace_bytes(nq, list_limit);
    DevBuf ds, de, dd, dt, df, dw;
    SFX_TRY(ds.alloc(nq * sizeof(uint32_t)));
    SFX_TRY(de.alloc(nq * sizeof(uint32_t)));
    SFX_TRY(dd.alloc(capacity * sizeof(uint32_t)));
    SFX_TRY(dt.alloc(capacity * sizeof(uint32_t)));
    if (first_out) SFX_TRY(df.alloc((nq + 1) * sizeof(uint64_t)));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    SFX_HIP(hipMemcpyAsync(ds.p, start, nq * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(de.p, end, nq * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    SFX_TRY(doclist_list_dev(dx, (const uint32_t*)ds.p, (const uint32_t*)de.p, nq, order, top_k, list_limit, capacity ? (uint32_t*)dd.p : nullptr,
                             capacity ? (uint32_t*)dt.p : nullptr, capacity, (uint64_t*)df.p, listed_out, count_out, dw.p, wsb, st));
    if (*listed_out > list_limit) return SFX_OK;                           // (refused: nothing was written)
    const uint64_t z = dmin<uint64_t>(*count_out, capacity);
    if (z) {
        SFX_HIP(hipMemcpyAsync(doc_out, dd.p, z * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SFX_HIP(hipMemcpyAsync(tf_out, dt.p, z * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    if (first_out) SFX_HIP(hipMemcpyAsync(first_out, df.p, (nq + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}

// ---- Lyndon arrays and maximal repetitions (runs) of a plain text (include/suffix_hip.h) ----------------------------
uint64_t sfx_lyndon_array_workspace_bytes(uint64_t n) { return lyndon_array_workspace_bytes(n); }
int sfx_lyndon_array_dev(const uint32_t* d_isa, uint64_t n, uint32_t* d_lyn, void* d_workspace, uint64_t workspace_bytes, void* stream)
{
    SFX_NEED_U32(d_isa, d_lyn);
    SFX_NEED_WS(d_workspace, workspace_bytes, lyndon_array_workspace_bytes(n));
    return lyndon_array_dev(d_isa, n, d_lyn, d_workspace, workspace_bytes, (hipStream_t)stream);
}
int sfx_lyndon_array_u32(const uint8_t* text, uint64_t n, const uint32_t* sa, int order, uint32_t* lyn_out)
{
    if (order != 0 && order != 1) return SFX_ERR_ARG;
    if (n > kRunsMaxN) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if ((!sa && !text) || !lyn_out) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    const uint64_t bytes = n * sizeof(uint32_t);
    const uint64_t wsb = dmax(sa ? 0 : sa_workspace_bytes(n), lyndon_array_workspace_bytes(n));
    DevBuf dt, ds, di, dl, dw;
    if (!sa) SFX_TRY(dt.alloc(n));
    SFX_TRY(ds.alloc(bytes));
    SFX_TRY(di.alloc(bytes));
    SFX_TRY(dl.alloc(bytes));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    if (sa) {
        SFX_HIP(hipMemcpyAsync(ds.p, sa, bytes, hipMemcpyHostToDevice, st));
    } else {
        SFX_HIP(hipMemcpyAsync(dt.p, text, n, hipMemcpyHostToDevice, st));
        if (order == 1) SFX_LAUNCH("runs_complement", (double)n * 2, k_runs_complement, lce_grid(n), kBlock, st, (const uint8_t*)dt.p, n, (uint8_t*)dt.p);
        SFX_TRY(build_sa_u32_dev((const uint8_t*)dt.p, n, (uint32_t*)ds.p, dw.p, wsb, st));
    }
    SFX_TRY(lyndon_from_table_dev((const uint32_t*)ds.p, n, (uint32_t*)di.p, (uint32_t*)dl.p, dw.p, wsb, st));
    SFX_HIP(hipMemcpyAsync(lyn_out, dl.p, bytes, hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}
uint64_t sfx_runs_workspace_bytes(uint64_t n) { return runs_workspace_bytes(n); }
int sfx_runs_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint32_t* d_lcp, const sfx_runs_filter_t* filter, uint32_t* d_begin,
                 uint32_t* d_end, uint32_t* d_period, uint64_t capacity, uint64_t* count_out, void* d_workspace, uint64_t workspace_bytes,
                 void* stream)
{
    SFX_NEED_U32(d_sa, d_lcp, d_begin, d_end, d_period);
    SFX_NEED_WS(d_workspace, workspace_bytes, runs_workspace_bytes(n));
    return runs_dev(d_text, n, d_sa, d_lcp, filter, d_begin, d_end, d_period, capacity, count_out, d_workspace, workspace_bytes,
                    (hipStream_t)stream);
}
int sfx_runs_u32(const uint8_t* text, uint64_t n, const uint32_t* sa, const uint32_t* lcp, const sfx_runs_filter_t* filter, uint32_t* begin,
                 uint32_t* end, uint32_t* period, uint64_t capacity, uint64_t* count_out)
{
    if (!count_out) return SFX_ERR_ARG;
    *count_out = 0;
    if (n > kRunsMaxN) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!text || (lcp && !sa) || (capacity && (!begin || !end || !period))) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    if (capacity > n) capacity = n;                                      // (fewer than n runs)
    const uint64_t bytes = n * sizeof(uint32_t);
    const uint64_t wsb = dmax(sa ? (lcp ? 0 : lcp_workspace_bytes(n)) : sa_lcp_workspace_bytes(n), runs_workspace_bytes(n));
    DevBuf dt, ds, dl, dout, dw;
    SFX_TRY(dt.alloc(n));
    SFX_TRY(ds.alloc(bytes));
    SFX_TRY(dl.alloc(bytes));
    ArenaSizer osz;
    for (int i = 0; i < 3; i++) osz.take<uint32_t>(capacity);
    SFX_TRY(dout.alloc(osz.used));
    Arena oa(dout.p, dmax<uint64_t>(osz.used, 1));
    uint32_t* const db = oa.take<uint32_t>(capacity);
    uint32_t* const de = oa.take<uint32_t>(capacity);
    uint32_t* const dp = oa.take<uint32_t>(capacity);
    if (oa.overflow) return SFX_ERR_INTERNAL;
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    SFX_HIP(hipMemcpyAsync(dt.p, text, n, hipMemcpyHostToDevice, st));
    if (!sa) {
        SFX_TRY(build_sa_lcp_u32_dev((const uint8_t*)dt.p, n, (uint32_t*)ds.p, (uint32_t*)dl.p, dw.p, wsb, st));
    } else {
        SFX_HIP(hipMemcpyAsync(ds.p, sa, bytes, hipMemcpyHostToDevice, st));
        if (lcp)
            SFX_HIP(hipMemcpyAsync(dl.p, lcp, bytes, hipMemcpyHostToDevice, st));
        else
            SFX_TRY(build_lcp_u32_dev((const uint8_t*)dt.p, n, (const uint32_t*)ds.p, (uint32_t*)dl.p, dw.p, wsb, st));
    }
    SFX_TRY(runs_dev((const uint8_t*)dt.p, n, (const uint32_t*)ds.p, (const uint32_t*)dl.p, filter, db, de, dp,
                     capacity, count_out, dw.p, wsb, st));
    const uint64_t k = dmin<uint64_t>(*count_out, capacity);
    if (k) {
        SFX_HIP(hipMemcpyAsync(begin, db, k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SFX_HIP(hipMemcpyAsync(end, de, k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SFX_HIP(hipMemcpyAsync(period, dp, k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}

// ---- LZ77 factorization from the EARLIER repeat lengths, and its decoder (include/suffix_hip.h) -----------------
uint64_t sfx_lz_parse_workspace_bytes(uint64_t n) { return lz_parse_workspace_bytes(n); }
int sfx_lz_parse_dev(const uint32_t* d_rep, const uint32_t* d_src, const uint8_t* d_text, uint64_t n, uint32_t min_len, uint32_t* d_begin,
                     uint32_t* d_len, uint32_t* d_psrc, uint8_t* d_lit, uint64_t capacity, uint64_t* count_out, void* d_workspace,
                     uint64_t workspace_bytes, void* stream)
{
    SFX_NEED_U32(d_rep, d_src, d_begin, d_len, d_psrc);
    SFX_NEED_WS(d_workspace, workspace_bytes, lz_parse_workspace_bytes(n));
    return lz_parse_dev(d_rep, d_src, d_text, n, min_len, d_begin, d_len, d_psrc, d_lit, capacity, count_out, d_workspace, workspace_bytes,
                        (hipStream_t)stream);
}
uint64_t sfx_lz_decode_workspace_bytes(uint64_t n, uint64_t z) { return lz_decode_workspace_bytes(n, z); }
int sfx_lz_decode_dev(const uint32_t* d_len, const uint32_t* d_psrc, const uint8_t* d_lit, uint64_t z, uint64_t n, uint8_t* d_text_out,
                      void* d_workspace, uint64_t workspace_bytes, void* stream)
{
    SFX_NEED_U32(d_len, d_psrc);
    SFX_NEED_WS(d_workspace, workspace_bytes, lz_decode_workspace_bytes(n, z));
    return lz_decode_dev(d_len, d_psrc, d_lit, z, n, d_text_out, d_workspace, workspace_bytes, (hipStream_t)stream);
}
int sfx_lz77_u32(const uint8_t* text, uint64_t n, const uint32_t* sa, const uint32_t* lcp, uint32_t min_len, uint32_t* begin_out,
                 uint32_t* len_out, uint32_t* src_out, uint8_t* lit_out, uint64_t capacity, uint64_t* count_out)
{
    if (!count_out || min_len == 0) return SFX_ERR_ARG;
    *count_out = 0;
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!text || (capacity && (!len_out || !src_out || !lit_out))) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    if (capacity > n) capacity = n;                                      // (no parse is longer)
    const uint64_t bytes = n * sizeof(uint32_t);
    const uint64_t wsb = dmax(dmax(sa ? (lcp ? 0 : lcp_workspace_bytes(n)) : sa_lcp_workspace_bytes(n),
                                   repeat_lens_workspace_bytes(n, SFX_REP_EARLIER)), lz_parse_workspace_bytes(n));
    // (seven buffers, not ten: the pool keeps kPoolMaxBuffers, and a loop at one size is to allocate once -- the phrase
    // arrays are carved from one)
    struct Carved { void* p = nullptr; } db, dn, dp, dc;
    DevBuf dt, ds, dl, dr, dq, dout, dw;
    SFX_TRY(dt.alloc(n));
    SFX_TRY(ds.alloc(bytes));
    SFX_TRY(dl.alloc(bytes));
    SFX_TRY(dr.alloc(bytes));
    SFX_TRY(dq.alloc(bytes));
    ArenaSizer osz;
    for (int i = 0; i < 3; i++) osz.take<uint32_t>(capacity);
    osz.take<uint8_t>(capacity);
    SFX_TRY(dout.alloc(osz.used));
    Arena oa(dout.p, dmax<uint64_t>(osz.used, 1));
    db.p = oa.take<uint32_t>(capacity);
    dn.p = oa.take<uint32_t>(capacity);
    dp.p = oa.take<uint32_t>(capacity);
    dc.p = oa.take<uint8_t>(capacity);
    if (oa.overflow) return SFX_ERR_INTERNAL;
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    SFX_HIP(hipMemcpyAsync(dt.p, text, n, hipMemcpyHostToDevice, st));
    if (!sa) {
        SFX_TRY(build_sa_lcp_u32_dev((const uint8_t*)dt.p, n, (uint32_t*)ds.p, (uint32_t*)dl.p, dw.p, wsb, st));
    } else {
        SFX_HIP(hipMemcpyAsync(ds.p, sa, bytes, hipMemcpyHostToDevice, st));
        if (lcp)
            SFX_HIP(hipMemcpyAsync(dl.p, lcp, bytes, hipMemcpyHostToDevice, st));
        else
            SFX_TRY(build_lcp_u32_dev((const uint8_t*)dt.p, n, (const uint32_t*)ds.p, (uint32_t*)dl.p, dw.p, wsb, st));
    }
    SFX_TRY(repeat_lens_dev((const uint32_t*)ds.p, (const uint32_t*)dl.p, nullptr, n, SFX_REP_EARLIER, (uint32_t*)dr.p, (uint32_t*)dq.p, dw.p,
                            wsb, st));
    SFX_TRY(lz_parse_dev((const uint32_t*)dr.p, (const uint32_t*)dq.p, (const uint8_t*)dt.p, n, min_len, begin_out ? (uint32_t*)db.p : nullptr,
                         (uint32_t*)dn.p, (uint32_t*)dp.p, (uint8_t*)dc.p, capacity, count_out, dw.p, wsb, st));
    const uint64_t k = dmin<uint64_t>(*count_out, capacity);
    if (k) {
        if (begin_out) SFX_HIP(hipMemcpyAsync(begin_out, db.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SFX_HIP(hipMemcpyAsync(len_out, dn.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SFX_HIP(hipMemcpyAsync(src_out, dp.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SFX_HIP(hipMemcpyAsync(lit_out, dc.p, k, hipMemcpyDeviceToHost, st));
    }
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}
int sfx_unlz(const uint32_t* len, const uint32_t* src, const uint8_t* lit, uint64_t z, uint64_t n, uint8_t* text_out)
{
    if (n > 0xFFFFFFFFull || z > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return z == 0 ? SFX_OK : SFX_ERR_ARG;
    if (z == 0 || z > n || !len || !src || !lit || !text_out) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    const uint64_t wsb = lz_decode_workspace_bytes(n, z);
    DevBuf dn, dp, dc, dt, dw;
    SFX_TRY(dn.alloc(z * sizeof(uint32_t)));
    SFX_TRY(dp.alloc(z * sizeof(uint32_t)));
    SFX_TRY(dc.alloc(z));
    SFX_TRY(dt.alloc(n));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};
    SFX_HIP(hipMemcpyAsync(dn.p, len, z * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(dp.p, src, z * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(dc.p, lit, z, hipMemcpyHostToDevice, st));
    SFX_TRY(lz_decode_dev((const uint32_t*)dn.p, (const uint32_t*)dp.p, (const uint8_t*)dc.p, z, n, (uint8_t*)dt.p, dw.p, wsb, st));
    SFX_HIP(hipMemcpyAsync(text_out, dt.p, n, hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}

// ---- maximal exact matches of a query text (include/suffix_hip.h) ---------------------------------------------
uint64_t sfx_mems_workspace_bytes(uint64_t m, uint64_t pair_limit) { return mems_workspace_bytes(m, pair_limit); }
#define SFX_MEM_TAIL_PARAMS                                                                                                     \
    uint32_t min_len, uint32_t flags, uint64_t pair_limit, uint32_t *d_qpos, uint32_t *d_tpos, uint32_t *d_len, uint64_t capacity, \
        uint64_t *pairs_out, uint64_t *count_out, void *d_workspace, uint64_t workspace_bytes, void *stream
#define SFX_MEM_TAIL_ARGS \
    min_len, flags, pair_limit, d_qpos, d_tpos, d_len, capacity, pairs_out, count_out, d_workspace, workspace_bytes, (hipStream_t)stream
int sfx_mems_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint8_t* d_query, uint64_t m, SFX_MEM_TAIL_PARAMS)
{
    SFX_NEED_U32(d_sa, d_qpos, d_tpos, d_len);
    SFX_NEED_WS(d_workspace, workspace_bytes, mems_workspace_bytes(m, pair_limit));
    const MemSource s = {d_text, n, d_sa, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, 0};
    return mems_dev(s, d_query, m, SFX_MEM_TAIL_ARGS);
}
int sfx_index_mems_dev(const sfx_index* ix, const uint8_t* d_query, uint64_t m, SFX_MEM_TAIL_PARAMS)
{
    SFX_NEED_U32(d_qpos, d_tpos, d_len);
    if (!ix) return SFX_ERR_ARG;
    SFX_NEED_WS(d_workspace, workspace_bytes, mems_workspace_bytes(m, pair_limit));
    // (a directory that was never built, or a cap below its k symbols, takes the whole-table search: match_stats_dir_dev)
    const MemSource s = {ix->d_text, ix->n, ix->d_sa, ix->d_dir, ix->d_lut, ix->bits, ix->k, ix->dbits, nullptr, nullptr, 0};
    return mems_dev(s, d_query, m, SFX_MEM_TAIL_ARGS);
}
int sfx_gindex_mems_dev(const sfx_gindex* gx, const uint8_t* d_query, uint64_t m, SFX_MEM_TAIL_PARAMS)
{
    SFX_NEED_U32(d_qpos, d_tpos, d_len);
    if (!gx) return SFX_ERR_ARG;
    SFX_NEED_WS(d_workspace, workspace_bytes, mems_workspace_bytes(m, pair_limit));
    if (gx->n && (!gx->d_starts || !gx->d_da || gx->ndocs == 0)) return SFX_ERR_ARG;
    const MemSource s = {gx->d_text, gx->n, gx->d_sa, nullptr, nullptr, 0, 0, 0, gx->d_starts, gx->d_da, gx->ndocs};
    return mems_dev(s, d_query, m, SFX_MEM_TAIL_ARGS);
}
#undef SFX_MEM_TAIL_PARAMS
#undef SFX_MEM_TAIL_ARGS
// host buffers staged through HBM on the calling thread's stream; exactly one of ix / gx is given
static int mems_host(const sfx_index* ix, const sfx_gindex* gx, const uint8_t* query, uint64_t m, uint32_t min_len, uint32_t flags,
                     uint64_t pair_limit, uint32_t* qpos_out, uint32_t* tpos_out, uint32_t* len_out, uint64_t capacity,
                     uint64_t* pairs_out, uint64_t* count_out)
{
    if ((!ix && !gx) || !pairs_out || !count_out || min_len == 0 || pair_limit == 0 || (flags & ~(uint32_t)SFX_MEM_UNIQUE)) return SFX_ERR_ARG;
    *pairs_out = *count_out = 0;
    const uint64_t n = ix ? ix->n : gx->n;
    if (m > 0xFFFFFFFFull || n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (capacity && (!qpos_out || !tpos_out || !len_out)) return SFX_ERR_ARG;
    if (m == 0 || n == 0 || min_len > dmin(m, n)) return SFX_OK;
    if (!query) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    pair_limit = dmin(pair_limit, m * n);                                // (P cannot be larger: the workspace need not be either)
    capacity = dmin(capacity, pair_limit);
    const uint64_t wsb = mems_workspace_bytes(m, pair_limit), cb = capacity * sizeof(uint32_t);
    DevBuf dq, di, dp, dl, dw;
    SFX_TRY(dq.alloc(m));
    SFX_TRY(di.alloc(cb));
    SFX_TRY(dp.alloc(cb));
    SFX_TRY(dl.alloc(cb));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    SFX_HIP(hipMemcpyAsync(dq.p, query, m, hipMemcpyHostToDevice, st));
    uint32_t *oi = capacity ? (uint32_t*)di.p : nullptr, *op = capacity ? (uint32_t*)dp.p : nullptr, *ol = capacity ? (uint32_t*)dl.p : nullptr;
    if (ix)
        SFX_TRY(sfx_index_mems_dev(ix, (const uint8_t*)dq.p, m, min_len, flags, pair_limit, oi, op, ol, capacity, pairs_out, count_out, dw.p,
                                   wsb, st));
    else
        SFX_TRY(sfx_gindex_mems_dev(gx, (const uint8_t*)dq.p, m, min_len, flags, pair_limit, oi, op, ol, capacity, pairs_out, count_out, dw.p,
                                    wsb, st));
    const uint64_t k = dmin<uint64_t>(*count_out, capacity);
    if (k) {
        SFX_HIP(hipMemcpyAsync(qpos_out, di.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SFX_HIP(hipMemcpyAsync(tpos_out, dp.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SFX_HIP(hipMemcpyAsync(len_out, dl.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}
int sfx_index_mems(const sfx_index* ix, const uint8_t* query, uint64_t m, uint32_t min_len, uint32_t flags, uint64_t pair_limit,
                   uint32_t* qpos_out, uint32_t* tpos_out, uint32_t* len_out, uint64_t capacity, uint64_t* pairs_out, uint64_t* count_out)
{
    return mems_host(ix, nullptr, query, m, min_len, flags, pair_limit, qpos_out, tpos_out, len_out, capacity, pairs_out, count_out);
}
int sfx_gindex_mems(const sfx_gindex* gx, const uint8_t* query, uint64_t m, uint32_t min_len, uint32_t flags, uint64_t pair_limit,
                    uint32_t* qpos_out, uint32_t* tpos_out, uint32_t* len_out, uint64_t capacity, uint64_t* pairs_out, uint64_t* count_out)
{
    return mems_host(nullptr, gx, query, m, min_len, flags, pair_limit, qpos_out, tpos_out, len_out, capacity, pairs_out, count_out);
}

// ---- k-mismatch pattern search (include/suffix_hip.h) ------------------------------------
uint64_t sfx_hamming_workspace_bytes(uint64_t nq, uint32_t max_mismatches, uint64_t cand_limit)
{
    return hamming_workspace_bytes(nq, max_mismatches, cand_limit);
}
#define SFX_HM_TAIL_PARAMS                                                                                                      \
    const uint8_t *d_qbytes, const uint64_t *d_qoff, uint64_t nq, uint32_t max_mismatches, uint64_t cand_limit, uint32_t *d_pattern, \
        uint32_t *d_tpos, uint8_t *d_mism, uint64_t capacity, uint64_t *d_first, uint64_t *cands_out, uint64_t *count_out,       \
        void *d_workspace, uint64_t workspace_bytes, void *stream
#define SFX_HM_TAIL_ARGS                                                                                                       \
    d_qbytes, d_qoff, nq, max_mismatches, cand_limit, d_pattern, d_tpos, d_mism, capacity, d_first, cands_out, count_out, d_workspace, \
        workspace_bytes, (hipStream_t)stream
#define SFX_HM_NEED()                                                                                          \
    SFX_NEED_U64(d_qoff, d_first);                                                                             \
    SFX_NEED_U32(d_pattern, d_tpos);                                                                           \
    SFX_NEED_WS(d_workspace, workspace_bytes, hamming_workspace_bytes(nq, max_mismatches, cand_limit))
int sfx_hamming_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, SFX_HM_TAIL_PARAMS)
{
    SFX_NEED_U32(d_sa);
    SFX_HM_NEED();
    const HmSource s = {d_text, n, d_sa, nullptr, nullptr, 0};
    auto search = [&](const uint8_t* q, const uint64_t* po, uint64_t np, uint32_t* lo, uint32_t* hi, hipStream_t st) {
        return query_batch_dev(d_text, n, d_sa, n, q, po, np, lo, hi, nullptr, nullptr, st);
    };
    return hamming_dev(s, search, SFX_HM_TAIL_ARGS);
}
int sfx_index_hamming_dev(const sfx_index* ix, SFX_HM_TAIL_PARAMS)
{
    SFX_HM_NEED();
    if (!ix) return SFX_ERR_ARG;
    const HmSource s = {ix->d_text, ix->n, ix->d_sa, nullptr, nullptr, 0};
    // the directory and the key tree, as for any batch; the tree's phase-2 scratch belongs to the calling thread
    auto search = [&](const uint8_t* q, const uint64_t* po, uint64_t np, uint32_t* lo, uint32_t* hi, hipStream_t st) {
        return sfx_index_query_dev(ix, q, po, np, lo, hi, nullptr, nullptr, st);
    };
    return hamming_dev(s, search, SFX_HM_TAIL_ARGS);
}
int sfx_gindex_hamming_dev(const sfx_gindex* gx, SFX_HM_TAIL_PARAMS)
{
    SFX_HM_NEED();
    if (!gx) return SFX_ERR_ARG;
    if (gx->n && (!gx->d_starts || !gx->d_da || gx->ndocs == 0)) return SFX_ERR_ARG;
    const HmSource s = {gx->d_text, gx->n, gx->d_sa, gx->d_starts, gx->d_da, gx->ndocs};
    auto search = [&](const uint8_t* q, const uint64_t* po, uint64_t np, uint32_t* lo, uint32_t* hi, hipStream_t st) {
        return gindex_query_dev(gx->d_text, gx->n, gx->d_starts, gx->ndocs, gx->d_sa, gx->d_da, gx->d_prev, q, po, np, lo, hi, nullptr,
                                nullptr, nullptr, nullptr, 0, st);
    };
    return hamming_dev(s, search, SFX_HM_TAIL_ARGS);
}
#undef SFX_HM_TAIL_PARAMS
#undef SFX_HM_TAIL_ARGS
#undef SFX_HM_NEED
// host buffers staged through HBM on the calling thread's stream; exactly one of ix / gx is given
static int hamming_host(const sfx_index* ix, const sfx_gindex* gx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t nq, uint32_t k,
                        uint64_t cand_limit, uint32_t* pattern_out, uint32_t* tpos_out, uint8_t* mism_out, uint64_t capacity,
                        uint64_t* first_out, uint64_t* cands_out, uint64_t* count_out)
{
    if ((!ix && !gx) || !cands_out || !count_out || cand_limit == 0 || k > kHmMaxK) return SFX_ERR_ARG;
    *cands_out = *count_out = 0;
    const uint64_t n = ix ? ix->n : gx->n;
    if (n > 0xFFFFFFFFull || (nq && hm_piece_count(nq, k) == 0)) return SFX_ERR_TOO_LARGE;
    if (capacity && (!pattern_out || !tpos_out || !mism_out)) return SFX_ERR_ARG;
    if (nq && !qoff) return SFX_ERR_ARG;
    if (nq == 0 || n == 0) {
        if (first_out) memset(first_out, 0, (nq + 1) * sizeof(uint64_t));
        return SFX_OK;
    }
    for (uint64_t j = 0; j < nq; j++) {
        if (qoff[j + 1] < qoff[j]) return SFX_ERR_ARG;
        if (qoff[j + 1] - qoff[j] > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    }
    const uint64_t qtotal = qoff[nq];
    if (qtotal && !qbytes) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    cand_limit = dmin(cand_limit, nq * (k + 1) * n);                       // (C cannot be larger: the workspace need not be either)
    capacity = dmin(capacity, cand_limit);
    const uint64_t wsb = hamming_workspace_bytes(nq, k, cand_limit);
    DevBuf dq, doff, dj, dp, dm, df, dw;
    SFX_TRY(dq.alloc(dmax<uint64_t>(qtotal, 1)));
    SFX_TRY(doff.alloc((nq + 1) * sizeof(uint64_t)));
    SFX_TRY(dj.alloc(capacity * sizeof(uint32_t)));
    SFX_TRY(dp.alloc(capacity * sizeof(uint32_t)));
    SFX_TRY(dm.alloc(capacity));
    if (first_out) SFX_TRY(df.alloc((nq + 1) * sizeof(uint64_t)));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    if (qtotal) SFX_HIP(hipMemcpyAsync(dq.p, qbytes, qtotal, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(doff.p, qoff, (nq + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    uint32_t *oj = capacity ? (uint32_t*)dj.p : nullptr, *op = capacity ? (uint32_t*)dp.p : nullptr;
    uint8_t* om = capacity ? (uint8_t*)dm.p : nullptr;
    if (ix)
        SFX_TRY(sfx_index_hamming_dev(ix, (const uint8_t*)dq.p, (const uint64_t*)doff.p, nq, k, cand_limit, oj, op, om, capacity,
                                      (uint64_t*)df.p, cands_out, count_out, dw.p, wsb, st));
    else
        SFX_TRY(sfx_gindex_hamming_dev(gx, (const uint8_t*)dq.p, (const uint64_t*)doff.p, nq, k, cand_limit, oj, op, om, capacity,
                                       (uint64_t*)df.p, cands_out, count_out, dw.p, wsb, st));
    if (*cands_out > cand_limit) return SFX_OK;                            // (refused: nothing was written)
    const uint64_t z = dmin<uint64_t>(*count_out, capacity);
    if (z) {
        SFX_HIP(hipMemcpyAsync(pattern_out, dj.p, z * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SFX_HIP(hipMemcpyAsync(tpos_out, dp.p, z * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SFX_HIP(hipMemcpyAsync(mism_out, dm.p, z, hipMemcpyDeviceToHost, st));
    }
    if (first_out) SFX_HIP(hipMemcpyAsync(first_out, df.p, (nq + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}
int sfx_index_hamming(const sfx_index* ix, const uint8_t* qbytes, const uint64_t* qoff, uint64_t nq, uint32_t max_mismatches,
                      uint64_t cand_limit, uint32_t* pattern_out, uint32_t* tpos_out, uint8_t* mism_out, uint64_t capacity,
                      uint64_t* first_out, uint64_t* cands_out, uint64_t* count_out)
{
    return hamming_host(ix, nullptr, qbytes, qoff, nq, max_mismatches, cand_limit, pattern_out, tpos_out, mism_out, capacity, first_out,
                        cands_out, count_out);
}
int sfx_gindex_hamming(const sfx_gindex* gx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t nq, uint32_t max_mismatches,
                       uint64_t cand_limit, uint32_t* pattern_out, uint32_t* tpos_out, uint8_t* mism_out, uint64_t capacity,
                       uint64_t* first_out, uint64_t* cands_out, uint64_t* count_out)
{
    return hamming_host(nullptr, gx, qbytes, qoff, nq, max_mismatches, cand_limit, pattern_out, tpos_out, mism_out, capacity, first_out,
                        cands_out, count_out);
}

// ---- k-error pattern search (include/suffix_hip.h) ----------------------------------------
uint64_t sfx_edit_workspace_bytes(uint64_t nq, uint32_t max_errors, uint64_t cand_limit, uint64_t hit_limit)
{
    return edit_workspace_bytes(nq, max_errors, cand_limit, hit_limit);
}
#define SFX_ED_TAIL_PARAMS                                                                                                      \
    const uint8_t *d_qbytes, const uint64_t *d_qoff, uint64_t nq, uint32_t max_errors, uint64_t cand_limit, uint64_t hit_limit,  \
        uint32_t *d_pattern, uint32_t *d_tbegin, uint32_t *d_tend, uint8_t *d_dist, uint64_t capacity, uint64_t *d_first,        \
        uint64_t *cands_out, uint64_t *hits_out, uint64_t *count_out, void *d_workspace, uint64_t workspace_bytes, void *stream
#define SFX_ED_TAIL_ARGS                                                                                                        \
    d_qbytes, d_qoff, nq, max_errors, cand_limit, hit_limit, d_pattern, d_tbegin, d_tend, d_dist, capacity, d_first, cands_out,  \
        hits_out, count_out, d_workspace, workspace_bytes, (hipStream_t)stream
#define SFX_ED_NEED()                                                                                          \
    SFX_NEED_U64(d_qoff, d_first);                                                                             \
    SFX_NEED_U32(d_pattern, d_tbegin, d_tend);                                                                 \
    SFX_NEED_WS(d_workspace, workspace_bytes, edit_workspace_bytes(nq, max_errors, cand_limit, hit_limit))
int sfx_edit_dev(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, SFX_ED_TAIL_PARAMS)
{
    SFX_NEED_U32(d_sa);
    SFX_ED_NEED();
    const HmSource s = {d_text, n, d_sa, nullptr, nullptr, 0};
    auto search = [&](const uint8_t* q, const uint64_t* po, uint64_t np, uint32_t* lo, uint32_t* hi, hipStream_t st) {
        return query_batch_dev(d_text, n, d_sa, n, q, po, np, lo, hi, nullptr, nullptr, st);
    };
    return edit_dev(s, search, SFX_ED_TAIL_ARGS);
}
int sfx_index_edit_dev(const sfx_index* ix, SFX_ED_TAIL_PARAMS)
{
    SFX_ED_NEED();
    if (!ix) return SFX_ERR_ARG;
    const HmSource s = {ix->d_text, ix->n, ix->d_sa, nullptr, nullptr, 0};
    // the directory and the key tree, as for any batch; the tree's phase-2 scratch belongs to the calling thread
    auto search = [&](const uint8_t* q, const uint64_t* po, uint64_t np, uint32_t* lo, uint32_t* hi, hipStream_t st) {
        return sfx_index_query_dev(ix, q, po, np, lo, hi, nullptr, nullptr, st);
    };
    return edit_dev(s, search, SFX_ED_TAIL_ARGS);
}
int sfx_gindex_edit_dev(const sfx_gindex* gx, SFX_ED_TAIL_PARAMS)
{
    SFX_ED_NEED();
    if (!gx) return SFX_ERR_ARG;
    if (gx->n && (!gx->d_starts || !gx->d_da || gx->ndocs == 0)) return SFX_ERR_ARG;
    const HmSource s = {gx->d_text, gx->n, gx->d_sa, gx->d_starts, gx->d_da, gx->ndocs};
    auto search = [&](const uint8_t* q, const uint64_t* po, uint64_t np, uint32_t* lo, uint32_t* hi, hipStream_t st) {
        return gindex_query_dev(gx->d_text, gx->n, gx->d_starts, gx->ndocs, gx->d_sa, gx->d_da, gx->d_prev, q, po, np, lo, hi, nullptr,
                                nullptr, nullptr, nullptr, 0, st);
    };
    return edit_dev(s, search, SFX_ED_TAIL_ARGS);
}
#undef SFX_ED_TAIL_PARAMS
#undef SFX_ED_TAIL_ARGS
#undef SFX_ED_NEED
// host buffers staged through HBM on the calling thread's stream; exactly one of ix / gx is given
static int edit_host(const sfx_index* ix, const sfx_gindex* gx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t nq, uint32_t k,
                     uint64_t cand_limit, uint64_t hit_limit, uint32_t* pattern_out, uint32_t* tbegin_out, uint32_t* tend_out,
                     uint8_t* dist_out, uint64_t capacity, uint64_t* first_out, uint64_t* cands_out, uint64_t* hits_out, uint64_t* count_out)
{
    if ((!ix && !gx) || !cands_out || !hits_out || !count_out || cand_limit == 0 || hit_limit == 0 || hit_limit > kEdMaxHits || k > kEdMaxK)
        return SFX_ERR_ARG;
    *cands_out = *hits_out = *count_out = 0;
    const uint64_t n = ix ? ix->n : gx->n;
    if (n > 0xFFFFFFFFull || (nq && ed_piece_count(nq, k) == 0)) return SFX_ERR_TOO_LARGE;
    if (capacity && (!pattern_out || !tbegin_out || !tend_out || !dist_out)) return SFX_ERR_ARG;
    if (nq && !qoff) return SFX_ERR_ARG;
    if (nq == 0 || n == 0) {
        if (first_out) memset(first_out, 0, (nq + 1) * sizeof(uint64_t));
        return SFX_OK;
    }
    for (uint64_t j = 0; j < nq; j++) {
        if (qoff[j + 1] < qoff[j]) return SFX_ERR_ARG;
        if (qoff[j + 1] - qoff[j] > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    }
    for (uint64_t j = 0; j < nq; j++)
        if (qoff[j + 1] - qoff[j] <= k) return SFX_ERR_ARG;
    const uint64_t qtotal = qoff[nq];
    if (qtotal && !qbytes) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    cand_limit = dmin(cand_limit, nq * (k + 1) * n);                       // (C cannot be larger: the workspace need not be either)
    hit_limit = dmin(hit_limit, ed_hit_room(nq * (k + 1), k, cand_limit, hit_limit));
    capacity = dmin(capacity, dmin(hit_limit, nq * (n + 1)));              // (an occurrence per pattern and end at the most)
    const uint64_t wsb = edit_workspace_bytes(nq, k, cand_limit, hit_limit);
    DevBuf dq, doff, dj, db, de, dd, df, dw;
    SFX_TRY(dq.alloc(dmax<uint64_t>(qtotal, 1)));
    SFX_TRY(doff.alloc((nq + 1) * sizeof(uint64_t)));
    SFX_TRY(dj.alloc(capacity * sizeof(uint32_t)));
    SFX_TRY(db.alloc(capacity * sizeof(uint32_t)));
    SFX_TRY(de.alloc(capacity * sizeof(uint32_t)));
    SFX_TRY(dd.alloc(capacity));
    if (first_out) SFX_TRY(df.alloc((nq + 1) * sizeof(uint64_t)));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    SFX_HIP(hipMemcpyAsync(dq.p, qbytes, qtotal, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(doff.p, qoff, (nq + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    uint32_t *oj = capacity ? (uint32_t*)dj.p : nullptr, *ob = capacity ? (uint32_t*)db.p : nullptr, *oe = capacity ? (uint32_t*)de.p : nullptr;
    uint8_t* od = capacity ? (uint8_t*)dd.p : nullptr;
    if (ix)
        SFX_TRY(sfx_index_edit_dev(ix, (const uint8_t*)dq.p, (const uint64_t*)doff.p, nq, k, cand_limit, hit_limit, oj, ob, oe, od, capacity,
                                   (uint64_t*)df.p, cands_out, hits_out, count_out, dw.p, wsb, st));
    else
        SFX_TRY(sfx_gindex_edit_dev(gx, (const uint8_t*)dq.p, (const uint64_t*)doff.p, nq, k, cand_limit, hit_limit, oj, ob, oe, od, capacity,
                                    (uint64_t*)df.p, cands_out, hits_out, count_out, dw.p, wsb, st));
    if (*cands_out > cand_limit || *hits_out > hit_limit) return SFX_OK;   // (refused: nothing was written)
    const uint64_t z = dmin<uint64_t>(*count_out, capacity);
    if (z) {
        SFX_HIP(hipMemcpyAsync(pattern_out, dj.p, z * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SFX_HIP(hipMemcpyAsync(tbegin_out, db.p, z * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SFX_HIP(hipMemcpyAsync(tend_out, de.p, z * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SFX_HIP(hipMemcpyAsync(dist_out, dd.p, z, hipMemcpyDeviceToHost, st));
    }
    if (first_out) SFX_HIP(hipMemcpyAsync(first_out, df.p, (nq + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}
int sfx_index_edit(const sfx_index* ix, const uint8_t* qbytes, const uint64_t* qoff, uint64_t nq, uint32_t max_errors, uint64_t cand_limit,
                   uint64_t hit_limit, uint32_t* pattern_out, uint32_t* tbegin_out, uint32_t* tend_out, uint8_t* dist_out, uint64_t capacity,
                   uint64_t* first_out, uint64_t* cands_out, uint64_t* hits_out, uint64_t* count_out)
{
    return edit_host(ix, nullptr, qbytes, qoff, nq, max_errors, cand_limit, hit_limit, pattern_out, tbegin_out, tend_out, dist_out, capacity,
                     first_out, cands_out, hits_out, count_out);
}
int sfx_gindex_edit(const sfx_gindex* gx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t nq, uint32_t max_errors, uint64_t cand_limit,
                    uint64_t hit_limit, uint32_t* pattern_out, uint32_t* tbegin_out, uint32_t* tend_out, uint8_t* dist_out, uint64_t capacity,
                    uint64_t* first_out, uint64_t* cands_out, uint64_t* hits_out, uint64_t* count_out)
{
    return edit_host(nullptr, gx, qbytes, qoff, nq, max_errors, cand_limit, hit_limit, pattern_out, tbegin_out, tend_out, dist_out, capacity,
                     first_out, cands_out, hits_out, count_out);
}

// ---- suffix-tree topology, generalized suffix array -------------------------------------------
uint64_t sfx_lcp_intervals_workspace_bytes(uint64_t n) { return lcp_intervals_workspace_bytes(n); }
int sfx_lcp_intervals_dev(const uint32_t* d_lcp, uint64_t n, uint32_t* d_lb, uint32_t* d_rb, uint32_t* d_node,
                          uint32_t* d_parent, uint32_t* d_leaf_parent, void* d_workspace, uint64_t workspace_bytes,
                          void* stream)
{
    SFX_NEED_U32(d_lcp, d_lb, d_rb, d_node, d_parent, d_leaf_parent);
    SFX_NEED_WS(d_workspace, workspace_bytes, lcp_intervals_workspace_bytes(n));
    return lcp_intervals_dev(d_lcp, n, d_lb, d_rb, d_node, d_parent, d_leaf_parent, d_workspace, workspace_bytes,
                             (hipStream_t)stream);
}
int sfx_doc_lookup_dev(const uint32_t* d_positions, uint64_t count, const uint64_t* d_doc_starts, uint64_t ndocs,
                       uint32_t* d_doc, uint32_t* d_offset, void* stream)
{
    SFX_NEED_U64(d_doc_starts);
    SFX_NEED_U32(d_positions, d_doc, d_offset);
    return doc_lookup_dev(d_positions, count, d_doc_starts, ndocs, d_doc, d_offset, (hipStream_t)stream);
}

// ---- suffix-tree node table ---------------------------------------------------------------------------------
uint64_t sfx_suffix_tree_workspace_bytes(uint64_t n) { return suffix_tree_workspace_bytes(n); }
int sfx_suffix_tree_dev(const uint8_t* d_text, const uint32_t* d_sa, const uint32_t* d_lcp, uint64_t n, uint64_t node_capacity,
                        uint64_t child_capacity, uint32_t* d_node_lb, uint32_t* d_node_rb, uint32_t* d_node_depth,
                        uint32_t* d_node_parent, uint32_t* d_node_terminal, uint64_t* d_child_off, uint32_t* d_child_lb,
                        uint32_t* d_child_node, uint8_t* d_child_byte, uint32_t* d_leaf_parent, uint64_t* nodes_out,
                        uint64_t* children_out, void* d_workspace, uint64_t workspace_bytes, void* stream)
{
    SFX_NEED_U64(d_child_off);
    SFX_NEED_U32(d_sa, d_lcp, d_node_lb, d_node_rb, d_node_depth, d_node_parent, d_node_terminal, d_child_lb, d_child_node,
                 d_leaf_parent);
    SFX_NEED_WS(d_workspace, workspace_bytes, suffix_tree_workspace_bytes(n));
    return suffix_tree_dev(d_text, d_sa, d_lcp, n, node_capacity, child_capacity, d_node_lb, d_node_rb, d_node_depth, d_node_parent,
                           d_node_terminal, d_child_off, d_child_lb, d_child_node, d_child_byte, d_leaf_parent, nodes_out,
                           children_out, d_workspace, workspace_bytes, (hipStream_t)stream);
}
int sfx_suffix_tree_u32(const uint8_t* text, const uint32_t* sa, const uint32_t* lcp, uint64_t n, uint64_t node_capacity,
                        uint64_t child_capacity, uint32_t* node_lb, uint32_t* node_rb, uint32_t* node_depth, uint32_t* node_parent,
                        uint32_t* node_terminal, uint64_t* child_off, uint32_t* child_lb, uint32_t* child_node, uint8_t* child_byte,
                        uint32_t* leaf_parent, uint64_t* nodes_out, uint64_t* children_out)
{
    if (!nodes_out || !children_out) return SFX_ERR_ARG;
    *nodes_out = 0;
    *children_out = 0;
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if ((text == nullptr) != (child_byte == nullptr)) return SFX_ERR_ARG;
    if (n == 0) return SFX_OK;
    if (!sa || !lcp) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    if (node_capacity > n) node_capacity = n;                            // (no table is longer)
    if (child_capacity > 2 * n) child_capacity = 2 * n;
    const bool fill = node_lb && node_rb && node_depth && node_parent && node_terminal && child_off && child_lb && child_node;
    DevBuf dt, ds, dl, dn[5], doff, dc[2], db, dp, dw;
    const uint64_t wsb = suffix_tree_workspace_bytes(n), bytes = n * sizeof(uint32_t);
    if (text) SFX_TRY(dt.alloc(n));
    SFX_TRY(ds.alloc(bytes));
    SFX_TRY(dl.alloc(bytes));
    if (fill) {
        for (DevBuf& b : dn) SFX_TRY(b.alloc(node_capacity * sizeof(uint32_t)));
        SFX_TRY(doff.alloc((node_capacity + 1) * sizeof(uint64_t)));
        for (DevBuf& b : dc) SFX_TRY(b.alloc(child_capacity * sizeof(uint32_t)));
        if (child_byte) SFX_TRY(db.alloc(child_capacity));
        if (leaf_parent) SFX_TRY(dp.alloc(bytes));
    }
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    if (text) SFX_HIP(hipMemcpyAsync(dt.p, text, n, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(ds.p, sa, bytes, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(dl.p, lcp, bytes, hipMemcpyHostToDevice, st));
    SFX_TRY(suffix_tree_dev((const uint8_t*)dt.p, (const uint32_t*)ds.p, (const uint32_t*)dl.p, n, fill ? node_capacity : 0,
                            fill ? child_capacity : 0, (uint32_t*)dn[0].p, (uint32_t*)dn[1].p, (uint32_t*)dn[2].p, (uint32_t*)dn[3].p,
                            (uint32_t*)dn[4].p, (uint64_t*)doff.p, (uint32_t*)dc[0].p, (uint32_t*)dc[1].p, (uint8_t*)db.p,
                            (uint32_t*)dp.p, nodes_out, children_out, dw.p, wsb, st));
    const uint64_t m = *nodes_out, c = *children_out;
    if (m > node_capacity || c > child_capacity) return SFX_OK;
    if (!fill) return SFX_ERR_ARG;                                       // (room for everything, and nowhere to put it)
    uint32_t* const node_out[5] = {node_lb, node_rb, node_depth, node_parent, node_terminal};
    for (int i = 0; i < 5; i++) SFX_HIP(hipMemcpyAsync(node_out[i], dn[i].p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SFX_HIP(hipMemcpyAsync(child_off, doff.p, (m + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (c) {
        SFX_HIP(hipMemcpyAsync(child_lb, dc[0].p, c * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SFX_HIP(hipMemcpyAsync(child_node, dc[1].p, c * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (child_byte) SFX_HIP(hipMemcpyAsync(child_byte, db.p, c, hipMemcpyDeviceToHost, st));
    }
    if (leaf_parent) SFX_HIP(hipMemcpyAsync(leaf_parent, dp.p, bytes, hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}

// ---- generalized suffix array over documents ------------------------------------------------------------
uint64_t sfx_gsa_workspace_bytes(uint64_t n, uint64_t ndocs)
{
    (void)ndocs;                                       // (the document starts are read in place)
    return gsa_workspace_bytes(n);
}
int sfx_build_gsa_u32_dev(const uint8_t* d_text, uint64_t n, const uint64_t* d_doc_starts, uint64_t ndocs, uint32_t* d_sa,
                          uint32_t* d_da, uint32_t* d_lcp, void* d_workspace, uint64_t workspace_bytes, void* stream)
{
    SFX_NEED_U64(d_doc_starts);
    SFX_NEED_U32(d_sa, d_da, d_lcp);
    SFX_NEED_WS(d_workspace, workspace_bytes, gsa_workspace_bytes(n));
    return gsa_build_dev(d_text, n, d_doc_starts, ndocs, d_sa, d_da, d_lcp, d_workspace, workspace_bytes, (hipStream_t)stream);
}
int sfx_build_gsa_u32(const uint8_t* text, uint64_t n, const uint64_t* doc_starts, uint64_t ndocs, uint32_t* sa_out,
                      uint32_t* da_out, uint32_t* lcp_out)
{
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!text || !doc_starts || ndocs == 0 || !sa_out) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    DevBuf dt, dst, ds, dd, dl, dw;
    const uint64_t wsb = gsa_workspace_bytes(n);
    SFX_TRY(dt.alloc(n));
    SFX_TRY(dst.alloc(ndocs * sizeof(uint64_t)));
    SFX_TRY(ds.alloc(n * sizeof(uint32_t)));
    if (da_out) SFX_TRY(dd.alloc(n * sizeof(uint32_t)));
    if (lcp_out) SFX_TRY(dl.alloc(n * sizeof(uint32_t)));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    SFX_HIP(hipMemcpyAsync(dt.p, text, n, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(dst.p, doc_starts, ndocs * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    SFX_TRY(gsa_build_dev((const uint8_t*)dt.p, n, (const uint64_t*)dst.p, ndocs, (uint32_t*)ds.p, (uint32_t*)dd.p, (uint32_t*)dl.p,
                          dw.p, wsb, st));
    SFX_HIP(hipMemcpyAsync(sa_out, ds.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (da_out) SFX_HIP(hipMemcpyAsync(da_out, dd.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (lcp_out) SFX_HIP(hipMemcpyAsync(lcp_out, dl.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}

// ---- merge of two generalized suffix arrays (include/suffix_hip.h) -----------------
uint64_t sfx_gsa_merge_workspace_bytes(uint64_t n_a, uint64_t n_b) { return gsa_merge_workspace_bytes(n_a, n_b); }
int sfx_gsa_merge_dev(const uint8_t* d_text, const uint64_t* d_doc_starts, uint64_t ndocs, uint64_t ndocs_a, const uint32_t* d_sa_a,
                      const uint32_t* d_da_a, const uint32_t* d_lcp_a, uint64_t n_a, const uint32_t* d_sa_b, const uint32_t* d_da_b,
                      const uint32_t* d_lcp_b, uint64_t n_b, uint32_t match_limit, uint32_t* d_sa, uint32_t* d_da, uint32_t* d_lcp,
                      uint64_t* longest_out, void* d_workspace, uint64_t workspace_bytes, void* stream)
{
    if (n_a > 0xFFFFFFFFull || n_b > 0xFFFFFFFFull || n_a + n_b > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    SFX_NEED_U64(d_doc_starts);
    SFX_NEED_U32(d_sa_a, d_da_a, d_lcp_a, d_sa_b, d_da_b, d_lcp_b, d_sa, d_da, d_lcp);
    SFX_NEED_WS(d_workspace, workspace_bytes, gsa_merge_workspace_bytes(n_a, n_b));
    const GmIn in{d_text, d_doc_starts, ndocs, ndocs_a, n_a + n_b, n_a, n_b, d_sa_a, d_da_a, d_lcp_a, d_sa_b, d_da_b, d_lcp_b};
    return gsa_merge_dev(in, match_limit, d_sa, d_da, d_lcp, longest_out, d_workspace, workspace_bytes, (hipStream_t)stream);
}
// device copies of one array set; a NULL host array stays NULL on the device
struct GsaSetBufs {
    DevBuf sa, da, lcp;
    int upload(const uint32_t* h_sa, const uint32_t* h_da, const uint32_t* h_lcp, uint64_t cnt, hipStream_t st)
    {
        const uint64_t bytes = cnt * sizeof(uint32_t);
        const struct { DevBuf* d; const uint32_t* h; } all[] = {{&sa, h_sa}, {&da, h_da}, {&lcp, h_lcp}};
        for (const auto& x : all) {
            if (!x.h) continue;
            SFX_TRY(x.d->alloc(bytes));
            if (bytes) SFX_HIP(hipMemcpyAsync(x.d->p, x.h, bytes, hipMemcpyHostToDevice, st));
        }
        return SFX_OK;
    }
};
int sfx_gsa_merge_u32(const uint8_t* text, const uint64_t* doc_starts, uint64_t ndocs, uint64_t ndocs_a, const uint32_t* sa_a,
                      const uint32_t* da_a, const uint32_t* lcp_a, uint64_t n_a, const uint32_t* sa_b, const uint32_t* da_b,
                      const uint32_t* lcp_b, uint64_t n_b, uint32_t match_limit, uint32_t* sa_out, uint32_t* da_out, uint32_t* lcp_out,
                      uint64_t* longest_out)
{
    if (n_a > 0xFFFFFFFFull || n_b > 0xFFFFFFFFull || n_a + n_b > 0xFFFFFFFFull || ndocs > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (!longest_out || ndocs_a > ndocs) return SFX_ERR_ARG;
    *longest_out = 0;
    const uint64_t n = n_a + n_b, bytes = n * sizeof(uint32_t);
    if (n == 0) return SFX_OK;
    if (ndocs == 0 || !text || !doc_starts || !sa_out) return SFX_ERR_ARG;
    if ((n_a && (!sa_a || (lcp_out && !lcp_a))) || (n_b && (!sa_b || (lcp_out && !lcp_b)))) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    DevBuf dt, dst, ds, dd, dl, dw;
    GsaSetBufs A, B;
    const uint64_t wsb = gsa_merge_workspace_bytes(n_a, n_b);
    SFX_TRY(dt.alloc(n));
    SFX_TRY(dst.alloc(ndocs * sizeof(uint64_t)));
    SFX_TRY(ds.alloc(bytes));
    if (da_out) SFX_TRY(dd.alloc(bytes));
    if (lcp_out) SFX_TRY(dl.alloc(bytes));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    SFX_HIP(hipMemcpyAsync(dt.p, text, n, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(dst.p, doc_starts, ndocs * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    SFX_TRY(A.upload(n_a ? sa_a : nullptr, n_a ? da_a : nullptr, n_a ? lcp_a : nullptr, n_a, st));
    SFX_TRY(B.upload(n_b ? sa_b : nullptr, n_b ? da_b : nullptr, n_b ? lcp_b : nullptr, n_b, st));
    const GmIn in{(const uint8_t*)dt.p, (const uint64_t*)dst.p, ndocs, ndocs_a, n, n_a, n_b, (const uint32_t*)A.sa.p, (const uint32_t*)A.da.p,
                  (const uint32_t*)A.lcp.p, (const uint32_t*)B.sa.p, (const uint32_t*)B.da.p, (const uint32_t*)B.lcp.p};
    SFX_TRY(gsa_merge_dev(in, match_limit, (uint32_t*)ds.p, (uint32_t*)dd.p, (uint32_t*)dl.p, longest_out, dw.p, wsb, st));
    if (match_limit && *longest_out > match_limit) return SFX_OK;        // refused: the outputs stay as they are
    SFX_HIP(hipMemcpyAsync(sa_out, ds.p, bytes, hipMemcpyDeviceToHost, st));
    if (da_out) SFX_HIP(hipMemcpyAsync(da_out, dd.p, bytes, hipMemcpyDeviceToHost, st));
    if (lcp_out) SFX_HIP(hipMemcpyAsync(lcp_out, dl.p, bytes, hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}
int sfx_gsa_extend_u32(const uint8_t* text, uint64_t n, const uint64_t* doc_starts, uint64_t ndocs, uint64_t ndocs_a, const uint32_t* sa_a,
                       const uint32_t* da_a, const uint32_t* lcp_a, uint32_t match_limit, int rebuild_on_limit, uint32_t* sa_out,
                       uint32_t* da_out, uint32_t* lcp_out, uint64_t* longest_out, uint32_t* route_out)
{
    if (n > 0xFFFFFFFFull || ndocs > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (!longest_out || !route_out || ndocs_a > ndocs) return SFX_ERR_ARG;
    *longest_out = 0;
    *route_out = SFX_GSA_ROUTE_NONE;
    if (n == 0) { *route_out = SFX_GSA_ROUTE_MERGE; return SFX_OK; }
    if (ndocs == 0 || !text || !doc_starts || !sa_out) return SFX_ERR_ARG;
    const uint64_t n_a = ndocs_a < ndocs ? doc_starts[ndocs_a] : n;
    if (n_a > n) return SFX_ERR_ARG;
    const uint64_t n_b = n - n_a, ndocs_b = ndocs - ndocs_a, bytes = n * sizeof(uint32_t);
    if (n_a && (!sa_a || !lcp_a)) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    std::vector<uint64_t> starts_b(ndocs_b);
    for (uint64_t d = 0; d < ndocs_b; d++) starts_b[d] = doc_starts[ndocs_a + d] - n_a;   // (a start below n_a wraps: the build's check names it)
    DevBuf dt, dst, dsb, ds, dd, dl, dw, dbs, dbd, dbl;
    GsaSetBufs A;
    const uint64_t build_b = gsa_workspace_bytes(n_b), wsb = dmax(build_b, gsa_merge_workspace_bytes(n_a, n_b));
    SFX_TRY(dt.alloc(n));
    SFX_TRY(dst.alloc(ndocs * sizeof(uint64_t)));
    SFX_TRY(dsb.alloc(ndocs_b * sizeof(uint64_t)));
    SFX_TRY(ds.alloc(bytes));
    SFX_TRY(dd.alloc(bytes));
    SFX_TRY(dl.alloc(bytes));
    SFX_TRY(dbs.alloc(n_b * sizeof(uint32_t)));
    SFX_TRY(dbd.alloc(n_b * sizeof(uint32_t)));
    SFX_TRY(dbl.alloc(n_b * sizeof(uint32_t)));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    SFX_HIP(hipMemcpyAsync(dt.p, text, n, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(dst.p, doc_starts, ndocs * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (ndocs_b) SFX_HIP(hipMemcpyAsync(dsb.p, starts_b.data(), ndocs_b * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    SFX_TRY(A.upload(n_a ? sa_a : nullptr, n_a ? da_a : nullptr, n_a ? lcp_a : nullptr, n_a, st));
    if (n_b) {
        if (ndocs_b == 0) return SFX_ERR_ARG;
        SFX_TRY(gsa_build_dev((const uint8_t*)dt.p + n_a, n_b, (const uint64_t*)dsb.p, ndocs_b, (uint32_t*)dbs.p, (uint32_t*)dbd.p, (uint32_t*)dbl.p,
                              dw.p, wsb, st));
    }
    const GmIn in{(const uint8_t*)dt.p, (const uint64_t*)dst.p, ndocs, ndocs_a, n, n_a, n_b, (const uint32_t*)A.sa.p, (const uint32_t*)A.da.p,
                  (const uint32_t*)A.lcp.p, (const uint32_t*)dbs.p, (const uint32_t*)dbd.p, (const uint32_t*)dbl.p};
    SFX_TRY(gsa_merge_dev(in, match_limit, (uint32_t*)ds.p, (uint32_t*)dd.p, (uint32_t*)dl.p, longest_out, dw.p, wsb, st));
    if (match_limit && *longest_out > match_limit) {
        if (!rebuild_on_limit) return SFX_OK;                            // refused: the outputs stay as they are
        SFX_HIP(hipStreamSynchronize(st));
        dw.release();
        const uint64_t whole = gsa_workspace_bytes(n);
        SFX_TRY(dw.alloc(whole));
        SFX_TRY(gsa_build_dev((const uint8_t*)dt.p, n, (const uint64_t*)dst.p, ndocs, (uint32_t*)ds.p, (uint32_t*)dd.p, (uint32_t*)dl.p, dw.p, whole, st));
        *route_out = SFX_GSA_ROUTE_REBUILD;
    } else {
        *route_out = SFX_GSA_ROUTE_MERGE;
    }
    SFX_HIP(hipMemcpyAsync(sa_out, ds.p, bytes, hipMemcpyDeviceToHost, st));
    if (da_out) SFX_HIP(hipMemcpyAsync(da_out, dd.p, bytes, hipMemcpyDeviceToHost, st));
    if (lcp_out) SFX_HIP(hipMemcpyAsync(lcp_out, dl.p, bytes, hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}

// ---- repeat lengths, repeated spans ---------------------------------------------------------------------
uint64_t sfx_repeat_lens_workspace_bytes(uint64_t n, int scope) { return repeat_lens_workspace_bytes(n, scope); }
int sfx_repeat_lens_dev(const uint32_t* d_sa, const uint32_t* d_lcp, const uint32_t* d_da, uint64_t n, int scope, uint32_t* d_rep,
                        uint32_t* d_src, void* d_workspace, uint64_t workspace_bytes, void* stream)
{
    SFX_NEED_U32(d_sa, d_lcp, d_da, d_rep, d_src);
    SFX_NEED_WS(d_workspace, workspace_bytes, repeat_lens_workspace_bytes(n, scope));
    return repeat_lens_dev(d_sa, d_lcp, d_da, n, scope, d_rep, d_src, d_workspace, workspace_bytes, (hipStream_t)stream);
}
uint64_t sfx_repeat_spans_workspace_bytes(uint64_t n) { return repeat_spans_workspace_bytes(n); }
int sfx_repeat_spans_dev(const uint32_t* d_rep, uint64_t n, uint32_t min_len, const uint64_t* d_doc_starts, uint64_t ndocs,
                         uint32_t* d_begin, uint32_t* d_end, uint64_t capacity, uint64_t* count_out, void* d_workspace,
                         uint64_t workspace_bytes, void* stream)
{
    SFX_NEED_U64(d_doc_starts);
    SFX_NEED_U32(d_rep, d_begin, d_end);
    SFX_NEED_WS(d_workspace, workspace_bytes, repeat_spans_workspace_bytes(n));
    return repeat_spans_dev(d_rep, n, min_len, d_doc_starts, ndocs, d_begin, d_end, capacity, count_out, d_workspace, workspace_bytes,
                            (hipStream_t)stream);
}
int sfx_repeat_lens_u32(const uint32_t* sa, const uint32_t* lcp, const uint32_t* da, uint64_t n, int scope, uint32_t* rep_out,
                        uint32_t* src_out)
{
    if (scope != SFX_REP_ANY && scope != SFX_REP_EARLIER && scope != SFX_REP_OTHER_DOC) return SFX_ERR_ARG;
    if (scope == SFX_REP_OTHER_DOC && !da && n) return SFX_ERR_ARG;
    if (n > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!sa || !lcp || !rep_out) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    const bool docs = scope == SFX_REP_OTHER_DOC;
    DevBuf ds, dl, dd, dr, dq, dw;
    const uint64_t wsb = repeat_lens_workspace_bytes(n, scope), bytes = n * sizeof(uint32_t);
    SFX_TRY(ds.alloc(bytes));
    SFX_TRY(dl.alloc(bytes));
    if (docs) SFX_TRY(dd.alloc(bytes));
    SFX_TRY(dr.alloc(bytes));
    if (src_out) SFX_TRY(dq.alloc(bytes));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    SFX_HIP(hipMemcpyAsync(ds.p, sa, bytes, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(dl.p, lcp, bytes, hipMemcpyHostToDevice, st));
    if (docs) SFX_HIP(hipMemcpyAsync(dd.p, da, bytes, hipMemcpyHostToDevice, st));
    SFX_TRY(repeat_lens_dev((const uint32_t*)ds.p, (const uint32_t*)dl.p, (const uint32_t*)dd.p, n, scope, (uint32_t*)dr.p, (uint32_t*)dq.p,
                            dw.p, wsb, st));
    SFX_HIP(hipMemcpyAsync(rep_out, dr.p, bytes, hipMemcpyDeviceToHost, st));
    if (src_out) SFX_HIP(hipMemcpyAsync(src_out, dq.p, bytes, hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}
int sfx_repeat_spans_u32(const uint32_t* rep, uint64_t n, uint32_t min_len, const uint64_t* doc_starts, uint64_t ndocs,
                         uint32_t* begin_out, uint32_t* end_out, uint64_t capacity, uint64_t* count_out)
{
    if (!count_out || min_len == 0) return SFX_ERR_ARG;
    *count_out = 0;
    if (n > 0xFFFFFFFFull || ndocs > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n == 0) return SFX_OK;
    if (!rep || (capacity && (!begin_out || !end_out)) || (doc_starts && ndocs == 0)) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    if (capacity > n / min_len + 1) capacity = n / min_len + 1;          // (no report is longer)
    DevBuf dr, dst, db, de, dw;
    const uint64_t wsb = repeat_spans_workspace_bytes(n);
    SFX_TRY(dr.alloc(n * sizeof(uint32_t)));
    if (doc_starts) SFX_TRY(dst.alloc(ndocs * sizeof(uint64_t)));
    SFX_TRY(db.alloc(capacity * sizeof(uint32_t)));
    SFX_TRY(de.alloc(capacity * sizeof(uint32_t)));
    SFX_TRY(dw.alloc(wsb));
    hipStream_t st = call_stream();
    StreamDrain drain{st};
    SFX_HIP(hipMemcpyAsync(dr.p, rep, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (doc_starts) SFX_HIP(hipMemcpyAsync(dst.p, doc_starts, ndocs * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    SFX_TRY(repeat_spans_dev((const uint32_t*)dr.p, n, min_len, (const uint64_t*)dst.p, ndocs, (uint32_t*)db.p, (uint32_t*)de.p, capacity,
                             count_out, dw.p, wsb, st));
    const uint64_t k = dmin<uint64_t>(*count_out, capacity);
    if (k) {
        SFX_HIP(hipMemcpyAsync(begin_out, db.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SFX_HIP(hipMemcpyAsync(end_out, de.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}

int sfx_gindex_create_dev(const uint8_t* d_text, uint64_t n, const uint64_t* d_doc_starts, uint64_t ndocs, const uint32_t* d_sa,
                          const uint32_t* d_da, void* stream, sfx_gindex** out)
{
    SFX_NEED_U64(d_doc_starts);
    SFX_NEED_U32(d_sa, d_da);
    if (!out) return SFX_ERR_ARG;
    *out = nullptr;
    if (n > 0xFFFFFFFFull || ndocs > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n && (!d_text || !d_doc_starts || ndocs == 0 || !d_sa || !d_da)) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    sfx_gindex* gx = new sfx_gindex();
    gx->d_text = d_text;
    gx->d_starts = d_doc_starts;
    gx->d_sa = d_sa;
    gx->d_da = d_da;
    gx->n = n;
    gx->ndocs = ndocs;
    int rc = SFX_OK;
    if (n) {
        hipStream_t st = (hipStream_t)stream;
        do {
            hipError_t e = dev_malloc((void**)&gx->d_prev, n * sizeof(uint32_t));
            if (e != hipSuccess) { note_hip_error(e, "prev buffer", __FILE__, __LINE__); gx->d_prev = nullptr; rc = SFX_ERR_HIP; break; }
            DevBuf dw;
            const uint64_t wsb = gindex_workspace_bytes(n);
            rc = dw.alloc(wsb);
            if (rc != SFX_OK) break;
            bool bad = false;
            rc = gindex_build_dev(d_doc_starts, ndocs, n, d_sa, d_da, gx->d_prev, dw.p, wsb, st, &bad);
            // (the workspace returns to the pool: nothing may still use it, and the index serves other streams)
            e = hipStreamSynchronize(st);
            if (rc == SFX_OK && e != hipSuccess) { note_hip_error(e, "sync", __FILE__, __LINE__); rc = SFX_ERR_HIP; }
            if (rc == SFX_OK && bad) rc = SFX_ERR_ARG;
        } while (0);
    }
    if (rc != SFX_OK) { sfx_gindex_destroy(gx); return rc; }
    *out = gx;
    return SFX_OK;
}

int sfx_gindex_create(const uint8_t* text, uint64_t n, const uint64_t* doc_starts, uint64_t ndocs, const uint32_t* sa,
                      const uint32_t* da, sfx_gindex** out)
{
    if (!out) return SFX_ERR_ARG;
    *out = nullptr;
    if (n > 0xFFFFFFFFull || ndocs > 0xFFFFFFFFull) return SFX_ERR_TOO_LARGE;
    if (n && (!text || !doc_starts || ndocs == 0 || !sa || !da)) return SFX_ERR_ARG;
    SFX_TRY(check_device());
    void* p[4] = {nullptr, nullptr, nullptr, nullptr};
    const uint64_t bytes[4] = {n, ndocs * sizeof(uint64_t), n * sizeof(uint32_t), n * sizeof(uint32_t)};
    const void* src[4] = {text, doc_starts, sa, da};
    int rc = SFX_OK;
    hipStream_t st = call_stream();
    for (int i = 0; i < 4 && rc == SFX_OK; i++) {
        if (!bytes[i]) continue;
        hipError_t e = dev_malloc(&p[i], bytes[i]);
        if (e == hipSuccess) e = hipMemcpyAsync(p[i], src[i], bytes[i], hipMemcpyHostToDevice, st);
        if (e != hipSuccess) { note_hip_error(e, "gindex copy", __FILE__, __LINE__); rc = SFX_ERR_HIP; }
    }
    sfx_gindex* gx = nullptr;
    if (rc == SFX_OK)
        rc = sfx_gindex_create_dev((const uint8_t*)p[0], n, (const uint64_t*)p[1], ndocs, (const uint32_t*)p[2], (const uint32_t*)p[3],
                                   st, &gx);
    if (rc != SFX_OK) {
        (void)hipStreamSynchronize(st);
        for (void* q : p) if (q) (void)dev_free(q);
        return rc;
    }
    for (int i = 0; i < 4; i++) gx->own[i] = p[i];
    *out = gx;
    return SFX_OK;
}

int sfx_gindex_query_dev(const sfx_gindex* gx, const uint8_t* d_qbytes, const uint64_t* d_qoff, uint64_t nq, uint32_t* d_start,
                         uint32_t* d_end, uint8_t* d_found, uint32_t* d_any, uint32_t* d_ndocs, void* stream)
{
    SFX_NEED_U64(d_qoff);
    SFX_NEED_U32(d_start, d_end, d_any, d_ndocs);
    if (!gx) return SFX_ERR_ARG;
    if (nq == 0) return SFX_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!d_ndocs)
        return gindex_query_dev(gx->d_text, gx->n, gx->d_starts, gx->ndocs, gx->d_sa, gx->d_da, gx->d_prev, d_qbytes, d_qoff, nq, d_start,
                                d_end, d_found, d_any, nullptr, nullptr, 0, st);
    sfx_gindex* g = const_cast<sfx_gindex*>(gx);
    std::lock_guard<std::mutex> lk(g->mu);
    const uint64_t need = gindex_query_scratch_bytes(nq);
    if (!g->done) SFX_HIP(event_create(&g->done, hipEventDisableTiming));
    if (g->scratch_bytes < need) {
        if (g->scratch) {
            if (g->used) SFX_HIP(hipEventSynchronize(g->done));
            (void)dev_free(g->scratch);
            g->scratch = nullptr;
            g->scratch_bytes = 0;
            g->used = false;
        }
        SFX_HIP(dev_malloc(&g->scratch, need));
        g->scratch_bytes = need;
    }
    if (g->used) SFX_HIP(hipStreamWaitEvent(st, g->done, 0));
    const int rc = gindex_query_dev(gx->d_text, gx->n, gx->d_starts, gx->ndocs, gx->d_sa, gx->d_da, gx->d_prev, d_qbytes, d_qoff, nq,
                                    d_start, d_end, d_found, d_any, d_ndocs, g->scratch, g->scratch_bytes, st);
    SFX_HIP(hipEventRecord(g->done, st));
    g->used = true;
    return rc;
}

int sfx_gindex_query(const sfx_gindex* gx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t nq, uint32_t* start_out,
                     uint32_t* end_out, uint8_t* found_out, uint32_t* any_out, uint32_t* ndocs_out)
{
    if (!gx || (nq && !qoff)) return SFX_ERR_ARG;
    if (nq == 0) return SFX_OK;
    const uint64_t qtotal = qoff[nq];
    if (qtotal && !qbytes) return SFX_ERR_ARG;
    for (uint64_t k = 0; k < nq; k++) if (qoff[k + 1] < qoff[k]) return SFX_ERR_ARG;
    DevBuf dq, doff, ds, de, df, da, dn;
    SFX_TRY(dq.alloc(qtotal));
    SFX_TRY(doff.alloc((nq + 1) * sizeof(uint64_t)));
    if (start_out) SFX_TRY(ds.alloc(nq * 4));
    if (end_out) SFX_TRY(de.alloc(nq * 4));
    if (found_out) SFX_TRY(df.alloc(nq));
    if (any_out) SFX_TRY(da.alloc(nq * 4));
    if (ndocs_out) SFX_TRY(dn.alloc(nq * 4));
    hipStream_t st = call_stream();
    StreamDrain drain{st};            // (declared after the buffers: runs before they return to the pool)
    if (qtotal) SFX_HIP(hipMemcpyAsync(dq.p, qbytes, qtotal, hipMemcpyHostToDevice, st));
    SFX_HIP(hipMemcpyAsync(doff.p, qoff, (nq + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    SFX_TRY(sfx_gindex_query_dev(gx, (const uint8_t*)dq.p, (const uint64_t*)doff.p, nq, (uint32_t*)ds.p, (uint32_t*)de.p, (uint8_t*)df.p,
                                 (uint32_t*)da.p, (uint32_t*)dn.p, st));
    if (start_out) SFX_HIP(hipMemcpyAsync(start_out, ds.p, nq * 4, hipMemcpyDeviceToHost, st));
    if (end_out) SFX_HIP(hipMemcpyAsync(end_out, de.p, nq * 4, hipMemcpyDeviceToHost, st));
    if (found_out) SFX_HIP(hipMemcpyAsync(found_out, df.p, nq, hipMemcpyDeviceToHost, st));
    if (any_out) SFX_HIP(hipMemcpyAsync(any_out, da.p, nq * 4, hipMemcpyDeviceToHost, st));
    if (ndocs_out) SFX_HIP(hipMemcpyAsync(ndocs_out, dn.p, nq * 4, hipMemcpyDeviceToHost, st));
    SFX_HIP(hipStreamSynchronize(st));
    return SFX_OK;
}

void sfx_gindex_destroy(sfx_gindex* gx)
{
    if (!gx) return;
    if (gx->used) (void)hipEventSynchronize(gx->done);
    if (gx->done) (void)event_destroy(gx->done);
    if (gx->scratch) (void)dev_free(gx->scratch);
    if (gx->d_prev) (void)dev_free(gx->d_prev);
    for (void* p : gx->own) if (p) (void)dev_free(p);
    delete gx;
}

// ---- partitioned build ---------------------------------------------------------------------
int sfx_byte_histogram_dev(const uint8_t* d_text, uint64_t shard_begin, uint64_t shard_end,
                           uint64_t* d_bins256, void* stream)
{
    SFX_NEED_U64(d_bins256);
    return byte_histogram_dev(d_text, shard_begin, shard_end, d_bins256, (hipStream_t)stream);
}
int sfx_key_histogram_dev(const uint8_t* d_text, uint64_t n, uint64_t shard_begin,
                          uint64_t shard_end, const uint64_t* d_global_byte_bins256, int top_bits,
                          uint64_t* d_bins, void* stream)
{
    SFX_NEED_U64(d_global_byte_bins256, d_bins);
    return key_histogram_dev(d_text, n, shard_begin, shard_end, d_global_byte_bins256, top_bits,
                             d_bins, (hipStream_t)stream);
}
uint64_t sfx_sa_range_workspace_bytes(uint64_t n, uint64_t capacity) { return sa_range_workspace_bytes(n, capacity); }
int sfx_build_sa_range_u32_dev(const uint8_t* d_text, uint64_t n,
                               const uint64_t* d_global_byte_bins256, int top_bits, uint32_t bin_lo,
                               uint32_t bin_hi, uint64_t capacity, uint32_t* d_sa_part,
                               uint64_t* count_out, void* d_workspace, uint64_t workspace_bytes,
                               void* stream)
{
    SFX_NEED_U64(d_global_byte_bins256);
    SFX_NEED_U32(d_sa_part);
    SFX_NEED_WS(d_workspace, workspace_bytes, sa_range_workspace_bytes(n, capacity));
    return build_sa_range_u32_dev(d_text, n, d_global_byte_bins256, top_bits, bin_lo, bin_hi, capacity,
                                  d_sa_part, count_out, d_workspace, workspace_bytes,
                                  (hipStream_t)stream);
}

int sfx_pack_text_dev(const uint8_t* d_text, uint64_t count, const uint64_t* d_global_byte_bins256,
                      uint8_t* d_scratch256, uint32_t* d_words, uint64_t n_words, void* stream)
{
    SFX_NEED_U64(d_global_byte_bins256);
    SFX_NEED_U32(d_words);
    return pack_text_dev(d_text, count, d_global_byte_bins256, d_scratch256, d_words, n_words, (hipStream_t)stream);
}
int sfx_build_sa_range_packed_u32_dev(const uint32_t* d_packed, uint64_t n,
                                      const uint64_t* d_global_byte_bins256, int top_bits, uint32_t bin_lo,
                                      uint32_t bin_hi, uint64_t capacity, uint32_t* d_sa_part,
                                      uint64_t* count_out, void* d_workspace, uint64_t workspace_bytes,
                                      void* stream)
{
    SFX_NEED_U64(d_global_byte_bins256);
    SFX_NEED_U32(d_packed, d_sa_part);
    SFX_NEED_WS(d_workspace, workspace_bytes, sa_range_workspace_bytes(n, capacity));
    if (!d_packed) return SFX_ERR_ARG;
    return build_sa_range_u32_dev(nullptr, n, d_global_byte_bins256, top_bits, bin_lo, bin_hi, capacity, d_sa_part,
                                  count_out, d_workspace, workspace_bytes, (hipStream_t)stream, d_packed);
}

void sfx_release_cached_buffers(void)
{
    std::vector<PooledBuf> take;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        take.swap(g_pool);
    }
    for (PooledBuf& b : take) (void)dev_free(b.p);
    thread_res().release_scratch();                  // the calling thread's phase-2 scratch: the next large batch makes it again
}

int sfx_resource_stats(sfx_resource_stats_t* out)
{
    if (!out) return SFX_ERR_ARG;
    memset(out, 0, sizeof(*out));
    const auto rd = [](const std::atomic<uint64_t>& a) { return a.load(std::memory_order_relaxed); };
    out->device_bytes = rd(g_res.device_bytes);
    out->device_allocs = rd(g_res.device_allocs);
    out->pinned_bytes = rd(g_res.pinned_bytes);
    out->pinned_allocs = rd(g_res.pinned_allocs);
    out->streams = rd(g_res.streams);
    out->events = rd(g_res.events);
    out->device_allocs_total = rd(g_res.device_allocs_total);
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (const PooledBuf& b : g_pool) out->pooled_bytes += b.bytes;
    out->pooled_buffers = g_pool.size();
    return SFX_OK;
}

// ---- profiling --------------------------------------------------------------------------------
void sfx_profile_enable(int on) { g_profile = on != 0; }
void sfx_profile_reset(void)
{
    profile_fold();
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_stats.clear();
}
int sfx_profile_report(sfx_kernel_stat* out, int cap)
{
    profile_fold();
    std::lock_guard<std::mutex> lk(g_prof_mu);
    int n = (int)g_prof_stats.size();
    for (int i = 0; i < n && i < cap && out; i++) {
        memset(&out[i], 0, sizeof(out[i]));
        snprintf(out[i].name, sizeof(out[i].name), "%s", g_prof_stats[i].name.c_str());
        out[i].launches = g_prof_stats[i].launches;
        out[i].total_ms = g_prof_stats[i].ms;
        out[i].algo_bytes = g_prof_stats[i].bytes;
    }
    return n;
}
void sfx_last_build_stats(sfx_build_stats* out)
{
    if (out) *out = tls_build_stats();
}
int sfx_set_option(int option, uint64_t value)
{
    if (option == SFX_OPT_TINY_MAX && value <= tiny_max_default()) { tiny_set_limit(value); return SFX_OK; }
    return SFX_ERR_ARG;
}
uint64_t sfx_get_option(int option)
{
    return option == SFX_OPT_TINY_MAX ? tiny_limit() : 0;
}
uint64_t sfx_build_stats_read(void* out, uint64_t out_bytes)
{
    if (out && out_bytes) {
        const sfx_build_stats& s = tls_build_stats();
        memcpy(out, &s, (size_t)(out_bytes < sizeof(s) ? out_bytes : sizeof(s)));
    }
    return (uint64_t)sizeof(sfx_build_stats);
}

}  // extern "C"
