"""What the library holds on to: the cases shared by test_lifetime_emu.py (the emulator, host
memory) and test_gpu_lifetime.py (libsuffix_hip.so on the MI355X).

Every case brackets calls with `sfx_resource_stats` and asserts exact equalities of counters: nothing here has a
tolerance.  On the emulator every reading is also compared, field for field, with the ledger the HIP shim keeps on its
own (tests/emu/emu_runtime.cpp: every pointer it handed out with its size, every stream and event token, frees of what
it never gave out), so the reference for the counters is not the code under test.  On the GPU only the library's counters
are asserted; the change of `torch.cuda.mem_get_info()` over a case is put into the assertion messages and printed, never
compared (the machines are shared).

The tables handed to the engine are the oracle's where a result is checked (the index batches); the inputs of the other
calls (generalized table, repeat lengths, phrase lists, document counts) are made once by the engine's own host entry
points before the baseline is taken -- their values are other modules' business, here they only have to be valid."""
import ctypes
import gc
import os
import subprocess
import sys
import threading
import time

import numpy as np
import torch

import _buffers
import _bwt
import _gen
import _gsa

OK, ERR_ARG, ERR_WORKSPACE = 0, 1, 5
NONE = 0xFFFFFFFF
LIVE = ("device_bytes", "device_allocs", "pinned_bytes", "pinned_allocs", "streams", "events")
POOL_MAX = 8                                                             # kPoolMaxBuffers (sfx_api.hip)
STAGE_BYTES = 4608                                                       # kStage + kPostArea (sfx_host.hpp)
STEP = 32                                                                # sample step of the (bwt, samples) pairs
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_vp, _u64 = ctypes.c_void_p, ctypes.c_uint64


def _u32a(x):
    return np.ascontiguousarray(x, dtype=np.uint32)


# ---- the ledger --------------------------------------------------------------------------------------------------------
class Ctx:
    """One engine on one device, with the baseline of the module: taken after a warm-up on the main thread (one
    host-pointer build and one two-phase batch) and one sfx_release_cached_buffers()."""

    def __init__(self, eng, device, orc):
        self.eng, self.lib, self.device, self.orc = eng, eng.lib, device, orc
        self.gpu = str(device).startswith("cuda")
        self.emu = getattr(eng.lib, "emu_resource_stats", None) if not self.gpu else None
        assert self.gpu or self.emu is not None, "the emulator library exports no emu_resource_stats"
        self.st = _buffers.stream_of(device)
        self.info = {}                                                  # case -> mem_get_info delta (GPU, information only)
        self._data = {}
        self.small = 20011 if self.gpu else 5003
        self.large = 70001 if self.gpu else 20011
        for kind in ("dna", "bytes"):
            self.data(kind, self.large)
        d = self.data("dna", self.small)
        # the warm-up: this thread's stream, pinned page and query scratch exist from here on
        sa = np.zeros(d.n, dtype=np.uint32)
        assert self.lib.sfx_build_sa_u32(_gsa.ptr(d.text), d.n, _gsa.ptr(sa)) == OK and np.array_equal(sa, d.sa)
        rc, h, keep = mk_index(self, d, False)
        assert rc == OK
        index_batch(self, h, d, 5000)
        self.sync()
        self.lib.sfx_index_destroy(h)
        del keep
        gc.collect()
        self.base = self.released()
        self.free0 = self.free_bytes()

    def sync(self):
        if self.gpu:
            torch.cuda.synchronize()

    def free_bytes(self):
        return int(torch.cuda.mem_get_info()[0]) if self.gpu else 0

    def note(self, case):
        """(information) how much less device memory the driver reports free than at the baseline"""
        self.info[case] = self.free0 - self.free_bytes()
        return f"[{case}: mem_get_info free changed by {-self.info[case]} bytes since the baseline (information only)]"

    def stats(self):
        self.sync()
        s = self.eng.resource_stats()
        if self.emu is not None:
            out = (_u64 * 8)()
            self.emu(out)
            shim = dict(zip(LIVE + ("bad_frees", "device_allocs_total"), (int(v) for v in out)))
            assert shim["bad_frees"] == 0, shim
            for k in LIVE + ("device_allocs_total",):
                assert s[k] == shim[k], (k, s, shim)
        assert s["pooled_buffers"] <= POOL_MAX and s["pooled_buffers"] <= s["device_allocs"] and s["pooled_bytes"] <= s["device_bytes"], s
        return s

    def live(self):
        s = self.stats()
        return {k: s[k] for k in LIVE}

    def released(self):
        """sfx_release_cached_buffers() on this thread, then the live fields"""
        self.sync()
        self.eng.release_cached_buffers()
        s = self.stats()
        assert s["pooled_buffers"] == 0 and s["pooled_bytes"] == 0, s
        return {k: s[k] for k in LIVE}

    def at_baseline(self, case):
        got = self.released()
        note = self.note(case)
        assert got == self.base, (case, got, self.base, note)

    def total(self):
        return self.stats()["device_allocs_total"]

    def data(self, kind, n):
        if (kind, n) not in self._data:
            self._data[(kind, n)] = Data(self, kind, n)
        return self._data[(kind, n)]


class Data:
    """One text with everything the entry points take."""

    def __init__(self, c, kind, n):
        lib, orc = c.lib, c.orc
        self.n = n
        self.text = np.ascontiguousarray(_gen.dna(n, seed=7) if kind == "dna" else _gen.uniform_bytes(n, 200, 11), dtype=np.uint8)
        tb = self.text.tobytes()
        self.tb = tb
        self.sa = _u32a(orc.sais(tb))
        self.lcp = _u32a(orc.lcp_kasai(tb, self.sa))
        self.bwt, self.samples = _bwt.definition(tb, self.sa, STEP)
        self.bwt, self.samples = np.ascontiguousarray(self.bwt), _u32a(self.samples)
        self.starts = np.array([0, n // 7, n // 7, n // 3, n // 2 + 1, n - 5], dtype=np.uint64)     # (one empty document)
        nd = self.starts.size
        self.gsa, self.gda, self.glcp = (np.zeros(n, dtype=np.uint32) for _ in range(3))
        assert lib.sfx_build_gsa_u32(_gsa.ptr(self.text), n, _gsa.ptr(self.starts), nd, _gsa.ptr(self.gsa), _gsa.ptr(self.gda), _gsa.ptr(self.glcp)) == OK
        self.rep, self.rsrc = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        assert lib.sfx_repeat_lens_u32(_gsa.ptr(self.sa), _gsa.ptr(self.lcp), None, n, 1, _gsa.ptr(self.rep), _gsa.ptr(self.rsrc)) == OK
        self.zlen, self.zsrc, self.zlit = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
        z = _u64(0)
        assert lib.sfx_lz77_u32(_gsa.ptr(self.text), n, _gsa.ptr(self.sa), _gsa.ptr(self.lcp), 1, None, _gsa.ptr(self.zlen), _gsa.ptr(self.zsrc),
                                _gsa.ptr(self.zlit), n, ctypes.byref(z)) == OK
        self.z = int(z.value)
        self.zlen, self.zsrc, self.zlit = self.zlen[:self.z].copy(), self.zsrc[:self.z].copy(), self.zlit[:self.z].copy()
        self.df = np.zeros(n, dtype=np.uint32)
        assert lib.sfx_doc_counts_u32(_gsa.ptr(self.gda), _gsa.ptr(self.glcp), n, nd, None, _gsa.ptr(self.df)) == OK
        self._q = {}

    def queries(self, nq):
        """nq queries of 3 .. 22 bytes, three quarters of them substrings -> (qbytes, qoff u64, (start, end) of the oracle)"""
        if nq not in self._q:
            rng = np.random.default_rng(nq)
            pos = rng.integers(0, self.n - 24, nq)
            ln = rng.integers(3, 23, nq)
            qs = [self.tb[p:p + k] for p, k in zip(pos.tolist(), ln.tolist())]
            for j in range(0, nq, 4):
                qs[j] = qs[j][:-1] + b"\xfe"                            # (no text holds 0xFE)
            self._q[nq] = (*_buffers.query_arrays(qs), None)
        return self._q[nq]

    def expected(self, orc, nq):
        qb, qoff, exp = self.queries(nq)
        if exp is None:
            exp = tuple(_u32a(x) for x in orc.positions_batch(self.tb, self.sa, qb, qoff))
            self._q[nq] = (qb, qoff, exp)
        return exp


def ws_buf(c, need, mode="ok"):
    """A workspace of `need` bytes -- or one byte short, or large enough and 8 bytes off its boundary -> (buffer, bytes)"""
    if mode == "short":
        return _buffers.guarded(max(need - 1, 0), c.device, 0, 0xFF), max(need - 1, 0)
    if mode == "misaligned":
        return _buffers.guarded(need + 16, c.device, 8, 0xFF), need + 16
    return _buffers.guarded(need, c.device, 0, 0xFF), need


def out32(c, count, off=0):
    return _buffers.guarded(4 * int(count), c.device, off, 0xFF)


# ---- the four handles, each with its host and its _dev constructor ------------------------------------------------------
def mk_index(c, d, host, sa=None):
    sa = d.sa if sa is None else sa
    h = _vp(0xDEAD)
    if host:
        return c.lib.sfx_index_create(_gsa.ptr(d.text), d.n, _gsa.ptr(sa), ctypes.byref(h)), h, None
    keep = (_buffers.inp(d.text, c.device), _buffers.inp(sa, c.device))
    return c.lib.sfx_index_create_dev(keep[0].ptr, d.n, keep[1].ptr, c.st, ctypes.byref(h)), h, keep


def mk_gindex(c, d, host, starts=None, da=None):
    starts = d.starts if starts is None else starts
    da = d.gda if da is None else da
    h = _vp(0xDEAD)
    if host:
        return c.lib.sfx_gindex_create(_gsa.ptr(d.text), d.n, _gsa.ptr(starts), starts.size, _gsa.ptr(d.gsa), _gsa.ptr(da), ctypes.byref(h)), h, None
    keep = tuple(_buffers.inp(a, c.device) for a in (d.text, starts, d.gsa, da))
    return c.lib.sfx_gindex_create_dev(keep[0].ptr, d.n, keep[1].ptr, starts.size, keep[2].ptr, keep[3].ptr, c.st, ctypes.byref(h)), h, keep


def mk_fm(c, d, host, samples=None):
    sm = d.samples if samples is None else samples
    h = _vp(0xDEAD)
    if host:
        return c.lib.sfx_fm_create(_gsa.ptr(d.bwt), d.n, _gsa.ptr(sm), sm.size, STEP, 0, ctypes.byref(h)), h, None
    keep = (_buffers.inp(d.bwt, c.device), _buffers.inp(sm, c.device))
    return c.lib.sfx_fm_create_dev(keep[0].ptr, d.n, keep[1].ptr, sm.size, STEP, 0, c.st, ctypes.byref(h)), h, keep


def mk_lce(c, d, host, docs=False, sa=None, starts=None):
    """docs: over the generalized table with doc_starts"""
    table, lcp = (d.gsa, d.glcp) if docs else (d.sa, d.lcp)
    table = table if sa is None else sa
    starts = (d.starts if docs else None) if starts is None else starts
    nd = 0 if starts is None else starts.size
    h = _vp(0xDEAD)
    if host:
        return c.lib.sfx_lce_create(_gsa.ptr(table), _gsa.ptr(lcp), d.n, _gsa.ptr(starts) if nd else None, nd, ctypes.byref(h)), h, None
    keep = (_buffers.inp(table, c.device), _buffers.inp(lcp, c.device)) + ((_buffers.inp(starts, c.device),) if nd else ())
    return c.lib.sfx_lce_create_dev(keep[0].ptr, keep[1].ptr, d.n, keep[2].ptr if nd else None, nd, c.st, ctypes.byref(h)), h, keep


def index_batch(c, h, d, nq, check=True, stream=None):
    """One batch of nq queries through sfx_index_query_dev (two-phase from 4096 queries on), against the oracle."""
    qb, qoff, _ = d.queries(nq)
    b = (_buffers.inp(qb, c.device, 1), _buffers.inp(qoff, c.device, 8))
    o = _buffers.query_outputs(nq, c.device, 0xFF, offs=(0, 0, 0, 0))
    rc = c.lib.sfx_index_query_dev(h, b[0].ptr, b[1].ptr, nq, o["start"].ptr, o["end"].ptr, o["found"].ptr, o["any"].ptr, c.st if stream is None else stream)
    assert rc == OK, rc
    if check:
        ps, pe = d.expected(c.orc, nq)
        s, e = o["start"].host(np.uint32), o["end"].host(np.uint32)
        hit = pe > ps
        assert np.array_equal(s[hit], ps[hit]) and np.array_equal(e[hit], pe[hit]) and np.array_equal(e[~hit], s[~hit]), nq
        assert np.array_equal(o["found"].host() != 0, hit), nq
    return b, o


def use_index(c, h, d):
    for nq in (100, 5000, 12000):
        index_batch(c, h, d, nq)


def use_gindex(c, h, d):
    for nq in (100, 5000, 12000):                                       # (with document counts: the handle's scratch regrows)
        qb, qoff, _ = d.queries(nq)
        b = (_buffers.inp(qb, c.device, 1), _buffers.inp(qoff, c.device, 8))
        o = _buffers.query_outputs(nq, c.device, 0xFF, offs=(0, 0, 0, 0))
        nd = out32(c, nq)
        assert c.lib.sfx_gindex_query_dev(h, b[0].ptr, b[1].ptr, nq, o["start"].ptr, o["end"].ptr, o["found"].ptr, o["any"].ptr, nd.ptr, c.st) == OK
        s, e, k = o["start"].host(np.uint32), o["end"].host(np.uint32), nd.host(np.uint32)
        assert (k <= e - s).all() and ((k > 0) == (e > s)).all() and (k <= d.starts.size).all()
        c.sync()


def use_fm(c, h, d):
    for nq in (100, 5000, 12000):
        qb, qoff, _ = d.queries(nq)
        b = (_buffers.inp(qb, c.device, 1), _buffers.inp(qoff, c.device, 8))
        s, e = out32(c, nq), out32(c, nq)
        assert c.lib.sfx_fm_count_dev(h, b[0].ptr, b[1].ptr, nq, s.ptr, e.ptr, c.st) == OK
        ps, pe = d.expected(c.orc, nq)
        assert np.array_equal(e.host(np.uint32) - s.host(np.uint32), pe - ps), nq
        k = min(nq, 400)                                                # (a lookup walks up to STEP rows: kept short for the emulator)
        pos = out32(c, k)
        assert c.lib.sfx_fm_lookup_dev(h, None, d.n - k + 3, k, pos.ptr, c.st) == OK         # (the last three ranks are >= n)
        r = np.arange(d.n - k + 3, d.n + 3)
        assert np.array_equal(pos.host(np.uint32), np.where(r < d.n, d.sa[np.minimum(r, d.n - 1)], NONE)), nq
        c.sync()


def use_lce(c, h, d):
    for nq in (100, 5000, 12000):
        rng = np.random.default_rng(nq + 1)
        a, b_ = _u32a(rng.integers(0, d.n, nq)), _u32a(rng.integers(0, d.n, nq))
        ia, ib, o = _buffers.inp(a, c.device), _buffers.inp(b_, c.device), out32(c, nq)
        assert c.lib.sfx_lce_query_dev(h, ia.ptr, ib.ptr, nq, 0, o.ptr, c.st) == OK
        got = o.host(np.uint32)
        assert (got <= d.n - np.maximum(a, b_)).all()
        r = out32(c, nq)
        assert c.lib.sfx_lce_ranks_dev(h, ia.ptr, nq, r.ptr, c.st) == OK
        c.sync()


CONSTRUCTORS = {
    "index_host": (lambda c, d: mk_index(c, d, True), use_index, "sfx_index_destroy", None),
    "index_dev": (lambda c, d: mk_index(c, d, False), use_index, "sfx_index_destroy", None),
    "gindex_host": (lambda c, d: mk_gindex(c, d, True), use_gindex, "sfx_gindex_destroy", None),
    "gindex_dev": (lambda c, d: mk_gindex(c, d, False), use_gindex, "sfx_gindex_destroy", None),
    "fm_host": (lambda c, d: mk_fm(c, d, True), use_fm, "sfx_fm_destroy", lambda c, d: int(c.lib.sfx_fm_bytes(d.n, STEP, 0))),
    "fm_dev": (lambda c, d: mk_fm(c, d, False), use_fm, "sfx_fm_destroy", lambda c, d: int(c.lib.sfx_fm_bytes(d.n, STEP, 0))),
    "lce_host": (lambda c, d: mk_lce(c, d, True), use_lce, "sfx_lce_destroy", lambda c, d: int(c.lib.sfx_lce_bytes(d.n))),
    "lce_dev": (lambda c, d: mk_lce(c, d, False), use_lce, "sfx_lce_destroy", lambda c, d: int(c.lib.sfx_lce_bytes(d.n))),
    "lce_docs_host": (lambda c, d: mk_lce(c, d, True, docs=True), use_lce, "sfx_lce_destroy", lambda c, d: int(c.lib.sfx_lce_bytes(d.n))),
    "lce_docs_dev": (lambda c, d: mk_lce(c, d, False, docs=True), use_lce, "sfx_lce_destroy", lambda c, d: int(c.lib.sfx_lce_bytes(d.n))),
}


# ---- a. handles ---------------------------------------------------------------------------------------------------------
def handles(c, name, reps):
    """create -> grown; (fm, lce) growth minus the pool <= sfx_*_bytes; use; destroy + release -> the baseline; then
    `reps` times create / destroy with the live fields equal after every repetition."""
    make, use, destroy, bound = CONSTRUCTORS[name]
    destroy = getattr(c.lib, destroy)
    for kind in ("dna", "bytes"):
        d = c.data(kind, c.large)
        c.at_baseline(f"{name}/{kind} before")
        rc, h, keep = make(c, d)
        assert rc == OK and h.value, (name, kind, rc)
        s = c.stats()
        grown = s["device_bytes"] - c.base["device_bytes"]
        assert grown > 0 and s["device_allocs"] > c.base["device_allocs"], (name, kind, s)
        if bound is not None:
            held = grown - s["pooled_bytes"]
            if name.startswith("lce") and name.endswith("host"):        # (the host form also owns its copies of lcp and doc_starts)
                held -= 4 * d.n + (8 * d.starts.size if "docs" in name else 0)
            assert 0 < held <= bound(c, d), (name, kind, held, bound(c, d), s)
        use(c, h, d)
        c.sync()
        destroy(h)
        c.at_baseline(f"{name}/{kind} after destroy")
        after = None
        for it in range(reps):
            rc, h, keep = make(c, d)
            assert rc == OK, (name, kind, it, rc)
            c.sync()
            destroy(h)
            got = c.live()
            after = got if after is None else after
            assert got == after, (name, kind, it, got, after, c.note(f"{name}/{kind} repeat"))
        del keep
        c.at_baseline(f"{name}/{kind} after {reps} repetitions")


# ---- c. the *_dev calls: what they take, with a good, a short and a misaligned workspace ---------------------------------
def _dev_calls(c, d):
    """name -> (call(mode) -> rc, has a workspace).  Every array is a guarded buffer of its full size."""
    lib, n, st, dev = c.lib, d.n, c.st, c.device
    I = lambda a, off=0: _buffers.inp(a, dev, off)                       # noqa: E731
    nd = d.starts.size
    qb, qoff, _ = d.queries(50)
    query = np.ascontiguousarray(d.text[n // 3:n // 3 + 2000])
    m = query.size
    calls = {}

    def build_sa(mode):
        w, wb = ws_buf(c, int(lib.sfx_sa_workspace_bytes(n)), mode)
        b = (I(d.text), out32(c, n), w)
        return lib.sfx_build_sa_u32_dev(b[0].ptr, n, b[1].ptr, w.ptr, wb, st), b
    calls["build_sa"] = (build_sa, True)

    def build_lcp(mode):
        w, wb = ws_buf(c, int(lib.sfx_lcp_workspace_bytes(n)), mode)
        b = (I(d.text), I(d.sa), out32(c, n), w)
        return lib.sfx_build_lcp_u32_dev(b[0].ptr, n, b[1].ptr, b[2].ptr, w.ptr, wb, st), b
    calls["build_lcp"] = (build_lcp, True)

    def build_sa_lcp(mode):
        w, wb = ws_buf(c, int(lib.sfx_sa_lcp_workspace_bytes(n)), mode)
        b = (I(d.text), out32(c, n), out32(c, n), w)
        return lib.sfx_build_sa_lcp_u32_dev(b[0].ptr, n, b[1].ptr, b[2].ptr, w.ptr, wb, st), b
    calls["build_sa_lcp"] = (build_sa_lcp, True)

    def query_batch(mode):
        b = (I(d.text), I(d.sa), I(qb, 1), I(qoff, 8))
        o = _buffers.query_outputs(50, dev, 0xFF, offs=(0, 0, 0, 0))
        return lib.sfx_query_batch_dev(b[0].ptr, n, b[1].ptr, b[2].ptr, b[3].ptr, 50, o["start"].ptr, o["end"].ptr, o["found"].ptr, o["any"].ptr, st), (b, o)
    calls["query_batch"] = (query_batch, False)

    def lcp_intervals(mode):
        w, wb = ws_buf(c, int(lib.sfx_lcp_intervals_workspace_bytes(n)), mode)
        b = (I(d.lcp),) + tuple(out32(c, n) for _ in range(5)) + (w,)
        return lib.sfx_lcp_intervals_dev(b[0].ptr, n, *[x.ptr for x in b[1:6]], w.ptr, wb, st), b
    calls["lcp_intervals"] = (lcp_intervals, True)

    def suffix_tree(mode):
        w, wb = ws_buf(c, int(lib.sfx_suffix_tree_workspace_bytes(n)), mode)
        b = (I(d.text), I(d.sa), I(d.lcp)) + tuple(out32(c, n) for _ in range(5)) + (_buffers.guarded(8 * (n + 1), dev, 0, 0xFF), out32(c, 2 * n), out32(c, 2 * n),
                                                                                  _buffers.guarded(2 * n, dev, 0, 0xFF), out32(c, n), w)
        nodes, children = _u64(0), _u64(0)
        rc = lib.sfx_suffix_tree_dev(b[0].ptr, b[1].ptr, b[2].ptr, n, n, 2 * n, *[x.ptr for x in b[3:13]], ctypes.byref(nodes), ctypes.byref(children), w.ptr, wb, st)
        return rc, b
    calls["suffix_tree"] = (suffix_tree, True)

    def build_gsa(mode):
        w, wb = ws_buf(c, int(lib.sfx_gsa_workspace_bytes(n, nd)), mode)
        b = (I(d.text), I(d.starts), out32(c, n), out32(c, n), out32(c, n), w)
        return lib.sfx_build_gsa_u32_dev(b[0].ptr, n, b[1].ptr, nd, b[2].ptr, b[3].ptr, b[4].ptr, w.ptr, wb, st), b
    calls["build_gsa"] = (build_gsa, True)

    def repeat_lens(mode):
        w, wb = ws_buf(c, int(lib.sfx_repeat_lens_workspace_bytes(n, 1)), mode)
        b = (I(d.sa), I(d.lcp), out32(c, n), out32(c, n), w)
        return lib.sfx_repeat_lens_dev(b[0].ptr, b[1].ptr, None, n, 1, b[2].ptr, b[3].ptr, w.ptr, wb, st), b
    calls["repeat_lens"] = (repeat_lens, True)

    def repeat_spans(mode):
        w, wb = ws_buf(c, int(lib.sfx_repeat_spans_workspace_bytes(n)), mode)
        b = (I(d.rep), out32(c, n + 1), out32(c, n + 1), w)
        count = _u64(0)
        return lib.sfx_repeat_spans_dev(b[0].ptr, n, 8, None, 0, b[1].ptr, b[2].ptr, n + 1, ctypes.byref(count), w.ptr, wb, st), b
    calls["repeat_spans"] = (repeat_spans, True)

    def match_stats(mode):
        b = (I(d.text), I(d.sa), I(query, 1)) + tuple(out32(c, m) for _ in range(4))
        return lib.sfx_match_stats_dev(b[0].ptr, n, b[1].ptr, b[2].ptr, m, 64, *[x.ptr for x in b[3:]], st), b
    calls["match_stats"] = (match_stats, False)

    def bwt(mode):
        b = (I(d.text), I(d.sa), _buffers.guarded(n, dev, 0, 0xFF), out32(c, d.samples.size))
        return lib.sfx_bwt_dev(b[0].ptr, n, b[1].ptr, STEP, b[2].ptr, b[3].ptr, st), b
    calls["bwt"] = (bwt, False)

    def unbwt(mode):
        w, wb = ws_buf(c, int(lib.sfx_unbwt_workspace_bytes(n)), mode)
        b = (I(d.bwt), I(d.samples), _buffers.guarded(n, dev, 0, 0xFF), w)
        return lib.sfx_unbwt_dev(b[0].ptr, n, b[1].ptr, d.samples.size, STEP, b[2].ptr, w.ptr, wb, st), b
    calls["unbwt"] = (unbwt, True)

    def lz_parse(mode):
        w, wb = ws_buf(c, int(lib.sfx_lz_parse_workspace_bytes(n)), mode)
        b = (I(d.rep), I(d.rsrc), I(d.text), out32(c, n), out32(c, n), out32(c, n), _buffers.guarded(n, dev, 0, 0xFF), w)
        count = _u64(0)
        return lib.sfx_lz_parse_dev(b[0].ptr, b[1].ptr, b[2].ptr, n, 1, b[3].ptr, b[4].ptr, b[5].ptr, b[6].ptr, n, ctypes.byref(count), w.ptr, wb, st), b
    calls["lz_parse"] = (lz_parse, True)

    def lz_decode(mode):
        w, wb = ws_buf(c, int(lib.sfx_lz_decode_workspace_bytes(n, d.z)), mode)
        b = (I(d.zlen), I(d.zsrc), I(d.zlit), _buffers.guarded(n, dev, 0, 0xFF), w)
        return lib.sfx_lz_decode_dev(b[0].ptr, b[1].ptr, b[2].ptr, d.z, n, b[3].ptr, w.ptr, wb, st), b
    calls["lz_decode"] = (lz_decode, True)

    def mems(mode):
        limit = 1 << 16
        w, wb = ws_buf(c, int(lib.sfx_mems_workspace_bytes(m, limit)), mode)
        b = (I(d.text), I(d.sa), I(query, 1), out32(c, limit), out32(c, limit), out32(c, limit), w)
        pairs, count = _u64(0), _u64(0)
        rc = lib.sfx_mems_dev(b[0].ptr, n, b[1].ptr, b[2].ptr, m, 20, 0, limit, b[3].ptr, b[4].ptr, b[5].ptr, limit, ctypes.byref(pairs), ctypes.byref(count), w.ptr, wb, st)
        return rc, b
    calls["mems"] = (mems, True)

    def hamming(mode):
        limit = 1 << 16
        w, wb = ws_buf(c, int(lib.sfx_hamming_workspace_bytes(50, 1, limit)), mode)
        b = (I(d.text), I(d.sa), I(qb, 1), I(qoff, 8), out32(c, limit), out32(c, limit), _buffers.guarded(limit, dev, 0, 0xFF),
             _buffers.guarded(8 * 51, dev, 0, 0xFF), w)
        cands, count = _u64(0), _u64(0)
        rc = lib.sfx_hamming_dev(b[0].ptr, n, b[1].ptr, b[2].ptr, b[3].ptr, 50, 1, limit, b[4].ptr, b[5].ptr, b[6].ptr, limit, b[7].ptr, ctypes.byref(cands),
                                 ctypes.byref(count), w.ptr, wb, st)
        return rc, b
    calls["hamming"] = (hamming, True)

    def inverse_table(mode):
        w, wb = ws_buf(c, int(lib.sfx_inverse_table_workspace_bytes(n)), mode)
        b = (I(d.sa), out32(c, n), w)
        return lib.sfx_inverse_table_dev(b[0].ptr, n, b[1].ptr, w.ptr, wb, st), b
    calls["inverse_table"] = (inverse_table, True)

    def doc_counts(mode):
        w, wb = ws_buf(c, int(lib.sfx_doc_counts_workspace_bytes(n)), mode)
        b = (I(d.gda), I(d.glcp), out32(c, n), out32(c, n), w)
        return lib.sfx_doc_counts_dev(b[0].ptr, b[1].ptr, n, nd, b[2].ptr, b[3].ptr, w.ptr, wb, st), b
    calls["doc_counts"] = (doc_counts, True)

    def common_substrings(mode):
        w, wb = ws_buf(c, int(lib.sfx_common_substrings_workspace_bytes(nd)), mode)
        b = (I(d.gsa), I(d.glcp), I(d.df), I(d.starts), out32(c, nd), out32(c, nd), w)
        return lib.sfx_common_substrings_dev(b[0].ptr, b[1].ptr, b[2].ptr, n, b[3].ptr, nd, b[4].ptr, b[5].ptr, w.ptr, wb, st), b
    calls["common_substrings"] = (common_substrings, True)
    return calls


def hot_path(c):
    """c. Every *_dev entry that takes a caller workspace or none leaves device_allocs_total unchanged; the fm and lce
    queries likewise; sfx_index_query_dev makes or grows its thread's scratch at most once per size step."""
    d = c.data("dna", c.small)
    for name, (call, _) in _dev_calls(c, d).items():
        t0 = c.total()
        rc, keep = call("ok")
        t1 = c.total()
        assert rc == OK, (name, rc)
        assert t1 == t0, (name, t0, t1)
        del keep
    for mk, use in ((lambda: mk_fm(c, d, False), use_fm), (lambda: mk_lce(c, d, False), use_lce), (lambda: mk_lce(c, d, False, docs=True), use_lce)):
        rc, h, keep = mk()
        assert rc == OK
        t0 = c.total()
        use(c, h, d)
        assert c.total() == t0, (use.__name__, t0, c.total())
        (c.lib.sfx_fm_destroy if use is use_fm else c.lib.sfx_lce_destroy)(h)
    rc, h, keep = mk_index(c, d, False)
    assert rc == OK
    c.released()                                                        # (this thread's scratch is gone: the first step makes it)
    grew = []
    for nq in (100, 5000, 5000, 12000, 12000, 5000, 100):
        t0 = c.total()
        index_batch(c, h, d, nq)
        grew.append(c.total() - t0)
    assert all(g <= a for g, a in zip(grew, [0, 1, 0, 1, 0, 0, 0])) and sum(grew) == 2, grew
    # the other calls on the index take a workspace or none
    query = np.ascontiguousarray(d.text[100:1100])
    b = (_buffers.inp(query, c.device, 1),) + tuple(out32(c, query.size) for _ in range(4))
    t0 = c.total()
    assert c.lib.sfx_index_match_stats_dev(h, b[0].ptr, query.size, 64, *[x.ptr for x in b[1:]], c.st) == OK
    assert c.total() == t0
    c.sync()
    c.lib.sfx_index_destroy(h)
    c.at_baseline("hot path")


# ---- b. refusals that come after something was allocated ----------------------------------------------------------------
def _peek_hip():
    """hipPeekAtLastError of the HIP runtime this process has already loaded (torch's), or None on the emulator"""
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    assert paths, "no HIP runtime is loaded"
    lib = ctypes.CDLL(paths[0])
    lib.hipPeekAtLastError.restype = ctypes.c_int
    return lib.hipPeekAtLastError


def refusals(c):
    """Each refusal is one the header documents as safe; after each: the documented status, *out == NULL, the ledger at the
    baseline after sfx_release_cached_buffers(), and (GPU) no sticky HIP error for the caller's framework."""
    d = c.data("dna", c.small)
    n = d.n
    peek = _peek_hip() if c.gpu else None

    def after(case, rc, want, h=None):
        assert rc == want, (case, rc, want)
        if h is not None:
            assert not h.value, (case, h.value)
        c.at_baseline(case)
        if peek is not None:
            assert peek() == 0, (case, peek())
            torch.cuda.synchronize()

    over = d.sa.copy()
    over[n // 3] = n
    twice = d.sa.copy()
    twice[5] = twice[n - 2]
    bad_starts = np.array([0, 9, 8, n - 5], dtype=np.uint64)
    bad_da = d.gda.copy()
    bad_da[n // 2] = d.starts.size
    sm_over, sm_twice = d.samples.copy(), d.samples.copy()
    sm_over[3] = n + 1
    sm_twice[4] = sm_twice[9]
    for host in (True, False):
        tag = "host" if host else "dev"
        rc, h, keep = mk_index(c, d, host, sa=over)
        after(f"index_create/{tag}: an entry >= n", rc, ERR_ARG, h)
        rc, h, keep = mk_gindex(c, d, host, starts=bad_starts)
        after(f"gindex_create/{tag}: bad doc_starts", rc, ERR_ARG, h)
        rc, h, keep = mk_gindex(c, d, host, da=bad_da)
        after(f"gindex_create/{tag}: a bad DA entry", rc, ERR_ARG, h)
        rc, h, keep = mk_fm(c, d, host, samples=sm_over)
        after(f"fm_create/{tag}: a sample >= n", rc, ERR_ARG, h)
        rc, h, keep = mk_fm(c, d, host, samples=sm_twice)
        after(f"fm_create/{tag}: a duplicated sample", rc, ERR_ARG, h)
        rc, h, keep = mk_lce(c, d, host, sa=twice)
        after(f"lce_create/{tag}: not a permutation", rc, ERR_ARG, h)
        rc, h, keep = mk_lce(c, d, host, docs=True, starts=bad_starts)
        after(f"lce_create/{tag}: bad doc_starts", rc, ERR_ARG, h)
        del keep
    # sfx_unbwt of a mutated pair (a sample moved: the cycle breaks), sfx_unlz of a phrase list with a forward copy
    sm = d.samples.copy()
    sm[2] = sm[2] % n + 1
    out = np.zeros(n, dtype=np.uint8)
    rc = c.lib.sfx_unbwt(_gsa.ptr(d.bwt), n, _gsa.ptr(sm), sm.size, STEP, _gsa.ptr(out))
    if rc == OK:                                                         # (accepted only if it IS some text's transform)
        back = out.tobytes()
        vb, vs = _bwt.definition(back, _bwt.table_of(c.orc, back), STEP)
        assert np.array_equal(vb, d.bwt) and np.array_equal(vs, sm)
    after("unbwt: a mutated pair", rc, rc if rc == OK else ERR_ARG)
    assert rc == ERR_ARG, "the mutated pair was accepted: the case did not refuse"
    zl, zs, zc = _u32a([1, 1]), _u32a([NONE, 1]), np.frombuffer(b"a\x00", dtype=np.uint8).copy()
    out2 = np.zeros(2, dtype=np.uint8)
    after("unlz: a forward copy", c.lib.sfx_unlz(_gsa.ptr(zl), _gsa.ptr(zs), _gsa.ptr(zc), 2, 2, _gsa.ptr(out2)), ERR_ARG)
    zs2 = d.zsrc.copy()
    k = int(np.flatnonzero(d.zlen > 1)[-1])                              # the last copy phrase: its source moved to its own end
    zs2[k] = n - 1
    out3 = np.zeros(n, dtype=np.uint8)
    after("unlz: a source at or behind its phrase", c.lib.sfx_unlz(_gsa.ptr(d.zlen), _gsa.ptr(zs2), _gsa.ptr(d.zlit), d.z, n, _gsa.ptr(out3)), ERR_ARG)
    # one workspace-short and one misaligned call per family
    for name, (call, has_ws) in _dev_calls(c, d).items():
        if not has_ws:
            continue
        for mode, want in (("short", ERR_WORKSPACE), ("misaligned", ERR_ARG)):
            t0 = c.total()
            rc, keep = call(mode)
            assert c.total() == t0, (name, mode)
            keep[-1].check_guards(f"{name}: workspace")
            after(f"{name}: workspace {mode}", rc, want)
            del keep


# ---- d. the pool --------------------------------------------------------------------------------------------------------
def _host_calls(c, d, h, g):
    """name -> call() -> rc: the host-pointer entry points at one size (h: an sfx_index, g: an sfx_gindex over d)"""
    lib, n = c.lib, d.n
    P = _gsa.ptr
    o = [np.zeros(n + 1, dtype=np.uint32) for _ in range(4)]
    ob = np.zeros(n, dtype=np.uint8)
    qb, qoff, _ = d.queries(5000)
    pq, pqoff, _ = d.queries(50)
    query = np.ascontiguousarray(d.text[n // 3:n // 3 + 2000])
    m = query.size
    cnt, cnt2 = _u64(0), _u64(0)
    lim = 1 << 16
    big = [np.zeros(lim, dtype=np.uint32) for _ in range(3)]
    first = np.zeros(51, dtype=np.uint64)
    return {
        "sfx_build_sa_u32": lambda: lib.sfx_build_sa_u32(P(d.text), n, P(o[0])),
        "sfx_build_lcp_u32": lambda: lib.sfx_build_lcp_u32(P(d.text), n, P(d.sa), P(o[1])),
        "sfx_build_sa_lcp_u32": lambda: lib.sfx_build_sa_lcp_u32(P(d.text), n, P(o[0]), P(o[1])),
        "sfx_positions_batch": lambda: lib.sfx_positions_batch(h, P(qb), P(qoff), 5000, P(o[2]), P(o[3])),
        "sfx_bwt_u32": lambda: lib.sfx_bwt_u32(P(d.text), n, P(d.sa), STEP, P(ob), P(o[2])),
        "sfx_unbwt": lambda: lib.sfx_unbwt(P(d.bwt), n, P(d.samples), d.samples.size, STEP, P(ob)),
        "sfx_lz77_u32": lambda: lib.sfx_lz77_u32(P(d.text), n, P(d.sa), P(d.lcp), 1, P(o[0]), P(o[1]), P(o[2]), P(ob), n, ctypes.byref(cnt)),
        "sfx_unlz": lambda: lib.sfx_unlz(P(d.zlen), P(d.zsrc), P(d.zlit), d.z, n, P(ob)),
        "sfx_index_match_stats": lambda: lib.sfx_index_match_stats(h, P(query), m, 64, P(o[0]), P(o[1]), P(o[2]), P(o[3])),
        "sfx_gindex_match_stats": lambda: lib.sfx_gindex_match_stats(g, P(query), m, 64, P(o[0]), P(o[1]), P(o[2]), P(o[3])),
        "sfx_index_mems": lambda: lib.sfx_index_mems(h, P(query), m, 20, 0, lim, P(big[0]), P(big[1]), P(big[2]), lim, ctypes.byref(cnt), ctypes.byref(cnt2)),
        "sfx_index_hamming": lambda: lib.sfx_index_hamming(h, P(pq), P(pqoff), 50, 1, lim, P(big[0]), P(big[1]), P(ob), min(lim, n), P(first),
                                                           ctypes.byref(cnt), ctypes.byref(cnt2)),
        "sfx_doc_counts_u32": lambda: lib.sfx_doc_counts_u32(P(d.gda), P(d.glcp), n, d.starts.size, P(o[0]), P(o[1])),
    }


def pool_one_size(c):
    """Each host-pointer entry three times at one size: device_allocs_total may grow during the first call only (the
    header: "a loop ... at one size allocates it once")."""
    d = c.data("dna", c.small)
    rc, h, _ = mk_index(c, d, True)
    assert rc == OK
    rc, g, _ = mk_gindex(c, d, True)
    assert rc == OK
    for name, call in _host_calls(c, d, h, g).items():
        c.released()
        totals = [c.total()]
        for _ in range(3):
            assert call() == OK, name
            totals.append(c.total())
        assert totals[2] == totals[1] and totals[3] == totals[2], (name, totals, c.note(name))
    c.lib.sfx_index_destroy(h)
    c.lib.sfx_gindex_destroy(g)
    c.at_baseline("pool at one size")


def pool_ladder(c, base_len):
    """Twelve builds at lengths base_len * 2.5^k: at every step at most POOL_MAX buffers idle, and between calls nothing
    is held but them; after release, the baseline."""
    c.at_baseline("ladder before")
    seen = 0
    for k in range(12):
        n = int(base_len * 2.5 ** k)
        text = np.ascontiguousarray(_gen.dna(n, seed=k + 1), dtype=np.uint8)
        sa = np.zeros(n, dtype=np.uint32)
        assert c.lib.sfx_build_sa_u32(_gsa.ptr(text), n, _gsa.ptr(sa)) == OK, n
        assert sa[0] != sa[n - 1] and int(sa.max()) == n - 1
        s = c.stats()
        assert s["pooled_buffers"] <= POOL_MAX, (k, s)
        assert s["device_allocs"] - c.base["device_allocs"] == s["pooled_buffers"], (k, s)       # nothing live but the idle pool
        assert s["device_bytes"] - c.base["device_bytes"] == s["pooled_bytes"], (k, s)
        seen = max(seen, s["pooled_buffers"])
    assert seen == POOL_MAX, seen                                        # (the ladder did fill the pool: evictions happened)
    c.at_baseline("ladder after")


# ---- e. threads ---------------------------------------------------------------------------------------------------------
def _settled(c, want, seconds=10.0):
    """A joined Python thread may still be inside its thread-exit destructors: poll (never longer than `seconds`) until
    the live fields are `want`; -> the last reading."""
    end = time.monotonic() + seconds
    while True:
        got = c.released()
        if got == want or time.monotonic() > end:
            return got
        time.sleep(0.005)


def threads(c, count, together):
    """`count` fresh threads, one after another or all behind a barrier: each makes one host-pointer build (its own stream
    and pinned page), one 5000-query batch on a shared index through sfx_index_query_dev on a stream of its own (its own
    scratch and event), and ends.  After the joins and one release everything equals what it was before the first."""
    d = c.data("dna", c.small)
    rc, h, keep = mk_index(c, d, False)
    assert rc == OK
    d.expected(c.orc, 5000)
    before = c.released()
    errors, peaks = [], []
    barrier = threading.Barrier(count) if together else None

    def worker(j):
        try:
            if barrier is not None:
                barrier.wait(timeout=60)
            sa = np.zeros(d.n, dtype=np.uint32)
            assert c.lib.sfx_build_sa_u32(_gsa.ptr(d.text), d.n, _gsa.ptr(sa)) == OK and np.array_equal(sa, d.sa)
            if c.gpu:
                side = torch.cuda.Stream()
                with torch.cuda.stream(side):
                    b, o = index_batch(c, h, d, 5000, check=False, stream=_vp(side.cuda_stream))
                    side.synchronize()
                    ps, pe = d.expected(c.orc, 5000)
                    hit = pe > ps
                    s, e = o["start"].host(np.uint32), o["end"].host(np.uint32)
                    assert np.array_equal(s[hit], ps[hit]) and np.array_equal(e[hit], pe[hit])
            else:
                index_batch(c, h, d, 5000)
            if not together:
                peaks.append(c.eng.resource_stats())
        except BaseException as e:                                       # noqa: BLE001 (reported below)
            errors.append((j, repr(e)))
    ts = [threading.Thread(target=worker, args=(j,)) for j in range(count)]
    for t in ts:
        t.start()
        if not together:
            t.join()
    for t in ts:
        t.join()
    assert not errors, errors
    for s in peaks:                                                      # while a thread lives it does hold its own four
        assert s["streams"] >= before["streams"] + 1 and s["events"] >= before["events"] + 1 and s["pinned_bytes"] >= before["pinned_bytes"] + STAGE_BYTES, s
    got = _settled(c, before)
    leaked = {k: got[k] - before[k] for k in LIVE}
    assert got == before, (f"{count} threads left behind", leaked, c.note(f"threads x{count}"))
    c.sync()
    c.lib.sfx_index_destroy(h)
    c.at_baseline("threads")


def long_lived_thread_gives_its_scratch_back(c):
    d = c.data("dna", c.small)
    rc, h, keep = mk_index(c, d, False)
    assert rc == OK
    empty = c.released()
    index_batch(c, h, d, 5000)
    held = c.live()
    assert held["device_allocs"] == empty["device_allocs"] + 1 and held["events"] == empty["events"] + 1, (held, empty)
    assert held["device_bytes"] - empty["device_bytes"] == (256 + 12 * 5000 + 255) // 256 * 256, (held, empty)       # query_scratch_bytes(nq)
    assert c.released() == empty
    t0 = c.total()
    index_batch(c, h, d, 5000)                                           # allocates it again and answers correctly (the oracle's intervals)
    assert c.total() == t0 + 1
    assert c.live() == held
    c.sync()
    c.lib.sfx_index_destroy(h)
    c.at_baseline("long-lived thread")


# ---- f. steady state ------------------------------------------------------------------------------------------------------
def steady_state(c, n, iters, marks):
    """build -> index -> queries -> bwt -> fm -> lce -> destroy all, a new text each iteration: the live fields at the
    marked iterations are equal and device_allocs_total per iteration is constant from iteration 10 on."""
    lib, P = c.lib, _gsa.ptr
    c.at_baseline("steady state before")
    live, per_iter = {}, []
    last = c.total()
    for it in range(1, iters + 1):
        text = np.ascontiguousarray(_gen.dna(n, seed=1000 + it), dtype=np.uint8)
        sa, lcp = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        assert lib.sfx_build_sa_lcp_u32(P(text), n, P(sa), P(lcp)) == OK
        hi, hf, hl = _vp(), _vp(), _vp()
        assert lib.sfx_index_create(P(text), n, P(sa), ctypes.byref(hi)) == OK
        qs = [text[p:p + 9].tobytes() for p in range(7, n - 9, n // 200)]
        qb, qoff = _buffers.query_arrays(qs)
        s, e = np.zeros(len(qs), dtype=np.uint32), np.zeros(len(qs), dtype=np.uint32)
        assert lib.sfx_positions_batch(hi, P(qb), P(qoff), len(qs), P(s), P(e)) == OK and (e > s).all()
        bw, sm = np.zeros(n, dtype=np.uint8), np.zeros(-(-n // STEP), dtype=np.uint32)
        assert lib.sfx_bwt_u32(P(text), n, P(sa), STEP, P(bw), P(sm)) == OK
        assert lib.sfx_fm_create(P(bw), n, P(sm), sm.size, STEP, 0, ctypes.byref(hf)) == OK
        fs, fe = np.zeros(len(qs), dtype=np.uint32), np.zeros(len(qs), dtype=np.uint32)
        assert lib.sfx_fm_count(hf, P(qb), P(qoff), len(qs), P(fs), P(fe)) == OK and np.array_equal(fe - fs, e - s), it
        assert lib.sfx_lce_create(P(sa), P(lcp), n, None, 0, ctypes.byref(hl)) == OK
        a = _u32a(np.arange(0, n, 97))
        ln = np.zeros(a.size, dtype=np.uint32)
        assert lib.sfx_lce_query(hl, P(a), P(a), a.size, 0, P(ln)) == OK and np.array_equal(ln, n - a), it
        lib.sfx_lce_destroy(hl)
        lib.sfx_fm_destroy(hf)
        lib.sfx_index_destroy(hi)
        now = c.total()
        per_iter.append(now - last)
        last = now
        if it in marks:
            live[it] = c.live()
    first = live[marks[0]]
    assert all(live[m] == first for m in marks), (live, c.note("steady state"))
    assert len(set(per_iter[9:])) == 1, per_iter
    c.at_baseline("steady state after")


# ---- g. process exit -----------------------------------------------------------------------------------------------------
CHILD = """
import sys, threading
sys.path[:0] = [{root!r}, {here!r}]
import oracle
import _lifetime as L
from suffix_amd import Engine
oracle.build()
eng = Engine({lib!r}) if {lib!r} else __import__("suffix_amd").default_engine()
L.child(eng, {device!r}, oracle, {mode!r})
"""


def child(eng, device, orc, mode):
    """What the child processes of `process_exit` run."""
    c = Ctx.__new__(Ctx)
    c.eng, c.lib, c.device, c.orc = eng, eng.lib, device, orc
    c.gpu = str(device).startswith("cuda")
    c.st = _buffers.stream_of(device)
    c._data = {}
    d = c.data("dna", 5003)
    made = []

    def everything():
        for name in ("index_host", "gindex_dev", "fm_host", "lce_docs_dev"):
            make, use, destroy, _ = CONSTRUCTORS[name]
            rc, h, keep = make(c, d)
            assert rc == OK, name
            use(c, h, d)
            made.append((getattr(c.lib, destroy), h, keep))
        c.sync()

    if mode == "normal":
        t = threading.Thread(target=everything)
        t.start()
        t.join()
        for destroy, h, _ in made:
            destroy(h)
        del made[:]
        everything()
        for destroy, h, _ in made:
            destroy(h)
        eng.release_cached_buffers()
        print("DONE", flush=True)
    elif mode == "handles_alive":
        everything()
        print("DONE", flush=True)
        sys.exit(0)
    else:
        parked, used = threading.Event(), threading.Event()

        def daemon():
            everything()
            used.set()
            parked.wait()
        threading.Thread(target=daemon, daemon=True).start()
        assert used.wait(timeout=120)
        print("DONE", flush=True)


def process_exit(c, mode, lib_path, tmp_path, limit=180):
    script = tmp_path / f"exit_{mode}.py"
    script.write_text(CHILD.format(root=ROOT, here=HERE, lib=lib_path, device=str(c.device), mode=mode))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=limit)
    assert r.returncode == 0 and r.stdout.strip().endswith("DONE"), (mode, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    low = r.stderr.lower()
    for word in ("hip", "hsa", "abort", "segmentation", "terminate", "core dumped", "traceback"):
        assert word not in low, (mode, word, r.stderr[-3000:])


# ---- the sources: no raw call outside the wrappers ------------------------------------------------------------------------
RAW = r"\bhip(?:Malloc|Free|HostMalloc|HostFree|StreamCreate\w*|StreamDestroy|EventCreate\w*|EventDestroy)\s*\("


def raw_calls():
    """-> [(file, line number, text)] of every call of the eight HIP functions in suffix_amd/csrc outside the wrapper
    section of sfx_host.hpp (comments and string literals do not count)."""
    import re
    csrc = os.path.join(ROOT, "suffix_amd", "csrc")
    found, wrapped = [], 0
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".hpp", ".h", ".cpp")):
            continue
        inside = False
        block = False
        for no, line in enumerate(open(os.path.join(csrc, f), errors="replace"), 1):
            if f == "sfx_host.hpp" and line.startswith("// ----"):
                inside = "resource ledger" in line
            code = re.sub(r'"(?:\\.|[^"\\])*"', '""', line)
            if block:
                if "*/" not in code:
                    continue
                code, block = code.split("*/", 1)[1], False
            code = re.sub(r"/\*.*?\*/", "", code)
            if "/*" in code:
                code, block = code.split("/*", 1)[0], True
            code = code.split("//", 1)[0]
            for _ in re.finditer(RAW, code):
                if inside:
                    wrapped += 1
                else:
                    found.append((f, no, line.strip()))
    return found, wrapped
