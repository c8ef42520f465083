"""The cases of the document listing (sfx_doclist_*), shared by test_doclist_emu.py (the emulator
build, host memory) and test_gpu_doclist.py (libsuffix_hip.so, HBM).

Nothing expected comes from the engine: per interval `np.unique(da[s:e], return_counts=True)`, the BY_TF order by
`np.lexsort((doc, -tf))`, top_k a slice.  Small tables are the definition's (GeneralizedSuffixTable.new_naive); pattern
intervals come from the collection's search and are held to Python's `in` before they are used."""
import contextlib
import ctypes
import itertools
import os
import random
import subprocess
import threading

import numpy as np
import torch

import _buffers
import _gen
import _gsa
from suffix_amd import GeneralizedSuffixTable
from suffix_amd import device as sdev

OK, ERR_ARG, ERR_TOO_LARGE, ERR_WORKSPACE = 0, 1, 2, 5
BY_DOC, BY_TF = 0, 1
TILE = 2048                                                             # kDlTile: items per tile
CUTS = (1, 1 << 60, 0)                                                  # route B wherever it can run, route A only, automatic
COMMON = {"doclist_work", "doclist_offsets", "doclist_first", "doclist_cut", "doclist_publish"}
ROUTE_A = {"doclist_count", "doclist_emit"}
ROUTE_B = {"doclist_count_docs", "doclist_emit_docs"}
ORDERING = {"doclist_keys", "doclist_write"}
KERNELS = COMMON | ROUTE_A | ROUTE_B | ORDERING | {"doclist_check"}
HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
CSRC = os.path.join(HERE, os.pardir, "suffix_amd", "csrc")


def build_emulator():
    """`make -C tests/emu`; sfx_doclist.hip is compiled as part of sfx_api.hip's translation unit and tests/emu/Makefile
    does not name it: when it (or a unit it includes) is newer than the library, sfx_api.hip is declared new."""
    lib = os.path.join(EMU_DIR, "libsuffix_emu.so")
    cmd = ["make", "-s", "-j8", "-C", EMU_DIR]
    units = ("sfx_doclist.hip", "sfx_docs.hip", "sfx_lce.hip", "sfx_mem.hip")
    if os.path.exists(lib) and any(os.path.getmtime(os.path.join(CSRC, f)) > os.path.getmtime(lib) for f in units):
        cmd += ["-W", "../../suffix_amd/csrc/sfx_api.hip"]
    subprocess.check_call(cmd)
    return lib


def _u32a(x):
    return np.ascontiguousarray(x, dtype=np.uint32)


def _sync(device):
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()


# ---- the known answers -------------------------------------------------------------------------------------------------
def expected_list(da, s, e, order=BY_DOC, top_k=0):
    """(docs, tf) of one interval, and |D_j|."""
    u, c = np.unique(np.asarray(da[int(s):int(e)]), return_counts=True)
    if order == BY_TF:
        idx = np.lexsort((u, -c.astype(np.int64)))
        u, c = u[idx], c[idx]
    k = u.size if top_k == 0 else min(top_k, u.size)
    return u[:k].astype(np.uint32), c[:k].astype(np.uint32), int(u.size)


def expected_batch(da, s, e, order=BY_DOC, top_k=0):
    """-> (doc, tf, first, Z_full) of a batch in CSR form."""
    docs, tfs, first, zfull = [np.zeros(0, dtype=np.uint32)], [np.zeros(0, dtype=np.uint32)], [0], 0
    for a, b in zip(s, e):
        d, t, full = expected_list(da, a, b, order, top_k)
        docs.append(d)
        tfs.append(t)
        first.append(first[-1] + d.size)
        zfull += full
    return np.concatenate(docs).astype(np.uint32), np.concatenate(tfs).astype(np.uint32), np.array(first, dtype=np.uint64), zfull


def starts_of(da, ndocs):
    """doc_starts of a synthetic da: the cumulative counts (every text position contributes one suffix)."""
    cnt = np.bincount(np.asarray(da, dtype=np.int64), minlength=ndocs)
    st = np.zeros(ndocs, dtype=np.uint64)
    st[1:] = np.cumsum(cnt[:-1])
    return st


def node_intervals(lcp):
    """[lb, rb + 1) of every lcp-interval, by walking outwards from every boundary (small tables)."""
    n = len(lcp)
    out = {(0, n)}
    for p in range(1, n):
        v = int(lcp[p])
        if not v:
            continue
        lb = p - 1
        while lb > 0 and lcp[lb] >= v:
            lb -= 1
        rb = p
        while rb + 1 < n and lcp[rb + 1] >= v:
            rb += 1
        out.add((lb, rb + 1))
    return sorted(out)


# ---- the raw ABI over guarded buffers ------------------------------------------------------------------------------------
class Index:
    """sfx_doclist_create_dev over guarded inputs; `with Index(...) as ix`.  pooled: no caller workspace."""

    def __init__(self, eng, device, da, starts, occ_cut=0, ndocs=None, da_off=4, fill=0xFF, pooled=False, ws_bytes=None, ws_off=0, n=None):
        self.eng, self.device = eng, device
        da, st = _u32a(da), np.ascontiguousarray(starts, dtype=np.uint64)
        self.n = int(da.size) if n is None else n
        self.ndocs = int(st.size) if ndocs is None else ndocs
        need = int(eng.lib.sfx_doclist_create_workspace_bytes(self.n))
        self.b = {"da": _buffers.inp(da, device, da_off), "starts": _buffers.inp(st, device, 8)}
        if not pooled:
            self.b["workspace"] = _buffers.guarded(need if ws_bytes is None else ws_bytes, device, ws_off, fill)
        self.h = ctypes.c_void_p()
        ws = self.b.get("workspace")
        self.rc = eng.lib.sfx_doclist_create_dev(self.b["da"].ptr if da.size else None, self.n, self.b["starts"].ptr if st.size else None, self.ndocs,
                                                 occ_cut, ws.ptr if ws else None, ws.nbytes if ws else 0, _buffers.stream_of(device),
                                                 ctypes.byref(self.h))
        _sync(device)
        _buffers.check_all(self.b)
        assert np.array_equal(self.b["da"].host(np.uint32), da), "da was written"
        assert (self.rc == OK) == bool(self.h.value), (self.rc, self.h.value)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _sync(self.device)
        if self.h.value:
            self.eng.lib.sfx_doclist_destroy(self.h)
        self.h = ctypes.c_void_p()
        return False


def list_raw(ix, s, e, order=BY_DOC, top_k=0, list_limit=None, capacity=None, fill=0xFF, offs=(4, 8, 12, 4), ws_bytes=None, ws_off=0,
             want_first=True, nq=None, first_off=8):
    """-> dict(rc, doc, tf, first, listed, count): every array between guard bands, the workspace exactly as long as stated
    and pre-filled; doc / tf hold `capacity` entries (default: 3 more than the sum of the interval lengths allows)."""
    eng, device = ix.eng, ix.device
    s, e = _u32a(s), _u32a(e)
    nq = int(s.size) if nq is None else nq
    bound = int(np.minimum(e.astype(np.int64) - s.astype(np.int64), max(ix.ndocs, 1)).clip(0).sum())
    limit = max(bound, 1) if list_limit is None else list_limit
    cap = bound + 3 if capacity is None else capacity
    need = int(eng.lib.sfx_doclist_workspace_bytes(nq, limit))
    b = {"start": _buffers.inp(s, device, offs[0]), "end": _buffers.inp(e, device, offs[1]),
         "doc": _buffers.guarded(4 * cap, device, offs[2], _buffers.out_fill(fill)),
         "tf": _buffers.guarded(4 * cap, device, offs[3], _buffers.out_fill(fill)),
         "first": _buffers.guarded(8 * (int(s.size) + 1), device, first_off, _buffers.out_fill(fill)),
         "workspace": _buffers.guarded(need if ws_bytes is None else ws_bytes, device, ws_off, fill)}
    listed, count = ctypes.c_uint64(777), ctypes.c_uint64(777)
    rc = eng.lib.sfx_doclist_list_dev(ix.h, b["start"].ptr if s.size else None, b["end"].ptr if e.size else None, nq, order, top_k, limit,
                                      b["doc"].ptr if cap else None, b["tf"].ptr if cap else None, cap, b["first"].ptr if want_first else None,
                                      ctypes.byref(listed), ctypes.byref(count), b["workspace"].ptr, b["workspace"].nbytes,
                                      _buffers.stream_of(device))
    _sync(device)
    _buffers.check_all(b)
    assert np.array_equal(b["start"].host(np.uint32), s) and np.array_equal(b["end"].host(np.uint32), e), "an input was written"
    return {"rc": rc, "doc": b["doc"].host(np.uint32), "tf": b["tf"].host(np.uint32), "first": b["first"].host(np.uint64),
            "listed": int(listed.value), "count": int(count.value), "fill": _buffers.out_fill(fill), "cap": cap,
            "items": b["workspace"].host()[256:256 + 4 * int(s.size)].view(np.uint32) if b["workspace"].nbytes >= 256 + 4 * int(s.size) else None}


def untouched(arr):
    """An output that started as 0xFF bytes still holds them."""
    return bool((np.ascontiguousarray(arr).view(np.uint8) == 0xFF).all())


def check_result(r, da, s, e, order, top_k, what=()):
    doc, tf, first, zfull = expected_batch(da, s, e, order, top_k)
    z = doc.size
    assert r["rc"] == OK, (r["rc"], what)
    assert r["listed"] == zfull and r["count"] == z, (r["listed"], zfull, r["count"], z, what)
    assert np.array_equal(r["first"], first), (what, r["first"][:8], first[:8])
    w = min(z, r["cap"])
    assert np.array_equal(r["doc"][:w], doc[:w]), (what, np.flatnonzero(r["doc"][:w] != doc[:w])[:4], r["doc"][:8], doc[:8])
    assert np.array_equal(r["tf"][:w], tf[:w]), (what, np.flatnonzero(r["tf"][:w] != tf[:w])[:4], r["tf"][:8], tf[:8])
    if r["fill"] == 0xFF:                                               # nothing behind the entries reported
        assert (r["doc"][w:] == 0xFFFFFFFF).all() and (r["tf"][w:] == 0xFFFFFFFF).all(), what


def check_batch(eng, device, da, starts, s, e, t=0, topks=(0,), cuts=CUTS, orders=(BY_DOC, BY_TF), every=False):
    """One batch of intervals under every occ_cut and both orders with top_k = 0; the other top_k values on one rotating
    (cut, order) pair -- or, with every=True, on all of them."""
    da = _u32a(da)
    pairs = list(itertools.product(cuts, orders))
    done = 0
    for ci, cut in enumerate(cuts):
        with Index(eng, device, da, starts, occ_cut=cut, da_off=(4, 8, 12)[(t + ci) % 3], pooled=(t + ci) % 2 == 1,
                   fill=_buffers.FILLS[(t + ci) % 3]) as ix:
            assert ix.rc == OK, (ix.rc, cut)
            for oi, order in enumerate(orders):
                for k in topks:
                    if k and not every and pairs[(t + k) % len(pairs)] != (cut, order):
                        continue
                    fill = _buffers.FILLS[(t + ci + oi + k) % 3]
                    offs = [(4, 8, 12, 4), (8, 12, 4, 8), (12, 4, 8, 12)][(t + oi) % 3]
                    r = list_raw(ix, s, e, order, k, fill=fill, offs=offs, first_off=(8, 0)[(t + k) % 2])
                    check_result(r, da, s, e, order, k, what=(cut, order, k, t))
                    done += 1
    return done


def tables(docs, eng):
    g = GeneralizedSuffixTable.new_naive(docs, engine=eng)
    return b"".join(docs), _u32a(g.table()), _u32a(g.doc_array()), _u32a(g.lcp_lens()), _gsa.doc_starts(docs).astype(np.uint64)


def topk_values(da, s, e, pick):
    """{0, 1, 2, |D_j|, |D_j| + 1} for the interval `pick` chooses."""
    if not len(s):
        return (0, 1, 2)
    j = pick % len(s)
    d = int(np.unique(da[int(s[j]):int(e[j])]).size)
    return tuple(sorted({0, 1, 2, max(d, 1), d + 1}))


# ---- known answers ---------------------------------------------------------------------------------------------------------
def known_answers(eng, device):
    lib = eng.lib
    # hand-written collections: empty documents at the start, in the middle and at the end; one document; ndocs == 1
    for t, docs in enumerate(([b"", b"abcab", b"", b"cab", b"b", b""], [b"mississippi"], [b"a"], [b"", b"", b"xyz"], [b"ab", b"ab", b"ab"],
                              [b"aaaa", b"aa", b"", b"a"])):
        text, sa, da, lcp, starts = tables(docs, eng)
        n = len(text)
        iv = node_intervals(lcp) + [(r, r + 1) for r in range(n)] + [(0, 0), (n, n), (n // 2, n // 2)]
        s, e = np.array([a for a, _ in iv]), np.array([b for _, b in iv])
        check_batch(eng, device, da, starts, s, e, t=t, topks=(0, 1, 2, 3), every=True)
    # the answers spelled out: "ab" occurs twice in document 1, once in 3; "b" in 1, 3, 4
    docs = [b"", b"abcab", b"", b"cab", b"b", b""]
    g = GeneralizedSuffixTable.new_naive(docs, engine=eng)
    res = g.query_batch([b"ab", b"b", b"zz", b"", b"c"])
    with Index(eng, device, g.doc_array(), g.doc_starts()) as ix:
        r = list_raw(ix, res["start"], res["end"], BY_TF)
        assert r["rc"] == OK and r["first"].tolist() == [0, 2, 5, 5, 5, 7]
        assert r["doc"][:7].tolist() == [1, 3, 1, 3, 4, 1, 3] and r["tf"][:7].tolist() == [2, 1, 2, 1, 1, 1, 1]
        r = list_raw(ix, res["start"], res["end"], BY_TF, top_k=1)
        assert r["first"].tolist() == [0, 1, 2, 2, 2, 3] and r["doc"][:3].tolist() == [1, 1, 1] and r["listed"] == 7 and r["count"] == 3
    # nothing at all: no intervals, no ranks
    with Index(eng, device, [], [0, 0], pooled=True) as ix:
        assert ix.rc == OK
        r = list_raw(ix, [0, 0], [0, 0])
        assert r["rc"] == OK and r["listed"] == 0 and r["count"] == 0 and r["first"].tolist() == [0, 0, 0]
    with Index(eng, device, [0, 0, 1], [0, 2]) as ix:
        r = list_raw(ix, [], [])
        assert r["rc"] == OK and r["listed"] == 0 and r["first"].tolist() == [0]
    h = ctypes.c_void_p()
    assert lib.sfx_doclist_create(None, 0, None, 0, 0, ctypes.byref(h)) == OK and h.value
    lib.sfx_doclist_destroy(h)
    lib.sfx_doclist_destroy(None)
    # the public class
    d, f = g.document_listing(b"ab", order="tf")
    assert d.dtype == np.uint32 and f.dtype == np.uint32 and d.tolist() == [1, 3] and f.tolist() == [2, 1]
    d, f = g.document_listing(b"b")
    assert d.tolist() == [1, 3, 4] and f.tolist() == [2, 1, 1]
    out = g.document_listing_batch([b"ab", b"zz", b"b"], order="tf", top_k=2)
    assert [x[0].tolist() for x in out] == [[1, 3], [], [1, 3]] and [x[1].tolist() for x in out] == [[2, 1], [], [2, 1]]
    d, f = g.interval_documents(0, g.len())
    assert d.tolist() == [1, 3, 4] and f.tolist() == [5, 3, 1]
    d, f = g.interval_documents(0, g.len(), order="tf", top_k=1)
    assert d.tolist() == [1] and f.tolist() == [5]
    with contextlib.suppress(IndexError):
        g.interval_documents(0, g.len() + 1)
        raise AssertionError("an interval past the table")
    with contextlib.suppress(ValueError):
        g.document_listing(b"ab", order="length")
        raise AssertionError("an unknown order")
    assert g.documents_batch([b"ab", b"b", b"zz", b""]) == [[1, 3], [1, 3, 4], [], []]
    empty = GeneralizedSuffixTable.new_naive([b"", b""], engine=eng)
    assert empty.documents(b"a") == [] and empty.document_listing(b"a")[0].size == 0
    # the torch-tensor classes
    text, sa, da, lcp, starts = tables(docs, eng)
    t32 = lambda x: torch.from_numpy(_u32a(x).view(np.int32).copy()).to(device)
    dx = sdev.DocListDeviceIndex(t32(da), torch.from_numpy(starts.astype(np.int64)).to(device), engine=eng)
    try:
        doc, tf, first, listed = dx.list(t32(res["start"]), t32(res["end"]), order="tf")
        _sync(device)
        assert listed == 7 and first.cpu().numpy().tolist() == [0, 2, 5, 5, 5, 7]
        assert doc.cpu().numpy().tolist() == [1, 3, 1, 3, 4, 1, 3] and tf.cpu().numpy().tolist() == [2, 1, 2, 1, 1, 1, 1]
        doc, tf, first, listed = dx.list(t32(res["start"]), t32(res["end"]), order="doc", top_k=1, capacity=2)
        _sync(device)
        assert listed == 7 and first.cpu().numpy().tolist() == [0, 1, 2, 2, 2, 3] and doc.cpu().numpy().tolist() == [1, 1]
        assert dx.nbytes == lib.sfx_doclist_bytes(len(text))
    finally:
        dx.close()
    gx = sdev.GeneralizedDeviceIndex(torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(device),
                                     torch.from_numpy(starts.astype(np.int64)).to(device), t32(sa), t32(da), engine=eng)
    try:
        qb, qoff = _buffers.query_arrays([b"ab", b"b", b"zz"])
        doc, tf, first, listed = gx.documents(torch.from_numpy(qb.copy()).to(device), torch.from_numpy(qoff.astype(np.int64)).to(device), order="tf")
        _sync(device)
        assert first.cpu().numpy().tolist() == [0, 2, 5, 5] and doc.cpu().numpy().tolist() == [1, 3, 1, 3, 4]
    finally:
        gx.close()


def small_random(eng, device, sigma, count=150, seed=61):
    """Up to 6 documents of 0 - 40 bytes over `sigma` symbols: every pattern of up to 4 symbols, every lcp-interval."""
    rng = random.Random(seed + sigma)
    alpha = bytes(range(97, 97 + sigma))
    pats = [bytes(p) for k in range(1, 5) for p in itertools.product(alpha, repeat=k)]
    done = 0
    for t in range(count):
        m = rng.randint(1, 6)
        docs = [bytes(97 + rng.randrange(sigma) for _ in range(rng.choice((0, 1, 2, 40)) if rng.random() < 0.2 else rng.randint(0, 40)))
                for _ in range(m)]
        if t % 7 == 3:
            docs[rng.randrange(m)] = b""
        if t % 9 == 4 and m > 1:
            docs[-1] = docs[0]
        if not sum(len(d) for d in docs):
            docs[0] = b"a"
        g = GeneralizedSuffixTable.new_naive(docs, engine=eng)
        da, lcp = _u32a(g.doc_array()), g.lcp_lens()
        res = g.query_batch(pats)
        for k in range(0, len(pats), 7):                                 # the intervals are the patterns': Python's `in` says so
            assert int(np.unique(da[int(res["start"][k]):int(res["end"][k])]).size) == sum(pats[k] in d for d in docs), (docs, pats[k])
        nodes = node_intervals(lcp)
        s = np.concatenate([res["start"], [a for a, _ in nodes]]).astype(np.uint32)
        e = np.concatenate([res["end"], [b for _, b in nodes]]).astype(np.uint32)
        check_batch(eng, device, da, g.doc_starts(), s, e, t=t, topks=topk_values(da, s, e, rng.randrange(1 << 20)))
        done += 1
    return done


# ---- synthetic da arrays ---------------------------------------------------------------------------------------------------
def synthetic(eng, device, seed=62, big=4097):
    """da arrays that need no text (doc_starts = the cumulative counts): interval lengths around the tile, 5000 one-rank
    intervals, empty intervals in between, [0, n), document counts around the route-B tile, documents of length 0 and 1,
    a document on every second rank, and ties cut by top_k."""
    nrng = np.random.default_rng(seed)
    done = 0
    # lengths 2047, 2048, 2049, 3 * 2048 + 1 at aligned and unaligned starts, with empty intervals in between
    n = 5 * TILE + 77
    for t, nd in enumerate((1, 3, 255, 256, 257, big)):
        da = nrng.integers(0, nd, n).astype(np.uint32)
        if nd > 3:
            da[da == 1] = 0                                              # document 1 is empty
            da[da == nd - 1] = nd - 2                                    # ... and the last one
            if nd > 256:
                da[7] = nd - 1                                           # (or has a single rank)
        st = starts_of(da, nd)
        iv = []
        for ln in (TILE - 1, TILE, TILE + 1, 3 * TILE + 1):
            for a in (0, 1, 4, n - ln):
                iv += [(a, a + ln), (a, a)]
        iv += [(0, n), (n, n), (5, 6), (0, n)]
        s, e = np.array([a for a, _ in iv]), np.array([b for _, b in iv])
        done += check_batch(eng, device, da, st, s, e, t=t, topks=(0, 1, 10, nd, nd + 1) if t % 2 == 0 else (0, 2))
    # 5000 one-rank intervals
    nd = 40
    da = nrng.integers(0, nd, 6000).astype(np.uint32)
    s = nrng.integers(0, 6000, 5000)
    done += check_batch(eng, device, da, starts_of(da, nd), s, s + 1, t=1, topks=(0, 1))
    # one document on every second rank (long PREV chains), the others seen once each
    n = 3 * TILE + 5
    da = np.arange(n, dtype=np.uint32) // 2 + 1
    da[::2] = 0
    nd = int(da.max()) + 1
    iv = [(0, n), (1, n), (2, TILE), (TILE - 3, 2 * TILE + 1), (n - 1, n)]
    s, e = np.array([a for a, _ in iv]), np.array([b for _, b in iv])
    done += check_batch(eng, device, da, starts_of(da, nd), s, e, t=2, topks=(0, 1, 2, 5))
    # all tf equal: ties by id, top_k cutting inside the tie
    nd, reps = 300, 4
    da = np.tile(nrng.permutation(nd).astype(np.uint32), reps)
    iv = [(0, nd * reps), (0, nd), (nd, 3 * nd), (17, 17 + nd)]
    s, e = np.array([a for a, _ in iv]), np.array([b for _, b in iv])
    done += check_batch(eng, device, da, starts_of(da, nd), s, e, t=3, topks=(0, 1, 7, nd - 1, nd), every=True)
    return done


def routes_are_named(eng, device):
    """occ_cut >= n: only the by-occurrence instances are launched; below n the instances with the by-document code; the
    BY_TF key kernel only for that order.  All of them give the expected arrays.  Which route an interval took is read from
    the call's own workspace: behind its 64 result words stand the work items per interval (DlWs in sfx_doclist.hip), which
    count and emit walk -- ndocs of them for an interval that went by document, e - s for one that went by occurrence."""
    nrng = np.random.default_rng(63)
    nd, n = 50, 1500
    da = nrng.integers(0, nd, n).astype(np.uint32)
    st = starts_of(da, nd)
    s, e = np.array([0, 10, 500]), np.array([n, 11, 1400])
    got = {}
    for cut in CUTS + (200,):
        with Index(eng, device, da, st, occ_cut=cut) as ix:
            for order in (BY_DOC, BY_TF):
                res = {}

                def run():
                    res["r"] = list_raw(ix, s, e, order)
                    check_result(res["r"], da, s, e, order, 0)
                names = _gsa.profile_names(eng, run)
                got[cut, order] = {x for x in names if x.startswith("doclist_")}
                by_doc = cut in (1, 200)                                 # (the automatic 32 * 50 and 2^60 are >= n)
                assert res["r"]["items"].tolist() == ([nd, 1, nd] if by_doc else [n, 1, 900]), (cut, res["r"]["items"])
    for order in (BY_DOC, BY_TF):
        tail = {"doclist_write"} | ({"doclist_keys"} if order == BY_TF else set())
        assert got[1, order] == COMMON | ROUTE_B | tail, sorted(got[1, order])
        assert got[200, order] == COMMON | ROUTE_B | tail, sorted(got[200, order])
        assert got[1 << 60, order] == COMMON | ROUTE_A | tail, sorted(got[1 << 60, order])
        assert got[0, order] == COMMON | ROUTE_A | tail, sorted(got[0, order])      # (automatic: 32 * 50 >= n)

    def create():
        with Index(eng, device, da, st):
            pass
    names = _gsa.profile_names(eng, create)
    assert {"doclist_check", "gsa_prev"} <= names, sorted(names)


def cross_check_queries(eng, device, count=1000, seed=64):
    """|D_j| against the engine's two other counts (the linear pass of sfx_gindex_query, the prefix sums of
    interval_document_frequency), and documents_batch against the expression it replaced."""
    rng = random.Random(seed)
    docs = [_gen.dna(rng.choice((1, 150, 400)), seed=s).tobytes() for s in range(8)] + [b"", _gen.dna(400, seed=2).tobytes()[50:300]]
    text = b"".join(docs)
    g = GeneralizedSuffixTable.new_naive(docs, engine=eng)
    qs = []
    for k in range(count):
        a = rng.randrange(len(text))
        q = bytearray(text[a:a + rng.randint(1, 12)])
        if k % 3 == 0:
            q[rng.randrange(len(q))] = rng.choice(b"acgtn")
        qs.append(bytes(q))
    res = g.query_batch(qs)
    lists = g.document_listing_batch(qs, order="tf")
    sizes = np.array([d.size for d, _ in lists])
    assert np.array_equal(sizes, res["ndocs"]) and np.array_equal(sizes, g.interval_document_frequency(res["start"], res["end"]))
    da = g.doc_array()
    old = [sorted(set(da[int(s):int(e)].tolist())) for s, e in zip(res["start"], res["end"])]
    assert g.documents_batch(qs) == old
    for k in range(0, count, 37):
        d, f, _ = expected_list(da, res["start"][k], res["end"][k], BY_TF)
        assert np.array_equal(lists[k][0], d) and np.array_equal(lists[k][1], f), qs[k]
    return count


def the_handle_is_made_once(eng):
    docs = [_gen.english_like(1500, seed=s).tobytes() for s in (1, 2, 1)] + [b""]
    g = GeneralizedSuffixTable.new_naive(docs, engine=eng)
    first = _gsa.profile_names(eng, lambda: g.document_listing(b"the"))
    assert "doclist_check" in first and "doclist_publish" in first, sorted(first)
    again = _gsa.profile_names(eng, lambda: g.documents_batch([b"the", b"of"]))
    assert "doclist_check" not in again and "gsa_prev" not in again and "doclist_publish" in again, sorted(again)


# ---- refusals and limits -----------------------------------------------------------------------------------------------------
def refusals(eng, device):
    lib, st = eng.lib, _buffers.stream_of(device)
    nrng = np.random.default_rng(65)
    nd, n = 9, 700
    da = nrng.integers(0, nd, n).astype(np.uint32)
    da[da == 4] = 3                                                      # an empty document
    starts = starts_of(da, nd)
    # creation: a da entry >= ndocs; a da inconsistent with doc_starts; doc_starts not monotone / past n; ndocs == 0
    for where, val in ((n // 2, nd), (0, 0xFFFFFFFF), (n - 1, nd + 5)):
        bad = da.copy()
        bad[where] = val
        for pooled in (False, True):
            with Index(eng, device, bad, starts, pooled=pooled) as ix:
                assert ix.rc == ERR_ARG, (ix.rc, where, val)
        h = ctypes.c_void_p()
        assert lib.sfx_doclist_create(_gsa.ptr(bad), n, _gsa.ptr(starts), nd, 0, ctypes.byref(h)) == ERR_ARG and not h.value
    shifted = starts.copy()
    shifted[2] += 1                                                      # the counts of documents 1 and 2 shifted by one
    with Index(eng, device, da, shifted) as ix:
        assert ix.rc == ERR_ARG
    swapped = da.copy()
    a, b = int(np.flatnonzero(da == 0)[0]), int(np.flatnonzero(da == 1)[0])
    swapped[a], swapped[b] = 1, 0                                        # the same counts: still one rank per text position
    with Index(eng, device, swapped, starts) as ix:
        assert ix.rc == OK
    for bad_starts in ([1] + starts.tolist()[1:], starts.tolist()[:3] + [2] + starts.tolist()[4:], starts.tolist()[:-1] + [n + 1]):
        with Index(eng, device, da, bad_starts) as ix:
            assert ix.rc == ERR_ARG, bad_starts
    with Index(eng, device, da, starts, ndocs=0) as ix:
        assert ix.rc == ERR_ARG
    with Index(eng, device, da, starts, n=1 << 32, ws_bytes=256) as ix:
        assert ix.rc == ERR_TOO_LARGE
    need = int(lib.sfx_doclist_create_workspace_bytes(n))
    with Index(eng, device, da, starts, ws_bytes=need - 1) as ix:
        assert ix.rc == ERR_WORKSPACE
    with Index(eng, device, da, starts, ws_off=8) as ix:
        assert ix.rc == ERR_ARG
    with Index(eng, device, da, starts, da_off=2) as ix:
        assert ix.rc == ERR_ARG
    # listing
    s, e = np.array([0, 5, 100, 300]), np.array([n, 5, 400, 700])
    doc, tf, first, zfull = expected_batch(da, s, e)
    for cut in (1, 0):
        with Index(eng, device, da, starts, occ_cut=cut) as ix:
            assert ix.rc == OK
            for bs, be in (([0, 9], [n, 8]), ([0, 9], [n + 1, 10]), ([n + 1, 9], [n + 1, 10])):      # s > e, e > n
                r = list_raw(ix, bs, be, capacity=2 * n, list_limit=2 * n)
                assert r["rc"] == ERR_ARG and untouched(r["doc"]) and untouched(r["tf"]) and untouched(r["first"]), (bs, be)
            r = list_raw(ix, s, e, order=2)
            assert r["rc"] == ERR_ARG and untouched(r["first"])
            for cap in (0, 1, zfull - 1):                                # capacity < Z: a prefix, the rest of the arrays as they were
                r = list_raw(ix, s, e, capacity=cap)
                check_result(r, da, s, e, BY_DOC, 0, what=("capacity", cap))
            lib_doc = _buffers.guarded(4 * (zfull + 8), device, 4, 0xFF)  # ... and behind a short capacity inside a longer array
            lib_tf = _buffers.guarded(4 * (zfull + 8), device, 8, 0xFF)
            ws = _buffers.guarded(int(lib.sfx_doclist_workspace_bytes(4, zfull)), device, 0, "count")
            bs_, be_ = _buffers.inp(_u32a(s), device, 4), _buffers.inp(_u32a(e), device, 4)
            listed, count = ctypes.c_uint64(0), ctypes.c_uint64(0)
            assert lib.sfx_doclist_list_dev(ix.h, bs_.ptr, be_.ptr, 4, BY_TF, 0, zfull, lib_doc.ptr, lib_tf.ptr, 5, None, ctypes.byref(listed),
                                            ctypes.byref(count), ws.ptr, ws.nbytes, st) == OK
            _sync(device)
            xd, xt, _, _ = expected_batch(da, s, e, BY_TF)
            assert listed.value == zfull and count.value == zfull
            assert np.array_equal(lib_doc.host(np.uint32)[:5], xd[:5]) and (lib_doc.host(np.uint32)[5:] == 0xFFFFFFFF).all()
            assert np.array_equal(lib_tf.host(np.uint32)[:5], xt[:5]) and (lib_tf.host(np.uint32)[5:] == 0xFFFFFFFF).all()
            _buffers.check_all({"doc": lib_doc, "tf": lib_tf, "workspace": ws})
            for limit in (zfull - 1, 1):                                 # Z_full > list_limit: nothing written
                r = list_raw(ix, s, e, list_limit=limit, capacity=zfull)
                assert r["rc"] == OK and r["listed"] == zfull and r["count"] == 0, r
                assert untouched(r["doc"]) and untouched(r["tf"]) and untouched(r["first"])
            r = list_raw(ix, s, e, list_limit=zfull)
            check_result(r, da, s, e, BY_DOC, 0)
            need = int(lib.sfx_doclist_workspace_bytes(4, zfull))
            for short in (need - 1, 0):
                r = list_raw(ix, s, e, list_limit=zfull, ws_bytes=short)
                assert r["rc"] == ERR_WORKSPACE and untouched(r["doc"]) and untouched(r["first"])
            for ws_off in (1, 4, 8):
                r = list_raw(ix, s, e, list_limit=zfull, ws_off=ws_off)
                assert r["rc"] == ERR_ARG and untouched(r["doc"]), ws_off
            for k in range(4):
                offs = [4, 8, 12, 4]
                offs[k] = 2
                assert list_raw(ix, s, e, offs=tuple(offs))["rc"] == ERR_ARG, k
            assert list_raw(ix, s, e, first_off=4)["rc"] == ERR_ARG
            assert list_raw(ix, s, e, nq=1 << 32, ws_bytes=256)["rc"] == ERR_TOO_LARGE
            r = list_raw(ix, s, e, want_first=False)
            assert r["rc"] == OK and untouched(r["first"]) and np.array_equal(r["doc"][:zfull], doc)
    listed = ctypes.c_uint64(0)
    assert lib.sfx_doclist_list_dev(None, None, None, 0, 0, 0, 1, None, None, 0, None, ctypes.byref(listed), ctypes.byref(listed), None, 0, st) == ERR_ARG
    # the host route
    h = ctypes.c_void_p()
    assert lib.sfx_doclist_create(_gsa.ptr(da), n, _gsa.ptr(starts), nd, 1, ctypes.byref(h)) == OK
    try:
        s32, e32 = _u32a(s), _u32a(e)
        od, ot, of = np.full(zfull + 2, 0xA5A5A5A5, dtype=np.uint32), np.full(zfull + 2, 0xA5A5A5A5, dtype=np.uint32), np.zeros(5, dtype=np.uint64)
        listed, count = ctypes.c_uint64(0), ctypes.c_uint64(0)
        assert lib.sfx_doclist_list(h, _gsa.ptr(s32), _gsa.ptr(e32), 4, BY_DOC, 0, 1 << 40, _gsa.ptr(od), _gsa.ptr(ot), zfull + 2, _gsa.ptr(of),
                                    ctypes.byref(listed), ctypes.byref(count)) == OK
        assert listed.value == zfull and count.value == zfull and np.array_equal(od[:zfull], doc) and np.array_equal(ot[:zfull], tf)
        assert (od[zfull:] == 0xA5A5A5A5).all() and np.array_equal(of, first)
        bad_e = e32.copy()
        bad_e[1] = n + 1
        assert lib.sfx_doclist_list(h, _gsa.ptr(s32), _gsa.ptr(bad_e), 4, BY_DOC, 0, 1 << 40, _gsa.ptr(od), _gsa.ptr(ot), zfull, None,
                                    ctypes.byref(listed), ctypes.byref(count)) == ERR_ARG
        assert lib.sfx_doclist_list(h, _gsa.ptr(s32), _gsa.ptr(e32), 4, BY_DOC, 0, 3, _gsa.ptr(od), _gsa.ptr(ot), zfull, None,
                                    ctypes.byref(listed), ctypes.byref(count)) == OK and listed.value == zfull and count.value == 0
    finally:
        lib.sfx_doclist_destroy(h)


def size_formulas(eng):
    """The header's bounds: the object 8n (+ 512), creation scratch <= 24.5 n + 9 MiB, a listing <= 36 nq + 25 L + 9 MiB."""
    lib = eng.lib
    for n in (1, 2, 63, 64, 65, 1025, 100003, (1 << 20) + 5, 10 ** 8, (1 << 32) - 1):
        assert 8 * n <= lib.sfx_doclist_bytes(n) <= 8 * n + 512, n
        assert 24 * n <= lib.sfx_doclist_create_workspace_bytes(n) <= 24 * n + n // 2 + (9 << 20), n
    for f in (lib.sfx_doclist_bytes, lib.sfx_doclist_create_workspace_bytes):
        assert f(0) == 0 and f(1 << 32) == 0
    for nq in (1, 2, 255, 4097, 1 << 16, 10 ** 6):
        for L in (1, 2, 1000, 1 << 20, 10 ** 8, (1 << 32) - 1):
            got = lib.sfx_doclist_workspace_bytes(nq, L)
            assert 32 * nq + 24 * L <= got <= 36 * nq + 25 * L + (9 << 20), (nq, L, got)
    assert lib.sfx_doclist_workspace_bytes(7, 1 << 40) == lib.sfx_doclist_workspace_bytes(7, (1 << 32) - 1)
    assert lib.sfx_doclist_workspace_bytes(0, 10) == 0 and lib.sfx_doclist_workspace_bytes(1 << 32, 10) == 0


def dirty_workspace_streams_and_threads(eng, device):
    """The same batch over the three kinds of dirt in a workspace of exactly the stated size, arrays at every offset, on
    the current and on a side stream; then two threads on one object, each with its own workspace."""
    nrng = np.random.default_rng(66)
    nd, n = 70, 2 * TILE + 100
    da = nrng.integers(0, nd, n).astype(np.uint32)
    st = starts_of(da, nd)
    s = np.array([0, 3, 100, TILE - 1, 7, n])
    e = np.array([n, 4, 2500, 2 * TILE + 2, 7, n])
    side = torch.cuda.Stream() if str(device).startswith("cuda") else None
    for cut in (1, 1 << 60):
        with Index(eng, device, da, st, occ_cut=cut) as ix:
            for t in range(6):
                with (torch.cuda.stream(side) if side is not None and t % 2 else contextlib.nullcontext()):
                    order, k = (BY_DOC, BY_TF)[t % 2], (0, 3, 9)[t % 3]
                    r = list_raw(ix, s, e, order, k, fill=_buffers.FILLS[t % 3], offs=[(4, 8, 12, 4), (12, 4, 8, 8), (8, 12, 4, 12)][t % 3])
                    check_result(r, da, s, e, order, k, what=("dirty", cut, t))
                    _sync(device)
            errors = []

            def worker(order, k):
                try:
                    stream = torch.cuda.Stream() if side is not None else None
                    with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
                        for _ in range(3):
                            check_result(list_raw(ix, s, e, order, k, fill="count"), da, s, e, order, k, what=("thread", order, k))
                except BaseException as ex:                              # noqa: BLE001 -- reported by the parent
                    errors.append(ex)
            threads = [threading.Thread(target=worker, args=a) for a in ((BY_DOC, 0), (BY_TF, 2))]
            concurrent = side is not None                            # (the emulator keeps threadIdx & co. in globals: one launch at a time)
            for th in threads:
                th.start()
                if not concurrent:
                    th.join()
            for th in threads:
                th.join()
            assert not errors, errors


def resources_come_back(eng, device):
    nrng = np.random.default_rng(67)
    da = nrng.integers(0, 9, 500).astype(np.uint32)
    st = starts_of(da, 9)
    s32, e32, out, out2 = _u32a([0]), _u32a([500]), np.zeros(9, dtype=np.uint32), np.zeros(9, dtype=np.uint32)
    listed = ctypes.c_uint64(0)

    def host_round():
        h = ctypes.c_void_p()
        assert eng.lib.sfx_doclist_create(_gsa.ptr(da), 500, _gsa.ptr(st), 9, 0, ctypes.byref(h)) == OK
        assert eng.lib.sfx_doclist_list(h, _gsa.ptr(s32), _gsa.ptr(e32), 1, 0, 0, 100, _gsa.ptr(out), _gsa.ptr(out2), 9, None, ctypes.byref(listed),
                                        ctypes.byref(listed)) == OK
        return h
    eng.lib.sfx_doclist_destroy(host_round())                            # (the calling thread's page and stream exist from here on)
    _sync(device)
    eng.release_cached_buffers()
    before = eng.resource_stats()
    for pooled in (True, False):
        with Index(eng, device, da, st, occ_cut=1, pooled=pooled) as ix:
            check_result(list_raw(ix, [0, 3], [500, 90], BY_TF), da, [0, 3], [500, 90], BY_TF, 0)
    h = host_round()
    held = eng.resource_stats()
    assert held["device_bytes"] >= before["device_bytes"] + eng.lib.sfx_doclist_bytes(500)
    eng.lib.sfx_doclist_destroy(h)
    eng.release_cached_buffers()
    after = eng.resource_stats()
    for k in ("device_bytes", "device_allocs", "pinned_bytes", "pinned_allocs", "streams", "events", "pooled_bytes", "pooled_buffers"):
        assert after[k] == before[k], (k, before, after)


def hooked(eng, device):
    """What a hooked child process runs (SFX_DOCLIST_SPLIT=1: the two-sort BY_TF key; SFX_MAX_GRID=3: more tiles than
    workgroups): the known, random and synthetic cases again."""
    known_answers(eng, device)
    small_random(eng, device, 2, count=25, seed=71)
    small_random(eng, device, 3, count=15, seed=72)
    synthetic(eng, device, big=513)
