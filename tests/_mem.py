"""The cases of the maximal exact matches of a query text (sfx_mems_dev, sfx_index_mems*, sfx_gindex_mems*; DESIGN.md
section 20), shared by test_mem_emu.py (the emulator build, host memory) and test_gpu_mem.py (libsuffix_hip.so, HBM).

Nothing expected comes from the engine under test alone: small inputs are held against `brute`, a plain double loop over
the definition; larger ones go through the serial checker tests/mem_check.c (every triple is a MEM, the list is strictly
ascending) and through the two identities that prove the list complete -- pairs == P_L, Z == P_L - P_(L+1) and the sum of
(len - L + 1) == P_L, with P_k summed from capped matching statistics that tests/ms_check.c accepted; runs of one letter
have closed-form answers."""
import contextlib
import ctypes
import os
import random
import subprocess
import threading

import numpy as np
import torch

import _buffers
import _gsa
import _match
from suffix_amd import GeneralizedSuffixTable, SuffixHipError, SuffixTable
from suffix_amd import device as sdev

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
CSRC_FROM_EMU = "../../suffix_amd/csrc"
OK, ERR_ARG, ERR_TOO_LARGE, ERR_WORKSPACE = 0, 1, 2, 5
UNIQUE = 1
KERNELS = {"mem_cand", "mem_count", "mem_emit"}
ROUTES = ("dev", "index_dev", "gindex_dev", "index_host", "gindex_host")
TILE = 2048                                                     # K of a hook-free build
_vp, _u64, _u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32


def build_emulator():
    """`make -C tests/emu`; sfx_mem.hip is compiled as part of sfx_api.hip's translation unit and tests/emu/Makefile does
    not name it, so after an edit to it alone sfx_api.hip is declared new (`make -W`).  -> the library's path."""
    lib = os.path.join(EMU_DIR, "libsuffix_emu.so")
    cmd = ["make", "-s", "-j8", "-C", EMU_DIR]
    src = os.path.join(HERE, os.pardir, "suffix_amd", "csrc", "sfx_mem.hip")
    if os.path.exists(lib) and os.path.getmtime(src) > os.path.getmtime(lib):
        cmd += ["-W", CSRC_FROM_EMU + "/sfx_api.hip"]
    subprocess.check_call(cmd)
    return lib


# ---- the definition --------------------------------------------------------------------------------------------------
def _doc_bounds(n, starts):
    """(lo, hi) per text position: its document's start and end; the whole text without starts."""
    lo, hi = np.zeros(n, dtype=np.int64), np.full(n, n, dtype=np.int64)
    if starts is not None:
        s = [int(x) for x in starts] + [n]
        for k in range(len(s) - 1):
            lo[s[k]:s[k + 1]] = s[k]
            hi[s[k]:s[k + 1]] = s[k + 1]
    return lo, hi


def brute(text, query, min_len, starts=None, unique=False, sa=None):
    """The MEMs by the definition, a plain double loop: [(i, p, l)] ascending by i, then by the rank of p -- in `sa`
    when given (equal truncated suffixes of a collection have no order of their own), else among the sorted truncated
    suffixes."""
    text, query = bytes(text), bytes(query)
    n, m = len(text), len(query)
    lo, hi = _doc_bounds(n, starts)
    order = sorted(range(n), key=lambda p: (text[p:hi[p]], p)) if sa is None else [int(x) for x in sa]
    rank = {p: r for r, p in enumerate(order)}
    out = []
    for i in range(m):
        found = []
        for p in range(n):
            if i > 0 and p > lo[p] and query[i - 1] == text[p - 1]:
                continue
            l = 0
            while i + l < m and p + l < hi[p] and query[i + l] == text[p + l]:
                l += 1
            if l < min_len:
                continue
            if unique and sum(1 for s in range(n) if s + l <= hi[s] and text[s:s + l] == text[p:p + l]) != 1:
                continue
            found.append((rank[p], p, l))
        out += [(i, p, l) for _, p, l in sorted(found)]
    return out


# hand-worked: T = "banana" (table 5 3 1 0 4 2: a, ana, anana, banana, na, nana), Q = "bandana", L = 1
#   i = 0  "ban" = T[0..3), then d against a
#   i = 1  b stands in front: p = 1 extends to the left (T[0] = b); p = 5 "a" (the text ends), p = 3 "an" (d against a)
#   i = 2  a stands in front, and in front of both n of the text: nothing;  i = 3  d: nothing
#   i = 4  d stands in front: every a is left-maximal: p = 5 "a", p = 3 "ana" (both end), p = 1 "ana" (Q ends)
#   i = 5  a in front of n, as in the text: nothing;  i = 6  n in front: only p = 1 has another byte (b) in front: "a", Q ends
HAND = [
    (b"banana", b"bandana", 1, False, [(0, 0, 3), (1, 5, 1), (1, 3, 2), (4, 5, 1), (4, 3, 3), (4, 1, 3), (6, 1, 1)]),
    (b"banana", b"bandana", 3, False, [(0, 0, 3), (4, 3, 3), (4, 1, 3)]),
    (b"banana", b"bandana", 1, True, [(0, 0, 3)]),              # "an" and "ana" occur twice
    (b"banana", b"bandana", 4, False, []),
    (b"abcabc", b"xabcy", 2, False, [(1, 3, 3), (1, 0, 3)]),    # rank of "abc" (3) < rank of "abcabc" (0)
    (b"aaa", b"aa", 1, False, [(0, 2, 1), (0, 1, 2), (0, 0, 2), (1, 0, 1)]),
    (b"aaa", b"aa", 2, False, [(0, 1, 2), (0, 0, 2)]),
    (b"aaa", b"aaa", 1, True, [(0, 0, 3)]),
]


def run_closed_form(n, m, L, unique=False, shift=0):
    """T = a^n, Q = a^m (query positions shifted by `shift`): (0, p, min(m, n - p)) by descending p -- the table of a^n
    holds the shortest suffix first -- then (i, 0, min(m - i, n)); under the unique flag only those with l = n."""
    out = [(shift, p, min(m, n - p)) for p in range(n - 1, -1, -1)]
    out += [(shift + i, 0, min(m - i, n)) for i in range(1, m)]
    return [(i, p, l) for i, p, l in out if l >= L and (not unique or l == n)]


# ---- the checker -------------------------------------------------------------------------------------------------------
def build_checker(out_dir):
    """tests/mem_check.c and tests/ms_check.c -> (mem_check lib, ms_check function), bound."""
    so = os.path.join(str(out_dir), "libmem_check.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "mem_check.c")])
    lib = ctypes.CDLL(so)
    lib.mem_check.restype = ctypes.c_int
    lib.mem_check.argtypes = [_vp, _u64, _vp, _vp, _u64, _vp, _u64, _u32, _u32, _vp, _vp, _vp, _u64, _vp, ctypes.POINTER(_u64),
                              ctypes.POINTER(ctypes.c_int64)]
    lib.mem_check_name.restype = ctypes.c_char_p
    lib.mem_check_name.argtypes = [ctypes.c_int]
    return lib, _match.build_checker(out_dir)


def _np(a, dtype):
    return _match._np(a, dtype)


def check(chk, text, sa, query, min_len, flags, trip, starts=None):
    """-> (fault name, triple index, Z, sum of (l - L + 1), uniqueness flags)."""
    t, q, s = _np(text, np.uint8), _np(query, np.uint8), _np(sa, np.uint32)
    ds = None if starts is None else _np(starts, np.uint64)
    arrs = [_np(a, np.uint32) for a in trip]
    z = arrs[0].size
    assert arrs[1].size == z and arrs[2].size == z
    uniq = np.zeros(z, dtype=np.uint8)
    total, where = _u64(0), ctypes.c_int64(-2)
    rc = chk[0].mem_check(_gsa.ptr(t), t.size, _gsa.ptr(s), _gsa.ptr(ds) if ds is not None else None, 0 if ds is None else ds.size,
                          _gsa.ptr(q), q.size, int(min_len), int(flags), *[_gsa.ptr(a) for a in arrs], z, _gsa.ptr(uniq),
                          ctypes.byref(total), ctypes.byref(where))
    return chk[0].mem_check_name(rc).decode(), int(where.value), z, int(total.value), uniq


def accept(chk, text, sa, query, min_len, flags, trip, starts=None):
    name, where, z, total, uniq = check(chk, text, sa, query, min_len, flags, trip, starts)
    assert name == "ok", f"mem_check: {name} at triple {where} (min_len {min_len}, flags {flags})"
    return z, total, uniq


def checker_self_test(chk):
    """Lists with one fault each: every fault is named."""
    text, query = b"xabcdeyabcdfz_abcde", b"qabcdew"
    sa = sorted(range(len(text)), key=lambda p: text[p:])
    good = brute(text, query, 3)
    assert good == [(1, 14, 5), (1, 1, 5), (1, 7, 4)], good
    cols = lambda tr: [np.array([t[k] for t in tr], dtype=np.uint32) for k in range(3)]
    assert check(chk, text, sa, query, 3, 0, cols(good))[:4] == ("ok", -1, 3, 3 + 3 + 2)
    faults = [([(1, 14, 4), (1, 1, 5), (1, 7, 4)], 0, "right-extendable", 0),          # a shortened match
              ([(1, 14, 5), (2, 2, 4), (1, 7, 4)], 0, "left-extendable", 1),
              ([(1, 1, 5), (1, 14, 5), (1, 7, 4)], 0, "order", 1),                     # a swapped pair
              ([(1, 14, 5), (1, 14, 5), (1, 1, 5)], 0, "order", 1),                    # a duplicate
              ([(1, 14, 5), (1, 1, 5), (1, 7, 4)], UNIQUE, "not unique", 0),
              ([(1, 14, 5), (1, 1, 5), (1, 8, 4)], 0, "bytes", 2),
              ([(1, 14, 5), (1, 1, 5), (1, 7, 2)], 0, "range", 2),
              ([(1, 14, 6)], 0, "range", 0)]
    for tr, flags, want, at in faults:
        got = check(chk, text, sa, query, 3, flags, cols(tr))
        assert got[:2] == (want, at), (tr, flags, got[:2])
    # a match that crosses a document end
    got = check(chk, b"abcd", [0, 1, 2, 3], b"abcd", 2, 0, cols([(0, 0, 4)]), starts=[0, 2])
    assert got[:2] == ("document", 0), got[:2]
    assert check(chk, b"abcd", [0, 1, 2, 3], b"abcd", 2, 0, cols([(0, 0, 2), (2, 2, 2)]), starts=[0, 2])[0] == "ok"
    # the uniqueness test: "abcde" stands twice and "abcd" three times; "abc" of "abcx" once
    assert check(chk, text, sa, query, 3, 0, cols(good))[4].tolist() == [0, 0, 0]
    assert check(chk, b"abcx", [0, 1, 2, 3], b"zabc", 2, UNIQUE, cols([(1, 0, 3)]))[3:] == (2, [1])
    return len(faults) + 1


# ---- the entry points ------------------------------------------------------------------------------------------------
def _t(a, device, dtype=np.uint8):
    return _match._t(a, device, dtype)


def _host(x):
    return x.cpu().numpy().view(np.uint32)


def _sync(device):
    _match._sync(device)


def _as_collection(n, starts, da):
    starts = np.zeros(1, dtype=np.int64) if starts is None else np.asarray(starts, dtype=np.int64)
    da = np.zeros(n, dtype=np.uint32) if da is None else da
    return starts, da


def run(eng, device, route, text, sa, query, min_len, unique=False, starts=None, da=None, max_pairs=1 << 30):
    """One entry point -> (qpos, tpos, len, pairs), the arrays on the host as uint32.  The gindex routes of a plain text
    see it as one document.  A refusal raises SuffixHipError (the device wrappers) or AssertionError("refused", P)."""
    n, m = len(text), len(query)
    if route.startswith("gindex"):
        starts, da = _as_collection(n, starts, da)
    else:
        assert starts is None
    if route.endswith("_host"):
        t, s, q = _np(text, np.uint8), _np(sa, np.uint32), _np(query, np.uint8)
        h = ctypes.c_void_p()
        if route == "index_host":
            assert eng.lib.sfx_index_create(_gsa.ptr(t), n, _gsa.ptr(s), ctypes.byref(h)) == OK
            call, destroy = eng.lib.sfx_index_mems, eng.lib.sfx_index_destroy
        else:
            ds, d = _np(starts, np.uint64), _np(da, np.uint32)
            assert eng.lib.sfx_gindex_create(_gsa.ptr(t), n, _gsa.ptr(ds), ds.size, _gsa.ptr(s), _gsa.ptr(d), ctypes.byref(h)) == OK
            call, destroy = eng.lib.sfx_gindex_mems, eng.lib.sfx_gindex_destroy
        pairs, count = _u64(0), _u64(0)
        try:
            rc = call(h, _gsa.ptr(q), m, min_len, UNIQUE if unique else 0, max_pairs, None, None, None, 0, ctypes.byref(pairs),
                      ctypes.byref(count))
            assert rc == OK, (route, rc)
            if pairs.value > max_pairs:
                raise SuffixHipError(f"refused: {pairs.value} pairs")
            z = int(count.value)
            out = [np.full(z + 3, 0xDEADBEEF, dtype=np.uint32) for _ in range(3)]
            rc = call(h, _gsa.ptr(q), m, min_len, UNIQUE if unique else 0, max_pairs, *[_gsa.ptr(a) for a in out], z + 3,
                      ctypes.byref(pairs), ctypes.byref(count))
            assert rc == OK and count.value == z, (route, rc, z, count.value)
        finally:
            destroy(h)
        for a in out:
            assert (a[z:] == 0xDEADBEEF).all(), (route, "written past z")
        return out[0][:z], out[1][:z], out[2][:z], int(pairs.value)
    dt, dsa, dq = _t(text, device), _t(sa, device, np.uint32), _t(query, device)
    kw = dict(unique=unique, max_pairs=max_pairs)
    if route == "dev":
        got = sdev.mems(dt, dsa, dq, min_len, engine=eng, **kw)
    elif route == "index_dev":
        ix = sdev.DeviceIndex(dt, dsa, engine=eng)
        try:
            got = ix.mems(dq, min_len, **kw)
        finally:
            _sync(device)
            ix.close()
    else:
        gx = sdev.GeneralizedDeviceIndex(dt, _t(starts, device, np.int64), dsa, _t(da, device, np.uint32), engine=eng)
        try:
            got = gx.mems(dq, min_len, **kw)
        finally:
            _sync(device)
            gx.close()
    _sync(device)
    return _host(got[0]), _host(got[1]), _host(got[2]), got[3]


def triples(res):
    return list(zip(res[0].tolist(), res[1].tolist(), res[2].tolist()))


def pair_count(eng, device, chk, text, sa, query, k, starts=None, da=None, index=None):
    """P_k from capped matching statistics that ms_check.c accepted: the sum of end - start over the positions whose
    capped length reaches k.  -> (P_k, the largest interval)."""
    if index is not None:
        res = [_host(x) for x in index.match_stats(_t(query, device), max_len=k, want_src=True, want_interval=True)]
    else:
        route = "dev" if starts is None else "gindex_dev"
        res = _match.run(eng, device, route, text, sa, query, k, starts=starts, da=da)
    _match.accept(chk[1], text, sa, query, k, res, starts)
    width = np.where(res[0] == k, res[3].astype(np.int64) - res[2].astype(np.int64), 0)
    return int(width.sum()), int(width.max()) if width.size else 0


def verify(eng, device, chk, text, sa, query, min_len, full, uniq=None, starts=None, da=None, index=None):
    """The full list is accepted by the checker and complete by the identities; the unique list is the full list
    filtered by the checker's own uniqueness test.  -> (P_L, Z, the largest interval)."""
    z, total, flags = accept(chk, text, sa, query, min_len, 0, full[:3], starts)
    p0, widest = pair_count(eng, device, chk, text, sa, query, min_len, starts, da, index)
    p1, _ = pair_count(eng, device, chk, text, sa, query, min_len + 1, starts, da, index)
    print(f"mems: min_len {min_len}: pairs {full[3]}, P_L {p0}, P_L+1 {p1}, Z {z}, sum {total}, largest interval {widest}")
    assert full[3] == p0 and z == p0 - p1 and total == p0, (full[3], p0, p1, z, total)
    if uniq is not None:
        accept(chk, text, sa, query, min_len, UNIQUE, uniq[:3], starts)
        keep = flags.astype(bool)
        assert uniq[3] == p0 and all(np.array_equal(uniq[k], full[k][keep]) for k in range(3)), (uniq[0].size, int(keep.sum()))
    return p0, z, widest


# ---- 1. against the definition ---------------------------------------------------------------------------------------------
def known_answers(eng, device):
    for text, query, L, unique, want in HAND:
        assert brute(text, query, L, unique=unique) == want, (text, query, L, unique, brute(text, query, L, unique=unique))
        sa = SuffixTable.new_naive(text, engine=eng).table()
        for route in ROUTES:
            got = run(eng, device, route, text, sa, query, L, unique)
            assert triples(got) == want, (route, text, query, L, unique, triples(got))
    # the host API
    r = SuffixTable(b"banana", engine=eng).mems(b"bandana", 1)
    assert r.triples() == HAND[0][4] and len(r) == 7 and r.pairs == 1 + 3 + 2 + 0 + 3 + 2 + 3 and "z=7" in repr(r)
    assert r.qpos.dtype == np.uint32 and r.tpos.tolist() == [0, 5, 3, 5, 3, 1, 1] and r.len.tolist() == [3, 1, 2, 1, 3, 3, 1]
    assert SuffixTable(b"banana", engine=eng).mems("bandana", 1, unique=True).triples() == [(0, 0, 3)]
    assert len(SuffixTable(b"banana", engine=eng).mems(b"", 1)) == 0 and len(SuffixTable(b"", engine=eng).mems(b"abc", 1)) == 0
    try:
        SuffixTable(b"aaaaaaaa", engine=eng).mems(b"aaaaaaaa", 1, max_pairs=63)
        raise AssertionError("64 pairs were not refused at max_pairs = 63")
    except SuffixHipError as e:
        assert "64" in str(e) and "63" in str(e), e
    assert len(SuffixTable(b"aaaaaaaa", engine=eng).mems(b"aaaaaaaa", 1, max_pairs=64)) == 15
    g = GeneralizedSuffixTable([b"abc", b"", b"bcd", b"c"], engine=eng)
    r = g.mems(b"abcd", 2)
    assert r.triples() == [(0, 0, 3), (1, 3, 3)] and r.doc.tolist() == [0, 2] and r.offset.tolist() == [0, 0]
    assert g.mems(b"abcd", 1).triples() == brute(b"abcbcdc", b"abcd", 1, starts=[0, 3, 3, 6], sa=g.table())
    text = b"".join(bytes([c, 97]) for c in range(100, 140))                      # 40 a, each behind another byte
    many = SuffixTable(text, engine=eng).mems(b"za" * 700, 1)                     # 40 matches per a: more than the first guess at the room
    assert len(many) > 20000 and many.triples() == brute(text, b"za" * 700, 1)


def small_random_pairs(eng, device, chk, iters=160, seed=20261019):
    """Alphabets of 1-4 symbols (and one the text lacks), |T| <= 70, |Q| <= 50, L in 1..5, both flag values, the routes
    alternating; every one through the checker and the identities too.  -> the number of pairs run."""
    rng = random.Random(seed)
    for it in range(iters):
        text, query = _match.random_pair(rng)
        text, query = (text + bytes(rng.choice(text) for _ in range(rng.randint(0, 10))))[:70], query[:50]
        sa = SuffixTable.new_naive(text, engine=eng).table()
        L = 1 + it % 5
        route = ROUTES[it % len(ROUTES)]
        res = {u: run(eng, device, route, text, sa, query, L, u) for u in (False, True)}
        for u in (False, True):
            assert triples(res[u]) == brute(text, query, L, unique=u, sa=sa), (route, text, query, L, u, triples(res[u]))
        if it % 4 == 0:
            verify(eng, device, chk, text, sa, query, L, res[False], res[True])
    return iters


def small_random_collections(eng, device, chk, iters=60, seed=11):
    """Collections of at most 70 bytes with empty documents, Q = pieces of the joined text laid across document ends."""
    rng = random.Random(seed)
    done = 0
    empties = 0
    while done < iters:
        docs = _gsa.random_collection(rng, max_docs=12, max_len=12)
        text = b"".join(docs)
        if not 1 <= len(text) <= 70:
            continue
        empties += any(len(d) == 0 for d in docs)
        g = GeneralizedSuffixTable.new_naive(docs, engine=eng)
        starts = _gsa.doc_starts(docs)
        a, b = rng.randrange(len(text)), rng.randrange(len(text))
        query = (text[a:a + rng.randint(1, 25)] + bytes([rng.choice(b"ab\x00\xffz")]) + text[b:b + rng.randint(0, 20)])[:50]
        L = 1 + done % 5
        route = ("gindex_dev", "gindex_host")[done % 2]
        res = {u: run(eng, device, route, text, g.table(), query, L, u, starts=starts, da=g.doc_array()) for u in (False, True)}
        for u in (False, True):
            want = brute(text, query, L, starts=starts, unique=u, sa=g.table())
            assert triples(res[u]) == want, (route, docs, query, L, u, triples(res[u]), want)
        if done % 4 == 0:
            verify(eng, device, chk, text, g.table(), query, L, res[False], res[True], starts=starts, da=g.doc_array())
        done += 1
    assert empties >= 5
    return done


# ---- 2. raw calls: capacity, limits, guards --------------------------------------------------------------------------------
class Raw:
    """The three `_dev` entry points over one (text, table) pair, as a plain table, an index and a collection of one
    document (or of `starts`), with every buffer between guard bands."""

    def __init__(self, eng, device, text, sa, starts=None, da=None, text_off=3, sa_off=4):
        self.eng, self.device, self.n = eng, device, len(text)
        self.t, self.s = _buffers.text_in(bytes(text), device, text_off), _buffers.inp(_np(sa, np.uint32), device, sa_off)
        self.plain = starts is None
        starts, da = _as_collection(self.n, starts, da)
        self.ds, self.da = _buffers.inp(starts, device), _buffers.inp(_np(da, np.uint32), device, 8)
        self.ix = sdev.DeviceIndex(self.t.u8(), self.s.view(torch.int32), engine=eng) if self.plain else None
        self.gx = sdev.GeneralizedDeviceIndex(self.t.u8(), self.ds.view(torch.int64), self.s.view(torch.int32), self.da.view(torch.int32),
                                              engine=eng)

    def routes(self):
        return ("dev", "index_dev", "gindex_dev") if self.plain else ("gindex_dev",)

    def call(self, route, q, m, L, flags, limit, outs, cap, ws, ws_bytes, stream=None):
        """-> (status, P, Z); q, outs, ws: pointers (c_void_p or None)."""
        pairs, count = _u64(0xAAAA), _u64(0xBBBB)
        tail = (m, L, flags, limit, *outs, cap, ctypes.byref(pairs), ctypes.byref(count), ws, ws_bytes, stream)
        lib = self.eng.lib
        if route == "dev":
            rc = lib.sfx_mems_dev(self.t.ptr, self.n, self.s.ptr, q, *tail)
        elif route == "index_dev":
            rc = lib.sfx_index_mems_dev(self.ix._h, q, *tail)
        else:
            rc = lib.sfx_gindex_mems_dev(self.gx._h, q, *tail)
        return rc, int(pairs.value), int(count.value)

    def mems(self, route, query, L, flags=0, limit=None, cap=None, q_off=1, out_offs=(4, 12, 8), fill=0xA5, ws_fill="count",
             ws_off=0):
        """One guarded call with a dirty workspace of exactly sfx_mems_workspace_bytes -> (status, P, Z, the three output
        arrays as they came back, all `cap` entries).  cap None: counts first, then room for exactly Z."""
        m = len(query)
        limit = m * self.n if limit is None else limit                     # (no call has more pairs: keeps the workspace small)
        q = _buffers.text_in(bytes(query), self.device, q_off)
        wsb = int(self.eng.lib.sfx_mems_workspace_bytes(m, limit))
        ws = _buffers.guarded(wsb, self.device, ws_off, ws_fill)
        st = _buffers.stream_of(self.device)
        if cap is None:
            rc, p, z = self.call(route, q.ptr, m, L, flags, limit, (None, None, None), 0, ws.ptr, wsb, st)
            assert rc == OK, (route, rc)
            cap = z
            ws.fill(ws_fill)
        bufs = [_buffers.guarded(4 * cap, self.device, off, fill) for off in out_offs]
        rc, p, z = self.call(route, q.ptr, m, L, flags, limit, [b.ptr if cap else None for b in bufs], cap, ws.ptr, wsb, st)
        for name, b in zip(("qpos", "tpos", "len", "workspace", "query"), bufs + [ws, q]):
            b.check_guards(f"{route} {name}")
        return rc, p, z, [b.host(np.uint32) for b in bufs]

    def close(self):
        _sync(self.device)
        for b, name in ((self.t, "text"), (self.s, "sa"), (self.ds, "doc_starts"), (self.da, "da")):
            b.check_guards(name)
        if self.ix is not None:
            self.ix.close()
        self.gx.close()


UNWRITTEN = 0xA5A5A5A5


def edges(eng, device, chk, orc):
    def one(text, query, L, want, starts=None, unique=False):
        sa = orc.sais(text) if starts is None and len(text) else GeneralizedSuffixTable.new_naive(_match.doc_list(text, starts), engine=eng).table()
        da = None if starts is None else GeneralizedSuffixTable.new_naive(_match.doc_list(text, starts), engine=eng).doc_array()
        if want is None:
            want = brute(text, query, L, starts=starts, unique=unique, sa=sa)
        for route in (ROUTES if starts is None else ("gindex_dev", "gindex_host")):
            got = run(eng, device, route, text, sa, query, L, unique, starts=starts, da=da)
            assert triples(got) == want, (route, text, query, L, triples(got), want)
        return want

    one(b"abcabc", b"ab", 3, [])                                              # m < L
    one(b"ab", b"abcabc", 3, [])                                              # n < L
    one(b"abcab", b"abcab", 5, [(0, 0, 5)])                                   # L = m = n, Q = T
    one(b"abcab", b"abcab", 6, [])
    assert one(b"abcdefgh" * 4, b"abzdezghzbczefz" * 2, 3, None) == []        # a byte T lacks at every third position
    w = one(b"xabcy_abc", b"abcq_rabc", 3, None)
    assert (0, 1, 3) in w and (6, 6, 3) in w and (0, 6, 3) in w and (6, 1, 3) in w      # i = 0; ending at m and at n
    assert one(b"abcx", b"zabc", 2, None) == [(1, 0, 3)]                      # p = 0
    assert one(b"abcx", b"abcx", 1, None, unique=True) == [(0, 0, 4)]
    # documents: one of a single byte, empty ones, a match that would cross an end
    w = one(b"abcaxbc", b"abcabc", 1, None, starts=[0, 3, 3, 4, 4, 7])
    assert (0, 0, 3) in w and (3, 3, 1) in w and (0, 3, 1) in w and all(l <= 3 for _, _, l in w)
    one(b"abcaxbc", b"abcabc", 1, None, starts=[0, 3, 3, 4, 4, 7], unique=True)
    one(b"abcaxbc", b"abcabc", 2, None, starts=[0, 3, 3, 4, 4, 7])

    # capacity and the pair limit, raw, between guard bands
    rng = random.Random(3)
    text = bytes(rng.choice(b"ab") for _ in range(300))
    query = bytes(rng.choice(b"abc") for _ in range(200))
    sa = orc.sais(text)
    L = 4
    want = brute(text, query, L, sa=sa)
    raw = Raw(eng, device, text, sa)
    P = None
    for route in raw.routes():
        rc, p, z, out = raw.mems(route, query, L)
        assert rc == OK and z == len(want) and [tuple(int(a[k]) for a in out) for k in range(z)] == want, (route, rc, z, len(want))
        P = p if P is None else P
        assert p == P and P > z > 10
        rc, p0, z0, _ = raw.mems(route, query, L, cap=0)                       # counts only, output pointers NULL
        assert (rc, p0, z0) == (OK, P, z)
        rc, p1, z1, out = raw.mems(route, query, L, cap=z - 1)                 # (the guards stand behind the last written triple)
        assert (rc, p1, z1) == (OK, P, z) and [tuple(int(a[k]) for a in out) for k in range(z - 1)] == want[:-1]
        rc, p1, z1, out = raw.mems(route, query, L, cap=z + 5)
        assert (rc, p1, z1) == (OK, P, z) and all((a[z:] == UNWRITTEN).all() for a in out), "written past Z"
        rc, p2, z2, out = raw.mems(route, query, L, limit=P, cap=z)
        assert (rc, p2, z2) == (OK, P, z) and [tuple(int(a[k]) for a in out) for k in range(z)] == want
        rc, p3, z3, out = raw.mems(route, query, L, limit=P - 1, cap=z)        # refused: nothing between the guards is written
        assert (rc, p3, z3) == (OK, P, 0) and all((a == UNWRITTEN).all() for a in out), (route, rc, p3, z3)
        for flags in (0, UNIQUE):
            rc, p4, z4, out = raw.mems(route, query, L, flags=flags, ws_fill=0xFF, q_off=5, out_offs=(12, 4, 4))
            assert rc == OK and p4 == P and [tuple(int(a[k]) for a in out) for k in range(z4)] == brute(text, query, L, unique=bool(flags), sa=sa)
    raw.close()
    verify(eng, device, chk, text, sa, query, L, run(eng, device, "dev", text, sa, query, L), run(eng, device, "dev", text, sa, query, L, True))


# ---- 3. runs with closed-form answers --------------------------------------------------------------------------------------
def _factor(P):
    a = max(d for d in range(1, int(P ** 0.5) + 1) if P % d == 0)
    return a, P // a


def runs(eng, device, K, routes=("dev", "index_dev", "gindex_dev")):
    """T = a^n, Q = a^m: P = (n - L + 1)(m - L + 1) around the tile size K -- K - 1, K, K + 1, 3K + 1 pairs; one position
    whose interval spans more than three tiles; tiles of single-pair positions (more positions than threads when K is
    the product's); more than 2K positions without a pair in the middle of Q."""
    L = 3
    shapes = [_factor(P) for P in (K - 1, K, K + 1, 3 * K + 1)]               # (a, b): m - L + 1 = a positions of b ranks
    shapes += [(2, 3 * K + 1), (3 * K + 5, 1), (K + 3, 2)]
    k = 0
    for a, b in shapes:
        n, m = b + L - 1, a + L - 1
        text, query = b"a" * n, b"a" * m
        sa = np.arange(n - 1, -1, -1, dtype=np.uint32)
        for unique in (False, True):
            route = routes[k % len(routes)]
            k += 1
            got = run(eng, device, route, text, sa, query, L, unique)
            assert got[3] == a * b, (route, a, b, got[3])
            assert triples(got) == run_closed_form(n, m, L, unique), (route, K, a, b, unique, triples(got)[:8])
    # candidates, more than 2K positions without one, candidates again
    n, x, gap, y = K // 2 + L + 1, K // 4 + L, 2 * K + 5, K + L
    text, query = b"a" * n, b"a" * x + b"b" * gap + b"a" * y
    sa = np.arange(n - 1, -1, -1, dtype=np.uint32)
    for unique in (False, True):
        got = run(eng, device, routes[k % len(routes)], text, sa, query, L, unique)
        k += 1
        want = run_closed_form(n, x, L, unique) + run_closed_form(n, y, L, unique, shift=x + gap)
        assert got[3] == (n - L + 1) * (x - L + 1 + y - L + 1) and triples(got) == want, (K, unique, got[3], len(want), got[0].size)


# ---- 4. buffers, streams, threads ------------------------------------------------------------------------------------------
def buffers_and_streams(eng, device, chk, orc):
    """Offset and unaligned Q and T, a dirty workspace of exactly the stated size, guard bands around the outputs, a
    side stream, two threads on one index, and the three entry points giving identical bytes."""
    rng = random.Random(5)
    text = bytes(rng.choice(b"acgt") for _ in range(3000))
    sa = orc.sais(text)
    query = b"".join(text[a:a + rng.randint(1, 30)] + b"n" for a in (rng.randrange(3000) for _ in range(40)))
    L = 5
    full, uniq = (run(eng, device, "dev", text, sa, query, L, u) for u in (False, True))
    verify(eng, device, chk, text, sa, query, L, full, uniq)
    side = torch.cuda.Stream() if str(device).startswith("cuda") else None
    k = 0
    for text_off, u32_off, fill in _buffers.combos():
        raw = Raw(eng, device, text, sa, text_off=text_off, sa_off=u32_off)
        for route in raw.routes():
            for want in (full, uniq):
                k += 1
                with (torch.cuda.stream(side) if side is not None and k % 2 else contextlib.nullcontext()):
                    rc, p, z, out = raw.mems(route, query, L, flags=UNIQUE if want is uniq else 0, q_off=(1, 3, 5, 9)[k % 4],
                                             out_offs=(u32_off, 4, 12), fill=0xA5, ws_fill=fill, ws_off=0)
                assert rc == OK and p == full[3] and z == want[0].size, (route, rc, p, z)
                assert all(np.array_equal(out[j], want[j]) for j in range(3)), (route, text_off, u32_off, fill)
        raw.close()

    # two threads on one index at once (on the emulator: one after the other), equal bytes
    dt, dsa = _t(text, device), _t(sa, device, np.uint32)
    ix = sdev.DeviceIndex(dt, dsa, engine=eng)
    qs = [query, query[::-1]]
    exps = [full, run(eng, device, "dev", text, sa, qs[1], L)]
    results, errors = [None, None], []

    def worker(j):
        try:
            for _ in range(3):
                got = ix.mems(_t(qs[j], device), L)
                _sync(device)
                results[j] = [_host(x) for x in got[:3]] + [got[3]]
        except Exception as e:                                             # noqa: BLE001 (reported below)
            errors.append(e)
    threads = [threading.Thread(target=worker, args=(j,)) for j in range(2)]
    concurrent = str(device).startswith("cuda")      # (the emulator keeps threadIdx & co. in globals: one launch at a time)
    for th in threads:
        th.start()
        if not concurrent:
            th.join()
    for th in threads:
        th.join()
    assert not errors, errors
    for j in range(2):
        assert results[j][3] == exps[j][3] and all(np.array_equal(results[j][c], exps[j][c]) for c in range(3)), j
    _sync(device)
    ix.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def workspace_bound(eng):
    """Hook-free: sfx_mems_workspace_bytes(m, limit) <= 24 m + limit / 4 + 64 KiB, and 0 where nothing can run."""
    f = eng.lib.sfx_mems_workspace_bytes
    for m in (1, 2, 255, 256, 4097, 1 << 18, 1 << 24, (1 << 32) - 1):
        for limit in (1, 2047, 2048, 2049, 1 << 20, (1 << 28) + 1, 1 << 30, 1 << 33, 1 << 40, (1 << 64) - 1):
            got = int(f(m, limit))
            assert 0 < got <= 24 * m + min(limit, m * 0xFFFFFFFF) // 4 + (64 << 10), (m, limit, got)
    assert f(0, 100) == 0 and f(1 << 32, 100) == 0 and f(100, 0) == 0


def refusals(eng, device, orc):
    text, query = b"abracadabra" * 20, b"cadabraabr" * 10
    sa = orc.sais(text)
    raw = Raw(eng, device, text, sa)
    m, L = len(query), 3
    q = _buffers.text_in(query, device, 1)
    wsb = int(eng.lib.sfx_mems_workspace_bytes(m, 1 << 20))
    ws = _buffers.guarded(wsb, device, 0, 0xA5)
    bufs = [_buffers.guarded(4 * 4096, device, 4, 0xA5) for _ in range(3)]
    o = [b.ptr for b in bufs]
    st = _buffers.stream_of(device)
    for route in raw.routes():
        c = lambda **kw: raw.call(route, kw.get("q", q.ptr), kw.get("m", m), kw.get("L", L), kw.get("flags", 0), kw.get("limit", 1 << 20),
                                  kw.get("outs", o), kw.get("cap", 4096), kw.get("ws", ws.ptr), kw.get("wsb", wsb), st)
        good = c()
        assert good[0] == OK and good[1] > good[2] > 0, (route, good)
        ws.fill(0xA5)
        for b in bufs:
            b.fill(0xA5)
        assert c(L=0)[0] == ERR_ARG, route
        assert c(limit=0)[0] == ERR_ARG, route
        assert c(flags=2)[0] == ERR_ARG and c(flags=0x80000001)[0] == ERR_ARG, route
        for j in range(3):
            assert c(outs=[None if k == j else o[k] for k in range(3)])[0] == ERR_ARG, (route, j)
        assert c(q=None)[0] == ERR_ARG, route
        assert c(m=1 << 32)[0] == ERR_TOO_LARGE, route
        assert c(ws=None)[0] == ERR_WORKSPACE and c(wsb=wsb - 1)[0] == ERR_WORKSPACE and c(wsb=0)[0] == ERR_WORKSPACE, route
        assert c(ws=ctypes.c_void_p(ws.ptr.value + 8), wsb=wsb)[0] == ERR_ARG, route         # large enough, off the boundary
        assert c(outs=[ctypes.c_void_p(o[0].value + 2), o[1], o[2]])[0] == ERR_ARG, route    # a u32 array off 4 bytes
        # nothing to do: SFX_OK, P = Z = 0, whatever the other pointers are
        assert c(m=0, q=None) == (OK, 0, 0) and c(L=m + 1) == (OK, 0, 0) and c(L=len(text) + 1) == (OK, 0, 0), route
        assert c(cap=0, outs=[None, None, None]) == good, route
    lib = eng.lib
    none2 = (ctypes.byref(_u64(0)), ctypes.byref(_u64(0)))
    assert lib.sfx_mems_dev(raw.t.ptr, 1 << 32, raw.s.ptr, q.ptr, m, L, 0, 1, None, None, None, 0, *none2, ws.ptr, wsb, st) == ERR_TOO_LARGE
    assert lib.sfx_mems_dev(raw.t.ptr, 0, raw.s.ptr, q.ptr, m, L, 0, 1, None, None, None, 0, *none2, None, 0, st) == OK       # n == 0
    assert lib.sfx_mems_dev(None, len(text), raw.s.ptr, q.ptr, m, L, 0, 1 << 20, None, None, None, 0, *none2, ws.ptr, wsb, st) == ERR_ARG
    assert lib.sfx_mems_dev(raw.t.ptr, len(text), None, q.ptr, m, L, 0, 1 << 20, None, None, None, 0, *none2, ws.ptr, wsb, st) == ERR_ARG
    assert lib.sfx_mems_dev(raw.t.ptr, len(text), raw.s.ptr, q.ptr, m, L, 0, 1 << 20, None, None, None, 0, None, none2[1], ws.ptr, wsb, st) == ERR_ARG
    assert lib.sfx_mems_dev(raw.t.ptr, len(text), raw.s.ptr, q.ptr, m, L, 0, 1 << 20, None, None, None, 0, none2[0], None, ws.ptr, wsb, st) == ERR_ARG
    for fn in (lib.sfx_index_mems_dev, lib.sfx_gindex_mems_dev):
        assert fn(None, q.ptr, m, L, 0, 1 << 20, None, None, None, 0, *none2, ws.ptr, wsb, st) == ERR_ARG
    hq = _np(query, np.uint8)
    for fn, h in ((lib.sfx_index_mems, raw.ix._h), (lib.sfx_gindex_mems, raw.gx._h)):
        assert fn(None, _gsa.ptr(hq), m, L, 0, 1 << 20, None, None, None, 0, *none2) == ERR_ARG
        assert fn(h, _gsa.ptr(hq), m, 0, 0, 1 << 20, None, None, None, 0, *none2) == ERR_ARG
        assert fn(h, _gsa.ptr(hq), m, L, 0, 0, None, None, None, 0, *none2) == ERR_ARG
        assert fn(h, _gsa.ptr(hq), m, L, 4, 1 << 20, None, None, None, 0, *none2) == ERR_ARG
        assert fn(h, _gsa.ptr(hq), m, L, 0, 1 << 20, None, None, None, 7, *none2) == ERR_ARG
        assert fn(h, None, m, L, 0, 1 << 20, None, None, None, 0, *none2) == ERR_ARG
        assert fn(h, _gsa.ptr(hq), 1 << 32, L, 0, 1 << 20, None, None, None, 0, *none2) == ERR_TOO_LARGE
        assert fn(h, _gsa.ptr(hq), m, L, 0, 1 << 20, None, None, None, 0, *none2) == OK
    for b in bufs:
        assert (b.host() == 0xA5).all(), "a refused call wrote"
        b.check_guards("refused")
    ws.check_guards("workspace")
    raw.close()


def launch_names(eng, device, orc):
    text, query = b"abracadabra" * 30, b"cadabraabr" * 12
    sa = orc.sais(text)
    for route, search in (("dev", "ms_search"), ("index_dev", "ms_search_dir"), ("gindex_dev", "ms_gsa_search")):
        names = _gsa.profile_names(eng, lambda: run(eng, device, route, text, sa, query, 6))
        assert KERNELS <= names and search in names, (route, sorted(names))
        assert not {n for n in names if n.startswith("mem_")} - KERNELS, sorted(names)


# ---- scale (test_gpu_mem.py, scripts/gpu_mem_time.py restates it) ------------------------------------------------------------
def mixture(text, other, noise, rng, qm, starts=None):
    """qm query bytes: half of them 4096-byte slices of the text with about every 200th byte replaced (with `starts`:
    every fourth slice laid across a document end), a quarter unrelated text of the same kind, a quarter noise."""
    t = np.frombuffer(text, dtype=np.uint8)
    parts, piece = [], 4096
    for k in range(qm // 2 // piece):
        a = rng.randrange(len(text) - piece)
        if starts is not None and k % 4 == 0:
            a = max(0, int(starts[rng.randrange(1, len(starts))]) - rng.randint(1, piece - 1))
        parts.append(t[a:a + piece].copy())
    half = np.concatenate(parts)
    flip = np.flatnonzero(np.random.default_rng(rng.randrange(1 << 30)).random(half.size) < 1 / 200)
    half[flip] = other[flip % other.size]
    q = np.concatenate([half, other[:qm // 4], noise[:qm // 4]])
    assert q.size == qm
    return q


def cut(text, rng, lo, hi):
    """Document starts every lo .. hi bytes, now and then an empty document."""
    starts, p = [0], 0
    while True:
        p += rng.randint(lo, hi)
        if p >= len(text):
            break
        starts.append(p)
        if rng.random() < 0.01:
            starts.append(p)
    return np.array(starts, dtype=np.int64)
