"""The cases of the LCE index (sfx_inverse_table_*, sfx_lce_*), shared by test_lce_emu.py (the
emulator build, host memory) and test_gpu_lce.py (libsuffix_hip.so, HBM).

Nothing expected comes from the engine.  The known answer is `brute`: plain byte comparison with a mismatch budget and
the document ends; larger inputs go through the serial checker tests/lce_check.c, which reads the text, doc_starts, the
pairs, k and the reported lengths only.  The tables handed to the engine are the oracle's (`oracle.sais` with its LCP)
and, for collections, the definition (`GeneralizedSuffixTable.new_naive`), so a wrong SA build can neither mask nor
cause a failure."""
import contextlib
import ctypes
import os
import random
import subprocess
import threading

import numpy as np
import torch

import _buffers
import _gen
import _gsa
from suffix_amd import GeneralizedSuffixTable, SuffixHipError, SuffixTable
from suffix_amd import device as sdev

OK, ERR_ARG, ERR_TOO_LARGE, ERR_WORKSPACE = 0, 1, 2, 5
NONE = 0xFFFFFFFF
KERNELS = {"lce_check", "lce_scatter", "lce_verify", "lce_levels", "lce_query", "lce_range_min", "lce_ranks"}
KS = (0, 1, 2, 7)
LEVEL_EDGES = (0, 1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 1057, 32767, 32768, 32769, 33825)
HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
CSRC_FROM_EMU = "../../suffix_amd/csrc"                                  # tests/emu/Makefile's CSRC
_vp, _u64, _u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32


def build_emulator():
    """`make -C tests/emu`; sfx_lce.hip is compiled as part of sfx_api.hip's translation unit and tests/emu/Makefile does
    not name it, so when it is newer than the library sfx_api.hip is declared new (`make -W`).  -> the library's path."""
    lib = os.path.join(EMU_DIR, "libsuffix_emu.so")
    cmd = ["make", "-s", "-j8", "-C", EMU_DIR]
    src = os.path.join(HERE, os.pardir, "suffix_amd", "csrc", "sfx_lce.hip")
    if os.path.exists(lib) and os.path.getmtime(src) > os.path.getmtime(lib):
        cmd += ["-W", CSRC_FROM_EMU + "/sfx_api.hip"]
    subprocess.check_call(cmd)
    return lib


def _sync(device):
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()


def _u32a(x):
    return np.ascontiguousarray(x, dtype=np.uint32)


# ---- the known answer ----------------------------------------------------------------------------------------------------
def end_of(p, n, starts):
    if starts is None:
        return n
    d = int(np.searchsorted(np.asarray(starts, dtype=np.int64), p, side="right")) - 1
    return int(starts[d + 1]) if d + 1 < len(starts) else n


def brute(text, i, j, k=0, starts=None):
    """LCE_k(i, j) by comparing bytes: the place of the (k + 1)-th difference, or the room to the nearer end."""
    n = len(text)
    if i > n or j > n:
        return NONE
    if i == n or j == n:
        return 0
    room = min(end_of(i, n, starts) - i, end_of(j, n, starts) - j)
    if i == j:
        return room
    t = np.frombuffer(text, dtype=np.uint8)
    diff = np.flatnonzero(t[i:i + room] != t[j:j + room])
    return int(diff[k]) if diff.size > k else room


def hand_worked():
    """(text, i, j, k, expected)"""
    return [(b"banana", 1, 3, 0, 3), (b"banana", 0, 0, 0, 6), (b"banana", 1, 3, 1, 3), (b"banana", 0, 2, 0, 0), (b"banana", 0, 2, 1, 4),
            (b"banana", 0, 2, 7, 4), (b"banana", 6, 0, 0, 0), (b"banana", 7, 0, 3, NONE), (b"abcabd", 0, 3, 0, 2), (b"abcabd", 0, 3, 1, 3),
            (b"abcabd", 3, 0, 1, 3), (b"abcabd", 1, 4, 0, 1), (b"abcabd", 5, 5, 9, 1), (b"aXbYc", 0, 2, 2, 2)]


def tables(orc, text):
    sa = orc.sais(text)
    lcp = orc.lcp_kasai(text, sa) if len(text) > 3000 else orc.lcp_quadratic(text, sa)
    return _u32a(sa), _u32a(lcp)


def collection_tables(docs):
    """-> (text, sa, lcp, starts uint64) by the definition."""
    g = GeneralizedSuffixTable.new_naive(docs)
    return b"".join(docs), _u32a(g.table()), _u32a(g.lcp_lens()), _gsa.doc_starts(docs).astype(np.uint64)


# ---- the checker -----------------------------------------------------------------------------------------------------------
def build_checker(out_dir):
    so = os.path.join(str(out_dir), "liblce_check.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "lce_check.c")])
    lib = ctypes.CDLL(so)
    i64p = ctypes.POINTER(ctypes.c_int64)
    lib.lce_check.restype = ctypes.c_int
    lib.lce_check.argtypes = [_vp, _u64, _vp, _u64, _vp, _vp, _u64, _u32, _vp, i64p]
    lib.lce_check_min.restype = ctypes.c_int
    lib.lce_check_min.argtypes = [_vp, _u64, _vp, _vp, _u64, _vp, i64p]
    lib.lce_check_isa.restype = ctypes.c_int
    lib.lce_check_isa.argtypes = [_vp, _vp, _u64, i64p]
    lib.lce_check_name.restype = ctypes.c_char_p
    lib.lce_check_name.argtypes = [ctypes.c_int]
    return lib


def check_pairs(chk, text, starts, a, b, k, got):
    """-> (verdict, index of the first wrong pair or -1)"""
    t = np.frombuffer(text, dtype=np.uint8)
    a, b, got = _u32a(a), _u32a(b), _u32a(got)
    assert a.size == b.size == got.size
    st = None if starts is None else np.ascontiguousarray(starts, dtype=np.uint64)
    where = ctypes.c_int64(-2)
    rc = chk.lce_check(_gsa.ptr(t), t.size, _gsa.ptr(st) if st is not None else None, 0 if st is None else st.size, _gsa.ptr(a), _gsa.ptr(b),
                       a.size, int(k), _gsa.ptr(got), ctypes.byref(where))
    return chk.lce_check_name(rc).decode(), int(where.value)


def accept_pairs(chk, text, starts, a, b, k, got):
    name, where = check_pairs(chk, text, starts, a, b, k, got)
    if name != "ok":
        raise AssertionError(f"lce_check: {name} at pair {where}: ({int(a[where])}, {int(b[where])}) k = {k}, reported {int(got[where])}, "
                             f"n = {len(text)}")


def accept_min(chk, lcp, lo, hi, got):
    lcp, lo, hi, got = _u32a(lcp), _u32a(lo), _u32a(hi), _u32a(got)
    where = ctypes.c_int64(-2)
    rc = chk.lce_check_min(_gsa.ptr(lcp), lcp.size, _gsa.ptr(lo), _gsa.ptr(hi), lo.size, _gsa.ptr(got), ctypes.byref(where))
    w = int(where.value)
    assert rc == 0, f"lce_check_min: {chk.lce_check_name(rc).decode()} at range {w}: [{int(lo[w])}, {int(hi[w])}) reported {int(got[w])}"


def accept_isa(chk, sa, isa):
    sa, isa = _u32a(sa), _u32a(isa)
    assert sa.size == isa.size
    where = ctypes.c_int64(-2)
    rc = chk.lce_check_isa(_gsa.ptr(sa), _gsa.ptr(isa), sa.size, ctypes.byref(where))
    assert rc == 0, f"lce_check_isa: {chk.lce_check_name(rc).decode()} at position {int(where.value)}"


def checker_self_test(chk):
    """One fault per mode, each named; and the faultless lists pass."""
    text = b"abcabdabcabd__abcabe"
    a, b = _u32a([0, 3, 0, 14, 20, 21, 5, 6]), _u32a([3, 0, 6, 0, 1, 1, 5, 12])
    for k in (0, 1, 3):
        good = _u32a([brute(text, int(i), int(j), k) for i, j in zip(a, b)])
        assert check_pairs(chk, text, None, a, b, k, good) == ("ok", -1)
        for q, delta, name in ((0, -1, "the extension goes on"), (1, 1, "more mismatches than allowed"), (2, 40, "past an end"),
                               (4, 1, "wrong mark for a position >= n"), (5, -1, "wrong mark for a position >= n"), (6, -1, "the extension goes on")):
            bad = good.copy()
            bad[q] = (int(bad[q]) + delta) & NONE
            if name == "more mismatches than allowed" and int(bad[q]) > min(len(text) - int(a[q]), len(text) - int(b[q])):
                continue
            assert check_pairs(chk, text, None, a, b, k, bad) == (name, q), (k, q, check_pairs(chk, text, None, a, b, k, bad))
    # document ends: the same bytes as two documents of 6 (and an empty one)
    starts = np.array([0, 6, 6, 12], dtype=np.uint64)
    good = _u32a([brute(text, 0, 6, 0, starts), brute(text, 1, 15, 2, starts)])
    assert good.tolist() == [6, 5]
    assert check_pairs(chk, text, starts, [0, 1], [6, 15], 0, [6, brute(text, 1, 15, 0, starts)]) == ("ok", -1)
    assert check_pairs(chk, text, starts, [0], [6], 0, [7]) == ("past an end", 0)
    assert check_pairs(chk, text, None, [0], [6], 0, [6]) == ("ok", -1)                 # (the plain text: abcabd twice, then 'a' against '_')
    lcp = _u32a([0, 5, 3, 9, 1, 7])
    with contextlib.suppress(AssertionError):
        accept_min(chk, lcp, [1], [4], [5])
        raise RuntimeError("lce_check_min accepted a wrong minimum")
    accept_min(chk, lcp, [1, 3, 2, 0, 5], [4, 3, 1, 7, 6], [3, NONE, NONE, NONE, 7])
    sa = _u32a([2, 0, 3, 1])
    accept_isa(chk, sa, [1, 3, 0, 2])
    with contextlib.suppress(AssertionError):
        accept_isa(chk, sa, [1, 3, 0, 1])
        raise RuntimeError("lce_check_isa accepted a wrong table")


# ---- the raw ABI over guarded buffers ----------------------------------------------------------------------------------------
class Lx:
    """sfx_lce_create[_dev] over arrays between guard bands: sa at +sa_off, lcp at +lcp_off behind a 256-byte boundary
    (4 / 8 / 12: level 0 is then read word by word).  The handle's queries write outputs between guard bands of their own."""

    def __init__(self, eng, device, sa, lcp, starts=None, host=False, sa_off=4, lcp_off=0, ndocs=None):
        self.eng, self.device, self.host = eng, device, host
        sa, lcp = _u32a(sa), _u32a(lcp)
        self.n = int(sa.size)
        st = None if starts is None else np.ascontiguousarray(starts, dtype=np.uint64)
        nd = (0 if st is None else int(st.size)) if ndocs is None else ndocs
        h = ctypes.c_void_p()
        if host:
            self.rc = eng.lib.sfx_lce_create(_gsa.ptr(sa), _gsa.ptr(lcp), self.n, _gsa.ptr(st) if st is not None else None, nd, ctypes.byref(h))
        else:
            self.bufs = {"sa": _buffers.inp(sa, device, sa_off), "lcp": _buffers.inp(lcp, device, lcp_off)}   # lcp is borrowed: kept
            if st is not None:
                self.bufs["starts"] = _buffers.inp(st, device, 8)
            self.rc = eng.lib.sfx_lce_create_dev(self.bufs["sa"].ptr, self.bufs["lcp"].ptr, self.n,
                                                 self.bufs["starts"].ptr if st is not None else None, nd, _buffers.stream_of(device),
                                                 ctypes.byref(h))
            _buffers.check_all(self.bufs)
            if self.rc == OK:
                self.bufs.pop("sa").fill(0xA5)                       # the table is free again after creation
        self.h = h if self.rc == OK else None
        assert (self.rc == OK) == bool(h), (self.rc, h)

    def _call(self, name, ins, out_off, *extra):
        nq = int(ins[0].size)
        fn = getattr(self.eng.lib, name + ("" if self.host else "_dev"))
        if self.host:
            out = np.full(nq, 0xDEADBEEF, dtype=np.uint32)
            rc = fn(self.h, *[_gsa.ptr(x) for x in ins], nq, *extra, _gsa.ptr(out))
            return rc, out
        b = {f"in{k}": _buffers.inp(x, self.device, (4, 12, 8)[(k + out_off // 4) % 3]) for k, x in enumerate(ins)}
        b["out"] = _buffers.guarded(4 * nq, self.device, out_off, "count")
        rc = fn(self.h, *[b[f"in{k}"].ptr for k in range(len(ins))], nq, *extra, b["out"].ptr, _buffers.stream_of(self.device))
        _buffers.check_all(b)
        _buffers.check_all(getattr(self, "bufs", {}))
        return rc, b["out"].host(np.uint32)

    def lce(self, a, b, k=0, out_off=8):
        rc, out = self._call("sfx_lce_query", [_u32a(a), _u32a(b)], out_off, int(k))
        assert rc == OK, rc
        return out

    def range_min(self, lo, hi, out_off=4):
        rc, out = self._call("sfx_lce_range_min", [_u32a(lo), _u32a(hi)], out_off)
        assert rc == OK, rc
        return out

    def ranks(self, pos, out_off=12):
        rc, out = self._call("sfx_lce_ranks", [_u32a(pos)], out_off)
        assert rc == OK, rc
        return out

    def close(self):
        _sync(self.device)
        h, self.h = self.h, None
        if h:
            self.eng.lib.sfx_lce_destroy(h)


def inverse_table_raw(eng, device, sa, sa_off=4, out_off=8, fill=0xFF, ws_bytes=None, ws_off=0):
    sa = _u32a(sa)
    n = int(sa.size)
    need = int(eng.lib.sfx_inverse_table_workspace_bytes(n))
    b = {"sa": _buffers.inp(sa, device, sa_off), "isa": _buffers.guarded(4 * n, device, out_off, _buffers.out_fill(fill)),
         "workspace": _buffers.guarded(need if ws_bytes is None else ws_bytes, device, ws_off, fill)}
    rc = eng.lib.sfx_inverse_table_dev(b["sa"].ptr, n, b["isa"].ptr, b["workspace"].ptr, b["workspace"].nbytes, _buffers.stream_of(device))
    _buffers.check_all(b)
    return rc, b["isa"].host(np.uint32)


def expected_isa(sa):
    isa = np.zeros(len(sa), dtype=np.uint32)
    isa[np.asarray(sa, dtype=np.int64)] = np.arange(len(sa), dtype=np.uint32)
    return isa


def special_positions(n):
    return [p for p in (0, 1, n // 2, n - 2, n - 1, n, n + 1, n + 5) if 0 <= p <= NONE]


def pair_list(n, rng, limit=500):
    """All pairs of positions 0 .. n where there are at most `limit`, else that many random ones; then the specials."""
    if (n + 1) * (n + 1) <= limit:
        pairs = [(i, j) for i in range(n + 1) for j in range(n + 1)]
    else:
        pairs = [(rng.randrange(n), rng.randrange(n)) for _ in range(limit)]
    sp = special_positions(n)
    pairs += [(p, p) for p in sp] + [(sp[k], sp[-1 - k]) for k in range(len(sp))] + [(p, rng.randrange(n + 1)) for p in sp]
    return _u32a([p[0] for p in pairs]), _u32a([p[1] for p in pairs])


def check_text(eng, device, text, sa, lcp, starts=None, ks=KS, rng=None, host=False, lcp_off=0, limit=500, closed_form=None, chk=None):
    """One handle over (sa, lcp[, starts]); every k over pair_list against `brute` (or the closed form / the checker);
    the ranks and the inverse table against the definition."""
    rng = rng or random.Random(len(text))
    n = len(text)
    lx = Lx(eng, device, sa, lcp, starts, host=host, lcp_off=lcp_off)
    assert lx.rc == OK, (lx.rc, n)
    try:
        a, b = pair_list(n, rng, limit)
        for k in ks:
            got = lx.lce(a, b, k, out_off=(4, 8, 12)[k % 3])
            if chk is not None:
                accept_pairs(chk, text, starts, a, b, k, got)
            if closed_form is not None:
                exp = _u32a([closed_form(int(i), int(j), k) for i, j in zip(a, b)])
            elif chk is None:
                exp = _u32a([brute(text, int(i), int(j), k, starts) for i, j in zip(a, b)])
            else:
                continue
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, (n, k, host, [(int(a[q]), int(b[q]), int(got[q]), int(exp[q])) for q in bad[:4]], text[:40], starts)
        pos = _u32a(special_positions(n) + [rng.randrange(n + 1) for _ in range(50)])
        exp_isa = expected_isa(sa)
        want = np.where(pos < n, exp_isa[np.minimum(pos, max(n, 1) - 1)] if n else NONE, NONE).astype(np.uint32)
        assert np.array_equal(lx.ranks(pos), want), (n, host)
    finally:
        lx.close()
    return a.size * len(ks)


# ---- 1. known answers ------------------------------------------------------------------------------------------------------
def known_answers(eng, device, orc):
    for text, i, j, k, exp in hand_worked():
        assert brute(text, i, j, k) == exp, (text, i, j, k, brute(text, i, j, k))
        sa, lcp = tables(orc, text)
        for host in (False, True):
            lx = Lx(eng, device, sa, lcp, host=host)
            assert lx.rc == OK and lx.lce([i], [j], k).tolist() == [exp], (text, i, j, k, host)
            lx.close()
        one, ai, bj = np.full(1, 0xDEADBEEF, dtype=np.uint32), _u32a([i]), _u32a([j])
        assert eng.lib.sfx_lce_u32(_gsa.ptr(sa), _gsa.ptr(lcp), len(text), None, 0, _gsa.ptr(ai), _gsa.ptr(bj), 1, k, _gsa.ptr(one)) == OK
        assert int(one[0]) == exp, (text, i, j, k)
    # the public classes (their own LCP array and lazily made handle)
    st = SuffixTable.from_parts(b"banana", orc.sais(b"banana"), engine=eng)
    assert (st.lce(1, 3), st.lce(0, 0), st.lce(1, 3, mismatches=1), st.lce(0, 2, 7)) == (3, 6, 3, 4)
    assert st.lce_batch([1, 6, 7], [3, 0, 0]).tolist() == [3, 0, NONE]
    assert st.inverse_table().tolist() == expected_isa(orc.sais(b"banana")).tolist()
    lcp = orc.lcp_quadratic(b"banana", orc.sais(b"banana"))
    assert st.lcp_range_min(1, 4) == int(lcp[1:4].min()) and st.lcp_range_min(3, 3) == NONE and st.lcp_range_min(0, 7) == NONE
    assert st.lcp_range_min_batch([0, 2], [6, 3]).tolist() == [int(lcp.min()), int(lcp[2])]
    st2 = SuffixTable.from_parts(b"abcabd", orc.sais(b"abcabd"), engine=eng)
    assert (st2.lce(0, 3), st2.lce(0, 3, 1)) == (2, 3)
    with contextlib.suppress(ValueError):
        st2.lce_batch([0, 1], [2])
        raise AssertionError("lce_batch took lists of different lengths")
    bad = SuffixTable.from_parts(b"abcabd", np.array([0, 1, 2, 3, 4, 4], dtype=np.uint32), engine=eng)
    with contextlib.suppress(SuffixHipError):
        bad.inverse_table()
        raise AssertionError("inverse_table took a table that is no permutation")
    empty = SuffixTable.from_parts(b"", np.zeros(0, dtype=np.uint32), engine=eng)
    assert empty.inverse_table().size == 0 and empty.lce_batch([0, 1], [0, 0]).tolist() == [0, NONE]
    docs = [b"abcab", b"", b"cabx", b"b"]
    g = GeneralizedSuffixTable.new_naive(docs, engine=eng)
    assert g.lce((0, 0), (0, 3)) == 2 and g.lce((0, 2), (2, 0)) == 3 and g.lce((0, 2), (2, 0), 1) == 3 and g.lce((0, 1), (3, 0), 5) == 1
    assert g.lce((2, 0), (2, 0), 2) == 4
    text = b"".join(docs)
    a, b = np.arange(len(text) + 2, dtype=np.uint32), np.full(len(text) + 2, 7, dtype=np.uint32)
    for k in (0, 2):
        assert g.lce_batch(a, b, k).tolist() == [brute(text, int(i), 7, k, g.doc_starts()) for i in a], k
    with contextlib.suppress(IndexError):
        g.lce((1, 0), (0, 0))
        raise AssertionError("a position inside an empty document")
    # the torch-tensor classes
    sa, lcp = tables(orc, b"mississippi")
    dsa, dlcp = (torch.from_numpy(x.view(np.int32).copy()).to(device) for x in (sa, lcp))
    isa = sdev.inverse_table(dsa, engine=eng)
    _sync(device)
    assert np.array_equal(isa.cpu().numpy().view(np.uint32), expected_isa(sa))
    ix = sdev.LceDeviceIndex(dsa, dlcp, engine=eng)
    assert 4 * 11 <= ix.nbytes <= 4 * 11 + 11 // 7 + (64 << 10)
    t = lambda xs: torch.tensor(xs, dtype=torch.int64).to(torch.int32).to(device)
    got = ix.lce(t([1, 1, 11]), t([4, 4, 2]), mismatches=0)
    got1 = ix.lce(t([1, 1]), t([4, 7]), mismatches=1)
    rm = ix.range_min(t([0, 3]), t([11, 3]))
    rk = ix.rank_of(t([0, 10, 11]))
    _sync(device)
    assert got.cpu().numpy().view(np.uint32).tolist() == [4, 4, 0]
    assert got1.cpu().numpy().view(np.uint32).tolist() == [brute(b"mississippi", 1, 4, 1), brute(b"mississippi", 1, 7, 1)]
    assert rm.cpu().numpy().view(np.uint32).tolist() == [int(lcp.min()), NONE]
    assert rk.cpu().numpy().view(np.uint32).tolist() == [int(expected_isa(sa)[0]), int(expected_isa(sa)[10]), NONE]
    ix.close()


def handle_is_made_once(eng, orc):
    """SuffixTable's lazily made handle: the first lce() builds the LCP array and the index, every later call -- lce,
    lce_batch, lcp_range_min -- launches the query kernel and nothing else."""
    text = _gen.english_like(5000).tobytes()
    st = SuffixTable.from_parts(text, orc.sais(text), engine=eng)
    first = _gsa.profile_names(eng, lambda: st.lce(3, 700))
    assert {"lce_check", "lce_scatter", "lce_verify", "lce_levels", "lce_query"} <= first, sorted(first)
    assert first - KERNELS, ("the first call builds the LCP array", sorted(first))
    for call, kernel in ((lambda: st.lce(3, 700, 2), "lce_query"), (lambda: st.lce_batch([1, 2], [9, 4000]), "lce_query"),
                         (lambda: st.lcp_range_min(10, 4000), "lce_range_min"), (lambda: st.lcp_range_min_batch([0], [5000]), "lce_range_min")):
        names = _gsa.profile_names(eng, call)
        assert names == {kernel}, sorted(names)
    docs = [text[:1500], b"", text[1500:1510], text[700:2900]]
    g = GeneralizedSuffixTable.new_naive(docs, engine=eng)
    g.lce((0, 3), (3, 40))
    assert _gsa.profile_names(eng, lambda: g.lce((0, 5), (3, 800), 1)) == {"lce_query"}


# ---- 2. random small texts and collections ---------------------------------------------------------------------------------
def small_random(eng, device, orc, count=152, seed=21):
    rng = random.Random(seed)
    done = 0
    for t in range(count):
        sigma = (1, 2, 4, 256)[t % 4]
        n = rng.choice((1, 2, 3, 5, 17, 22, 33, 64, 65, 100, 300)) if t % 3 else rng.randint(1, 300)
        text = bytes(rng.randrange(sigma) + (97 if sigma <= 4 else 0) for _ in range(n))
        sa, lcp = tables(orc, text)
        done += bool(check_text(eng, device, text, sa, lcp, rng=rng, host=t % 5 == 2, lcp_off=(0, 4, 8, 12)[t % 4]))
        if t % 8 == 0:
            rc, isa = inverse_table_raw(eng, device, sa, sa_off=(4, 8, 12)[t % 3], out_off=(8, 12, 4)[t % 3], fill=_buffers.FILLS[t % 3])
            assert rc == OK and np.array_equal(isa, expected_isa(sa)), (rc, n)
    return done


def small_collections(eng, device, count=64, seed=22):
    rng = random.Random(seed)
    done = 0
    while done < count:
        docs = _gsa.random_collection(rng, max_docs=12, max_len=20)
        if done % 3 == 0:                                                # empty and one-byte documents, in front and behind too
            docs = [b""] + docs[:4] + [b"a", b""] + docs[4:] + [b"b", b""]
        if not sum(len(d) for d in docs):
            continue
        text, sa, lcp, starts = collection_tables(docs)
        check_text(eng, device, text, sa, lcp, starts, rng=rng, host=done % 4 == 1, lcp_off=(0, 4)[done % 2], limit=300)
        done += 1
    return done


# ---- 3. sizes at the level edges: create / range_min over synthetic arrays -----------------------------------------------------
def edge_ranges(n, rng, fan=32, extra=120):
    """Ranges that start or end on node boundaries, of length 1, the whole array, empty ones, hi = n and hi = n + 1."""
    r = [(0, n), (0, n + 1), (n, n), (n, n + 1), (0, 0), (5, 3), (n - 1, n), (0, 1)]
    edges = sorted({e for f in (fan, fan * fan, fan ** 3) for e in range(0, n + 1, f) if e % f == 0 and (e // f < 6 or e + 6 * f > n)})
    for e in edges:
        for lo, hi in ((e, n), (0, e), (e, e + 1), (e - 1, e), (e - 1, e + 1), (e, e + fan), (e + 1, e + fan), (e, e + fan + 1), (e + 1, e + 2 * fan - 1)):
            r.append((lo, hi))
    for _ in range(extra):
        lo = rng.randrange(n + 1)
        r.append((lo, rng.randint(lo, n) if rng.random() < 0.7 else min(n, lo + rng.randrange(70))))
    r = [(max(lo, 0), hi) for lo, hi in r if hi >= 0]
    return _u32a([x[0] for x in r]), _u32a([x[1] for x in r])


def expected_min(lcp, lo, hi):
    n = len(lcp)
    return _u32a([int(lcp[l:h].min()) if l < h <= n else NONE for l, h in zip(lo.tolist(), hi.tolist())])


def level_edges(eng, device, sizes=LEVEL_EDGES, seed=23):
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    for t, n in enumerate(sizes):
        sa = nrng.permutation(n).astype(np.uint32)
        # a landscape with deep and shallow stretches, so that minima come from every level
        lcp = (nrng.integers(0, 1 << 20, n) >> nrng.integers(0, 20, n)).astype(np.uint32) + np.uint32(3)
        if n:
            lcp[nrng.integers(0, n, 1 + n // 50)] = nrng.integers(0, 3, 1 + n // 50)
        for host, lcp_off in ((False, (0, 4, 8, 12)[t % 4]), (True, 0)) if n < 2000 or t % 2 else ((False, (0, 4)[t % 2]),):
            lx = Lx(eng, device, sa, lcp, host=host, lcp_off=lcp_off)
            assert lx.rc == OK, (lx.rc, n)
            lo, hi = edge_ranges(n, rng)
            got = lx.range_min(lo, hi)
            exp = expected_min(lcp, lo, hi)
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, (n, host, lcp_off, [(int(lo[q]), int(hi[q]), int(got[q]), int(exp[q])) for q in bad[:4]])
            pos = _u32a([0, n // 2, max(n, 1) - 1, n, n + 1])
            assert np.array_equal(lx.ranks(pos), np.where(pos < n, expected_isa(sa)[np.minimum(pos, max(n, 1) - 1)] if n else NONE, NONE))
            assert lx.lce([0, n, n + 1], [0, 0, n], 3).tolist() == [n, 0, NONE]
            lx.close()


# ---- 4. edge texts -----------------------------------------------------------------------------------------------------------
def fibonacci(n):
    k = 2
    while len(_gen.fibonacci_string(k)) < n:
        k += 1
    return bytes(_gen.fibonacci_string(k)[:n])


def edge_texts(eng, device, orc, n=1500, limit=400):
    rng = random.Random(24)
    run = b"a" * n
    sa, lcp = tables(orc, run)
    for host in (False, True):
        check_text(eng, device, run, sa, lcp, rng=rng, host=host, limit=limit,
                   closed_form=lambda i, j, k: NONE if max(i, j) > n else n - max(i, j))
    half = bytes(rng.randrange(256) for _ in range(40))
    crossing = bytes(_gen.uniform_bytes(n // 2 - 20, 200, 5, base=0)) + half + bytes(_gen.uniform_bytes(n // 2 - 60, 55, 6, base=200)) + half
    for text in (fibonacci(n), b"ab" * (n // 2), b"ab" * (n // 2) + b"a", crossing):
        sa, lcp = tables(orc, text)
        check_text(eng, device, text, sa, lcp, rng=rng, limit=limit, lcp_off=4)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def refusals(eng, device, orc):
    text = _gen.dna(700, seed=9).tobytes()
    n = len(text)
    sa, lcp = tables(orc, text)
    lib, st = eng.lib, _buffers.stream_of(device)
    for host in (False, True):
        over, twice = sa.copy(), sa.copy()
        over[n // 3] = n
        twice[5] = twice[n - 2]
        for bad_sa in (over, twice, np.full(n, NONE, dtype=np.uint32), np.zeros(n, dtype=np.uint32)):
            assert Lx(eng, device, bad_sa, lcp, host=host).rc == ERR_ARG
            if not host:
                rc, _ = inverse_table_raw(eng, device, bad_sa)
                assert rc == ERR_ARG
            else:
                isa = np.zeros(n, dtype=np.uint32)
                assert lib.sfx_inverse_table_u32(_gsa.ptr(bad_sa), n, _gsa.ptr(isa)) == ERR_ARG
        for bad_starts in ([1, 5], [0, 9, 8], [0, n + 1], [0, 5, 1 << 40]):
            assert Lx(eng, device, sa, lcp, np.array(bad_starts, dtype=np.uint64), host=host).rc == ERR_ARG, bad_starts
        assert Lx(eng, device, sa, lcp, np.array([0, 5], dtype=np.uint64), host=host, ndocs=0).rc == ERR_ARG       # starts without a count
        ok = Lx(eng, device, sa, lcp, np.array([0, 0, 5, n, n], dtype=np.uint64), host=host)
        assert ok.rc == OK and ok.lce([0, 4, 5], [1, 6, 5], 2).tolist() == [brute(text, 0, 1, 2, [0, 0, 5, n, n]), 1, n - 5]
        ok.close()
    h = ctypes.c_void_p()
    s_, l_ = _buffers.inp(sa, device, 4), _buffers.inp(lcp, device, 4)
    assert lib.sfx_lce_create_dev(s_.ptr, l_.ptr, 1 << 32, None, 0, st, ctypes.byref(h)) == ERR_TOO_LARGE and not h
    assert lib.sfx_lce_create(_gsa.ptr(sa), _gsa.ptr(lcp), 1 << 32, None, 0, ctypes.byref(h)) == ERR_TOO_LARGE and not h
    assert lib.sfx_lce_create_dev(None, l_.ptr, n, None, 0, st, ctypes.byref(h)) == ERR_ARG
    assert lib.sfx_lce_create_dev(s_.ptr, None, n, None, 0, st, ctypes.byref(h)) == ERR_ARG
    assert lib.sfx_lce_create_dev(s_.ptr, l_.ptr, n, None, 3, st, ctypes.byref(h)) == ERR_ARG                      # a count without starts
    assert lib.sfx_lce_create_dev(s_.ptr, l_.ptr, n, None, 0, st, None) == ERR_ARG
    assert lib.sfx_lce_create(None, _gsa.ptr(lcp), n, None, 0, ctypes.byref(h)) == ERR_ARG and not h
    for off in (1, 2):                                                   # u32 arrays off 4 bytes, doc_starts off 8
        assert lib.sfx_lce_create_dev(_vp(s_.ptr.value + off), l_.ptr, n, None, 0, st, ctypes.byref(h)) == ERR_ARG
        assert lib.sfx_lce_create_dev(s_.ptr, _vp(l_.ptr.value + off), n, None, 0, st, ctypes.byref(h)) == ERR_ARG
    d_ = _buffers.inp(np.array([0, 5], dtype=np.uint64), device, 4)
    assert lib.sfx_lce_create_dev(s_.ptr, l_.ptr, n, d_.ptr, 2, st, ctypes.byref(h)) == ERR_ARG
    assert not h
    # the empty index: a valid handle
    for host in (False, True):
        e = Lx(eng, device, [], [], host=host)
        assert e.rc == OK
        assert e.lce([0, 1, 0], [0, 0, 9], 4).tolist() == [0, NONE, NONE] and e.range_min([0, 0], [0, 1]).tolist() == [NONE, NONE]
        assert e.ranks([0, 3]).tolist() == [NONE, NONE]
        e.close()
    # the queries: no handle, missing arrays, arrays off 4 bytes; nq == 0 is fine whatever the pointers
    lx = Lx(eng, device, sa, lcp)
    q = _buffers.inp(_u32a([1, 2, 3]), device, 4)
    o = _buffers.guarded(12, device, 4, 0xA5)
    assert lib.sfx_lce_query_dev(None, q.ptr, q.ptr, 3, 0, o.ptr, st) == ERR_ARG
    assert lib.sfx_lce_query_dev(lx.h, None, q.ptr, 3, 0, o.ptr, st) == ERR_ARG
    assert lib.sfx_lce_query_dev(lx.h, q.ptr, None, 3, 0, o.ptr, st) == ERR_ARG
    assert lib.sfx_lce_query_dev(lx.h, q.ptr, q.ptr, 3, 0, None, st) == ERR_ARG
    assert lib.sfx_lce_query_dev(lx.h, q.ptr, q.ptr, 3, 0, _vp(o.ptr.value + 2), st) == ERR_ARG
    assert lib.sfx_lce_query_dev(lx.h, _vp(q.ptr.value + 1), q.ptr, 3, 0, o.ptr, st) == ERR_ARG
    assert lib.sfx_lce_range_min_dev(None, q.ptr, q.ptr, 3, o.ptr, st) == ERR_ARG
    assert lib.sfx_lce_range_min_dev(lx.h, q.ptr, None, 3, o.ptr, st) == ERR_ARG
    assert lib.sfx_lce_range_min_dev(lx.h, q.ptr, q.ptr, 3, _vp(o.ptr.value + 3), st) == ERR_ARG
    assert lib.sfx_lce_ranks_dev(None, q.ptr, 3, o.ptr, st) == ERR_ARG
    assert lib.sfx_lce_ranks_dev(lx.h, None, 3, o.ptr, st) == ERR_ARG
    assert lib.sfx_lce_ranks_dev(lx.h, q.ptr, 3, None, st) == ERR_ARG
    assert lib.sfx_lce_query_dev(lx.h, None, None, 0, 0, None, st) == OK and lib.sfx_lce_ranks_dev(lx.h, None, 0, None, st) == OK
    hq = _u32a([1, 2, 3])
    ho = np.full(3, 0xA5A5A5A5, dtype=np.uint32)
    assert lib.sfx_lce_query(None, _gsa.ptr(hq), _gsa.ptr(hq), 3, 0, _gsa.ptr(ho)) == ERR_ARG
    assert lib.sfx_lce_query(lx.h, _gsa.ptr(hq), None, 3, 0, _gsa.ptr(ho)) == ERR_ARG
    assert lib.sfx_lce_range_min(lx.h, None, _gsa.ptr(hq), 3, _gsa.ptr(ho)) == ERR_ARG
    assert lib.sfx_lce_ranks(lx.h, _gsa.ptr(hq), 3, None) == ERR_ARG
    assert (ho == 0xA5A5A5A5).all() and (o.host() == 0xA5).all(), "a refused call wrote"
    o.check_guards("refused")
    lx.close()
    lib.sfx_lce_destroy(None)
    # the inverse table's workspace: short, missing, off its boundary
    need = int(lib.sfx_inverse_table_workspace_bytes(n))
    assert need > 0 and lib.sfx_inverse_table_workspace_bytes(0) == 0 and lib.sfx_inverse_table_workspace_bytes(1 << 32) == 0
    assert inverse_table_raw(eng, device, sa, ws_bytes=need - 1)[0] == ERR_WORKSPACE
    assert inverse_table_raw(eng, device, sa, ws_bytes=0)[0] == ERR_WORKSPACE
    for ws_off in (1, 4, 8):
        rc, isa = inverse_table_raw(eng, device, sa, ws_off=ws_off)
        assert rc == ERR_ARG and (isa == NONE).all(), (rc, ws_off)
    for off in (1, 2, 3):
        assert inverse_table_raw(eng, device, sa, out_off=off)[0] == ERR_ARG and inverse_table_raw(eng, device, sa, sa_off=off)[0] == ERR_ARG
    i_ = _buffers.guarded(4 * n, device, 0, 0xFF)
    w_ = _buffers.guarded(need, device, 0, 0xFF)
    assert lib.sfx_inverse_table_dev(s_.ptr, 1 << 32, i_.ptr, w_.ptr, need, st) == ERR_TOO_LARGE
    assert lib.sfx_inverse_table_dev(None, n, i_.ptr, w_.ptr, need, st) == ERR_ARG and lib.sfx_inverse_table_dev(s_.ptr, n, None, w_.ptr, need, st) == ERR_ARG
    assert lib.sfx_inverse_table_dev(s_.ptr, n, i_.ptr, None, need, st) == ERR_WORKSPACE
    assert lib.sfx_inverse_table_dev(None, 0, None, None, 0, st) == OK
    assert lib.sfx_inverse_table_u32(None, 0, None) == OK and lib.sfx_inverse_table_u32(_gsa.ptr(sa), 1 << 32, _gsa.ptr(sa)) == ERR_TOO_LARGE
    assert (i_.host() == 0xFF).all()
    _buffers.check_all({"isa": i_, "workspace": w_, "sa": s_, "lcp": l_})


# ---- 6. a corrupted lcp ------------------------------------------------------------------------------------------------------
def corrupted_lcp(eng, device, orc):
    """lcp is not verified: with random values, or UINT32_MAX everywhere, every call returns, writes inside its outputs and
    stays within min(end - i, end - j)."""
    rng = random.Random(26)
    nrng = np.random.default_rng(26)
    docs = [bytes(rng.choice(b"ab") for _ in range(rng.choice((0, 1, 40, 130)))) for _ in range(14)]
    text, sa, _, starts = collection_tables(docs)
    n = len(text)
    a, b = pair_list(n, rng, 600)
    for starts_ in (None, starts):
        psa = orc.sais(text) if starts_ is None else sa
        for lcp in (nrng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), np.full(n, NONE, dtype=np.uint32),
                    nrng.integers(0, 2 * n, n).astype(np.uint32)):
            for host in (False, True):
                lx = Lx(eng, device, psa, lcp, starts_, host=host, lcp_off=4)
                assert lx.rc == OK
                for k in (0, 3, NONE):
                    got = lx.lce(a, b, k)
                    for i, j, v in zip(a.tolist(), b.tolist(), got.tolist()):
                        if i > n or j > n:
                            assert v == NONE
                        elif i == n or j == n:
                            assert v == 0
                        else:
                            assert v <= min(end_of(i, n, starts_) - i, end_of(j, n, starts_) - j), (i, j, k, v)
                lo, hi = edge_ranges(n, rng, extra=40)
                assert np.array_equal(lx.range_min(lo, hi), expected_min(lcp, lo, hi))        # (still the minimum of what is stored)
                lx.close()


# ---- 7. streams, threads, sizes, launch names ------------------------------------------------------------------------------------
def streams_and_threads(eng, device, orc):
    text = _gen.english_like(4000).tobytes()
    n = len(text)
    sa, lcp = tables(orc, text)
    rng = random.Random(27)
    a, b = pair_list(n, rng, 800)
    exp = {k: _u32a([brute(text, int(i), int(j), k) for i, j in zip(a, b)]) for k in (0, 2)}
    side = torch.cuda.Stream() if str(device).startswith("cuda") else None
    for t in range(4):
        with (torch.cuda.stream(side) if side is not None and t % 2 else contextlib.nullcontext()):
            lx = Lx(eng, device, sa, lcp, sa_off=(4, 8, 12, 4)[t], lcp_off=(0, 4, 8, 12)[t])
            assert lx.rc == OK
            for k in (0, 2):
                assert np.array_equal(lx.lce(a, b, k), exp[k]), (t, k)
            rc, isa = inverse_table_raw(eng, device, sa, fill=_buffers.FILLS[t % 3])
            assert rc == OK and np.array_equal(isa, expected_isa(sa))
            lx.close()
    # two threads on one handle at once (on the emulator: one after the other), equal answers
    dsa, dlcp = (torch.from_numpy(x.view(np.int32).copy()).to(device) for x in (sa, lcp))
    ix = sdev.LceDeviceIndex(dsa, dlcp, engine=eng)
    da, db = (torch.from_numpy(x.view(np.int32).copy()).to(device) for x in (a, b))
    results, errors = [None, None], []

    def worker(j):
        try:
            for _ in range(3):
                got = ix.lce(da, db, mismatches=(0, 2)[j])
                _sync(device)
                results[j] = got.cpu().numpy().view(np.uint32)
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
    assert np.array_equal(results[0], exp[0]) and np.array_equal(results[1], exp[2])
    _sync(device)
    ix.close()


def size_bound(eng):
    """Hook-free: 4n <= sfx_lce_bytes(n) <= 4n + n / 7 + 64 KiB, and 0 where there is nothing to hold."""
    assert "SFX_LCE_FAN" not in os.environ
    f = eng.lib.sfx_lce_bytes
    for n in (1, 2, 31, 32, 33, 1023, 1024, 1025, 1057, 32768, 32769, 33825, 100003, 1 << 20, (1 << 20) + 5, (1 << 22) + 5, 10 ** 9, (1 << 32) - 1):
        got = int(f(n))
        assert 4 * n <= got <= 4 * n + n // 7 + (64 << 10), (n, got)
    assert int(f((1 << 22))) - 4 * (1 << 22) == 4 * (131072 + 4096 + 128 + 32)           # the levels of 2^22 entries, the top one padded to a line
    assert f(0) == 0 and f(1 << 32) == 0


def launch_names(eng, device, orc):
    text = _gen.dna(3000, seed=3).tobytes()
    sa, lcp = tables(orc, text)

    def run():
        lx = Lx(eng, device, sa, lcp)
        lx.lce([1, 2], [5, 9], 1)
        lx.range_min([0], [2000])
        lx.ranks([7])
        lx.close()
    names = _gsa.profile_names(eng, run)
    assert KERNELS <= names, sorted(names)
    assert not {x for x in names if x.startswith("lce_")} - KERNELS, sorted(names)


def hooked(eng, device, orc):
    """What a hooked child process runs (SFX_LCE_FAN, SFX_MAX_GRID, SFX_PARTITION_MIN): the random and edge cases again."""
    known_answers(eng, device, orc)
    small_random(eng, device, orc, count=40, seed=31)
    small_collections(eng, device, count=12, seed=32)
    level_edges(eng, device, sizes=(0, 1, 2, 3, 4, 5, 31, 33, 64, 65, 1025, 4097, 5000))
    edge_texts(eng, device, orc, n=3000, limit=200)


# ---- scale (test_gpu_lce.py) -------------------------------------------------------------------------------------------------
def scale_pairs(n, sa, nq, seed):
    """nq pairs: a quarter uniform, a quarter rank neighbours at distance d in (1, 2, 31, 32, 33, 1024, 32768), a quarter
    (i, i + a small offset), a quarter i == j and the positions n - 1, n, n + 1."""
    rng = np.random.default_rng(seed)
    q = nq // 4
    a = [rng.integers(0, n, q)]
    b = [rng.integers(0, n, q)]
    d = np.array([1, 2, 31, 32, 33, 1024, 32768])[rng.integers(0, 7, q)]
    r = rng.integers(0, n - 32768, q)
    a.append(sa[r].astype(np.int64))
    b.append(sa[r + d].astype(np.int64))
    i = rng.integers(0, n, q)
    a.append(i)
    b.append(np.minimum(i + rng.integers(1, 64, q), n + 1))
    rest = nq - 3 * q
    i = rng.integers(0, n, rest)
    j = i.copy()
    tail = np.array([n - 1, n, n + 1])
    i[:300] = tail[rng.integers(0, 3, 300)]
    j[:300] = np.where(rng.random(300) < 0.5, rng.integers(0, n, 300), tail[rng.integers(0, 3, 300)])
    a.append(i)
    b.append(j)
    return _u32a(np.concatenate(a)), _u32a(np.concatenate(b))
