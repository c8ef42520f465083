"""The cases of the maximal repetitions and the Lyndon array (sfx_runs_*, sfx_lyndon_array_*), shared
by test_runs_emu.py (the emulator build, host memory) and test_gpu_runs.py (libsuffix_hip.so, HBM).

Nothing expected comes from the engine.  The known answer of a small text is `brute`: for every period p the maximal
stretches of T[k] == T[k+p], kept when they are two periods long and p is their smallest period -- the definition.  Larger
texts go through the serial checker tests/runs_check.c, which reads the text and the triples only.  The Lyndon array is
compared with a stack over the oracle's inverse table.  The tables handed to the engine are the oracle's."""
import concurrent.futures
import contextlib
import ctypes
import os
import random
import subprocess

import numpy as np
import torch

import _buffers
import _gen
import _gsa
from suffix_amd import SuffixHipError, SuffixTable
from suffix_amd import device as sdev
from suffix_amd._lib import RunsFilter

OK, ERR_ARG, ERR_TOO_LARGE, ERR_WORKSPACE = 0, 1, 2, 5
NONE = 0xFFFFFFFF
KERNELS = {"runs_complement", "runs_check", "runs_scatter", "runs_verify", "runs_levels", "runs_lyndon_tile", "runs_lyndon_open",
           "runs_candidates", "runs_offsets", "runs_compact", "runs_extend", "runs_gather", "runs_write"}
HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
CSRC_FROM_EMU = "../../suffix_amd/csrc"                                  # tests/emu/Makefile's CSRC
_vp, _u64, _u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32

KNOWN = [(b"mississippi", [(1, 8, 3), (2, 4, 1), (5, 7, 1), (8, 10, 1)]), (b"banana", [(1, 6, 2)]), (b"aaaa", [(0, 4, 1)]),
         (b"abracadabra", []),
         (b"abaababaabaab", [(0, 6, 3), (0, 11, 5), (2, 4, 1), (3, 8, 2), (5, 13, 3), (7, 9, 1), (10, 12, 1)])]
FIB_RUNS = {13: 7, 21: 13, 34: 23, 55: 39, 89: 65, 144: 107, 233: 175, 377: 285, 610: 463, 987: 751}


def build_emulator():
    """`make -C tests/emu`; sfx_runs.hip is compiled as part of sfx_api.hip's translation unit and tests/emu/Makefile does
    not name it, so when it is newer than the library sfx_api.hip is declared new (`make -W`).  -> the library's path."""
    lib = os.path.join(EMU_DIR, "libsuffix_emu.so")
    cmd = ["make", "-s", "-j8", "-C", EMU_DIR]
    src = os.path.join(HERE, os.pardir, "suffix_amd", "csrc", "sfx_runs.hip")
    if os.path.exists(lib) and os.path.getmtime(src) > os.path.getmtime(lib):
        cmd += ["-W", CSRC_FROM_EMU + "/sfx_api.hip"]
    subprocess.check_call(cmd)
    return lib


def _u32a(x):
    return np.ascontiguousarray(x, dtype=np.uint32)


def _arr(text):
    return np.frombuffer(text, dtype=np.uint8)


def fibonacci(length):
    """f0 = b, f1 = a, fk = f(k-1) f(k-2), the one of exactly `length` bytes."""
    a, b = b"b", b"a"
    while len(b) < length:
        a, b = b, b + a
    assert len(b) == length, length
    return b


def complement(text):
    return (255 - _arr(text)).astype(np.uint8).tobytes()


def tables(orc, text):
    sa = orc.sais(text)
    lcp = orc.lcp_kasai(text, sa) if len(text) > 3000 else orc.lcp_quadratic(text, sa)
    return _u32a(sa), _u32a(lcp)


# ---- the known answers -----------------------------------------------------------------------------------------------------
def _prime_factors(p):
    out, f = [], 2
    while f * f <= p:
        if p % f == 0:
            out.append(f)
            while p % f == 0:
                p //= f
        f += 1
    if p > 1:
        out.append(p)
    return out


def brute(text, min_period=1, max_period=None, min_len=0):
    """Every run of `text` from the definition, ascending by (begin, period)."""
    t = _arr(text)
    n = t.size
    out = []
    for p in range(max(1, min_period), min(n // 2, n if max_period is None else max_period) + 1):
        eq = np.concatenate(([0], (t[:n - p] == t[p:]).astype(np.int8), [0]))
        d = np.diff(eq)
        for s, k in zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()):   # the stretch [s, k) of equal pairs
            b, e = s, k + p
            if e - b < 2 * p or e - b < min_len:
                continue
            root = t[b:b + p]
            if any((root[:p - p // f] == root[p // f:]).all() for f in _prime_factors(p)):
                continue
            out.append((b, e, p))
    return sorted(out, key=lambda r: (r[0], r[2]))


def lyndon_stack(isa):
    """lyn[i] = (the next j > i with isa[j] < isa[i], or n) - i, by one pass with a stack."""
    n = len(isa)
    out = np.zeros(n, dtype=np.uint32)
    stack = []
    for j, v in enumerate(isa.tolist()):
        while stack and stack[-1][1] > v:
            i, _ = stack.pop()
            out[i] = j - i
        stack.append((j, v))
    for i, _ in stack:
        out[i] = n - i
    return out


def inverse(sa):
    isa = np.zeros(len(sa), dtype=np.uint32)
    isa[np.asarray(sa, dtype=np.int64)] = np.arange(len(sa), dtype=np.uint32)
    return isa


def expected_lyndon(orc, text, order):
    return lyndon_stack(inverse(orc.sais(text if order == 0 else complement(text)))) if text else np.zeros(0, dtype=np.uint32)


# ---- the checker -----------------------------------------------------------------------------------------------------------
def build_checker(out_dir):
    so = os.path.join(str(out_dir), "libruns_check.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "runs_check.c")])
    lib = ctypes.CDLL(so)
    i64p, u64p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(_u64)
    lib.runs_check_verify.restype = ctypes.c_int
    lib.runs_check_verify.argtypes = [_vp, _u64, _vp, _vp, _vp, _u64, _u32, _u32, _u32, i64p]
    lib.runs_check_sweep.restype = ctypes.c_int
    lib.runs_check_sweep.argtypes = [_vp, _u64, _vp, _vp, _vp, _u64, _u64, _u64, _u32, _u32, _u32, u64p, i64p]
    lib.runs_check_lyndon.restype = ctypes.c_int
    lib.runs_check_lyndon.argtypes = [_vp, _u64, _vp, i64p]
    lib.runs_check_name.restype = ctypes.c_char_p
    lib.runs_check_name.argtypes = [ctypes.c_int]
    return lib


def _cols(triples):
    if isinstance(triples, tuple) and len(triples) == 3 and isinstance(triples[0], np.ndarray):
        return tuple(_u32a(x) for x in triples)
    tr = list(triples)
    return tuple(_u32a([r[k] for r in tr]) for k in range(3))


def verify(chk, text, triples, flt=(1, 0, 0)):
    """-> (verdict, index of the first bad triple or -1)"""
    t = _arr(text)
    b, e, p = _cols(triples)
    where = ctypes.c_int64(-2)
    rc = chk.runs_check_verify(_gsa.ptr(t), t.size, _gsa.ptr(b), _gsa.ptr(e), _gsa.ptr(p), b.size, *flt, ctypes.byref(where))
    return chk.runs_check_name(rc).decode(), int(where.value)


def sweep(chk, text, triples, P, flt=(1, 0, 0), threads=1):
    """-> (verdict, index, the number of runs of period <= P the sweep found).  threads > 1: the periods 1 .. P in that many
    ranges, one checker call each (ctypes releases the interpreter lock); the first range that objects gives the verdict."""
    t = _arr(text)
    b, e, p = _cols(triples)
    P = int(P)

    def one(lo, hi):
        where, found = ctypes.c_int64(-2), _u64(0)
        rc = chk.runs_check_sweep(_gsa.ptr(t), t.size, _gsa.ptr(b), _gsa.ptr(e), _gsa.ptr(p), b.size, lo, hi, *flt, ctypes.byref(found),
                                  ctypes.byref(where))
        return chk.runs_check_name(rc).decode(), int(where.value), int(found.value)
    if threads <= 1 or P < 4 * threads:
        return one(1, P)
    # (a period costs about n byte compares whatever it is: equal ranges)
    cuts = [1 + (P * k) // threads for k in range(threads)] + [P + 1]
    with concurrent.futures.ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(lambda k: one(cuts[k], cuts[k + 1] - 1), range(threads)))
    bad = [x for x in parts if x[0] != "ok"]
    return bad[0] if bad else ("ok", -1, sum(x[2] for x in parts))


def check_threads():
    try:
        return max(1, min(16, len(os.sched_getaffinity(0))))
    except AttributeError:
        return 4


def accept_lyndon(chk, isa, lyn):
    isa, lyn = _u32a(isa), _u32a(lyn)
    assert isa.size == lyn.size
    where = ctypes.c_int64(-2)
    rc = chk.runs_check_lyndon(_gsa.ptr(isa), isa.size, _gsa.ptr(lyn), ctypes.byref(where))
    w = int(where.value)
    assert rc == 0, f"runs_check_lyndon: {chk.runs_check_name(rc).decode()} at position {w}: reported {int(lyn[w])}"


def accept(chk, text, triples, P, flt=(1, 0, 0), threads=1):
    """verify, then sweep P; -> the sweep's count"""
    v = verify(chk, text, triples, flt)
    assert v == ("ok", -1), (v, len(text))
    s = sweep(chk, text, triples, P, flt, threads)
    assert s[:2] == ("ok", -1), (s, len(text), P)
    return s[2]


def checker_self_test(chk):
    """One fault per kind, each named; the faultless lists pass; the sweep agrees with `brute` on random texts."""
    for text, want in KNOWN:
        assert verify(chk, text, want) == ("ok", -1), text
        assert sweep(chk, text, want, len(text) // 2) == ("ok", -1, len(want)), text
    text, good = KNOWN[4]
    assert verify(chk, text, good[:2] + good[3:]) == ("ok", -1)                       # verify alone cannot see a missing run ...
    assert sweep(chk, text, good[:2] + good[3:], 6)[:2] == ("a run is missing", 2)    # ... the sweep does
    assert sweep(chk, text, good[:-1], 6)[:2] == ("a run is missing", 6)
    assert sweep(chk, b"abcabcab", [(0, 8, 3), (1, 7, 3)], 4)[:2] == ("not a run of the sweep", 1)     # an extra triple
    assert verify(chk, b"abcabcab", [(0, 8, 3), (1, 7, 3)]) == ("extends to the left", 1)
    assert verify(chk, b"xabababy", [(1, 5, 2)]) == ("extends to the right", 0)       # an extendable one
    assert verify(chk, b"xabababy", [(3, 7, 2)]) == ("extends to the left", 0)
    assert verify(chk, b"xabababy", [(1, 7, 2)]) == ("ok", -1)
    assert verify(chk, b"aaaaaaaa", [(0, 8, 2)]) == ("not the smallest period", 0)
    assert verify(chk, b"aaaaaaaa", [(0, 8, 4)]) == ("not the smallest period", 0)
    assert verify(chk, b"aaaaaaaa", [(0, 8, 1)]) == ("ok", -1)
    assert verify(chk, text, [good[1], good[0]] + good[2:]) == ("not ascending by (begin, period)", 1)  # a swapped pair
    assert verify(chk, text, good[:3] + good[2:]) == ("not ascending by (begin, period)", 3)            # a duplicate
    assert verify(chk, b"abab", [(0, 5, 2)]) == ("out of bounds", 0)
    assert verify(chk, b"abab", [(2, 2, 1)]) == ("out of bounds", 0)
    assert verify(chk, b"abaab", [(0, 3, 2)]) == ("shorter than two periods", 0)
    assert verify(chk, b"abcabd", [(0, 6, 3)]) == ("not periodic", 0)
    assert verify(chk, text, good, (2, 0, 0)) == ("fails the filter", 2)
    assert verify(chk, text, good, (1, 3, 0)) == ("fails the filter", 1)
    assert verify(chk, text, good, (1, 0, 6)) == ("fails the filter", 2)
    assert sweep(chk, text, [r for r in good if r[2] >= 2 and r[1] - r[0] >= 6], 6, (2, 0, 6)) == ("ok", -1, 3)
    fib = fibonacci(987)
    assert sweep(chk, fib, brute(fib), 493, threads=5) == ("ok", -1, FIB_RUNS[987])           # the periods in five ranges
    assert sweep(chk, fib, brute(fib)[:-1], 493, threads=5)[0] == "a run is missing"
    accept_lyndon(chk, [2, 0, 3, 1], [1, 3, 1, 1])
    with contextlib.suppress(AssertionError):
        accept_lyndon(chk, [2, 0, 3, 1], [1, 2, 1, 1])
        raise RuntimeError("runs_check_lyndon accepted a wrong array")
    rng = random.Random(44)
    for _ in range(200):
        t = bytes(rng.randrange(rng.choice((1, 2, 3))) for _ in range(rng.randint(0, 60)))
        assert accept(chk, t, brute(t), len(t) // 2) == len(brute(t)), t


# ---- the raw ABI over guarded buffers ----------------------------------------------------------------------------------------
def _filter(flt):
    return None if flt is None else RunsFilter(int(flt[0]), int(flt[1]), int(flt[2]), 0)


def call_runs(eng, device, text, sa, lcp, flt=None, capacity=None, fill=0xFF, text_off=1, u32_off=4, ws_bytes=None, ws_off=0):
    """sfx_runs_dev over arrays between guard bands, the workspace exactly sfx_runs_workspace_bytes(n) long and filled with
    `fill`.  -> (rc, count, the written triples as a list, the buffers)"""
    n = len(text)
    cap = n if capacity is None else capacity
    need = int(eng.lib.sfx_runs_workspace_bytes(n))
    offs = _buffers.U32_OFFSETS
    k = offs.index(u32_off)
    b = {"text": _buffers.text_in(text, device, text_off), "sa": _buffers.inp(_u32a(sa), device, u32_off),
         "lcp": _buffers.inp(_u32a(lcp), device, offs[(k + 1) % 3]),
         "begin": _buffers.guarded(4 * cap, device, offs[(k + 2) % 3], _buffers.out_fill(fill)),
         "end": _buffers.guarded(4 * cap, device, u32_off, _buffers.out_fill(fill)),
         "period": _buffers.guarded(4 * cap, device, offs[(k + 1) % 3], _buffers.out_fill(fill)),
         "workspace": _buffers.guarded(need if ws_bytes is None else ws_bytes, device, ws_off, fill)}
    count = _u64(987654321)
    f = _filter(flt)
    rc = eng.lib.sfx_runs_dev(b["text"].ptr, n, b["sa"].ptr, b["lcp"].ptr, ctypes.byref(f) if f is not None else None, b["begin"].ptr,
                              b["end"].ptr, b["period"].ptr, cap, ctypes.byref(count), b["workspace"].ptr, b["workspace"].nbytes,
                              _buffers.stream_of(device))
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()
    _buffers.check_all(b)
    got = [b[x].host(np.uint32) for x in ("begin", "end", "period")]
    z = int(count.value)
    w = min(z, cap) if rc == OK else 0
    if rc == OK:
        filler = _buffers.guarded(4 * cap, "cpu", 0, _buffers.out_fill(fill)).host(np.uint32)
        for g in got:
            assert np.array_equal(g[w:], filler[w:]), "something was written behind the reported triples"
    return rc, z, list(zip(*(g[:w].tolist() for g in got))), b


def host_runs(eng, text, sa=None, lcp=None, flt=None, capacity=None):
    n = len(text)
    cap = n if capacity is None else capacity
    t = _arr(text)
    out = [np.full(cap + 4, NONE, dtype=np.uint32) for _ in range(3)]
    count = _u64(5)
    f = _filter(flt)
    rc = eng.lib.sfx_runs_u32(_gsa.ptr(t), n, None if sa is None else _gsa.ptr(_u32a(sa)), None if lcp is None else _gsa.ptr(_u32a(lcp)),
                              ctypes.byref(f) if f is not None else None, *[_gsa.ptr(o) for o in out], cap, ctypes.byref(count))
    z = int(count.value)
    w = min(z, cap) if rc == OK else 0
    for o in out:
        assert (o[w:] == NONE).all()
    return rc, z, list(zip(*(o[:w].tolist() for o in out)))


def call_lyndon(eng, device, isa, fill=0xFF, off=4, ws_bytes=None, ws_off=0):
    n = len(isa)
    need = int(eng.lib.sfx_lyndon_array_workspace_bytes(n))
    b = {"isa": _buffers.inp(_u32a(isa), device, off), "lyn": _buffers.guarded(4 * n, device, _buffers.U32_OFFSETS[(off // 4) % 3], _buffers.out_fill(fill)),
         "workspace": _buffers.guarded(need if ws_bytes is None else ws_bytes, device, ws_off, fill)}
    rc = eng.lib.sfx_lyndon_array_dev(b["isa"].ptr, n, b["lyn"].ptr, b["workspace"].ptr, b["workspace"].nbytes, _buffers.stream_of(device))
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()
    _buffers.check_all(b)
    return rc, b["lyn"].host(np.uint32), b


def host_lyndon(eng, text, order, sa=None):
    t = _arr(text)
    out = np.full(len(text) + 4, NONE, dtype=np.uint32)
    rc = eng.lib.sfx_lyndon_array_u32(_gsa.ptr(t), len(text), None if sa is None else _gsa.ptr(_u32a(sa)), order, _gsa.ptr(out))
    assert (out[len(text):] == NONE).all()
    return rc, out[:len(text)]


def _dev32(x, device):
    return torch.from_numpy(_u32a(x).view(np.int32).copy()).to(device)


def _dev8(text, device):
    return torch.from_numpy(_arr(text).copy()).to(device)


def check_text(eng, device, orc, text, want=None, host=True, lyndon=True, fill=0xFF, k=0):
    """One text through sfx_runs_dev (and the host route, and both Lyndon arrays) against `want` (default: brute)."""
    want = brute(text) if want is None else want
    sa, lcp = tables(orc, text) if text else (_u32a([]), _u32a([]))
    rc, z, got, _ = call_runs(eng, device, text, sa, lcp, fill=fill, text_off=_buffers.TEXT_OFFSETS[k % 4], u32_off=_buffers.U32_OFFSETS[k % 3])
    assert rc == OK and z == len(want) and got == want, (rc, z, text[:80], got[:6], want[:6])
    if host:
        assert host_runs(eng, text) == (OK, len(want), want), text[:80]
    if lyndon:
        for order in (0, 1):
            exp = expected_lyndon(orc, text, order)
            rc, lyn, _ = call_lyndon(eng, device, inverse(orc.sais(text if order == 0 else complement(text))) if text else exp, fill=fill)
            assert rc == OK and np.array_equal(lyn, exp), (order, text[:80], np.flatnonzero(lyn != exp)[:4])
    return want


# ---- cases -----------------------------------------------------------------------------------------------------------------
def known_answers(eng, device, orc):
    """The issue's tables through every entry point and binding."""
    for text, want in KNOWN:
        assert brute(text) == want, text
        check_text(eng, device, orc, text, want)
        sa, lcp = tables(orc, text)
        assert host_runs(eng, text, sa, lcp) == (OK, len(want), want)
        assert host_runs(eng, text, sa) == (OK, len(want), want)
        b, e, p, z = sdev.runs(_dev8(text, device), _dev32(sa, device), _dev32(lcp, device), engine=eng)
        assert z == len(want) and list(zip(*(x.cpu().numpy().view(np.uint32).tolist() for x in (b, e, p)))) == want
        st = SuffixTable.from_parts(text, sa, engine=eng)
        r = st.runs()
        assert len(r) == len(want) and r.triples() == want and r.n == len(text)
        assert np.allclose(r.exponent, [(e_ - b_) / p_ for b_, e_, p_ in want])
        for order in (0, 1):
            exp = expected_lyndon(orc, text, order)
            assert np.array_equal(st.lyndon_array(order), exp)
            tsa = orc.sais(text if order == 0 else complement(text))
            assert host_lyndon(eng, text, order, tsa)[0] == OK and np.array_equal(host_lyndon(eng, text, order, tsa)[1], exp)
            isa = sdev.inverse_table(_dev32(tsa, device), engine=eng)
            assert np.array_equal(sdev.lyndon_array(isa, engine=eng).cpu().numpy().view(np.uint32), exp)
    st = SuffixTable(b"banana", engine=eng)
    assert st.lyndon_factorization().tolist() == [0, 1, 3, 5]
    assert st.lyndon_array(0).tolist() == [1, 2, 1, 2, 1, 1]
    assert SuffixTable(b"", engine=eng).runs().triples() == [] and SuffixTable(b"", engine=eng).lyndon_factorization().size == 0
    assert repr(SuffixTable(b"aaaa", engine=eng).runs()) == "Runs(n=4, runs=1)"
    for length, count in FIB_RUNS.items():
        text = fibonacci(length)
        want = brute(text)
        assert len(want) == count, (length, len(want))
        check_text(eng, device, orc, text, want, host=length in (13, 89), lyndon=length in (13, 89, 987))


def small_random(eng, device, orc, count=300, seed=19, max_len=300):
    """Random texts of 0 .. max_len bytes over 1, 2, 3, 4 and 256 symbols against `brute`; -> how many were checked."""
    rng = random.Random(seed)
    edge = 0
    for it in range(count):
        n = rng.choice((0, 1, 2, 3)) if it < 8 else rng.randint(0, max_len)
        sigma = (1, 2, 3, 4, 256)[it % 5]
        base = 0 if sigma == 256 else rng.choice((0, 97, 256 - sigma))
        text = bytes(base + rng.randrange(sigma) for _ in range(n))
        want = check_text(eng, device, orc, text, host=it % 10 == 0, lyndon=it % 3 == 0, fill=_buffers.FILLS[it % 3], k=it)
        edge += any(b == 0 or e == n for b, e, _ in want)
    assert edge * 10 >= count * 4, (edge, count)                       # runs that begin at 0 or end at n: the exactly-once rule's cases
    return count


def edge_texts(eng, device, orc, tile=2048, lyndon_every=1):
    """n = 0 .. 3, one repeated byte around the Lyndon tile, (ab)^k, ascending and descending inverse tables, one Lyndon word
    over many tiles, a^k b a^k, a run of period 1500 across a tile boundary, the bytes 0x00 and 0xFF."""
    T = tile
    for text in (b"", b"a", b"aa", b"ab", b"aaa", b"aba", b"abb", b"\x00", b"\xff\xff", b"\x00\xff\x00", b"\xff\x00\xff\x00"):
        check_text(eng, device, orc, text)
    for n in (T - 1, T, T + 1, 2 * T + 1):
        assert check_text(eng, device, orc, b"a" * n, [(0, n, 1)], host=n == T + 1) == [(0, n, 1)]
    k = T + 7
    cases = [(b"ab" * k, [(0, 2 * k, 2)]), (b"a" * (2 * T + 3) + b"b", [(0, 2 * T + 3, 1)]), (b"b" + b"a" * (2 * T + 3), [(1, 2 * T + 4, 1)]),
             (b"a" + b"b" * (3 * T), [(1, 3 * T + 1, 1)]), (b"a" * k + b"b" + b"a" * k, [(0, k, 1), (k + 1, 2 * k + 1, 1)]), (b"a" * k + b"b" + b"a" * k + b"b", [(0, k, 1), (0, 2 * k + 2, k + 1), (k + 1, 2 * k + 1, 1)]),
             (b"\x00" * 70 + b"\xff" * 70 + b"\x00\xff" * 40, None), (b"\xff" * (T + 1) + b"\x00", [(0, T + 1, 1)])]
    unit = _gen.uniform_bytes(1500, 256, 77).tobytes()
    pad = _gen.uniform_bytes(4 * 2048, 250, 78, base=3).tobytes()
    lead = 1300 + (-1300) % T + T // 2                                   # the run begins in the middle of a tile whatever T is
    cases.append((pad[:lead] + unit * 2 + unit[:600] + pad[lead:lead + 90], None))
    for i, (text, want) in enumerate(cases):
        if want is None or len(text) <= 2200:
            assert want is None or brute(text) == want, i
        got = check_text(eng, device, orc, text, want, host=i == 0, lyndon=i % lyndon_every == 0, fill=_buffers.FILLS[i % 3], k=i)
        if i == len(cases) - 1:
            assert [(b, e) for b, e, p in got if p == 1500] == [(lead, lead + 3600)], got
            assert lead % T == T // 2 and lead // T + 1 < (lead + 3600) // T        # it begins inside a tile and crosses tile boundaries


def filters(eng, device, orc):
    """Each filter alone and all together; min_period > max_period and min_len > n are empty."""
    rng = random.Random(23)
    texts = [b"abaababaabaab" * 3, fibonacci(233), bytes(rng.randrange(2) for _ in range(260)), b"a" * 50 + b"ab" * 30 + b"abc" * 25]
    for text in texts:
        sa, lcp = tables(orc, text)
        n = len(text)
        full = brute(text)
        for flt in ((2, 0, 0), (1, 3, 0), (1, 0, 9), (2, 5, 8), (3, 2, 0), (1, 0, n + 1), (0, 0, 0), (1, n, 0), (1, NONE, n), (NONE, 0, 0)):
            lo, hi, ml = max(1, flt[0]), flt[1] or n, flt[2]
            want = [r for r in full if lo <= r[2] <= hi and r[1] - r[0] >= ml]
            assert want == brute(text, lo, hi, ml)
            if flt in ((3, 2, 0), (1, 0, n + 1), (NONE, 0, 0)):
                assert want == []
            rc, z, got, _ = call_runs(eng, device, text, sa, lcp, flt=flt)
            assert rc == OK and z == len(want) and got == want, (flt, got[:5], want[:5])
            assert host_runs(eng, text, sa, lcp, flt=flt) == (OK, len(want), want), flt
        st = SuffixTable.from_parts(text, sa, engine=eng)
        assert st.runs(min_period=2, max_period=5, min_len=8).triples() == brute(text, 2, 5, 8)
        b, e, p, z = sdev.runs(_dev8(text, device), _dev32(sa, device), _dev32(lcp, device), min_period=2, min_len=6, engine=eng)
        assert z == len(brute(text, 2, None, 6)) == b.numel()


def capacities(eng, device, orc):
    """capacity 0, count - 1, count: the count is always full, the prefix is the full list's prefix, nothing behind it."""
    for text in (b"abaababaabaab" * 4, fibonacci(144)):
        sa, lcp = tables(orc, text)
        want = brute(text)
        for cap in (0, 1, len(want) - 1, len(want), len(want) + 3):
            rc, z, got, _ = call_runs(eng, device, text, sa, lcp, capacity=cap)
            assert rc == OK and z == len(want) and got == want[:cap], cap
            assert host_runs(eng, text, sa, lcp, capacity=cap) == (OK, len(want), want[:cap]), cap
        b, e, p, z = sdev.runs(_dev8(text, device), _dev32(sa, device), _dev32(lcp, device), capacity=2, engine=eng)
        assert z == len(want) and b.numel() == 2


def buffers_and_streams(eng, device, orc):
    """Every offset and every kind of dirt in a workspace of exactly the stated size; a side stream."""
    text = _gen.uniform_bytes(2500, 2, 5, base=97).tobytes() + b"ab" * 40
    sa, lcp = tables(orc, text)
    want = brute(text)
    for text_off, u32_off, fill in _buffers.combos():
        rc, z, got, _ = call_runs(eng, device, text, sa, lcp, fill=fill, text_off=text_off, u32_off=u32_off)
        assert rc == OK and got == want, (text_off, u32_off, fill)
    isa = inverse(sa)
    exp = lyndon_stack(isa)
    for i, fill in enumerate(_buffers.FILLS):
        rc, lyn, _ = call_lyndon(eng, device, isa, fill=fill, off=_buffers.U32_OFFSETS[i])
        assert rc == OK and np.array_equal(lyn, exp), fill
    side = torch.cuda.Stream() if str(device).startswith("cuda") else None
    with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
        rc, z, got, _ = call_runs(eng, device, text, sa, lcp, fill="count")
        assert rc == OK and got == want
        rc, lyn, _ = call_lyndon(eng, device, isa, fill="count")
        assert rc == OK and np.array_equal(lyn, exp)


def no_allocations(eng, device, orc, stats):
    """The _dev routes allocate nothing over a caller workspace.  stats() -> device_allocs_total."""
    text = fibonacci(610)
    sa, lcp = tables(orc, text)
    call_runs(eng, device, text, sa, lcp)                              # (first use: the thread's pinned page, its stream)
    before = stats()
    rc, z, got, _ = call_runs(eng, device, text, sa, lcp)
    assert rc == OK and z == FIB_RUNS[610]
    assert call_lyndon(eng, device, inverse(sa))[0] == OK
    assert stats() == before


def size_bound(eng):
    """Hook-free: the workspace formula of include/suffix_hip.h, term by term, and its closed bound."""
    assert "SFX_LCE_FAN" not in os.environ
    up = lambda x: (x + 255) & ~255

    def tw(n):
        words, cnt = 0, n
        while cnt > 32:
            cnt = (cnt + 31) // 32
            words += (cnt + 31) & ~31
        return words
    ws, lw, sa_ws = eng.lib.sfx_runs_workspace_bytes, eng.lib.sfx_lyndon_array_workspace_bytes, eng.lib.sfx_sa_workspace_bytes
    for n in (1, 2, 31, 32, 33, 1023, 1025, 2048, 2049, 32769, 100003, (1 << 20) + 5, 10 ** 8, 10 ** 9, (1 << 32) - 2):
        got, sab = int(ws(n)), int(sa_ws(n))
        fixed = up(256) + 2 * up(8 * 2048) + 2 * up(8 * 2049) + up(n) + 5 * up(4 * n) + up(4 * tw(n))
        late_no_scratch = up(4 * tw(n)) + 3 * up(4 * n) + 2 * up(8 * n)
        assert got >= fixed + up(sab), (n, got)
        assert got <= fixed + max(up(sab), late_no_scratch + up(4 * ((2 << 20) + n // 8))), (n, got)
        assert got <= 21.13 * n + (80 << 10) + max(sab + 256, 28.63 * n + 8.1 * (1 << 20)), (n, got)
        assert int(lw(n)) == up(256) + up(4 * tw(n)) + up(4 * n) <= 4 * n + n // 7 + 2048, n
    for f in (ws, lw):
        assert f(0) == 0 and f((1 << 32) - 1) == 0 and f(1 << 33) == 0


def launch_names(eng, device, orc):
    """Every launch of the call is named runs_*, apart from the table build of the complemented text and the library's radix
    sort of the triples."""
    text = _gen.dna(6000, seed=3).tobytes() + b"ACGT" * 30
    sa, lcp = tables(orc, text)
    comp = complement(text)
    build = _gsa.profile_names(eng, lambda: _buffers.call_build_sa(eng, comp, device))
    assert build and not {x for x in build if x.startswith("runs_")}, sorted(build)
    names = _gsa.profile_names(eng, lambda: call_runs(eng, device, text, sa, lcp))
    assert KERNELS <= names, sorted(KERNELS - names)
    assert {x for x in names if not x.startswith(("runs_", "radix_"))} <= build, sorted(names - build)
    assert {x for x in names if x.startswith("runs_")} == KERNELS, sorted(names)
    names = _gsa.profile_names(eng, lambda: call_lyndon(eng, device, inverse(sa)))
    assert names == {"runs_levels", "runs_lyndon_tile", "runs_lyndon_open"}, sorted(names)


def refusals(eng, device, orc):
    """A repeated table entry, an entry >= n, short and misaligned workspaces, n too large, NULL arguments: decided before
    anything is written (or, for the table, through the one read-back with every guard band intact)."""
    text = _gen.dna(3000, seed=12).tobytes()
    n = len(text)
    sa, lcp = tables(orc, text)
    for bad in ("repeat", "large", "both"):
        s = sa.copy()
        if bad in ("repeat", "both"):
            s[17] = s[2000]
        if bad in ("large", "both"):
            s[n - 1] = n if bad == "large" else NONE
        rc, z, got, _ = call_runs(eng, device, text, s, lcp)
        assert rc == ERR_ARG and got == [], (bad, rc)
        assert host_runs(eng, text, s, lcp)[0] == ERR_ARG
        assert host_lyndon(eng, text, 0, s)[0] == ERR_ARG
        st = SuffixTable.from_parts(text, s, engine=eng)
        with contextlib.suppress(SuffixHipError):
            st.runs()
            raise AssertionError("a table that is no permutation was accepted")
    need = int(eng.lib.sfx_runs_workspace_bytes(n))
    assert call_runs(eng, device, text, sa, lcp, ws_bytes=need - 1)[0] == ERR_WORKSPACE
    assert call_runs(eng, device, text, sa, lcp, ws_bytes=0)[0] == ERR_WORKSPACE
    for off in (1, 4, 8):
        assert call_runs(eng, device, text, sa, lcp, ws_off=off)[0] == ERR_ARG
    isa = inverse(sa)
    lneed = int(eng.lib.sfx_lyndon_array_workspace_bytes(n))
    rc, lyn, _ = call_lyndon(eng, device, isa, ws_bytes=lneed - 1)
    assert rc == ERR_WORKSPACE and (lyn == NONE).all()
    rc, lyn, _ = call_lyndon(eng, device, isa, ws_off=8)
    assert rc == ERR_ARG and (lyn == NONE).all()
    lib, cnt = eng.lib, _u64(7)
    one = _buffers.guarded(64, device, 0, 0xFF)
    for big in ((1 << 32) - 1, 1 << 32, 1 << 40):
        assert lib.sfx_runs_dev(one.ptr, big, one.ptr, one.ptr, None, one.ptr, one.ptr, one.ptr, 4, ctypes.byref(cnt), one.ptr, 64,
                                _buffers.stream_of(device)) == ERR_TOO_LARGE
        assert lib.sfx_runs_u32(one.ptr, big, None, None, None, one.ptr, one.ptr, one.ptr, 4, ctypes.byref(cnt)) == ERR_TOO_LARGE
        assert lib.sfx_lyndon_array_dev(one.ptr, big, one.ptr, one.ptr, 64, _buffers.stream_of(device)) == ERR_TOO_LARGE
        assert lib.sfx_lyndon_array_u32(one.ptr, big, None, 0, one.ptr) == ERR_TOO_LARGE
    assert (one.host() == 0xFF).all()
    one.check_guards("untouched")
    t = _arr(text)
    assert lib.sfx_runs_u32(_gsa.ptr(t), n, None, _gsa.ptr(lcp), None, None, None, None, 0, ctypes.byref(cnt)) == ERR_ARG      # lcp without sa
    assert lib.sfx_runs_u32(_gsa.ptr(t), n, None, None, None, None, None, None, 3, ctypes.byref(cnt)) == ERR_ARG               # capacity, no arrays
    assert lib.sfx_runs_u32(_gsa.ptr(t), n, None, None, None, None, None, None, 0, None) == ERR_ARG
    assert lib.sfx_lyndon_array_u32(_gsa.ptr(t), n, None, 2, _gsa.ptr(lcp)) == ERR_ARG
    assert lib.sfx_runs_u32(None, 0, None, None, None, None, None, None, 0, ctypes.byref(cnt)) == OK and cnt.value == 0
    assert lib.sfx_runs_u32(_gsa.ptr(t), n, _gsa.ptr(sa), _gsa.ptr(lcp), None, None, None, None, 0, ctypes.byref(cnt)) == OK   # the count alone
    assert cnt.value == len(brute(text))


def corrupted_lcp(eng, device, orc):
    """lcp is not verified: with random values, UINT32_MAX or zeros everywhere the call returns, writes inside its outputs
    (guard bands), and every triple has 0 <= b < e <= n and 2p <= e - b."""
    nrng = np.random.default_rng(26)
    for text in (_gen.uniform_bytes(1500, 2, 6, base=97).tobytes(), b"ab" * 700, fibonacci(987)):
        n = len(text)
        sa, _ = tables(orc, text)
        for lcp in (nrng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), np.full(n, NONE, dtype=np.uint32),
                    nrng.integers(0, 2 * n, n).astype(np.uint32), np.zeros(n, dtype=np.uint32)):
            for host in (False, True):
                rc, z, got = host_runs(eng, text, sa, lcp) if host else call_runs(eng, device, text, sa, lcp)[:3]
                assert rc == OK and z <= n and len(got) == z
                for b, e, p in got:
                    assert 0 <= b < e <= n and p >= 1 and 2 * p <= e - b, (b, e, p)


def hooked(eng, device, orc):
    """What a hooked child process runs (SFX_MAX_GRID, SFX_LCE_FAN, SFX_RUNS_TILE, SFX_RUNS_LIST): the random and edge cases
    again, the edge texts around the small tile, so that the list overflows on texts of a few thousand bytes."""
    tile = int(os.environ["SFX_RUNS_TILE"])
    for text, want in KNOWN:
        check_text(eng, device, orc, text, want)
    small_random(eng, device, orc, count=60, seed=31)
    edge_texts(eng, device, orc, tile=tile)
    for text in (b"a" * 2100 + b"b", b"b" + b"a" * 2100, b"a" + b"b" * 3000, fibonacci(2584), _gen.dna(3000, seed=4).tobytes()):
        check_text(eng, device, orc, text, host=False)


# ---- scale (test_gpu_runs.py) ------------------------------------------------------------------------------------------------
def planted(n=1 << 20, seed=41):
    """Random bytes with tandem repeats written in: units of 1000, 5000 and 100 000 bytes, 2, 3.5 and 2.0 times; one begins at 0,
    one ends at n, one straddles a multiple of 2048.  -> (text, the exact (b, e, p) of each, by byte comparison)."""
    t = _gen.uniform_bytes(n, 256, seed).copy()
    rng = np.random.default_rng(seed)
    spots = [(0, 1000, 2.0), (n - 17500, 5000, 3.5), (300 * 2048 - 3100, 5000, 2.0), (700_000, 100_000, 2.0), (123_457, 1000, 3.5)]
    out = []
    for start, p, times in spots:
        unit = rng.integers(0, 256, p, dtype=np.uint8)
        ln = int(p * times)
        t[start:start + ln] = np.resize(unit, ln)
    for start, p, times in spots:
        b, e = start, start + int(p * times)
        while b > 0 and t[b - 1] == t[b - 1 + p]:
            b -= 1
        while e < n and t[e] == t[e - p]:
            e += 1
        assert (t[b:e - p] == t[b + p:e]).all()
        out.append((b, e, p))
    assert out[0][0] == 0 and out[1][1] == n and out[2][0] < 300 * 2048 < out[2][1]
    return t.tobytes(), out
