"""Shared pieces of the matching-statistics tests (test_match_emu.py on the emulator, test_gpu_match.py on the GPU):
the brute-force definition for inputs of at most 80 bytes, the serial checker tests/ms_check.c, the five entry points
behind one call, and the cases both suites run."""
import contextlib
import ctypes
import os
import random
import subprocess
import threading

import numpy as np
import torch

import _buffers
import _cases
import _gsa
import _repeats
from suffix_amd import GeneralizedSuffixTable, SuffixTable
from suffix_amd import device as sdev

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF
OK, ERR_ARG, ERR_TOO_LARGE = 0, 1, 2
ROUTES = ("dev", "index_dev", "index_host", "gindex_dev", "gindex_host")

BANANA_T, BANANA_Q = b"banana", b"bandana nab"
BANANA = {"len": [3, 2, 1, 0, 3, 2, 1, 0, 2, 1, 1], "start": [3, 1, 4, 0, 1, 4, 0, 0, 4, 0, 3], "end": [4, 3, 6, 0, 3, 6, 3, 0, 6, 3, 4]}
# (by the definition of a covered byte, "ban" at 0 covers bytes 0, 1 and 2 exactly as "ana" at 4 covers 4, 5 and 6)
BANANA_SPANS_2 = [(0, 3), (4, 7), (8, 10)]


# ---- the definition ---------------------------------------------------------------------------------------------------
def doc_list(text, starts=None):
    if starts is None:
        return [text]
    s = [int(x) for x in starts] + [len(text)]
    return [text[s[k]:s[k + 1]] for k in range(len(s) - 1)]


def brute(text, sa, query, max_len=0, starts=None):
    """len / start / end by the definition, for inputs of at most 80 bytes: the longest prefix of query[i:] that is a
    substring of ONE document; the ranks whose truncated suffix begins with it.  `sa` = a table of the truncated
    suffixes in their order (SuffixTable.new_naive / GeneralizedSuffixTable.new_naive)."""
    assert len(text) <= 80 and len(query) <= 80
    docs = doc_list(text, starts)
    n, m = len(text), len(query)
    ends = np.zeros(n, dtype=np.int64)                                    # end of the document of every position
    p = 0
    for d in docs:
        ends[p:p + len(d)] = p + len(d)
        p += len(d)
    suf = [text[int(s):int(ends[int(s)])] for s in sa]
    ln, st, en = (np.zeros(m, dtype=np.uint32) for _ in range(3))
    for i in range(m):
        lim = m - i if not max_len else min(max_len, m - i)
        best = 0
        for k in range(lim, 0, -1):
            if any(query[i:i + k] in d for d in docs):
                best = k
                break
        ln[i] = best
        if best:
            ranks = [r for r in range(n) if suf[r].startswith(query[i:i + best])]
            assert ranks == list(range(ranks[0], ranks[-1] + 1))
            st[i], en[i] = ranks[0], ranks[-1] + 1
    return ln, st, en


# ---- the checker ----------------------------------------------------------------------------------------------------
_vp, _u64 = ctypes.c_void_p, ctypes.c_uint64


def build_checker(out_dir):
    """tests/ms_check.c -> a shared object in out_dir, bound."""
    so = os.path.join(str(out_dir), "libms_check.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "ms_check.c")])
    fn = ctypes.CDLL(so).ms_check
    fn.restype = ctypes.c_int
    fn.argtypes = [_vp, _u64, _vp, _vp, _u64, _vp, _u64, ctypes.c_uint32, _vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_int64)]
    return fn


def _np(a, dtype):
    if isinstance(a, (bytes, bytearray)):
        a = np.frombuffer(bytes(a), dtype=np.uint8)
    return np.ascontiguousarray(a, dtype=dtype)


def check(fn, text, sa, query, max_len, res, starts=None):
    """-> (code, position): 0 = the four arrays of `res` = (len, src, start, end) are accepted."""
    t, q, s = _np(text, np.uint8), _np(query, np.uint8), _np(sa, np.uint32)
    ds = None if starts is None else _np(starts, np.uint64)
    arrs = [_np(a, np.uint32) for a in res]
    assert all(a.size == q.size for a in arrs)
    where = ctypes.c_int64(-2)
    rc = fn(_gsa.ptr(t), t.size, _gsa.ptr(s), _gsa.ptr(ds) if ds is not None else None, 0 if ds is None else ds.size, _gsa.ptr(q),
            q.size, int(max_len), *[_gsa.ptr(a) for a in arrs], ctypes.byref(where))
    return rc, int(where.value)


def accept(fn, text, sa, query, max_len, res, starts=None):
    rc, where = check(fn, text, sa, query, max_len, res, starts)
    assert rc == 0, f"ms_check: check {rc} failed at query position {where} (max_len {max_len})"


def checker_self_test(fn, text, sa, query, max_len, res, rng, starts=None):
    """A correct answer is accepted; every one-off mutation of len, start or end at a random position is rejected."""
    accept(fn, text, sa, query, max_len, res, starts)
    m = len(query)
    rejected = 0
    for which in (0, 2, 3):
        for delta in (-1, 1):
            i = rng.randrange(m)
            bad = [np.array(a, dtype=np.int64) for a in res]
            bad[which][i] += delta
            if bad[which][i] < 0 or bad[which][i] > NONE:
                continue
            rc, where = check(fn, text, sa, query, max_len, [b.astype(np.uint32) for b in bad], starts)
            assert rc != 0 and where == i, (text, query, max_len, which, delta, i)
            rejected += 1
    return rejected


# ---- the five entry points ------------------------------------------------------------------------------------------
def _t(a, device, dtype=np.uint8):
    return torch.from_numpy(_np(a, dtype).view(np.int32 if dtype == np.uint32 else dtype).copy()).to(device)


def _host(x):
    return x.cpu().numpy().view(np.uint32)


def run(eng, device, route, text, sa, query, max_len=0, starts=None, da=None, want_src=True, want_interval=True):
    """One entry point -> (len, src, start, end) on the host as uint32 arrays (None for what was not asked).  The
    gindex routes of a plain text see it as one document."""
    n, m = len(text), len(query)
    if route.startswith("gindex"):
        starts = np.zeros(1, dtype=np.int64) if starts is None else starts
        da = np.zeros(n, dtype=np.uint32) if da is None else da
    else:
        assert starts is None
    if route.endswith("_host"):
        t, s, q = _np(text, np.uint8), _np(sa, np.uint32), _np(query, np.uint8)
        h = ctypes.c_void_p()
        if route == "index_host":
            assert eng.lib.sfx_index_create(_gsa.ptr(t), n, _gsa.ptr(s), ctypes.byref(h)) == OK
            call, destroy = eng.lib.sfx_index_match_stats, eng.lib.sfx_index_destroy
        else:
            ds, d = _np(starts, np.uint64), _np(da, np.uint32)
            assert eng.lib.sfx_gindex_create(_gsa.ptr(t), n, _gsa.ptr(ds), ds.size, _gsa.ptr(s), _gsa.ptr(d), ctypes.byref(h)) == OK
            call, destroy = eng.lib.sfx_gindex_match_stats, eng.lib.sfx_gindex_destroy
        out = [np.full(m, 0xDEADBEEF, dtype=np.uint32) if want else None for want in (True, want_src, want_interval, want_interval)]
        try:
            rc = call(h, _gsa.ptr(q), m, int(max_len), *[_gsa.ptr(a) if a is not None else None for a in out])
        finally:
            destroy(h)
        assert rc == OK, (route, rc)
        return tuple(out)
    dt, dsa, dq = _t(text, device), _t(sa, device, np.uint32), _t(query, device)
    kw = dict(max_len=max_len, want_src=want_src, want_interval=want_interval)
    if route == "dev":
        got = sdev.match_stats(dt, dsa, dq, engine=eng, **kw)
    elif route == "index_dev":
        ix = sdev.DeviceIndex(dt, dsa, engine=eng)
        got = ix.match_stats(dq, **kw)
        _sync(device)
        ix.close()
    else:
        gx = sdev.GeneralizedDeviceIndex(dt, _t(starts, device, np.int64), dsa, _t(da, device, np.uint32), engine=eng)
        got = gx.match_stats(dq, **kw)
        _sync(device)
        gx.close()
    _sync(device)
    got = [got] if isinstance(got, torch.Tensor) else list(got)
    ln = _host(got.pop(0))
    src = _host(got.pop(0)) if want_src else None
    st, en = (_host(got[0]), _host(got[1])) if want_interval else (None, None)
    return ln, src, st, en


def _sync(device):
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()


def same(a, b):
    """len, start, end equal (src is arbitrary by contract)."""
    return all(np.array_equal(a[k], b[k]) for k in (0, 2, 3))


# ---- the cases of both suites --------------------------------------------------------------------------------------
def known_answer(eng, device, fn):
    sa = SuffixTable.new_naive(BANANA_T, engine=eng).table()
    for route in ROUTES:
        res = run(eng, device, route, BANANA_T, sa, BANANA_Q)
        for k, name in ((0, "len"), (2, "start"), (3, "end")):
            assert res[k].tolist() == BANANA[name], (route, name, res[k].tolist())
        accept(fn, BANANA_T, sa, BANANA_Q, 0, res)
    assert _repeats.span_reference(BANANA["len"], 2) == BANANA_SPANS_2
    st = SuffixTable(BANANA_T, engine=eng)
    ln, src, a, e = st.match_stats(BANANA_Q.decode(), with_source=True, with_intervals=True)
    assert (ln.tolist(), a.tolist(), e.tolist()) == (BANANA["len"], BANANA["start"], BANANA["end"])
    assert all((s == NONE) == (k == 0) and (k == 0 or BANANA_T[s:s + k] == BANANA_Q[i:i + k])
               for i, (s, k) in enumerate(zip(src.tolist(), ln.tolist())))
    assert st.match_stats(BANANA_Q).tolist() == BANANA["len"] and st.match_stats(BANANA_Q, max_len=2).tolist() == [min(k, 2) for k in BANANA["len"]]
    assert st.shared_spans(BANANA_Q, 2) == BANANA_SPANS_2
    g = GeneralizedSuffixTable([BANANA_T], engine=eng)
    assert g.match_stats(BANANA_Q).tolist() == BANANA["len"] and g.shared_spans(BANANA_Q, 2) == BANANA_SPANS_2
    g2 = GeneralizedSuffixTable([b"ban", b"", b"ana"], engine=eng)          # no match crosses the end of "ban"
    assert g2.match_stats(b"banana").tolist() == [3, 3, 2, 3, 2, 1] and g2.shared_spans(b"banana", 3) == [(0, 6)]
    for bad in (0, -1):
        try:
            st.shared_spans(BANANA_Q, bad)
            raise RuntimeError("shared_spans accepted min_len < 1")
        except ValueError:
            pass


def random_pair(rng):
    sigma = rng.randint(1, 4)
    alpha = rng.sample([0, 97, 98, 255, 65, 10], sigma + 1)
    text = bytes(rng.choice(alpha[:sigma]) for _ in range(rng.randint(1, 60)))
    query = bytes(rng.choice(alpha) for _ in range(rng.randint(1, 60)))
    if rng.random() < 0.5:                                                # plant a piece of the text
        a = rng.randrange(len(text))
        piece = text[a:a + rng.randint(1, 20)]
        at = rng.randrange(len(query))
        query = (query[:at] + piece + query[at:])[:60]
    return text, query


CAPS = (0, 1, 3, 7)


def small_random_pairs(eng, device, fn, iters=300, seed=20261018):
    """Random pairs against the brute-force definition, the routes alternating; every tenth also through the checker's
    self-test.  -> the number of mutations the checker rejected."""
    rng = random.Random(seed)
    rejected = 0
    for it in range(iters):
        text, query = random_pair(rng)
        sa = SuffixTable.new_naive(text, engine=eng).table()
        cap = CAPS[it % 4]
        kind = it % 3
        if kind == 2:
            with _cases.general_build(eng):
                assert np.array_equal(SuffixTable(text, engine=eng).table(), sa)
                res = run(eng, device, "index_dev", text, sa, query, cap)
        else:
            res = run(eng, device, ("dev", "index_dev")[kind], text, sa, query, cap)
        exp = brute(text, sa, query, cap)
        assert same(res, (exp[0], None, exp[1], exp[2])), (text, query, cap, [r.tolist() for r in res], [e.tolist() for e in exp])
        accept(fn, text, sa, query, cap, res)
        if it % 6 == 0:
            rejected += checker_self_test(fn, text, sa, query, cap, res, rng)
    return rejected


def small_random_collections(eng, device, fn, iters=120, seed=7):
    """Random collections of at most 80 bytes with queries cut from the joined documents ACROSS document ends."""
    rng = random.Random(seed)
    rejected = 0
    done = 0
    while done < iters:
        docs = _gsa.random_collection(rng, max_docs=12, max_len=12)
        text = b"".join(docs)
        if not 1 <= len(text) <= 80:
            continue
        g = GeneralizedSuffixTable.new_naive(docs, engine=eng)
        starts = _gsa.doc_starts(docs)
        a = rng.randrange(len(text))
        query = text[a:a + rng.randint(1, 40)] + bytes([rng.choice(b"ab\x00\xffz")]) + text[:rng.randint(0, 10)]
        cap = CAPS[done % 4]
        route = ("gindex_dev", "gindex_host")[done % 2]
        res = run(eng, device, route, text, g.table(), query, cap, starts=starts, da=g.doc_array())
        exp = brute(text, g.table(), query, cap, starts)
        assert same(res, (exp[0], None, exp[1], exp[2])), (docs, query, cap, [r.tolist() for r in res], [e.tolist() for e in exp])
        accept(fn, text, g.table(), query, cap, res, starts)
        if done % 6 == 0:
            rejected += checker_self_test(fn, text, g.table(), query, cap, res, rng, starts)
        done += 1
    return rejected


PLANTED = (7, 8, 9, 15, 16, 17, 24, 25)


def planted_text(rng):
    """A text over a..p and a query over q..z that shares with it exactly one stretch of every PLANTED length, each
    followed by a differing byte."""
    text = bytes(rng.choice(b"abcdefghijklmnop") for _ in range(700))
    query, at = b"", {}
    for k, L in enumerate(PLANTED):
        query += bytes(rng.choice(b"qrstuvwxyz") for _ in range(rng.randint(1, 5)))
        at[L] = len(query)
        a = 40 + 80 * k
        follow = text[a + L]
        query += text[a:a + L] + bytes([follow + 1 if follow < ord("p") else ord("a")])
    return text, query + b"z", at


def edges(eng, device, fn, orc):
    """The edge cases, one assertion each (every result also goes through the checker)."""
    def go(text, query, cap=0, route="dev"):
        sa = orc.sais(text) if len(text) else np.zeros(0, dtype=np.uint32)
        res = run(eng, device, route, text, sa, query, cap)
        if len(query):
            accept(fn, text, sa, query, cap, res)
        return res, sa

    for route in ROUTES:                                                   # n == 0
        res, _ = go(b"", b"abc", route=route)
        assert res[0].tolist() == [0] * 3 and res[1].tolist() == [NONE] * 3 and not res[2].any() and not res[3].any(), route
        res, _ = go(b"abc", b"", route=route)                              # m == 0
        assert all(a.size == 0 for a in res), route
    res, _ = go(b"x", b"xxyx")                                             # n == 1
    assert res[0].tolist() == [1, 1, 0, 1] and res[3].tolist() == [1, 1, 0, 1]
    rng = random.Random(3)
    t = bytes(rng.choice(b"ab") for _ in range(200))
    res, _ = go(t, t, 5)                                                   # Q = T, capped at 5
    assert res[0].tolist() == [min(5, 200 - i) for i in range(200)]
    res, _ = go(t, t + b"ab")                                              # Q longer than T and equal to it on all n bytes
    assert res[0][0] == 200 and (res[2][0], res[3][0]) != (0, 0)
    for k in (0, 57, 150):                                                 # Q = T[k:] plus one byte: the match runs to the end of the text
        for extra in (b"\x00", b"a", b"\xff"):
            res, sa = go(t, t[k:] + extra)
            assert res[0][0] == 200 - k and sa[res[2][0]:res[3][0]].tolist() == [k], (k, extra)
    res, _ = go(b"mnop" * 5, b"a")                                         # below every suffix: p == 0
    assert res[0].tolist() == [0]
    res, _ = go(b"mnop" * 5, b"pzq")                                       # above every suffix: p == n
    assert res[0].tolist() == [1, 0, 0]
    res, _ = go(b"a" * 300, b"a" * 40 + b"b" + b"a" * 10)                  # one run
    assert res[0].tolist() == list(range(40, 0, -1)) + [0] + list(range(10, 0, -1))
    assert res[3][0] - res[2][0] == 261 and res[3][39] - res[2][39] == 300
    text, query, at = planted_text(rng)
    un, sa = go(text, query)
    for L in PLANTED:                                                      # they cross the 8-byte compare step and the 16-byte key
        assert un[0][at[L]] == L, (L, un[0][at[L]])
    for L in PLANTED:
        for cap in (L - 1, L, L + 1):
            for route in ("dev", "index_dev"):
                res, _ = go(text, query, cap, route)
                assert np.array_equal(res[0], np.minimum(un[0], cap)), (L, cap, route)
    docs = [b"abcab", b"", b"zz", b"abcab", b"ab"]                         # an empty document and two identical ones
    g = GeneralizedSuffixTable.new_naive(docs, engine=eng)
    text, starts = b"".join(docs), _gsa.doc_starts(docs)
    for route in ("gindex_dev", "gindex_host"):
        res = run(eng, device, route, text, g.table(), b"abcabzzab", starts=starts, da=g.doc_array())
        accept(fn, text, g.table(), b"abcabzzab", 0, res, starts)
        assert res[0].tolist() == [5, 4, 3, 2, 1, 2, 1, 2, 1] and res[3][0] - res[2][0] == 2, route


def directory_texts(eng, device, fn, orc, scale=1):
    """Every text of _cases.directory_texts() against the concatenation of its adversarial query list: the index entry
    and the undirected entry agree and the checker accepts, uncapped and at max_len = 12."""
    rng = np.random.default_rng(11)
    for text in _cases.directory_texts(scale):
        sa = orc.sais(text)
        query = b"".join(_cases.directory_query_list(text, rng))
        dt, dsa, dq = _t(text, device), _t(sa, device, np.uint32), _t(query, device)
        ix = sdev.DeviceIndex(dt, dsa, engine=eng)
        for cap in (0, 12):
            a = [_host(x) for x in ix.match_stats(dq, max_len=cap, want_src=True, want_interval=True)]
            b = [_host(x) for x in sdev.match_stats(dt, dsa, dq, max_len=cap, want_src=True, want_interval=True, engine=eng)]
            _sync(device)
            assert same(a, b), (len(text), cap)
            accept(fn, text, sa, query, cap, a)
            accept(fn, text, sa, query, cap, b)
        ix.close()


def buffers_and_streams(eng, device, fn, orc):
    """Q at odd byte offsets, every output at an odd u32 offset between guard bands, a side stream, every combination of
    the optional outputs, two threads on one index, and the refusals."""
    rng = random.Random(5)
    text = bytes(rng.choice(b"acgt") for _ in range(3000))
    sa = orc.sais(text)
    query = b"".join(text[a:a + rng.randint(1, 30)] + b"n" for a in (rng.randrange(3000) for _ in range(40)))
    m = len(query)
    t, s = _buffers.text_in(text, device, 3), _buffers.inp(sa, device, 4)
    ix = sdev.DeviceIndex(t.u8(), s.view(torch.int32), engine=eng)
    ds = np.zeros(1, dtype=np.int64)
    d_starts, d_da = _buffers.inp(ds, device), _buffers.inp(np.zeros(len(text), dtype=np.uint32), device, 8)
    gx = sdev.GeneralizedDeviceIndex(t.u8(), d_starts.view(torch.int64), s.view(torch.int32), d_da.view(torch.int32), engine=eng)
    exp = run(eng, device, "dev", text, sa, query)
    accept(fn, text, sa, query, 0, exp)
    side = torch.cuda.Stream() if str(device).startswith("cuda") else None

    def call(route, q, outs, stream, max_len=0):
        if route == "dev":
            return eng.lib.sfx_match_stats_dev(t.ptr, len(text), s.ptr, q.ptr, m, max_len, *outs, stream)
        fnc = eng.lib.sfx_index_match_stats_dev if route == "index_dev" else eng.lib.sfx_gindex_match_stats_dev
        return fnc(ix._h if route == "index_dev" else gx._h, q.ptr, m, max_len, *outs, stream)

    combos = [(qo, fill, ws, wi) for qo, fill in zip((1, 3, 5, 9), (0xA5, 0xA5, "count", 0xA5)) for ws in (False, True) for wi in (False, True)]
    for k, (qo, fill, want_src, want_iv) in enumerate(combos):
        route = ("dev", "index_dev", "gindex_dev")[k % 3]
        q = _buffers.text_in(query, device, qo)
        bufs = [_buffers.guarded(4 * m, device, off, fill) for off in (4, 12, 4, 12)]     # odd u32 offsets behind a 16-byte boundary
        outs = [b.ptr if want else None for b, want in zip(bufs, (True, want_src, want_iv, want_iv))]
        with (torch.cuda.stream(side) if side is not None and k % 2 else contextlib.nullcontext()):
            assert call(route, q, outs, _buffers.stream_of(device)) == OK, (route, qo)
            for b in bufs:
                b.check_guards(route)
            q.check_guards("query")
            got = [b.host(np.uint32) for b in bufs]
        before = _buffers.guarded(4 * m, device, 4, fill).host(np.uint32)
        for j, want in enumerate((True, want_src, want_iv, want_iv)):
            if not want:
                assert np.array_equal(got[j], before), (route, j, "an output that was not asked for was written")
            elif j != 1:
                assert np.array_equal(got[j], exp[j]), (route, qo, j)
        if want_src and want_iv:
            accept(fn, text, sa, query, 0, got)
    t.check_guards("text")
    s.check_guards("sa")

    # two threads on one index, different Q at the same time (on the emulator: one after the other)
    qs = [query, query[::-1]]
    exps = [exp, run(eng, device, "dev", text, sa, qs[1])]
    results, errors = [None, None], []

    def worker(k):
        try:
            for _ in range(3):
                results[k] = run_on_index(ix, qs[k], device)
        except Exception as e:                                             # noqa: BLE001 (reported below)
            errors.append(e)
    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    concurrent = str(device).startswith("cuda")      # (the emulator keeps threadIdx & co. in globals: one launch at a time)
    for th in threads:
        th.start()
        if not concurrent:
            th.join()
    for th in threads:
        th.join()
    assert not errors, errors
    for k in range(2):
        assert same(results[k], exps[k]), k

    # the refusals: nothing is written
    q = _buffers.text_in(query, device, 1)
    bufs = [_buffers.guarded(4 * m, device, 4, 0xA5) for _ in range(4)]
    p = [b.ptr for b in bufs]
    st = _buffers.stream_of(device)
    for route in ("dev", "index_dev", "gindex_dev"):
        assert call(route, q, [p[0], p[1], None, p[3]], st) == ERR_ARG, route
        assert call(route, q, [p[0], p[1], p[2], None], st) == ERR_ARG, route
        assert call(route, q, [None, p[1], p[2], p[3]], st) == ERR_ARG, route
    assert eng.lib.sfx_match_stats_dev(None, 0, None, None, 1 << 32, 0, None, None, None, None, None) == ERR_TOO_LARGE
    assert eng.lib.sfx_index_match_stats_dev(ix._h, None, 1 << 32, 0, None, None, None, None, None) == ERR_TOO_LARGE
    assert eng.lib.sfx_gindex_match_stats_dev(gx._h, None, 1 << 32, 0, None, None, None, None, None) == ERR_TOO_LARGE
    assert eng.lib.sfx_index_match_stats(ix._h, None, 1 << 32, 0, None, None, None, None) == ERR_TOO_LARGE
    assert eng.lib.sfx_gindex_match_stats(gx._h, None, 1 << 32, 0, None, None, None, None) == ERR_TOO_LARGE
    for b in bufs:
        assert (b.host() == 0xA5).all()
        b.check_guards("refused")
    _sync(device)
    ix.close()
    gx.close()


def index_route_threshold(eng, device, fn, orc):
    """The index entry enters through the bucket directory unless the cap leaves no position the directory's k symbols:
    3000 bytes over 4 symbols give 2-bit codes and a 10-bit key (log2 n - 2), k = 5.  Both sides of that threshold, in
    the launch names and against the undirected entry."""
    rng = random.Random(8)
    text = bytes(rng.choice(b"acgt") for _ in range(3000))
    sa = orc.sais(text)
    query = b"".join(text[a:a + rng.randint(1, 12)] + rng.choice([b"", b"n", b"a"]) for a in (rng.randrange(3000) for _ in range(60)))
    for cap, want in ((4, "ms_search"), (5, "ms_search_dir"), (0, "ms_search_dir")):
        got = {}
        names = _gsa.profile_names(eng, lambda: got.update(r=run(eng, device, "index_dev", text, sa, query, cap)))
        assert want in names and not ({"ms_search", "ms_search_dir", "ms_gsa_search"} - {want}) & names, (cap, sorted(names))
        assert same(got["r"], run(eng, device, "dev", text, sa, query, cap)), cap
        accept(fn, text, sa, query, cap, got["r"])
    names = _gsa.profile_names(eng, lambda: run(eng, device, "dev", text, sa, query))
    assert "ms_search" in names and "ms_search_dir" not in names, sorted(names)
    names = _gsa.profile_names(eng, lambda: run(eng, device, "gindex_dev", text, sa, query))
    assert "ms_gsa_search" in names and not {"ms_search", "ms_search_dir"} & names, sorted(names)


def run_on_index(ix, query, device):
    dq = _t(query, device)
    got = ix.match_stats(dq, want_src=True, want_interval=True)
    _sync(device)
    return [_host(x) for x in got]


def cli_files(tmp_path):
    """Two small files with a planted 100-byte and a planted 31-byte common stretch -> (path1, path2, a100, a31): the
    stretches' offsets in file 2."""
    rng = random.Random(9)
    one = bytes(rng.choice(b"abcdefgh") for _ in range(2000))
    two = bytearray(rng.choice(b"stuvwxyz") for _ in range(1500))
    two[200:300] = one[500:600]
    two[900:931] = one[1200:1231]
    p1, p2 = os.path.join(str(tmp_path), "one.txt"), os.path.join(str(tmp_path), "two.txt")
    with open(p1, "wb") as f:
        f.write(one)
    with open(p2, "wb") as f:
        f.write(bytes(two))
    return p1, p2, (200, 300, 500), (900, 931, 1200)
