"""The cases of the k-mismatch pattern search (sfx_hamming_dev, sfx_index_hamming*, sfx_gindex_hamming*; DESIGN.md
section 22), shared by test_hamming_emu.py (the emulator build, host memory) and test_gpu_hamming.py (libsuffix_hip.so,
HBM).

Nothing expected comes from the engine under test alone: small inputs are held against `brute`, the definition as a
double loop (ordering from the owning piece and the table of the oracle / of new_naive); larger ones go through the
serial checker tests/hm_check.c (every triple is an occurrence with the stated count, owners ascend, nothing twice, first
consistent, full window counts for the patterns marked complete); runs of one letter have closed-form answers."""
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
import _match
import _mem
from suffix_amd import GeneralizedSuffixTable, SuffixHipError, SuffixTable
from suffix_amd import device as sdev

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
OK, ERR_ARG, ERR_TOO_LARGE, ERR_WORKSPACE = 0, 1, 2, 5
KERNELS = {"hm_pieces", "hm_guard", "hm_cand", "hm_count", "hm_emit", "hm_first"}
ROUTES = ("dev", "index_dev", "gindex_dev", "index_host", "gindex_host")
TILE = 2048                                                     # K of a hook-free build
KS = (0, 1, 2, 3, 7)
UNWRITTEN32, UNWRITTEN8 = 0xA5A5A5A5, 0xA5
_vp, _u64, _u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
_np, _t, _sync = _match._np, _match._t, _match._sync


def build_emulator():
    """`make -C tests/emu`; sfx_hamming.hip is compiled as part of sfx_api.hip's translation unit and tests/emu/Makefile
    does not name it, so after an edit to it alone sfx_api.hip is declared new (`make -W`).  -> the library's path."""
    lib = os.path.join(EMU_DIR, "libsuffix_emu.so")
    cmd = ["make", "-s", "-j8", "-C", EMU_DIR]
    csrc = os.path.join(HERE, os.pardir, "suffix_amd", "csrc")
    newest = max(os.path.getmtime(os.path.join(csrc, f)) for f in ("sfx_hamming.hip", "sfx_mem.hip"))
    if os.path.exists(lib) and newest > os.path.getmtime(lib):
        cmd += ["-W", _mem.CSRC_FROM_EMU + "/sfx_api.hip"]
    subprocess.check_call(cmd)
    return lib


# ---- the definition --------------------------------------------------------------------------------------------------
def cuts(m, k):
    """b_0 .. b_(k+1): piece t of a pattern of m bytes is [b_t, b_(t+1))."""
    return [t * m // (k + 1) for t in range(k + 2)]


def brute(text, starts, patterns, k, sa):
    """The occurrences by the definition: every window of every pattern, its mismatches, its owning piece (the first
    piece that matches exactly; an empty one does).  -> ([(pattern, tpos, mism)], first) ordered by pattern, owning
    piece and the rank in `sa` of tpos + b_owner."""
    text = bytes(text)
    n = len(text)
    t = np.frombuffer(text, dtype=np.uint8)
    _, hi = _mem._doc_bounds(n, starts)
    rank = np.zeros(n, dtype=np.int64)
    rank[np.asarray(sa, dtype=np.int64)] = np.arange(n)
    out, first = [], [0]
    for j, pat in enumerate(patterns):
        m = len(pat)
        if 1 <= m <= n:
            p = np.frombuffer(bytes(pat), dtype=np.uint8)
            diff = np.lib.stride_tricks.sliding_window_view(t, m) != p            # (n - m + 1, m)
            mism = diff.sum(axis=1)
            pos = np.arange(n - m + 1)
            ok = (pos + m <= hi[:n - m + 1]) & (mism <= k)
            b = cuts(m, k)
            found = []
            for w in pos[ok].tolist():
                owner = next(s for s in range(k + 1) if not diff[w, b[s]:b[s + 1]].any())
                found.append((owner, int(rank[w + b[owner]]), w, int(mism[w])))
            out += [(j, w, c) for _, _, w, c in sorted(found)]
        first.append(len(out))
    return out, first


# hand-worked.  T = "banana": table 5 3 1 0 4 2 (a, ana, anana, banana, na, nana).
#   "ana", k = 0: one piece, interval [1, 3) = positions 3, 1.
#   "ana", k = 1: pieces "a" | "na"; both windows match piece 0 exactly, so piece 0 owns them: the ranks of "a" are
#       [0, 3) = positions 5 (no room), 3, 1 -> (3, 0), (1, 0); the candidates of "na" at 4, 2 give the same windows
#       and are dropped (piece 0 matches there).
#   "bna", k = 1: pieces "b" | "na": "b" at 0 -> window 0 "ban" differs in 2 bytes: dropped; "na" at 4, 2 -> windows
#       3, 1 = "ana" with piece 0 mismatching and 1 mismatch in all: (3, 1), (1, 1) owned by piece 1, rank of "na" (4)
#       < "nana" (5).
#   T = "abcabd" (table 0 3 1 4 2 5: abcabd, abd, bcabd, bd, cabd, d), "abd", k = 1: pieces "a" | "bd": piece 0 at
#       ranks 0, 1 = positions 0, 3: window 0 "abc" 1 mismatch, window 3 "abd" 0 -> (0, 1), (3, 0) in rank order.
HAND = [
    (b"banana", [b"ana"], 0, [(0, 3, 0), (0, 1, 0)]),
    (b"banana", [b"ana"], 1, [(0, 3, 0), (0, 1, 0)]),
    (b"banana", [b"bna"], 1, [(0, 3, 1), (0, 1, 1)]),
    (b"abcabd", [b"abd"], 1, [(0, 0, 1), (0, 3, 0)]),
    (b"banana", [b"", b"x", b"nan", b"bananas"], 1, [(1, 5, 1), (1, 3, 1), (1, 1, 1), (1, 0, 1), (1, 4, 1), (1, 2, 1), (2, 2, 0), (2, 0, 1)]),
]


def naive_table(text):
    return np.array(sorted(range(len(text)), key=lambda p: text[p:]), dtype=np.uint32)


# ---- the checker -------------------------------------------------------------------------------------------------------
def build_checker(out_dir):
    """tests/hm_check.c -> a shared object in out_dir, bound (with OpenMP for the full counts where the compiler has it)."""
    so = os.path.join(str(out_dir), "libhm_check.so")
    base = ["gcc", "-O2", "-std=c99", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "hm_check.c")]
    if subprocess.call(base + ["-fopenmp"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)
    lib = ctypes.CDLL(so)
    lib.hm_check.restype = ctypes.c_int
    lib.hm_check.argtypes = [_vp, _u64, _vp, _u64, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _u64, _vp, _vp, ctypes.POINTER(ctypes.c_int64)]
    lib.hm_check_name.restype = ctypes.c_char_p
    lib.hm_check_name.argtypes = [ctypes.c_int]
    return lib


def pack(patterns):
    """-> (qbytes with one spare byte, qoff uint64)."""
    qs = [bytes(p) for p in patterns]
    off = np.zeros(len(qs) + 1, dtype=np.uint64)
    if qs:
        off[1:] = np.cumsum([len(q) for q in qs], dtype=np.uint64)
    return np.frombuffer(b"".join(qs) + b"\x00", dtype=np.uint8), off


def check(chk, text, starts, patterns, k, res, complete=None):
    """res = (first, pattern, tpos, mism, ...).  -> (fault name, index)."""
    t = _np(text, np.uint8)
    qb, qoff = pack(patterns)
    ds = None if starts is None else _np(starts, np.uint64)
    first, pat, tpos, mism = _np(res[0], np.uint64), _np(res[1], np.uint32), _np(res[2], np.uint32), _np(res[3], np.uint8)
    assert first.size == len(patterns) + 1 and pat.size == tpos.size == mism.size
    comp = None if complete is None else _np(complete, np.uint8)
    where = ctypes.c_int64(-2)
    rc = chk.hm_check(_gsa.ptr(t), t.size, _gsa.ptr(ds) if ds is not None else None, 0 if ds is None else ds.size, _gsa.ptr(qb),
                      _gsa.ptr(qoff), len(patterns), int(k), _gsa.ptr(pat), _gsa.ptr(tpos), _gsa.ptr(mism), pat.size, _gsa.ptr(first),
                      _gsa.ptr(comp) if comp is not None else None, ctypes.byref(where))
    return chk.hm_check_name(rc).decode(), int(where.value)


def accept(chk, text, starts, patterns, k, res, complete=None):
    name, where = check(chk, text, starts, patterns, k, res, complete)
    assert name == "ok", f"hm_check: {name} at {where} (k {k})"


def _cols(trip, nq):
    pat = np.array([x[0] for x in trip], dtype=np.uint32)
    first = np.searchsorted(pat, np.arange(nq + 1)).astype(np.uint64)
    return first, pat, np.array([x[1] for x in trip], dtype=np.uint32), np.array([x[2] for x in trip], dtype=np.uint8)


def checker_self_test(chk):
    """One fault per rule: every one is named, at the item that is wrong."""
    text, pats, k = b"abcabdabc_abd", [b"abd", b"abc"], 1
    good, first = brute(text, None, pats, k, naive_table(text))
    assert sorted(x[:2] for x in good) == [(0, 0), (0, 3), (0, 6), (0, 10), (1, 0), (1, 3), (1, 6), (1, 10)] and first == [0, 4, 8], good
    all1 = [1, 1]
    assert check(chk, text, None, pats, k, _cols(good, 2), all1) == ("ok", -1)
    g = list(good)
    faults = [
        (g[:2] + [(g[2][0], g[2][1], g[2][2] ^ 1)] + g[3:], "count", 2, None),        # a wrong count
        (g[:3] + [g[2]] + g[4:], "duplicate", 3, None),                               # a duplicate in place of another
        (g[:3] + g[4:], "missing", 0, None),                                           # a missing occurrence
        (g[:4] + [(1, 1, 3)] + g[5:], "mismatches", 4, None),                          # "bca" against "abc": 3 > k
        (g[:4] + [(1, 11, 1)] + g[5:], "range", 4, None),
    ]
    for trip, want, at, note in faults:
        cols = _cols(sorted(trip, key=lambda x: x[0]), 2)
        got = check(chk, text, None, pats, k, cols, all1)
        assert got == (want, at), (trip, got, want, at)
    # first: not monotone, a wrong total, a triple filed under another pattern
    f, p, t, m = _cols(good, 2)
    bad = f.copy(); bad[1] = 9
    assert check(chk, text, None, pats, k, (bad, p, t, m))[0] == "first"
    bad = f.copy(); bad[2] = 7
    assert check(chk, text, None, pats, k, (bad, p, t, m))[0] == "first"
    bad = f.copy(); bad[1] = 5
    assert check(chk, text, None, pats, k, (bad, p, t, m)) == ("first", 4)
    # a window across a document end; the same list is fine when the documents allow it
    assert check(chk, b"abcd", [0, 2], [b"bc"], 0, _cols([(0, 1, 0)], 1)) == ("document", 0)
    assert check(chk, b"abcd", [0, 1], [b"bc"], 0, _cols([(0, 1, 0)], 1), [1]) == ("ok", -1)
    assert check(chk, b"abcd", [0, 2, 2], [b"cd", b"ab"], 1, _cols([(0, 2, 0), (1, 0, 0)], 2), [1, 1]) == ("ok", -1)
    # a wrong owner order: "abxd" against T = "abcd_xbxd": window 0 is owned by piece 0 ("ab"), window 5 by piece 1 ("xd")
    text, pats = b"abcd_xbxd", [b"abxd"]
    good, _ = brute(text, None, pats, 1, naive_table(text))
    assert good == [(0, 0, 1), (0, 5, 1)]
    assert check(chk, text, None, pats, 1, _cols(good, 1), [1]) == ("ok", -1)
    assert check(chk, text, None, pats, 1, _cols(good[::-1], 1), [1]) == ("owner order", 1)
    return len(faults) + 6


# ---- the entry points ------------------------------------------------------------------------------------------------
def _as_collection(n, starts, da):
    return _mem._as_collection(n, starts, da)


def run(eng, device, route, text, sa, patterns, k, starts=None, da=None, max_cands=1 << 30):
    """One entry point -> (first uint64, pattern uint32, tpos uint32, mism uint8, C) on the host.  The gindex routes of a
    plain text see it as one document.  A refusal raises SuffixHipError."""
    n = len(text)
    qb, qoff = pack(patterns)
    nq = len(patterns)
    if route.startswith("gindex"):
        starts, da = _as_collection(n, starts, da)
    else:
        assert starts is None
    if route.endswith("_host"):
        t, s = _np(text, np.uint8), _np(sa, np.uint32)
        h = ctypes.c_void_p()
        if route == "index_host":
            assert eng.lib.sfx_index_create(_gsa.ptr(t), n, _gsa.ptr(s), ctypes.byref(h)) == OK
            call, destroy = eng.lib.sfx_index_hamming, eng.lib.sfx_index_destroy
        else:
            ds, d = _np(starts, np.uint64), _np(da, np.uint32)
            assert eng.lib.sfx_gindex_create(_gsa.ptr(t), n, _gsa.ptr(ds), ds.size, _gsa.ptr(s), _gsa.ptr(d), ctypes.byref(h)) == OK
            call, destroy = eng.lib.sfx_gindex_hamming, eng.lib.sfx_gindex_destroy
        cands, count = _u64(0), _u64(0)
        first = np.full(nq + 1, 0xDEADBEEF, dtype=np.uint64)
        try:
            rc = call(h, _gsa.ptr(qb), _gsa.ptr(qoff), nq, k, max_cands, None, None, None, 0, _gsa.ptr(first), ctypes.byref(cands),
                      ctypes.byref(count))
            assert rc == OK, (route, rc)
            if cands.value > max_cands:
                raise SuffixHipError(f"refused: {cands.value} candidates")
            z = int(count.value)
            assert int(first[nq]) == z, (route, first, z)                    # (complete at capacity 0)
            f0 = first.copy()
            out = [np.full(z + 3, 0xDEADBEEF, dtype=np.uint32) for _ in range(2)] + [np.full(z + 3, 0xEF, dtype=np.uint8)]
            rc = call(h, _gsa.ptr(qb), _gsa.ptr(qoff), nq, k, max_cands, *[_gsa.ptr(a) for a in out], z + 3, _gsa.ptr(first),
                      ctypes.byref(cands), ctypes.byref(count))
            assert rc == OK and count.value == z and np.array_equal(first, f0), (route, rc, z, count.value)
        finally:
            destroy(h)
        assert (out[0][z:] == 0xDEADBEEF).all() and (out[1][z:] == 0xDEADBEEF).all() and (out[2][z:] == 0xEF).all(), (route, "written past z")
        return first, out[0][:z], out[1][:z], out[2][:z], int(cands.value)
    dt, dsa = _t(text, device), _t(sa, device, np.uint32)
    dq, doff = _t(qb, device), _t(qoff.astype(np.int64), device, np.int64)
    if route == "dev":
        got = sdev.hamming(dt, dsa, dq, doff, k, max_candidates=max_cands, engine=eng)
    elif route == "index_dev":
        ix = sdev.DeviceIndex(dt, dsa, engine=eng)
        try:
            got = ix.hamming(dq, doff, k, max_candidates=max_cands)
        finally:
            _sync(device)
            ix.close()
    else:
        gx = sdev.GeneralizedDeviceIndex(dt, _t(starts, device, np.int64), dsa, _t(da, device, np.uint32), engine=eng)
        try:
            got = gx.hamming(dq, doff, k, max_candidates=max_cands)
        finally:
            _sync(device)
            gx.close()
    _sync(device)
    return (got[0].cpu().numpy().view(np.uint64), got[1].cpu().numpy().view(np.uint32), got[2].cpu().numpy().view(np.uint32),
            got[3].cpu().numpy(), got[4])


def triples(res):
    return list(zip(res[1].tolist(), res[2].tolist(), res[3].tolist()))


def same_as_brute(res, want, route=None, note=None):
    trip, first = want
    assert triples(res) == trip and res[0].tolist() == first, (route, note, triples(res)[:12], trip[:12], res[0].tolist()[:8], first[:8])


def exact_intervals(eng, device, text, sa, patterns):
    """sa[start .. end) of sfx_index_query_dev per pattern, as the k = 0 triples."""
    qb, qoff = pack(patterns)
    ix = sdev.DeviceIndex(_t(text, device), _t(sa, device, np.uint32), engine=eng)
    try:
        start, end, _, _ = ix.query(_t(qb, device), _t(qoff.astype(np.int64), device, np.int64))
        _sync(device)
        s, e = start.cpu().numpy().view(np.uint32), end.cpu().numpy().view(np.uint32)
    finally:
        _sync(device)
        ix.close()
    sa = np.asarray(sa, dtype=np.uint32)
    trip, first = [], [0]
    for j, pat in enumerate(patterns):
        if len(pat):                                                         # (the empty pattern: every rank for the exact search, no occurrence here)
            trip += [(j, int(p), 0) for p in sa[int(s[j]):int(e[j])]]
        first.append(len(trip))
    return trip, first


# ---- patterns ----------------------------------------------------------------------------------------------------------
def make_patterns(rng, text, k, count, lo=0, hi=40, alphabet=None):
    """Sampled from the text with 0 .. k + 2 planted substitutions, sampled with one inserted byte, or random."""
    alphabet = alphabet or sorted(set(text)) + [1]
    n, out = len(text), []
    for _ in range(count):
        m = rng.randint(lo, hi)
        x = rng.random()
        if x < 0.6 and n:
            a = rng.randrange(n)
            p = bytearray(text[a:a + m])
            for _ in range(rng.randint(0, k + 2)):
                if p:
                    p[rng.randrange(len(p))] = rng.choice(alphabet)
        elif x < 0.8 and n:
            a = rng.randrange(n)
            p = bytearray(text[a:a + m])
            p.insert(rng.randint(0, len(p)), rng.choice(alphabet))
        else:
            p = bytearray(rng.choice(alphabet) for _ in range(m))
        out.append(bytes(p))
    return out


# ---- 1. against the definition ---------------------------------------------------------------------------------------------
def known_answers(eng, device):
    for text, pats, k, want in HAND:
        sa = naive_table(text)
        got = brute(text, None, pats, k, sa)
        assert got[0] == want, (text, pats, k, got[0])
        for route in ROUTES:
            same_as_brute(run(eng, device, route, text, sa, pats, k), got, route, (text, pats, k))
    # the host API
    t = SuffixTable(b"banana", engine=eng)
    pos, mm = t.approx_positions(b"ana", 0)
    assert pos.dtype == np.uint32 and mm.dtype == np.uint8 and pos.tolist() == [1, 3] and mm.tolist() == [0, 0]
    pos, mm = t.approx_positions("bna", 1)
    assert pos.tolist() == [1, 3] and mm.tolist() == [1, 1]
    first, tpos, mm = t.approx_positions_batch([b"ana", b"", b"bna"], 1)
    assert first.dtype == np.uint64 and first.tolist() == [0, 2, 2, 4] and tpos.tolist() == [3, 1, 3, 1] and mm.tolist() == [0, 0, 1, 1]
    first, tpos, mm = t.approx_positions_batch([b"ana", b"", b"bna"], 1, sort=True)
    assert first.tolist() == [0, 2, 2, 4] and tpos.tolist() == [1, 3, 1, 3] and mm.tolist() == [0, 0, 1, 1]
    assert t.approx_positions_batch([], 1)[0].tolist() == [0] and SuffixTable(b"", engine=eng).approx_positions(b"a", 1)[0].size == 0
    try:
        SuffixTable(b"aaaaaaaa", engine=eng).approx_positions_batch([b"aaaa"], 1, max_candidates=13)
        raise AssertionError("14 candidates were not refused at max_candidates = 13")
    except SuffixHipError as e:
        assert "14" in str(e) and "13" in str(e), e
    assert SuffixTable(b"aaaaaaaa", engine=eng).approx_positions_batch([b"aaaa"], 1, max_candidates=14)[1].tolist() == [4, 3, 2, 1, 0]
    for bad in (-1, 256):
        try:
            t.approx_positions(b"a", bad)
            raise AssertionError("mismatches out of range accepted")
        except ValueError:
            pass
    g = GeneralizedSuffixTable([b"abc", b"", b"bcd", b"c"], engine=eng)
    pos, mm = g.approx_positions(b"bcd", 1)
    assert pos.tolist() == [3] and mm.tolist() == [0]                       # ("bcb" at 1 would cross into the third document)
    pos, mm = g.approx_positions(b"bd", 1)
    assert pos.tolist() == [1, 3, 4] and mm.tolist() == [1, 1, 1]
    many = SuffixTable(b"ab" * 3000, engine=eng).approx_positions_batch([b"abab"], 1)      # more than the first guess at the room
    assert many[0].tolist() == [0, 2999] and sorted(many[1].tolist()) == list(range(0, 5998, 2))


def small_random_texts(eng, device, chk, iters=160, seed=20261019, routes=ROUTES):
    """Texts over 1 / 2 / 4 / 256 symbols, n <= 400, patterns of 0 .. 40 bytes; the routes and k alternate.  Every text
    is also answered at k = 0 and held against sa[start .. end) of sfx_index_query_dev.  -> the number of texts."""
    rng = random.Random(seed)
    for it in range(iters):
        sigma = (1, 2, 4, 256)[it % 4]
        alpha = list(range(256)) if sigma == 256 else rng.sample([0, 97, 98, 255, 65, 10], sigma)
        n = rng.choice((1, 2, 7, 40, 150, 400)) if it % 5 == 0 else rng.randint(1, 400)
        text = bytes(rng.choice(alpha) for _ in range(n))
        if sigma == 256 and n > 50:                                           # repeats, so that planted patterns have several windows
            text = (text[:n // 3] * 3 + text)[:n]
        sa = naive_table(text)
        k = KS[(it // 4) % len(KS)]
        pats = make_patterns(rng, text, k, 7, alphabet=alpha + [1]) + [b""]
        route = routes[it % len(routes)]
        res = run(eng, device, route, text, sa, pats, k)
        same_as_brute(res, brute(text, None, pats, k, sa), route, (it, text, pats, k))
        if it % 4 == 0:
            accept(chk, text, None, pats, k, res, [1] * len(pats))
        res0 = run(eng, device, route, text, sa, pats, 0)
        want0 = exact_intervals(eng, device, text, sa, pats)
        assert want0 == brute(text, None, pats, 0, sa), (it, text, pats)
        same_as_brute(res0, want0, route, (it, "k = 0"))
        assert all(c == 0 for c in res0[3].tolist())
    return iters


def small_random_collections(eng, device, chk, iters=60, seed=11):
    """Collections with empty and one-byte documents; patterns cut across document ends among them."""
    rng = random.Random(seed)
    done = empties = singles = 0
    while done < iters:
        docs = _gsa.random_collection(rng, max_docs=24, max_len=30)
        if done % 3 == 0:
            docs = docs + [bytes([rng.choice(docs[0] or b"a")])]
        text = b"".join(docs)
        if not 1 <= len(text) <= 400:
            continue
        empties += any(len(d) == 0 for d in docs)
        singles += any(len(d) == 1 for d in docs)
        g = GeneralizedSuffixTable.new_naive(docs, engine=eng)
        starts = _gsa.doc_starts(docs)
        k = KS[done % len(KS)]
        pats = make_patterns(rng, text, k, 6, hi=24) + [b""]
        for s in starts[1:4]:                                                 # across a document end
            pats.append(text[max(0, int(s) - 3):int(s) + 4])
        route = ("gindex_dev", "gindex_host")[done % 2]
        res = run(eng, device, route, text, g.table(), pats, k, starts=starts, da=g.doc_array())
        want = brute(text, starts, pats, k, g.table())
        same_as_brute(res, want, route, (docs, pats, k))
        accept(chk, text, starts, pats, k, res, [1] * len(pats))               # (no window crosses a document end)
        done += 1
    assert empties >= 5 and singles >= 5
    return done


# ---- 2. raw calls: capacity, limits, guards --------------------------------------------------------------------------------
def raw_call(raw, route, q, qoff, nq, k, limit, outs, cap, first, ws, ws_bytes, stream=None):
    """-> (status, C, Z); pointers as c_void_p or None.  raw: _mem.Raw (text, table, index and collection between guards)."""
    cands, count = _u64(0xAAAA), _u64(0xBBBB)
    tail = (q, qoff, nq, k, limit, *outs, cap, first, ctypes.byref(cands), ctypes.byref(count), ws, ws_bytes, stream)
    lib = raw.eng.lib
    if route == "dev":
        rc = lib.sfx_hamming_dev(raw.t.ptr, raw.n, raw.s.ptr, *tail)
    elif route == "index_dev":
        rc = lib.sfx_index_hamming_dev(raw.ix._h, *tail)
    else:
        rc = lib.sfx_gindex_hamming_dev(raw.gx._h, *tail)
    return rc, int(cands.value), int(count.value)


def guarded_call(raw, route, patterns, k, limit=None, cap=None, q_off=1, out_offs=(4, 12, 1), ws_fill="count", want_first=True):
    """One guarded call with a dirty workspace of exactly sfx_hamming_workspace_bytes -> (status, C, Z, pattern, tpos, mism,
    first) as they came back, all `cap` entries (first: None when not asked).  cap None: counts first, then exactly Z."""
    dev = raw.device
    qb, qoff = pack(patterns)
    nq = len(patterns)
    limit = max(1, nq * (k + 1) * raw.n) if limit is None else limit           # (no call has more: keeps the workspace small)
    q, qo = _buffers.inp(qb, dev, q_off), _buffers.inp(qoff, dev, 8)
    wsb = int(raw.eng.lib.sfx_hamming_workspace_bytes(nq, k, limit))
    ws = _buffers.guarded(wsb, dev, 0, ws_fill)
    st = _buffers.stream_of(dev)
    if cap is None:
        rc, c, z = raw_call(raw, route, q.ptr, qo.ptr, nq, k, limit, (None, None, None), 0, None, ws.ptr, wsb, st)
        assert rc == OK, (route, rc)
        cap = z
        ws.fill(ws_fill)
    bufs = [_buffers.guarded(4 * cap, dev, out_offs[0], 0xA5), _buffers.guarded(4 * cap, dev, out_offs[1], 0xA5),
            _buffers.guarded(cap, dev, out_offs[2], 0xA5)]
    fb = _buffers.guarded(8 * (nq + 1), dev, 8, 0xA5) if want_first else None
    rc, c, z = raw_call(raw, route, q.ptr, qo.ptr, nq, k, limit, [b.ptr if cap else None for b in bufs], cap,
                        fb.ptr if fb is not None else None, ws.ptr, wsb, st)
    for name, b in zip(("pattern", "tpos", "mism", "workspace", "qbytes", "qoff", "first"), bufs + [ws, q, qo] + ([fb] if fb is not None else [])):
        b.check_guards(f"{route} {name}")
    assert q.host().tobytes() == qb.tobytes() and np.array_equal(qo.host(np.uint64), qoff), "an input was written"
    return (rc, c, z, bufs[0].host(np.uint32), bufs[1].host(np.uint32), bufs[2].host(np.uint8),
            fb.host(np.uint64) if fb is not None else None)


def edges(eng, device, chk, orc):
    def one(text, pats, k, starts=None):
        docs = _match.doc_list(text, starts)
        if starts is None:
            sa, da = (orc.sais(text) if len(text) else np.zeros(0, dtype=np.uint32)), None
        else:
            g = GeneralizedSuffixTable.new_naive(docs, engine=eng)
            sa, da = g.table(), g.doc_array()
        want = brute(text, starts, pats, k, sa)
        for route in (ROUTES if starts is None else ("gindex_dev", "gindex_host")):
            same_as_brute(run(eng, device, route, text, sa, pats, k, starts=starts, da=da), want, route, (text, pats, k))
        return want[0]

    text = b"xabcdefghijklmnopqrstuvwxyz_abcdefghijklmnopqrstuvwxyy"
    n = len(text)
    for k in KS:
        # windows at p = 0 and p = n - m; m = 1, k, k + 1, k + 2 and lengths no multiple of k + 1; m > n
        pats = [text[:9], b"y" + text[1:9], text[n - 9:], text[n - 9:n - 1] + b"q", b"a", b"q", text[:k], text[3:3 + k + 1], text[3:3 + k + 2],
                text[5:5 + 2 * (k + 1) + 1], text[n - k - 2:], text + b"z", b"\x01\x02\x03\x04\x05\x06\x07\x08\x09"]
        w = one(text, pats, k)
        assert (0, 0, 0) in w and (2, n - 9, 0) in w
        if k:
            assert (1, 0, 1) in w and (3, n - 9, 1) in w and sum(1 for x in w if x[0] == 6) == n - k + 1       # (m = k occurs wherever there is room)
        assert not any(x[0] in (11, 12) for x in w)
    one(b"ab", [b"abc", b"ab", b"b", b""], 2)
    one(b"a", [b"a", b"b", b"aa"], 1)
    # documents: one of a single byte, empty ones, windows that would cross an end
    for k in (0, 1, 2):
        w = one(b"abcaxbc", [b"abca", b"bc", b"cax", b"a", b"xbc", b"xb", b""], k, starts=[0, 3, 3, 4, 4, 7])
        assert not any(x[0] == 0 for x in w) and ((2, 2, 0) not in w)
    # runs of 0x00 / 0xFF and the other directory texts (the small ones), patterns from them
    rng = random.Random(9)
    for text in _cases.directory_texts():
        if len(text) > 700:
            continue
        sa = orc.sais(text)
        for k in (1, 3):
            pats = make_patterns(rng, text, k, 6, lo=4, hi=40)
            res = run(eng, device, ("index_dev", "dev")[k // 2], text, sa, pats, k)
            same_as_brute(res, brute(text, None, pats, k, sa), None, (text[:20], k))
            accept(chk, text, None, pats, k, res, [1] * len(pats))

    # text and pattern buffers at every alignment 0 .. 7; capacity 0, below Z, exactly Z, above; first NULL; the limit
    rng = random.Random(3)
    text = bytes(rng.choice(b"ab") for _ in range(300))
    sa = orc.sais(text)
    k = 2
    pats = make_patterns(rng, text, k, 9, lo=6, hi=30, alphabet=[97, 98]) + [b"", b"ab"]
    want, wfirst = brute(text, None, pats, k, sa)
    Z = len(want)
    assert Z > 40
    col = lambda out, z: list(zip(out[3][:z].tolist(), out[4][:z].tolist(), out[5][:z].tolist()))
    for align in range(8):
        raw = _mem.Raw(eng, device, text, sa, text_off=align, sa_off=(4, 8, 12)[align % 3])
        for route in raw.routes():
            out = guarded_call(raw, route, pats, k, q_off=(align + 3) % 8)
            assert out[:3] == (OK, out[1], Z) and col(out, Z) == want and out[6].tolist() == wfirst, (route, align)
        C = out[1]
        if align in (0, 5):
            for route in raw.routes():
                out = guarded_call(raw, route, pats, k, cap=0)                 # counts only, output pointers NULL; first complete
                assert out[:3] == (OK, C, Z) and out[6].tolist() == wfirst, (route, out[:3])
                out = guarded_call(raw, route, pats, k, cap=Z - 1)             # (the guards stand behind the last written triple)
                assert out[:3] == (OK, C, Z) and col(out, Z - 1) == want[:-1] and out[6].tolist() == wfirst, route
                out = guarded_call(raw, route, pats, k, cap=Z + 5, want_first=False)
                assert out[:3] == (OK, C, Z) and col(out, Z) == want and out[6] is None, route
                assert (out[3][Z:] == UNWRITTEN32).all() and (out[4][Z:] == UNWRITTEN32).all() and (out[5][Z:] == UNWRITTEN8).all(), "written past Z"
                out = guarded_call(raw, route, pats, k, limit=C, cap=Z, ws_fill=0xFF)
                assert out[:3] == (OK, C, Z) and col(out, Z) == want, route
                out = guarded_call(raw, route, pats, k, limit=C - 1, cap=Z, ws_fill=0x00)    # refused: nothing is written
                assert out[:3] == (OK, C, 0), (route, out[:3])
                assert (out[3] == UNWRITTEN32).all() and (out[4] == UNWRITTEN32).all() and (out[5] == UNWRITTEN8).all(), route
                assert (out[6] == 0xA5A5A5A5A5A5A5A5).all(), (route, "first written after a refusal")
        raw.close()


# ---- 3. runs with closed-form answers --------------------------------------------------------------------------------------
def closed_forms(eng, device, sizes, routes=("dev", "index_dev", "gindex_dev")):
    """T = a^n.  a^32 at k = 1: two pieces a^16 with n - 15 hits each, C = 2 (n - 15), the n - 31 windows owned by piece
    0 with 0 mismatches, in table order (the table of a^n holds the shortest suffix first: n - 32 down to 0).
    a^31 b: piece 0 alone has hits, Z = n - 31 with 1 mismatch; none at k = 0.  b a^31: owner piece 1, Z = n - 31.
    A batch that mixes them with stretches of patterns without candidates in between."""
    A, AB, BA, B = b"a" * 32, b"a" * 31 + b"b", b"b" + b"a" * 31, b"b" * 20
    i = 0
    for n in sizes:
        text = b"a" * n
        sa = np.arange(n - 1, -1, -1, dtype=np.uint32)
        down = list(range(n - 32, -1, -1))
        for pats, k, C, want in (([A], 1, 2 * (n - 15), [(0, p, 0) for p in down]),
                                 ([AB], 1, n - 15, [(0, p, 1) for p in down]),
                                 ([AB], 0, 0, []),
                                 ([BA], 1, n - 15, [(0, p, 1) for p in down]),
                                 ([A, B, B, b"", B, BA, B, B, B, AB, B], 1, 4 * (n - 15),
                                  [(0, p, 0) for p in down] + [(5, p, 1) for p in down] + [(9, p, 1) for p in down])):
            route = routes[i % len(routes)]
            i += 1
            res = run(eng, device, route, text, sa, pats, k)
            assert res[4] == C, (route, n, pats[0][:3], k, res[4], C)
            assert triples(res) == want, (route, n, k, len(pats), triples(res)[:6], want[:6])
            first = [sum(1 for x in want if x[0] < j) for j in range(len(pats) + 1)]
            assert res[0].tolist() == first, (route, n, res[0].tolist(), first)


# ---- 4. buffers, streams, threads ------------------------------------------------------------------------------------------
def buffers_and_streams(eng, device, chk, orc):
    """The three entry points give identical bytes over offset buffers and the three kinds of workspace dirt, on a side
    stream too; two threads on one index at once."""
    rng = random.Random(5)
    text = bytes(rng.choice(b"acgt") for _ in range(3000))
    sa = orc.sais(text)
    k = 2
    pats = make_patterns(rng, text, k, 40, lo=12, hi=40, alphabet=list(b"acgt"))
    full = run(eng, device, "dev", text, sa, pats, k)
    accept(chk, text, None, pats, k, full, [1] * len(pats))
    Z = full[1].size
    assert Z >= 20
    side = torch.cuda.Stream() if str(device).startswith("cuda") else None
    j = 0
    for text_off, u32_off, fill in _buffers.combos():
        raw = _mem.Raw(eng, device, text, sa, text_off=text_off, sa_off=u32_off)
        for route in raw.routes():
            j += 1
            with (torch.cuda.stream(side) if side is not None and j % 2 else contextlib.nullcontext()):
                out = guarded_call(raw, route, pats, k, q_off=(1, 3, 5, 9)[j % 4], out_offs=(u32_off, 4, (0, 1, 2, 3)[j % 4]), ws_fill=fill)
            assert out[:3] == (OK, full[4], Z), (route, out[:3])
            assert all(np.array_equal(out[3 + c], full[1 + c]) for c in range(3)) and np.array_equal(out[6], full[0]), (route, text_off, fill)
        raw.close()

    dt, dsa = _t(text, device), _t(sa, device, np.uint32)
    ix = sdev.DeviceIndex(dt, dsa, engine=eng)
    sets = [pats, [p[::-1] for p in pats]]
    exps = [full, run(eng, device, "dev", text, sa, sets[1], k)]
    results, errors = [None, None], []

    def worker(w):
        try:
            qb, qoff = pack(sets[w])
            for _ in range(3):
                got = ix.hamming(_t(qb, device), _t(qoff.astype(np.int64), device, np.int64), k)
                _sync(device)
                results[w] = [got[0].cpu().numpy().view(np.uint64), got[1].cpu().numpy().view(np.uint32),
                              got[2].cpu().numpy().view(np.uint32), got[3].cpu().numpy(), got[4]]
        except Exception as e:                                             # noqa: BLE001 (reported below)
            errors.append(e)
    threads = [threading.Thread(target=worker, args=(w,)) for w in range(2)]
    concurrent = str(device).startswith("cuda")      # (the emulator keeps threadIdx & co. in globals: one launch at a time)
    for th in threads:
        th.start()
        if not concurrent:
            th.join()
    for th in threads:
        th.join()
    assert not errors, errors
    for w in range(2):
        assert results[w][4] == exps[w][4] and all(np.array_equal(results[w][c], exps[w][c]) for c in range(4)), w
    _sync(device)
    ix.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def workspace_bytes_bound(nq, k, limit):
    np_ = nq * (k + 1)
    return 32 * (np_ + 1) + min(limit, np_ * 0xFFFFFFFF) // 4 + (64 << 10)


def workspace_bound(eng):
    """Hook-free: sfx_hamming_workspace_bytes(nq, k, limit) <= 32 (nq (k + 1) + 1) + limit / 4 + 64 KiB, 0 where nothing can run."""
    f = eng.lib.sfx_hamming_workspace_bytes
    for nq in (1, 2, 255, 4097, 1 << 18, 1 << 24):
        for k in (0, 1, 3, 7, 255):
            if nq * (k + 1) >= 1 << 32:
                assert f(nq, k, 100) == 0
                continue
            for limit in (1, 2047, 2048, 2049, 1 << 20, (1 << 28) + 1, 1 << 34, 1 << 40, (1 << 64) - 1):
                got = int(f(nq, k, limit))
                assert 0 < got <= workspace_bytes_bound(nq, k, limit), (nq, k, limit, got)
    assert f(0, 1, 100) == 0 and f(100, 256, 100) == 0 and f(100, 1, 0) == 0 and f((1 << 32) - 1, 0, 100) > 0 and f(1 << 32, 0, 100) == 0


def refusals(eng, device, orc):
    text = b"abracadabra" * 20
    pats = [b"cadabra", b"abrXcad", b"", b"bra"]
    sa = orc.sais(text)
    raw = _mem.Raw(eng, device, text, sa)
    qb, qoff = pack(pats)
    nq, k = len(pats), 1
    q, qo = _buffers.inp(qb, device, 1), _buffers.inp(qoff, device, 8)
    wsb = int(eng.lib.sfx_hamming_workspace_bytes(nq, k, 1 << 20))
    ws = _buffers.guarded(wsb, device, 0, 0xA5)
    bufs = [_buffers.guarded(4 * 4096, device, 4, 0xA5), _buffers.guarded(4 * 4096, device, 4, 0xA5), _buffers.guarded(4096, device, 1, 0xA5)]
    fb = _buffers.guarded(8 * (nq + 1), device, 8, 0xA5)
    o = [b.ptr for b in bufs]
    bad_order = _buffers.inp(np.array([0, 7, 5, 14, 17], dtype=np.uint64), device, 8)
    too_long = _buffers.inp(np.array([0, 7, (1 << 32) + 8, (1 << 32) + 8, (1 << 32) + 11], dtype=np.uint64), device, 8)
    st = _buffers.stream_of(device)
    for route in raw.routes():
        c = lambda **kw: raw_call(raw, route, kw.get("q", q.ptr), kw.get("qoff", qo.ptr), kw.get("nq", nq), kw.get("k", k),
                                  kw.get("limit", 1 << 20), kw.get("outs", o), kw.get("cap", 4096), kw.get("first", fb.ptr),
                                  kw.get("ws", ws.ptr), kw.get("wsb", wsb), st)
        good = c()
        assert good[0] == OK and good[1] > good[2] > 0, (route, good)
        ws.fill(0xA5)
        for b in bufs + [fb]:
            b.fill(0xA5)
        assert c(limit=0)[0] == ERR_ARG, route
        assert c(k=256)[0] == ERR_ARG and c(k=0xFFFFFFFF)[0] == ERR_ARG, route
        for j in range(3):
            assert c(outs=[None if i == j else o[i] for i in range(3)])[0] == ERR_ARG, (route, j)
        assert c(q=None)[0] == ERR_ARG and c(qoff=None)[0] == ERR_ARG, route
        assert c(nq=1 << 32)[0] == ERR_TOO_LARGE and c(nq=1 << 24, k=255)[0] == ERR_TOO_LARGE and c(nq=1 << 31, k=1)[0] == ERR_TOO_LARGE, route
        assert c(ws=None)[0] == ERR_WORKSPACE and c(wsb=wsb - 1)[0] == ERR_WORKSPACE and c(wsb=0)[0] == ERR_WORKSPACE, route
        assert c(ws=ctypes.c_void_p(ws.ptr.value + 8), wsb=wsb)[0] == ERR_ARG, route          # large enough, off the boundary
        assert c(outs=[ctypes.c_void_p(o[0].value + 2), o[1], o[2]])[0] == ERR_ARG, route     # a u32 array off 4 bytes
        assert c(first=ctypes.c_void_p(fb.ptr.value + 4))[0] == ERR_ARG, route                # first off 8 bytes
        assert c(qoff=ctypes.c_void_p(qo.ptr.value + 4))[0] == ERR_ARG, route
        for b in bufs + [fb]:
            assert (b.host() == 0xA5).all(), "a call refused on the host wrote"
        # found on the device, reported through the one read-back; the triple arrays and first stay as they are
        assert c(qoff=bad_order.ptr)[0] == ERR_ARG, route
        assert c(qoff=too_long.ptr)[0] == ERR_TOO_LARGE, route
        for b in bufs + [fb]:
            assert (b.host() == 0xA5).all(), "a call refused on the device wrote"
        # nothing to do: SFX_OK, C = Z = 0, first all zero
        assert c(nq=0, q=None, qoff=None, ws=None, wsb=0) == (OK, 0, 0), route
        assert fb.host(np.uint64)[0] == 0 and (fb.host(np.uint64)[1:] == 0xA5A5A5A5A5A5A5A5).all()
        fb.fill(0xA5)
        assert c(cap=0, outs=[None, None, None]) == good, route
        assert c(first=None) == good, route
    lib = eng.lib
    none2 = (ctypes.byref(_u64(0)), ctypes.byref(_u64(0)))
    head = (q.ptr, qo.ptr, nq, k, 1 << 20, None, None, None, 0, None)
    assert lib.sfx_hamming_dev(raw.t.ptr, 1 << 32, raw.s.ptr, *head, *none2, ws.ptr, wsb, st) == ERR_TOO_LARGE
    fb.fill(0xA5)
    assert lib.sfx_hamming_dev(raw.t.ptr, 0, raw.s.ptr, *head[:9], fb.ptr, *none2, None, 0, st) == OK                      # n == 0
    _sync(device)
    assert (fb.host(np.uint64) == 0).all()
    assert lib.sfx_hamming_dev(None, len(text), raw.s.ptr, *head, *none2, ws.ptr, wsb, st) == ERR_ARG
    assert lib.sfx_hamming_dev(raw.t.ptr, len(text), None, *head, *none2, ws.ptr, wsb, st) == ERR_ARG
    assert lib.sfx_hamming_dev(raw.t.ptr, len(text), raw.s.ptr, *head, None, none2[1], ws.ptr, wsb, st) == ERR_ARG
    assert lib.sfx_hamming_dev(raw.t.ptr, len(text), raw.s.ptr, *head, none2[0], None, ws.ptr, wsb, st) == ERR_ARG
    for fn in (lib.sfx_index_hamming_dev, lib.sfx_gindex_hamming_dev):
        assert fn(None, *head, *none2, ws.ptr, wsb, st) == ERR_ARG
    hoff_bad = np.array([0, 7, 5, 14, 17], dtype=np.uint64)
    hoff_long = np.array([0, 7, (1 << 32) + 8, (1 << 32) + 8, (1 << 32) + 11], dtype=np.uint64)
    for fn, h in ((lib.sfx_index_hamming, raw.ix._h), (lib.sfx_gindex_hamming, raw.gx._h)):
        hc = lambda **kw: fn(kw.get("h", h), kw.get("q", _gsa.ptr(qb)), kw.get("qoff", _gsa.ptr(qoff)), kw.get("nq", nq), kw.get("k", k),
                             kw.get("limit", 1 << 20), None, None, None, kw.get("cap", 0), None, *none2)
        assert hc() == OK
        assert hc(h=None) == ERR_ARG and hc(limit=0) == ERR_ARG and hc(k=256) == ERR_ARG and hc(cap=7) == ERR_ARG
        assert hc(q=None) == ERR_ARG and hc(qoff=None) == ERR_ARG and hc(qoff=_gsa.ptr(hoff_bad)) == ERR_ARG
        assert hc(qoff=_gsa.ptr(hoff_long)) == ERR_TOO_LARGE and hc(nq=1 << 32) == ERR_TOO_LARGE and hc(nq=1 << 24, k=255) == ERR_TOO_LARGE
    for b in bufs:
        b.check_guards("refused")
    ws.check_guards("workspace")
    fb.check_guards("first")
    raw.close()


def foreign_table(eng, device):
    """A table with entries < n that is not the text's (sfx_hamming_dev takes it as it is): the call stays inside its
    buffers and ends; what it reports is unspecified."""
    class Plain:                                                              # what raw_call reads of a _mem.Raw on the "dev" route
        def __init__(self, text, sa):
            self.eng, self.device, self.n = eng, device, len(text)
            self.t, self.s = _buffers.text_in(text, device, 3), _buffers.inp(sa, device, 4)

        def close(self):
            self.t.check_guards("text")
            self.s.check_guards("sa")

    rng = random.Random(21)
    text = bytes(rng.choice(b"ab") for _ in range(500))
    for kind in ("shuffled", "constant", "reversed"):
        sa = {"shuffled": np.random.default_rng(1).permutation(500), "constant": np.full(500, 499), "reversed": np.arange(499, -1, -1)}[kind]
        raw = Plain(text, sa.astype(np.uint32))
        for k in (0, 2):
            pats = make_patterns(rng, text, k, 8, lo=0, hi=24, alphabet=[97, 98])
            out = guarded_call(raw, "dev", pats, k, cap=4096)
            assert out[0] == OK and out[2] <= out[1] <= len(pats) * (k + 1) * 500, (kind, out[:3])
            z = min(out[2], 4096)
            assert (out[4][:z] < 500).all() and (out[3][:z] < len(pats)).all()
        raw.close()


def launch_names(eng, device, orc):
    text = b"abracadabra" * 30
    pats = [b"cadabraabr", b"abrXcadabr", b"zzzzzzzz"]
    sa = orc.sais(text)
    for route in ("dev", "index_dev", "gindex_dev"):
        names = _gsa.profile_names(eng, lambda: run(eng, device, route, text, sa, pats, 1))
        assert KERNELS <= names, (route, sorted(names))
        assert not {x for x in names if x.startswith("hm_")} - KERNELS, sorted(names)


# ---- scale (test_gpu_hamming.py, scripts/gpu_hamming_time.py) ----------------------------------------------------------------
def scale_patterns(rng, text, k, count, lo=20, hi=64, starts=None):
    """`count` patterns of lo .. hi bytes: every eighth one sampled from the text with 0 .. k + 2 planted substitutions
    (-> origins: (pattern, position, differing bytes) where at most k bytes differ in the end), every eighth one sampled
    with one inserted byte, the rest random over the text's alphabet with a sampled piece of 5 .. 16 bytes at a random place
    -- candidates in plenty and hardly an occurrence.  With `starts` every fourth sampled pattern lies across a document end."""
    t = np.frombuffer(text, dtype=np.uint8)
    n = t.size
    alphabet = np.unique(t[:1 << 16])
    g = np.random.default_rng(rng.randrange(1 << 30))
    pats, origins = [], []
    for j in range(count):
        m = rng.randint(lo, hi)
        a = rng.randrange(n - m)
        if starts is not None and j % 32 in (0, 1):
            a = min(n - m, max(0, int(starts[rng.randrange(1, len(starts))]) - rng.randint(1, m - 1)))
        if j % 8 == 0:
            p = t[a:a + m].copy()
            for _ in range(rng.randint(0, k + 2)):
                p[rng.randrange(m)] = alphabet[rng.randrange(alphabet.size)]
            d = int((p != t[a:a + m]).sum())
            if d <= k:
                origins.append((j, a, d))
        elif j % 8 == 1:
            at = rng.randint(0, m - 1)
            p = np.concatenate([t[a:a + at], alphabet[rng.randrange(alphabet.size):][:1], t[a + at:a + m - 1]])
        else:
            p = alphabet[g.integers(0, alphabet.size, m)]
            ln = rng.randint(5, 16)
            at = rng.randint(0, m - ln)
            p[at:at + ln] = t[a:a + ln]
        assert p.size == m
        pats.append(p.tobytes())
    return pats, origins


def expected_counts(orc, text, sa, patterns, k, chunk=1 << 20):
    """(C, Z, the largest piece interval) on the CPU, without the engine: the exact intervals of the pieces from the
    oracle's search over the oracle's table; every candidate window compared in numpy, counted where its piece is the
    first that matches exactly and at most k bytes differ.  (Patterns of at least k + 1 bytes: no empty piece.)"""
    t = np.frombuffer(text, dtype=np.uint8)
    n = t.size
    pieces, meta = [], []
    for j, pat in enumerate(patterns):
        b = cuts(len(pat), k)
        assert len(pat) > k
        for s in range(k + 1):
            pieces.append(pat[b[s]:b[s + 1]])
            meta.append((j, s))
    qb, qoff = pack(pieces)
    lo_, hi_ = orc.positions_batch(text, sa, qb, qoff)
    width = hi_.astype(np.int64) - lo_.astype(np.int64)
    C, Z = int(width.sum()), 0
    sa = np.asarray(sa, dtype=np.int64)
    for e in np.flatnonzero(width):
        j, s = meta[e]
        pat = np.frombuffer(patterns[j], dtype=np.uint8)
        m, b = pat.size, cuts(pat.size, k)
        p = sa[int(lo_[e]):int(hi_[e])] - b[s]
        p = p[(p >= 0) & (p + m <= n)]
        for c0 in range(0, p.size, chunk):
            w = p[c0:c0 + chunk]
            diff = t[w[:, None] + np.arange(m)[None, :]] != pat[None, :]
            ok = diff.sum(axis=1) <= k
            for u in range(s):
                ok &= diff[:, b[u]:b[u + 1]].any(axis=1)
            Z += int(ok.sum())
    return C, Z, int(width.max()) if width.size else 0


def check_rank_order(text, sa, patterns, k, res):
    """Inside (pattern, owning piece) the table ranks of tpos + b_owner ascend strictly: numpy over the inverse table."""
    t = np.frombuffer(text, dtype=np.uint8)
    isa = np.zeros(t.size, dtype=np.int64)
    isa[np.asarray(sa, dtype=np.int64)] = np.arange(t.size)
    first, tpos = res[0].astype(np.int64), res[2].astype(np.int64)
    for j, pat in enumerate(patterns):
        a, z = int(first[j]), int(first[j + 1])
        if z - a < 2:
            continue
        pb = np.frombuffer(pat, dtype=np.uint8)
        b = cuts(pb.size, k)
        w = tpos[a:z]
        diff = t[w[:, None] + np.arange(pb.size)[None, :]] != pb[None, :]
        exact = np.stack([~diff[:, b[s]:b[s + 1]].any(axis=1) for s in range(k + 1)], axis=1)
        assert exact.any(axis=1).all(), j
        owner = exact.argmax(axis=1)
        key = owner * (t.size + 1) + isa[w + np.asarray(b)[owner]]
        assert (np.diff(key) > 0).all(), (j, "rank order inside (pattern, owner)")


def check_origins(origins, res):
    first, tpos, mism = res[0].astype(np.int64), res[2], res[3]
    for j, a, d in origins:
        sl = slice(int(first[j]), int(first[j + 1]))
        at = np.flatnonzero(tpos[sl] == a)
        assert at.size == 1 and int(mism[sl][at[0]]) == d, (j, a, d, tpos[sl][:8], mism[sl][:8])


def piece_intervals(index, patterns, k):
    """-> int64 array (pieces, 2): [start, end) of every piece through the index's exact batch search."""
    pieces = []
    for pat in patterns:
        b = cuts(len(pat), k)
        pieces += [pat[b[s]:b[s + 1]] for s in range(k + 1)]
    qb, qoff = pack(pieces)
    dev = index._text.device
    start, end, _, _ = index.query(torch.from_numpy(qb.copy()).to(dev), torch.from_numpy(qoff.astype(np.int64)).to(dev))
    _sync(dev)
    return np.stack([start.cpu().numpy().view(np.uint32).astype(np.int64), end.cpu().numpy().view(np.uint32).astype(np.int64)], axis=1)
