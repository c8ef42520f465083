"""The cases of the k-error pattern search (sfx_edit_dev, sfx_index_edit*, sfx_gindex_edit*),
shared by test_edit_emu.py (the emulator build, host memory) and test_gpu_edit.py (libsuffix_hip.so, HBM).

Nothing expected comes from the engine under test: small inputs are held against `brute`, Sellers' recurrence with
max-start tracking run per document; larger ones go through the serial checker tests/ed_check.c (every quadruple is the
least distance at its end with the largest begin, ends ascend strictly, `first` is consistent; a complete sweep for the
patterns marked); runs of one letter and of "ab" have closed-form answers; the candidate and hit counts C and H are
recomputed from the definition (`expected_counts`)."""
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
import _hamming
import _match
import _mem
from suffix_amd import GeneralizedSuffixTable, SuffixHipError, SuffixTable
from suffix_amd import device as sdev

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
OK, ERR_ARG, ERR_TOO_LARGE, ERR_WORKSPACE = 0, 1, 2, 5
KERNELS = {"hm_pieces", "ed_short", "hm_guard", "ed_cand", "ed_count", "ed_emit", "ed_heads", "ed_reduce", "ed_first"}
ROUTES = ("dev", "index_dev", "gindex_dev", "index_host", "gindex_host")
TILE = 2048                                                     # K of a hook-free build
KS = (0, 1, 2, 3, 4)
MAX_K = 31
UNWRITTEN32, UNWRITTEN8 = 0xA5A5A5A5, 0xA5
_vp, _u64, _u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
_np, _t, _sync = _match._np, _match._t, _match._sync
pack, naive_table, cuts = _hamming.pack, _hamming.naive_table, _hamming.cuts
_BIG = 1 << 32


def build_emulator():
    """`make -C tests/emu`; sfx_edit.hip is compiled as part of sfx_api.hip's translation unit and tests/emu/Makefile does
    not name it, so after an edit to it alone sfx_api.hip is declared new (`make -W`).  -> the library's path."""
    lib = os.path.join(EMU_DIR, "libsuffix_emu.so")
    cmd = ["make", "-s", "-j8", "-C", EMU_DIR]
    csrc = os.path.join(HERE, os.pardir, "suffix_amd", "csrc")
    newest = max(os.path.getmtime(os.path.join(csrc, f)) for f in ("sfx_edit.hip", "sfx_hamming.hip", "sfx_mem.hip"))
    if os.path.exists(lib) and newest > os.path.getmtime(lib):
        cmd += ["-W", _mem.CSRC_FROM_EMU + "/sfx_api.hip"]
    subprocess.check_call(cmd)
    return lib


# ---- the definition --------------------------------------------------------------------------------------------------
def _documents(n, starts):
    if starts is None:
        return [(0, n)]
    s = [int(x) for x in starts]
    return [(s[d], s[d + 1] if d + 1 < len(s) else n) for d in range(len(s))]


def brute(text, doc_starts, patterns, k):
    """Sellers' recurrence with max-start tracking, per document: D[i][e] = the least ed(P[0..i), T[s..e)) over s in the
    document, S[i][e] = the largest s that attains it.  A cell is the pair as one integer D * 2^32 - S, so that the least
    key is the least distance with the largest start; one pattern row at a time over all ends of the document, the
    horizontal step as a running minimum.  -> ([(pattern, tbegin, tend, dist)] ascending by pattern and tend, first)."""
    text = bytes(text)
    t = np.frombuffer(text, dtype=np.uint8).astype(np.int64)
    out, first = [], [0]
    for j, pat in enumerate(patterns):
        found = []
        for lo, hi in _documents(len(text), doc_starts):
            e = np.arange(lo, hi + 1, dtype=np.int64)
            step = (e - lo) * _BIG
            key = -e                                                          # row 0: distance 0 from s = e
            for c in bytes(pat):
                new = key + _BIG                                              # a pattern byte against nothing
                new[1:] = np.minimum(new[1:], key[:-1] + (t[lo:hi] != c) * _BIG)
                key = np.minimum.accumulate(new - step) + step                # a text byte against nothing, from any earlier end
            d = -((-key) // _BIG)
            s = d * _BIG - key
            found += [(int(e[x]), int(s[x]), int(d[x])) for x in np.flatnonzero(d <= k).tolist()]
        out += [(j, s, e, d) for e, s, d in sorted(found)]
        first.append(len(out))
    return out, first


def ed(a, b):
    """Unit-cost Levenshtein distance, the textbook table."""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j - 1] + (a[i - 1] != b[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(b)]


def expected_counts(text, doc_starts, patterns, k, sa):
    """(C, H, Z) from the definition of include/suffix_hip.h, on the CPU and without the engine: the exact interval of
    every piece by comparing every suffix (inside its document), then per candidate the left value L over its window and
    the right values R(e), all by the textbook table.  For small inputs."""
    text = bytes(text)
    n = len(text)
    docs = _documents(n, doc_starts)
    C = H = 0
    ends = set()
    for j, pat in enumerate(patterns):
        b = cuts(len(pat), k)
        for t in range(k + 1):
            piece = pat[b[t]:b[t + 1]]
            for q in (int(x) for x in sa):
                lo, hi = next((a, z) for a, z in docs if a <= q < z)
                if text[q:min(hi, q + len(piece))] != piece:
                    continue
                C += 1
                qe = q + len(piece)
                L = min(ed(pat[:b[t]], text[s:q]) for s in range(max(lo, q - b[t] - k), q + 1))
                if L > k:
                    continue
                right = pat[b[t + 1]:]
                for e in range(qe, min(hi, qe + len(right) + k) + 1):
                    if L + ed(right, text[qe:e]) <= k:
                        H += 1
                        ends.add((j, e))
    return C, H, len(ends)


# the hand-worked cases: (text, doc_starts, patterns, k); their answers are stated in hand_worked() below
#   T = "banana", P = "bnana": "banana" without its first a.
#   T = "abcdef": "abdef" is T without c (one deletion), "abxcdef" has one byte more (one insertion).
HAND = [
    (b"banana", None, [b"bnana"], 1),
    (b"abcdef", None, [b"abdef", b"abxcdef"], 1),
    (b"abcdef", None, [b"abcdef", b"bcd", b"f", b"xyz"], 0),
    (b"abcabdabc_abd", None, [b"abd", b"abc", b"ab"], 1),                      # m = k + 1
    (b"abcdefgh", [0, 4], [b"cdef", b"bcde", b"abcd", b"efgh"], 1),            # across the document border
    (b"aaaa", [0, 0, 1, 1, 4], [b"aa", b"aaa"], 1),                            # empty documents, one of a single byte
]


def hand_worked():
    """The hand-worked answers, stated here and held against `brute` (and, by the callers, against every entry point)."""
    got = brute(b"banana", None, [b"bnana"], 1)[0]
    # "bnana" is no substring of "banana", so no end has distance 0.  e = 4: T[0..4) = "bana" lacks the first n.  e = 6:
    # "banana" (one byte more), "anana" (b -> a) and "nana" (no b) are all one edit away: the largest begin, 2, is kept.
    # e = 5: "banan", "anan", "nan" are two edits away.
    assert got == [(0, 0, 4, 1), (0, 2, 6, 1)], got
    assert ed(b"bnana", b"bana") == ed(b"bnana", b"nana") == ed(b"bnana", b"anana") == ed(b"bnana", b"banana") == 1
    assert min(ed(b"bnana", b"banana"[s:5]) for s in range(6)) == 2
    got = brute(b"abcdef", None, [b"abdef", b"abxcdef"], 1)[0]
    assert (0, 0, 6, 1) in got and (1, 0, 6, 1) in got, got                  # one deletion, one insertion
    assert (0, 2, 6, 1) not in got
    got = brute(b"abcdefgh", [0, 4], [b"cdef", b"bcde", b"abcd", b"efgh"], 1)[0]
    assert not any(x[0] == 0 for x in got), got                              # "cdef" straddles the border: no match
    assert (1, 1, 4, 1) in got and (2, 0, 4, 0) in got and (3, 4, 8, 0) in got, got
    assert all(not (s < 4 < e) for _, s, e, _ in got)
    got = brute(b"abcabdabc_abd", None, [b"ab"], 1)[0]                        # m = k + 1: "a", "ab" and "abc" at every "ab"
    assert got[:3] == [(0, 0, 1, 1), (0, 0, 2, 0), (0, 0, 3, 1)] and len(got) == 12, got


# ---- the checker -------------------------------------------------------------------------------------------------------
def build_checker(out_dir):
    """tests/ed_check.c -> a shared object in out_dir, bound (with OpenMP where the compiler has it)."""
    so = os.path.join(str(out_dir), "libed_check.so")
    base = ["gcc", "-O2", "-std=c99", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "ed_check.c")]
    if subprocess.call(base + ["-fopenmp"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)
    lib = ctypes.CDLL(so)
    lib.ed_check.restype = ctypes.c_int
    lib.ed_check.argtypes = [_vp, _u64, _vp, _u64, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, _u64, _vp, _vp, ctypes.POINTER(ctypes.c_int64)]
    lib.ed_check_name.restype = ctypes.c_char_p
    lib.ed_check_name.argtypes = [ctypes.c_int]
    lib.ed_counts.restype = ctypes.c_int
    lib.ed_counts.argtypes = [_vp, _u64, _vp, _vp, _vp, _u64, _u32, _vp, _vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64)]
    lib.ed_occurrences.restype = ctypes.c_int
    lib.ed_occurrences.argtypes = [_vp, _u64, _vp, _u64, _vp, _vp, _u64, _u32, ctypes.POINTER(_u64)]
    return lib


def scale_counts(chk, orc, text, sa, patterns, k):
    """(C, H, Z) of a plain text on the CPU, without the engine: the exact intervals of the pieces from the oracle's search
    over the oracle's table, then tests/ed_check.c -- every candidate's two windows by full tables (ed_counts) and Sellers'
    recurrence over the whole text for every pattern (ed_occurrences).  What `expected_counts` does, at scale."""
    pieces = []
    for pat in patterns:
        b = cuts(len(pat), k)
        assert len(pat) > k
        pieces += [pat[b[s]:b[s + 1]] for s in range(k + 1)]
    pb, poff = pack(pieces)
    lo, hi = orc.positions_batch(text, sa, pb, poff)
    lo, hi = np.ascontiguousarray(lo, dtype=np.uint32), np.ascontiguousarray(hi, dtype=np.uint32)
    assert int((hi.astype(np.int64) - lo.astype(np.int64)).sum()) >= 0
    t, s = _np(text, np.uint8), _np(sa, np.uint32)
    qb, qoff = pack(patterns)
    C, H, Z = _u64(0), _u64(0), _u64(0)
    assert chk.ed_counts(_gsa.ptr(t), t.size, _gsa.ptr(s), _gsa.ptr(qb), _gsa.ptr(qoff), len(patterns), int(k), _gsa.ptr(lo), _gsa.ptr(hi),
                         ctypes.byref(C), ctypes.byref(H)) == 0
    assert chk.ed_occurrences(_gsa.ptr(t), t.size, None, 0, _gsa.ptr(qb), _gsa.ptr(qoff), len(patterns), int(k), ctypes.byref(Z)) == 0
    return int(C.value), int(H.value), int(Z.value)


def check(chk, text, starts, patterns, k, res, sweep=None):
    """res = (first, pattern, tbegin, tend, dist, ...).  -> (fault name, index)."""
    t = _np(text, np.uint8)
    qb, qoff = pack(patterns)
    ds = None if starts is None else _np(starts, np.uint64)
    first, pat, tb, te, dist = (_np(res[0], np.uint64), _np(res[1], np.uint32), _np(res[2], np.uint32), _np(res[3], np.uint32),
                                _np(res[4], np.uint8))
    assert first.size == len(patterns) + 1 and pat.size == tb.size == te.size == dist.size
    sw = None if sweep is None else _np(sweep, np.uint8)
    where = ctypes.c_int64(-2)
    rc = chk.ed_check(_gsa.ptr(t), t.size, _gsa.ptr(ds) if ds is not None else None, 0 if ds is None else ds.size, _gsa.ptr(qb),
                      _gsa.ptr(qoff), len(patterns), int(k), _gsa.ptr(pat), _gsa.ptr(tb), _gsa.ptr(te), _gsa.ptr(dist), pat.size,
                      _gsa.ptr(first), _gsa.ptr(sw) if sw is not None else None, ctypes.byref(where))
    return chk.ed_check_name(rc).decode(), int(where.value)


def accept(chk, text, starts, patterns, k, res, sweep=None):
    name, where = check(chk, text, starts, patterns, k, res, sweep)
    assert name == "ok", f"ed_check: {name} at {where} (k {k})"


def _cols(quads, nq):
    pat = np.array([x[0] for x in quads], dtype=np.uint32)
    first = np.searchsorted(pat, np.arange(nq + 1)).astype(np.uint64)
    return (first, pat, np.array([x[1] for x in quads], dtype=np.uint32), np.array([x[2] for x in quads], dtype=np.uint32),
            np.array([x[3] for x in quads], dtype=np.uint8))


def checker_self_test(chk):
    """One fault per rule: every one is named, at the item that is wrong."""
    text, pats, k = b"abcabdabc_abd", [b"abda", b"abc"], 1
    good, first = brute(text, None, pats, k)
    assert len(good) >= 8 and first[1] >= 3 and first[2] - first[1] >= 3, (good, first)
    all1 = [1, 1]
    assert check(chk, text, None, pats, k, _cols(good, 2), all1) == ("ok", -1)
    g = list(good)
    i = next(x for x in range(len(g)) if g[x] == (1, 0, 3, 0))                # "abc" at 0; its next end belongs to "abc" too
    assert g[i + 1][0] == 1 and g[2][0] == 0
    faults = [
        (g[:2] + g[3:], "missing", 0),                                        # a missing occurrence: named at its pattern
        (g[:i] + [(1, 0, 3, 1)] + g[i + 1:], "distance", i),                  # a wrong distance
        (g[:i] + [g[i], g[i]] + g[i + 1:], "order", i + 1),                   # a duplicate
        (g[:i] + [g[i + 1], g[i]] + g[i + 2:], "order", i + 1),               # a swapped pair
        (g[:i] + [(1, 0, 3, 2)] + g[i + 1:], "range", i),                     # a distance above k
    ]
    done = 0
    for quads, want, at in faults:
        got = check(chk, text, None, pats, k, _cols(quads, 2), all1)
        assert got == (want, at), (quads, got, want, at)
        done += 1
    # an extra occurrence: an end that is none, so the distance it states cannot be its stretch's
    text2, pats2 = b"abcdefgh", [b"cdef"]
    good2, _ = brute(text2, None, pats2, 1)
    assert [x[2] for x in good2] == [5, 6, 7], good2                          # "cde", "cdef", "cdefg"
    extra = sorted(good2 + [(0, 0, 3, 1)], key=lambda x: x[2])
    assert check(chk, text2, None, pats2, 1, _cols(extra, 1), [1]) == ("distance", 0)
    # a begin that is not the largest: P = "ab", T = "aab", e = 2: "aa" costs 1 from s = 0 and "a" costs 1 from s = 1
    good3, _ = brute(b"aab", None, [b"ab"], 1)
    assert (0, 1, 2, 1) in good3 and (0, 1, 3, 0) in good3, good3
    worse = [(0, 0, 2, 1) if x == (0, 1, 2, 1) else x for x in good3]
    at = worse.index((0, 0, 2, 1))
    assert check(chk, b"aab", None, [b"ab"], 1, _cols(worse, 1), [1]) == ("begin", at)
    # a distance that is not the least at its end: (0, 0, 3, 1) for "aab" is a true distance but s = 1 gives 0
    worse = [(0, 0, 3, 1) if x == (0, 1, 3, 0) else x for x in good3]
    assert check(chk, b"aab", None, [b"ab"], 1, _cols(worse, 1), [1]) == ("smaller", worse.index((0, 0, 3, 1)))
    # first: a wrong total, not monotone
    cols = list(_cols(good, 2))
    bad = cols[0].copy(); bad[2] -= 1
    assert check(chk, text, None, pats, k, (bad, *cols[1:]))[0] == "first"
    bad = cols[0].copy(); bad[1] = bad[2] + 1
    assert check(chk, text, None, pats, k, (bad, *cols[1:]))[0] == "first"
    # an occurrence across a document end; the same list is fine when the documents allow it
    assert check(chk, b"abcd", [0, 2], [b"bc"], 0, _cols([(0, 1, 3, 0)], 1)) == ("document", 0)
    assert check(chk, b"abcd", [0, 1], [b"bc"], 0, _cols([(0, 1, 3, 0)], 1), [1]) == ("ok", -1)
    return done + 7


# ---- the entry points ------------------------------------------------------------------------------------------------
def run(eng, device, route, text, sa, patterns, k, starts=None, da=None, max_cands=1 << 30, max_hits=1 << 22):
    """One entry point -> (first uint64, pattern uint32, tbegin uint32, tend uint32, dist uint8, C, H) on the host.  The
    gindex routes of a plain text see it as one document.  A refusal raises SuffixHipError."""
    n = len(text)
    qb, qoff = pack(patterns)
    nq = len(patterns)
    if route.startswith("gindex"):
        starts, da = _mem._as_collection(n, starts, da)
    else:
        assert starts is None
    if route.endswith("_host"):
        t, s = _np(text, np.uint8), _np(sa, np.uint32)
        h = ctypes.c_void_p()
        if route == "index_host":
            assert eng.lib.sfx_index_create(_gsa.ptr(t), n, _gsa.ptr(s), ctypes.byref(h)) == OK
            call, destroy = eng.lib.sfx_index_edit, eng.lib.sfx_index_destroy
        else:
            ds, d = _np(starts, np.uint64), _np(da, np.uint32)
            assert eng.lib.sfx_gindex_create(_gsa.ptr(t), n, _gsa.ptr(ds), ds.size, _gsa.ptr(s), _gsa.ptr(d), ctypes.byref(h)) == OK
            call, destroy = eng.lib.sfx_gindex_edit, eng.lib.sfx_gindex_destroy
        cands, hits, count = _u64(0), _u64(0), _u64(0)
        first = np.full(nq + 1, 0xDEADBEEF, dtype=np.uint64)
        try:
            rc = call(h, _gsa.ptr(qb), _gsa.ptr(qoff), nq, k, max_cands, max_hits, None, None, None, None, 0, _gsa.ptr(first),
                      ctypes.byref(cands), ctypes.byref(hits), ctypes.byref(count))
            assert rc == OK, (route, rc)
            if cands.value > max_cands or hits.value > max_hits:
                raise SuffixHipError(f"refused: {cands.value} candidates, {hits.value} hits")
            z = int(count.value)
            assert int(first[nq]) == z, (route, first, z)                    # (complete at capacity 0)
            f0 = first.copy()
            out = [np.full(z + 3, 0xDEADBEEF, dtype=np.uint32) for _ in range(3)] + [np.full(z + 3, 0xEF, dtype=np.uint8)]
            rc = call(h, _gsa.ptr(qb), _gsa.ptr(qoff), nq, k, max_cands, max_hits, *[_gsa.ptr(a) for a in out], z + 3, _gsa.ptr(first),
                      ctypes.byref(cands), ctypes.byref(hits), ctypes.byref(count))
            assert rc == OK and count.value == z and np.array_equal(first, f0), (route, rc, z, count.value)
        finally:
            destroy(h)
        assert all((a[z:] == 0xDEADBEEF).all() for a in out[:3]) and (out[3][z:] == 0xEF).all(), (route, "written past z")
        return first, out[0][:z], out[1][:z], out[2][:z], out[3][:z], int(cands.value), int(hits.value)
    dt, dsa = _t(text, device), _t(sa, device, np.uint32)
    dq, doff = _t(qb, device), _t(qoff.astype(np.int64), device, np.int64)
    kw = dict(max_candidates=max_cands, max_hits=max_hits)
    if route == "dev":
        got = sdev.edit_search(dt, dsa, dq, doff, k, engine=eng, **kw)
    elif route == "index_dev":
        ix = sdev.DeviceIndex(dt, dsa, engine=eng)
        try:
            got = ix.edit_search(dq, doff, k, **kw)
        finally:
            _sync(device)
            ix.close()
    else:
        gx = sdev.GeneralizedDeviceIndex(dt, _t(starts, device, np.int64), dsa, _t(da, device, np.uint32), engine=eng)
        try:
            got = gx.edit_search(dq, doff, k, **kw)
        finally:
            _sync(device)
            gx.close()
    _sync(device)
    return host(got)


def host(got):
    return (got[0].cpu().numpy().view(np.uint64), got[1].cpu().numpy().view(np.uint32), got[2].cpu().numpy().view(np.uint32),
            got[3].cpu().numpy().view(np.uint32), got[4].cpu().numpy(), got[5], got[6])


def quads(res):
    return list(zip(res[1].tolist(), res[2].tolist(), res[3].tolist(), res[4].tolist()))


def same_as_brute(res, want, route=None, note=None):
    q, first = want
    assert quads(res) == q and res[0].tolist() == first, (route, note, quads(res)[:12], q[:12], res[0].tolist()[:8], first[:8])


# ---- patterns ----------------------------------------------------------------------------------------------------------
def edit_bytes(rng, p, count, alphabet, floor):
    """`count` random edits of the bytearray p -- substitutions, insertions and deletions -- never below `floor` bytes."""
    for _ in range(count):
        x = rng.random()
        if x < 0.34 and len(p) > floor:
            del p[rng.randrange(len(p))]
        elif x < 0.67:
            p.insert(rng.randint(0, len(p)), rng.choice(alphabet))
        elif p:
            p[rng.randrange(len(p))] = rng.choice(alphabet)
    return p


def make_patterns(rng, text, k, count, lo=None, hi=40, alphabet=None):
    """Of at least k + 1 bytes: sampled from the text with 0 .. k + 1 planted edits, or random."""
    alphabet = alphabet or sorted(set(text)) + [1]
    lo = k + 1 if lo is None else max(lo, k + 1)
    n, out = len(text), []
    for _ in range(count):
        m = rng.randint(lo, max(lo, hi))
        if rng.random() < 0.7 and n:
            a = rng.randrange(n)
            p = edit_bytes(rng, bytearray(text[a:a + m]), rng.randint(0, k + 1), alphabet, k + 1)
            while len(p) < k + 1:
                p.append(rng.choice(alphabet))
        else:
            p = bytearray(rng.choice(alphabet) for _ in range(m))
        out.append(bytes(p))
    return out


def exact_quads(text, patterns):
    """The k = 0 answer from the exact search by the definition: (p, p + m, 0) for every position p, ascending."""
    out, first = [], [0]
    for j, pat in enumerate(patterns):
        p = text.find(pat)
        while p >= 0:
            out.append((j, p, p + len(pat), 0))
            p = text.find(pat, p + 1)
        first.append(len(out))
    return out, first


# ---- 1. against the definition ---------------------------------------------------------------------------------------------
def known_answers(eng, device):
    hand_worked()
    for text, starts, pats, k in HAND:
        want = brute(text, starts, pats, k)
        if starts is None:
            sa, da, routes = naive_table(text), None, ROUTES
        else:
            g = GeneralizedSuffixTable.new_naive(_match.doc_list(text, starts), engine=eng)
            sa, da, routes = g.table(), g.doc_array(), ("gindex_dev", "gindex_host")
        for route in routes:
            res = run(eng, device, route, text, sa, pats, k, starts=starts, da=da)
            same_as_brute(res, want, route, (text, pats, k))
            assert (res[5], res[6], len(want[0])) == expected_counts(text, starts, pats, k, sa), (route, text, pats, k, res[5:])
    # the host API
    t = SuffixTable(b"banana", engine=eng)
    want = [x[1:] for x in brute(b"banana", None, [b"bnana"], 1)[0]]
    assert t.edit_positions(b"bnana", 1) == want == [(0, 4, 1), (2, 6, 1)]
    assert t.edit_positions("ana", 0) == [(1, 4, 0), (3, 6, 0)]
    first, tb, te, dist = t.edit_positions_batch([b"bnana", b"ana"], 1)
    both = brute(b"banana", None, [b"bnana", b"ana"], 1)
    assert first.dtype == np.uint64 and tb.dtype == te.dtype == np.uint32 and dist.dtype == np.uint8
    assert first.tolist() == both[1] and list(zip(tb.tolist(), te.tolist(), dist.tolist())) == [x[1:] for x in both[0]]
    assert t.edit_positions_batch([], 1)[0].tolist() == [0] and SuffixTable(b"", engine=eng).edit_positions(b"ab", 1) == []
    for pat, bad in ((b"ab", -1), (b"ab", 32), (b"a", 1), (b"", 0), (b"ab", 2)):
        try:
            t.edit_positions(pat, bad)
            raise AssertionError(f"{pat!r} at k = {bad} was accepted")
        except ValueError:
            pass
    try:
        SuffixTable(b"aaaaaaaa", engine=eng).edit_positions_batch([b"aaaa"], 1, max_candidates=13)
        raise AssertionError("14 candidates were not refused at max_candidates = 13")
    except SuffixHipError as e:
        assert "14" in str(e) and "13" in str(e), e
    c, h, z = expected_counts(b"aaaaaaaa", None, [b"aaaa"], 1, naive_table(b"aaaaaaaa"))
    assert (c, z) == (14, 6) and h > z
    try:
        SuffixTable(b"aaaaaaaa", engine=eng).edit_positions_batch([b"aaaa"], 1, max_hits=h - 1)
        raise AssertionError(f"{h} hits were not refused at max_hits = {h - 1}")
    except SuffixHipError as e:
        assert str(h) in str(e) and str(h - 1) in str(e), e
    assert SuffixTable(b"aaaaaaaa", engine=eng).edit_positions_batch([b"aaaa"], 1, max_candidates=14, max_hits=h)[2].tolist() == [3, 4, 5, 6, 7, 8]
    docs = [b"abcd", b"", b"efgh", b"c"]
    g = GeneralizedSuffixTable(docs, engine=eng)
    assert g.edit_positions(b"cdef", 1) == []                                 # it straddles the border
    want = brute(b"".join(docs), [0, 4, 4, 8], [b"bcde"], 1)[0]
    assert g.edit_positions(b"bcde", 1) == [(0, s, e, d) for _, s, e, d in want] == [(0, 1, 4, 1)]
    assert g.edit_positions(b"fgh", 0) == [(2, 1, 4, 0)]
    first, tb, te, dist, doc = g.edit_positions_batch([b"c", b"gh"], 0)
    assert first.tolist() == [0, 2, 3] and te.tolist() == [3, 9, 8] and doc.tolist() == [0, 3, 2]
    many = SuffixTable(b"ab" * 3000, engine=eng).edit_positions_batch([b"abab"], 1)      # more than the first guess at the room
    assert many[0].tolist() == [0, 5998] and many[2].tolist() == list(range(3, 6001))
    # the device binding refuses a short pattern on the host
    dt, dsa = _t(b"banana", device), _t(naive_table(b"banana"), device, np.uint32)
    qb, qoff = pack([b"an", b"b"])
    try:
        sdev.edit_search(dt, dsa, _t(qb, device), _t(qoff.astype(np.int64), device, np.int64), 1, engine=eng)
        raise AssertionError("a pattern of k bytes was accepted")
    except ValueError:
        pass


def small_random_texts(eng, device, chk, iters=160, seed=20261020, routes=ROUTES):
    """Texts of 0 .. 300 bytes over 1 / 2 / 3 / 4 / 256 symbols, k = 0 .. 4; the routes alternate.  Every text is also
    answered at k = 0 and held against the exact positions; now and then C and H against the definition.  -> the number
    of texts."""
    rng = random.Random(seed)
    for it in range(iters):
        sigma = (1, 2, 3, 4, 256)[it % 5]
        alpha = list(range(256)) if sigma == 256 else rng.sample([0, 97, 98, 255, 65, 10], sigma)
        n = rng.choice((0, 1, 2, 7, 40, 150, 300)) if it % 5 == 0 else rng.randint(0, 300)
        text = bytes(rng.choice(alpha) for _ in range(n))
        if sigma == 256 and n > 50:                                           # repeats, so that planted patterns have several occurrences
            text = (text[:n // 3] * 3 + text)[:n]
        sa = naive_table(text)
        k = KS[(it // 5) % len(KS)]
        pats = make_patterns(rng, text, k, 6, hi=24 if sigma <= 2 else 40, alphabet=alpha + [1])
        route = routes[it % len(routes)]
        limits = dict(max_cands=1 << 30, max_hits=(1 << 24) - 1)
        res = run(eng, device, route, text, sa, pats, k, **limits)
        same_as_brute(res, brute(text, None, pats, k), route, (it, text, pats, k))
        if it % 3 == 0:
            accept(chk, text, None, pats, k, res, [1] * len(pats))
        if n <= 40:
            assert (res[5], res[6], res[1].size) == expected_counts(text, None, pats, k, sa), (it, text, pats, k, res[5:])
        res0 = run(eng, device, route, text, sa, pats, 0, **limits)
        want0 = exact_quads(text, pats)
        assert want0 == brute(text, None, pats, 0), (it, text, pats)
        same_as_brute(res0, want0, route, (it, "k = 0"))
    return iters


def small_random_collections(eng, device, chk, iters=60, seed=12):
    """Collections with empty and one-byte documents; patterns cut across document ends among them."""
    rng = random.Random(seed)
    done = empties = singles = 0
    while done < iters:
        docs = _gsa.random_collection(rng, max_docs=24, max_len=30)
        if done % 3 == 0:
            docs = docs + [bytes([rng.choice(docs[0] or b"a")])]
        text = b"".join(docs)
        if not 1 <= len(text) <= 300:
            continue
        empties += any(len(d) == 0 for d in docs)
        singles += any(len(d) == 1 for d in docs)
        g = GeneralizedSuffixTable.new_naive(docs, engine=eng)
        starts = _gsa.doc_starts(docs)
        k = KS[done % len(KS)]
        pats = make_patterns(rng, text, k, 6, hi=24)
        for s in starts[1:4]:                                                 # across a document end
            p = text[max(0, int(s) - 4):int(s) + 4]
            if len(p) > k:
                pats.append(p)
        route = ("gindex_dev", "gindex_host")[done % 2]
        res = run(eng, device, route, text, g.table(), pats, k, starts=starts, da=g.doc_array(), max_hits=(1 << 24) - 1)
        same_as_brute(res, brute(text, starts, pats, k), route, (docs, pats, k))
        accept(chk, text, starts, pats, k, res, [1] * len(pats))
        if len(text) <= 40:
            assert (res[5], res[6], res[1].size) == expected_counts(text, starts, pats, k, g.table()), (docs, pats, k, res[5:])
        done += 1
    assert empties >= 5 and singles >= 5
    return done


# ---- 2. raw calls: capacity, limits, guards --------------------------------------------------------------------------------
def raw_call(raw, route, q, qoff, nq, k, limit, hlimit, outs, cap, first, ws, ws_bytes, stream=None):
    """-> (status, C, H, Z); pointers as c_void_p or None.  raw: _mem.Raw (text, table, index and collection between guards)."""
    cands, hits, count = _u64(0xAAAA), _u64(0xCCCC), _u64(0xBBBB)
    tail = (q, qoff, nq, k, limit, hlimit, *outs, cap, first, ctypes.byref(cands), ctypes.byref(hits), ctypes.byref(count), ws, ws_bytes, stream)
    lib = raw.eng.lib
    if route == "dev":
        rc = lib.sfx_edit_dev(raw.t.ptr, raw.n, raw.s.ptr, *tail)
    elif route == "index_dev":
        rc = lib.sfx_index_edit_dev(raw.ix._h, *tail)
    else:
        rc = lib.sfx_gindex_edit_dev(raw.gx._h, *tail)
    return rc, int(cands.value), int(hits.value), int(count.value)


def guarded_call(raw, route, patterns, k, limit=None, hlimit=None, cap=None, q_off=1, out_offs=(4, 12, 8, 1), ws_fill="count", want_first=True):
    """One guarded call with a dirty workspace of exactly sfx_edit_workspace_bytes -> (status, C, H, Z, pattern, tbegin, tend,
    dist, first) as they came back, all `cap` entries (first: None when not asked).  cap None: counts first, then exactly Z."""
    dev = raw.device
    qb, qoff = pack(patterns)
    nq = len(patterns)
    limit = max(1, nq * (k + 1) * raw.n) if limit is None else limit           # (no call has more: keeps the workspace small)
    hlimit = min(limit * (2 * k + 1), (1 << 24) - 1) if hlimit is None else hlimit
    q, qo = _buffers.inp(qb, dev, q_off), _buffers.inp(qoff, dev, 8)
    wsb = int(raw.eng.lib.sfx_edit_workspace_bytes(nq, k, limit, hlimit))
    ws = _buffers.guarded(wsb, dev, 0, ws_fill)
    st = _buffers.stream_of(dev)
    if cap is None:
        rc, c, h, z = raw_call(raw, route, q.ptr, qo.ptr, nq, k, limit, hlimit, (None,) * 4, 0, None, ws.ptr, wsb, st)
        assert rc == OK, (route, rc)
        cap = z
        ws.fill(ws_fill)
    bufs = [_buffers.guarded(4 * cap, dev, out_offs[c], 0xA5) for c in range(3)] + [_buffers.guarded(cap, dev, out_offs[3], 0xA5)]
    fb = _buffers.guarded(8 * (nq + 1), dev, 8, 0xA5) if want_first else None
    rc, c, h, z = raw_call(raw, route, q.ptr, qo.ptr, nq, k, limit, hlimit, [b.ptr if cap else None for b in bufs], cap,
                           fb.ptr if fb is not None else None, ws.ptr, wsb, st)
    names = ("pattern", "tbegin", "tend", "dist", "workspace", "qbytes", "qoff", "first")
    for name, b in zip(names, bufs + [ws, q, qo] + ([fb] if fb is not None else [])):
        b.check_guards(f"{route} {name}")
    assert q.host().tobytes() == qb.tobytes() and np.array_equal(qo.host(np.uint64), qoff), "an input was written"
    return (rc, c, h, z, bufs[0].host(np.uint32), bufs[1].host(np.uint32), bufs[2].host(np.uint32), bufs[3].host(np.uint8),
            fb.host(np.uint64) if fb is not None else None)


def _unwritten(out):
    return all((out[c] == UNWRITTEN32).all() for c in (4, 5, 6)) and (out[7] == UNWRITTEN8).all()


def edges(eng, device, chk, orc):
    """Windows at both ends of the text, m = k + 1, patterns longer than the text, documents of one byte; then text and
    pattern buffers at every alignment, the capacities 0, Z - 1, Z, Z + 1 between guard bands and both limits."""
    def one(text, pats, k, starts=None):
        if starts is None:
            sa, da = (orc.sais(text) if len(text) else np.zeros(0, dtype=np.uint32)), None
        else:
            g = GeneralizedSuffixTable.new_naive(_match.doc_list(text, starts), engine=eng)
            sa, da = g.table(), g.doc_array()
        want = brute(text, starts, pats, k)
        for route in (ROUTES if starts is None else ("gindex_dev", "gindex_host")):
            same_as_brute(run(eng, device, route, text, sa, pats, k, starts=starts, da=da), want, route, (text, pats, k))
        return want[0]

    text = b"xabcdefghijklmnopqrstuvwxyz_abcdefghijklmnopqrstuvwxyy"
    n = len(text)
    for k in KS:
        pats = [text[:9], b"y" + text[1:9], text[n - 9:], text[n - 9:n - 1] + b"q", text[3:3 + k + 1], text[3:3 + k + 2],
                text[5:5 + 2 * (k + 1) + 1], text[n - k - 2:], text + b"z", text[:4] + text[5:12], text[:4] + b"#" + text[4:12],
                b"\x01\x02\x03\x04\x05\x06\x07\x08\x09"]
        w = one(text, pats, k)
        assert (0, 0, 9, 0) in w and (2, n - 9, n, 0) in w and not any(x[0] == 11 for x in w)
        if k:
            assert (1, 1, 9, 1) in w and (8, 0, n, 1) in w and (9, 0, 12, 1) in w and (10, 0, 12, 1) in w, (k, w)
    one(b"ab", [b"abc", b"ab", b"ba"], 1)
    one(b"a", [b"ab", b"ba", b"aa"], 1)
    for k in (0, 1, 2):
        w = one(b"abcaxbc", [b"abca", b"bca", b"cax", b"axb", b"xbc"], k, starts=[0, 3, 3, 4, 4, 7])
        assert all(not any(s < b < e for b in (3, 4)) for _, s, e, _ in w)
    rng = random.Random(9)
    for text in _cases.directory_texts():
        if len(text) > 700:
            continue
        sa = orc.sais(text)
        for k in (1, 3):
            pats = make_patterns(rng, text, k, 6, lo=8, hi=40)
            res = run(eng, device, ("index_dev", "dev")[k // 2], text, sa, pats, k, max_hits=(1 << 24) - 1)
            same_as_brute(res, brute(text, None, pats, k), None, (text[:20], k))
            accept(chk, text, None, pats, k, res, [1] * len(pats))

    rng = random.Random(3)
    text = bytes(rng.choice(b"ab") for _ in range(300))
    sa = orc.sais(text)
    k = 2
    pats = make_patterns(rng, text, k, 9, lo=8, hi=30, alphabet=[97, 98]) + [b"abb"]
    want, wfirst = brute(text, None, pats, k)
    Z = len(want)
    assert Z > 40
    col = lambda out, z: list(zip(out[4][:z].tolist(), out[5][:z].tolist(), out[6][:z].tolist(), out[7][:z].tolist()))
    for align in range(8):
        raw = _mem.Raw(eng, device, text, sa, text_off=align, sa_off=(4, 8, 12)[align % 3])
        for route in raw.routes():
            out = guarded_call(raw, route, pats, k, q_off=(align + 3) % 8)
            assert out[0] == OK and out[3] == Z and col(out, Z) == want and out[8].tolist() == wfirst, (route, align)
        C, H = out[1], out[2]
        assert C > 0 and H >= Z
        if align in (0, 5):
            for route in raw.routes():
                out = guarded_call(raw, route, pats, k, cap=0)                 # counts only, output pointers NULL; first complete
                assert out[:4] == (OK, C, H, Z) and out[8].tolist() == wfirst, (route, out[:4])
                out = guarded_call(raw, route, pats, k, cap=Z - 1)             # (the guards stand behind the last written quadruple)
                assert out[:4] == (OK, C, H, Z) and col(out, Z - 1) == want[:-1] and out[8].tolist() == wfirst, route
                out = guarded_call(raw, route, pats, k, cap=Z)
                assert out[:4] == (OK, C, H, Z) and col(out, Z) == want, route
                out = guarded_call(raw, route, pats, k, cap=Z + 1, want_first=False)
                assert out[:4] == (OK, C, H, Z) and col(out, Z) == want and out[8] is None, route
                assert out[4][Z] == out[5][Z] == out[6][Z] == UNWRITTEN32 and out[7][Z] == UNWRITTEN8, "written past Z"
                out = guarded_call(raw, route, pats, k, limit=C, hlimit=H, cap=Z, ws_fill=0xFF)
                assert out[:4] == (OK, C, H, Z) and col(out, Z) == want, route
                out = guarded_call(raw, route, pats, k, limit=C - 1, hlimit=H, cap=Z, ws_fill=0x00)   # refused: nothing is written
                assert out[:4] == (OK, C, 0, 0) and _unwritten(out), (route, out[:4])
                assert (out[8] == 0xA5A5A5A5A5A5A5A5).all(), (route, "first written after a refusal")
                out = guarded_call(raw, route, pats, k, limit=C, hlimit=H - 1, cap=Z, ws_fill=0xFF)
                assert out[:4] == (OK, C, H, 0) and _unwritten(out), (route, out[:4])
                assert (out[8] == 0xA5A5A5A5A5A5A5A5).all(), (route, "first written after a refusal")
        raw.close()


# ---- 3. runs with closed-form answers --------------------------------------------------------------------------------------
def run_of_a(n, m, k):
    """T = a^n, P = a^m: every end e >= m - k is an occurrence with dist = max(0, m - e) from tbegin = max(0, e - m); the
    pieces are runs of a, and a run of L bytes has n - L + 1 places."""
    b = cuts(m, k)
    C = sum(n - (b[t + 1] - b[t]) + 1 for t in range(k + 1))
    return C, [(max(0, e - m), e, max(0, m - e)) for e in range(max(1, m - k), n + 1)]


def run_of_ab(n, M):
    """T = the first n bytes of (ab)^*, P = (ab)^M, k = 1.  An even end e >= 2 M matches exactly from e - 2 M.  An odd end
    e >= 2 M - 1 has T[..e) end in a: P without its last b is T[e - 2 M + 1 .. e) (and P with an a appended is the
    stretch one byte longer on the left: the larger begin wins).  No other end is within one edit: an even end below
    2 M lacks two bytes, and the stretch of 2 M bytes before an odd end is (ba)^M, two edits away.  Both pieces are
    (ab)^(M/2) (M even), found at the even positions p with p + M <= n."""
    assert M % 2 == 0 and n >= 2 * M
    C = 2 * ((n - M) // 2 + 1)
    return C, [(e - 2 * M, e, 0) if e % 2 == 0 else (e - 2 * M + 1, e, 1) for e in range(2 * M - 1, n + 1)]


def closed_forms(eng, device, sizes, routes=("dev", "index_dev", "gindex_dev")):
    i = 0
    assert run_of_a(40, 7, 2)[1] == [x[1:] for x in brute(b"a" * 40, None, [b"a" * 7], 2)[0]]
    assert run_of_ab(41, 4)[1] == [x[1:] for x in brute((b"ab" * 21)[:41], None, [b"ab" * 4], 1)[0]]
    for n in sizes:
        for kind in ("a", "ab"):
            if kind == "a":
                text, sa = b"a" * n, np.arange(n - 1, -1, -1, dtype=np.uint32)
                cases = [([b"a" * 32], 1, *run_of_a(n, 32, 1)), ([b"a" * 33], 3, *run_of_a(n, 33, 3)), ([b"a" * 32], 0, *run_of_a(n, 32, 0))]
            else:
                text = (b"ab" * (n // 2 + 1))[:n]
                odd, even = np.arange(1, n, 2)[::-1], np.arange(0, n, 2)[::-1]     # shorter suffixes first among equal prefixes ...
                sa = naive_table(text) if n <= 300 else None
                # the table of a prefix of (ab)^*: a suffix that is a proper prefix of another sorts before it, so the
                # a-suffixes (even positions) come first, the shortest first, then the b-suffixes likewise
                tab = np.concatenate([even, odd]).astype(np.uint32)
                assert sa is None or np.array_equal(sa, tab)
                sa = tab
                cases = [([b"ab" * 16], 1, *run_of_ab(n, 16))]
            for pats, k, C, want in cases:
                route = routes[i % len(routes)]
                i += 1
                res = run(eng, device, route, text, sa, pats, k, max_hits=(1 << 24) - 1)
                assert res[5] == C, (route, n, kind, k, res[5], C)
                got = list(zip(res[2].tolist(), res[3].tolist(), res[4].tolist()))
                assert got == want, (route, n, kind, k, got[:6], want[:6], len(got), len(want))
                assert res[0].tolist() == [0, len(want)] and not res[1].any() and res[6] >= len(want)
    # a batch that mixes them with stretches of patterns without candidates in between
    n = sizes[0]
    text, sa = b"a" * n, np.arange(n - 1, -1, -1, dtype=np.uint32)
    A, B = b"a" * 32, b"b" * 20
    res = run(eng, device, routes[0], text, sa, [A, B, B, B, A, B, B], 1, max_hits=(1 << 24) - 1)
    one = run_of_a(n, 32, 1)
    assert res[5] == 2 * one[0] and quads(res) == [(0, *x) for x in one[1]] + [(4, *x) for x in one[1]]
    z = len(one[1])
    assert res[0].tolist() == [0, z, z, z, z, 2 * z, 2 * z, 2 * z]


# ---- 4. buffers, streams, threads ------------------------------------------------------------------------------------------
def buffers_and_streams(eng, device, chk, orc):
    """The three device entry points give identical bytes over offset buffers and the three kinds of workspace dirt, on a
    side stream too, and the host routes the same; two threads on one index at once."""
    rng = random.Random(5)
    text = bytes(rng.choice(b"acgt") for _ in range(3000))
    sa = orc.sais(text)
    k = 2
    pats = make_patterns(rng, text, k, 40, lo=12, hi=40, alphabet=list(b"acgt"))
    full = run(eng, device, "dev", text, sa, pats, k)
    accept(chk, text, None, pats, k, full, [1] * len(pats))
    Z = full[1].size
    assert Z >= 20
    for route in ("index_host", "gindex_host"):
        other = run(eng, device, route, text, sa, pats, k)
        assert other[5:] == full[5:] and all(np.array_equal(other[c], full[c]) for c in range(5)), route
    side = torch.cuda.Stream() if str(device).startswith("cuda") else None
    j = 0
    for text_off, u32_off, fill in _buffers.combos():
        raw = _mem.Raw(eng, device, text, sa, text_off=text_off, sa_off=u32_off)
        for route in raw.routes():
            j += 1
            with (torch.cuda.stream(side) if side is not None and j % 2 else contextlib.nullcontext()):
                out = guarded_call(raw, route, pats, k, q_off=(1, 3, 5, 9)[j % 4], out_offs=(u32_off, 4, 12, (0, 1, 2, 3)[j % 4]), ws_fill=fill)
            assert out[:4] == (OK, full[5], full[6], Z), (route, out[:4])
            assert all(np.array_equal(out[4 + c], full[1 + c]) for c in range(4)) and np.array_equal(out[8], full[0]), (route, text_off, fill)
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
                results[w] = host(ix.edit_search(_t(qb, device), _t(qoff.astype(np.int64), device, np.int64), k))
                _sync(device)
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
        assert results[w][5:] == exps[w][5:] and all(np.array_equal(results[w][c], exps[w][c]) for c in range(5)), w
    _sync(device)
    ix.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def workspace_bytes_bound(nq, k, limit, hlimit):
    """The header's closed form: 24 (P + 1) + cand_limit / 7 + 30 hit_limit + 9 MiB with P = nq (k + 1), a cand_limit above
    P * u32::MAX counting as that and a hit_limit above (2 k + 1) cand_limit (or 2^32 - 1) as that."""
    p = nq * (k + 1)
    limit = min(limit, p * 0xFFFFFFFF)
    hlimit = min(hlimit, limit * (2 * k + 1), 0xFFFFFFFF)
    return 24 * (p + 1) + limit // 7 + 30 * hlimit + (9 << 20)


def workspace_bound(eng):
    """Hook-free: sfx_edit_workspace_bytes stays below the header's closed form, and is 0 where nothing can run."""
    f = eng.lib.sfx_edit_workspace_bytes
    for nq in (1, 2, 255, 4097, 1 << 18, 1 << 24):
        for k in (0, 1, 3, 7, 31):
            for limit in (1, 2047, 2048, 2049, 1 << 20, (1 << 28) + 1, 1 << 34, 1 << 40, (1 << 64) - 1):
                for hlimit in (1, 1000, 1 << 20, (1 << 32) - 1, 1 << 40):
                    got = int(f(nq, k, limit, hlimit))
                    assert 0 < got <= workspace_bytes_bound(nq, k, limit, hlimit), (nq, k, limit, hlimit, got)
    assert f(0, 1, 100, 100) == 0 and f(100, 32, 100, 100) == 0 and f(100, 1, 0, 100) == 0 and f(100, 1, 100, 0) == 0
    assert f((1 << 32) - 1, 0, 100, 100) > 0 and f(1 << 32, 0, 100, 100) == 0 and f(1 << 28, 31, 100, 100) == 0


def refusals(eng, device, orc):
    """Every SFX_ERR_* the header names, on every route; nothing is written by a refused call."""
    text = b"abracadabra" * 20
    pats = [b"cadabra", b"abrXcad", b"bra"]
    sa = orc.sais(text)
    raw = _mem.Raw(eng, device, text, sa)
    qb, qoff = pack(pats)
    nq, k = len(pats), 1
    q, qo = _buffers.inp(qb, device, 1), _buffers.inp(qoff, device, 8)
    HL = 1 << 16
    wsb = int(eng.lib.sfx_edit_workspace_bytes(nq, k, 1 << 20, HL))
    ws = _buffers.guarded(wsb, device, 0, 0xA5)
    bufs = [_buffers.guarded(4 * 4096, device, 4, 0xA5) for _ in range(3)] + [_buffers.guarded(4096, device, 1, 0xA5)]
    fb = _buffers.guarded(8 * (nq + 1), device, 8, 0xA5)
    o = [b.ptr for b in bufs]
    bad_order = _buffers.inp(np.array([0, 7, 5, 14], dtype=np.uint64), device, 8)
    too_long = _buffers.inp(np.array([0, 7, (1 << 32) + 8, (1 << 32) + 11], dtype=np.uint64), device, 8)
    short = _buffers.inp(np.array([0, 7, 8, 17], dtype=np.uint64), device, 8)               # a pattern of k bytes
    empty = _buffers.inp(np.array([0, 7, 7, 17], dtype=np.uint64), device, 8)
    st = _buffers.stream_of(device)
    for route in raw.routes():
        c = lambda **kw: raw_call(raw, route, kw.get("q", q.ptr), kw.get("qoff", qo.ptr), kw.get("nq", nq), kw.get("k", k),
                                  kw.get("limit", 1 << 20), kw.get("hlimit", HL), kw.get("outs", o), kw.get("cap", 4096),
                                  kw.get("first", fb.ptr), kw.get("ws", ws.ptr), kw.get("wsb", wsb), st)
        good = c()
        assert good[0] == OK and good[1] > 0 and good[2] >= good[3] > 0, (route, good)
        ws.fill(0xA5)
        for b in bufs + [fb]:
            b.fill(0xA5)
        assert c(limit=0)[0] == ERR_ARG and c(hlimit=0)[0] == ERR_ARG and c(hlimit=1 << 32)[0] == ERR_ARG, route
        assert c(k=32)[0] == ERR_ARG and c(k=0xFFFFFFFF)[0] == ERR_ARG, route
        for j in range(4):
            assert c(outs=[None if i == j else o[i] for i in range(4)])[0] == ERR_ARG, (route, j)
        assert c(q=None)[0] == ERR_ARG and c(qoff=None)[0] == ERR_ARG, route
        assert c(nq=1 << 32)[0] == ERR_TOO_LARGE and c(nq=1 << 28, k=31)[0] == ERR_TOO_LARGE and c(nq=1 << 31, k=1)[0] == ERR_TOO_LARGE, route
        assert c(ws=None)[0] == ERR_WORKSPACE and c(wsb=wsb - 1)[0] == ERR_WORKSPACE and c(wsb=0)[0] == ERR_WORKSPACE, route
        assert c(ws=ctypes.c_void_p(ws.ptr.value + 8), wsb=wsb)[0] == ERR_ARG, route          # large enough, off the boundary
        for j in range(3):
            assert c(outs=[ctypes.c_void_p(o[i].value + 2) if i == j else o[i] for i in range(4)])[0] == ERR_ARG, (route, j)
        assert c(first=ctypes.c_void_p(fb.ptr.value + 4))[0] == ERR_ARG, route                # first off 8 bytes
        assert c(qoff=ctypes.c_void_p(qo.ptr.value + 4))[0] == ERR_ARG, route
        for b in bufs + [fb]:
            assert (b.host() == 0xA5).all(), "a call refused on the host wrote"
        # found on the device, reported through the read-back; the quadruple arrays and first stay as they are
        assert c(qoff=bad_order.ptr)[0] == ERR_ARG, route
        assert c(qoff=too_long.ptr)[0] == ERR_TOO_LARGE, route
        assert c(qoff=short.ptr)[0] == ERR_ARG and c(qoff=empty.ptr)[0] == ERR_ARG, route
        assert c(qoff=short.ptr, k=0)[0] == OK and c(qoff=empty.ptr, k=0)[0] == ERR_ARG, route
        for b in bufs + [fb]:
            b.fill(0xA5)
        assert c(qoff=short.ptr)[0] == ERR_ARG
        # the two limits: the counts come back, nothing is written
        assert c(limit=good[1] - 1) == (OK, good[1], 0, 0), route
        assert c(hlimit=good[2] - 1, wsb=wsb) == (OK, good[1], good[2], 0), route
        for b in bufs + [fb]:
            assert (b.host() == 0xA5).all(), "a call refused on the device wrote"
        # nothing to do: SFX_OK, C = H = Z = 0, first all zero
        assert c(nq=0, q=None, qoff=None, ws=None, wsb=0) == (OK, 0, 0, 0), route
        assert fb.host(np.uint64)[0] == 0 and (fb.host(np.uint64)[1:] == 0xA5A5A5A5A5A5A5A5).all()
        fb.fill(0xA5)
        assert c(cap=0, outs=[None] * 4) == good, route
        assert c(first=None) == good, route
    lib = eng.lib
    none3 = (ctypes.byref(_u64(0)), ctypes.byref(_u64(0)), ctypes.byref(_u64(0)))
    head = (q.ptr, qo.ptr, nq, k, 1 << 20, HL, None, None, None, None, 0, None)
    assert lib.sfx_edit_dev(raw.t.ptr, 1 << 32, raw.s.ptr, *head, *none3, ws.ptr, wsb, st) == ERR_TOO_LARGE
    fb.fill(0xA5)
    assert lib.sfx_edit_dev(raw.t.ptr, 0, raw.s.ptr, *head[:11], fb.ptr, *none3, None, 0, st) == OK                        # n == 0
    _sync(device)
    assert (fb.host(np.uint64) == 0).all()
    assert lib.sfx_edit_dev(None, len(text), raw.s.ptr, *head, *none3, ws.ptr, wsb, st) == ERR_ARG
    assert lib.sfx_edit_dev(raw.t.ptr, len(text), None, *head, *none3, ws.ptr, wsb, st) == ERR_ARG
    for j in range(3):
        assert lib.sfx_edit_dev(raw.t.ptr, len(text), raw.s.ptr, *head, *[None if i == j else none3[i] for i in range(3)], ws.ptr, wsb, st) == ERR_ARG
    for fn in (lib.sfx_index_edit_dev, lib.sfx_gindex_edit_dev):
        assert fn(None, *head, *none3, ws.ptr, wsb, st) == ERR_ARG
    hoff = lambda *v: np.array(v, dtype=np.uint64)
    for fn, h in ((lib.sfx_index_edit, raw.ix._h), (lib.sfx_gindex_edit, raw.gx._h)):
        hc = lambda **kw: fn(kw.get("h", h), kw.get("q", _gsa.ptr(qb)), kw.get("qoff", _gsa.ptr(qoff)), kw.get("nq", nq), kw.get("k", k),
                             kw.get("limit", 1 << 20), kw.get("hlimit", HL), None, None, None, None, kw.get("cap", 0), None, *none3)
        assert hc() == OK
        assert hc(h=None) == ERR_ARG and hc(limit=0) == ERR_ARG and hc(hlimit=0) == ERR_ARG and hc(hlimit=1 << 32) == ERR_ARG
        assert hc(k=32) == ERR_ARG and hc(cap=7) == ERR_ARG and hc(q=None) == ERR_ARG and hc(qoff=None) == ERR_ARG
        assert hc(qoff=_gsa.ptr(hoff(0, 7, 5, 14))) == ERR_ARG and hc(qoff=_gsa.ptr(hoff(0, 7, 8, 17))) == ERR_ARG
        assert hc(qoff=_gsa.ptr(hoff(0, 7, (1 << 32) + 8, (1 << 32) + 11))) == ERR_TOO_LARGE
        assert hc(nq=1 << 32) == ERR_TOO_LARGE and hc(nq=1 << 28, k=31) == ERR_TOO_LARGE
    for b in bufs:
        b.check_guards("refused")
    ws.check_guards("workspace")
    fb.check_guards("first")
    raw.close()


def foreign_table(eng, device):
    """A table with entries < n that is not the text's (sfx_edit_dev takes it as it is): the call stays inside its buffers
    and ends; what it reports is unspecified."""
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
            pats = make_patterns(rng, text, k, 8, lo=3, hi=24, alphabet=[97, 98])
            out = guarded_call(raw, "dev", pats, k, cap=4096)
            assert out[0] == OK and out[1] <= len(pats) * (k + 1) * 500 and out[3] <= out[2] <= out[1] * (2 * k + 1), (kind, out[:4])
            z = min(out[3], 4096)
            assert (out[6][:z] <= 500).all() and (out[5][:z] <= out[6][:z]).all() and (out[4][:z] < len(pats)).all() and (out[7][:z] <= k).all()
        raw.close()


def launch_names(eng, device, orc):
    text = b"abracadabra" * 30
    pats = [b"cadabraabr", b"abrXcadabr", b"zzzzzzzz"]
    sa = orc.sais(text)
    for route in ("dev", "index_dev", "gindex_dev"):
        names = _gsa.profile_names(eng, lambda: run(eng, device, route, text, sa, pats, 1))
        assert KERNELS <= names, (route, sorted(names))
        assert not {x for x in names if x.startswith("ed_")} - KERNELS, sorted(names)
        assert "hm_count" not in names and "hm_emit" not in names


# ---- scale (test_gpu_edit.py, scripts/gpu_edit_time.py) --------------------------------------------------------------------
def scale_patterns(rng, text, k, count, lo=24, hi=64):
    """`count` patterns of lo .. hi bytes: the even ones sampled from the text with 0 .. k + 1 random edits (insertions and
    deletions among them; -> origins (pattern, begin, end, edits)), the odd ones random over the text's alphabet."""
    t = np.frombuffer(text, dtype=np.uint8)
    n = t.size
    alphabet = [int(x) for x in np.unique(t[:1 << 16])]
    g = np.random.default_rng(rng.randrange(1 << 30))
    pats, origins = [], []
    for j in range(count):
        m = rng.randint(lo, hi)
        if j % 2 == 0:
            a = rng.randrange(n - m)
            edits = rng.randint(0, k + 1)
            p = bytes(edit_bytes(rng, bytearray(text[a:a + m]), edits, alphabet, lo))
            origins.append((j, a, a + m, edits))
        else:
            p = np.asarray(alphabet, dtype=np.uint8)[g.integers(0, len(alphabet), m)].tobytes()
        pats.append(p)
    return pats, origins


def check_origins(origins, res, k):
    """Every planted pattern with at most k edits is found with dist <= its edit count and an end within k of its origin's."""
    first, tend, dist = res[0].astype(np.int64), res[3].astype(np.int64), res[4]
    checked = 0
    for j, a, e, edits in origins:
        if edits > k:
            continue
        sl = slice(int(first[j]), int(first[j + 1]))
        near = np.flatnonzero(np.abs(tend[sl] - e) <= k)
        assert near.size and int(dist[sl][near].min()) <= edits, (j, a, e, edits, tend[sl][:8], dist[sl][:8])
        checked += 1
    return checked
