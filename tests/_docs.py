"""The cases of the document counts and the k-common substrings (sfx_doc_counts_*, sfx_common_substrings_*; DESIGN.md
section 23), shared by test_docs_emu.py (the emulator build, host memory) and test_gpu_docs.py (libsuffix_hip.so, HBM).

Nothing expected comes from the engine.  Small collections: `brute_df` (the set of documents of a boundary's interval,
found by walking outwards), `brute_dup` (the definition) and a dictionary of all substrings.  Larger ones: the serial
checker tests/dc_check.c (a stack sweep), and `expected_common`, a numpy reduction with the tie rule of the header over
a df the checker accepted.  The tables of small collections are the definition's (GeneralizedSuffixTable.new_naive)."""
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
from suffix_amd import GeneralizedSuffixTable, SuffixHipError
from suffix_amd import device as sdev

OK, ERR_ARG, ERR_TOO_LARGE, ERR_WORKSPACE = 0, 1, 2, 5
NONE = 0xFFFFFFFF
COUNT_KERNELS = {"docs_check", "docs_argmin", "docs_runs", "docs_counts"}
COMMON_KERNELS = {"docs_longest", "docs_best", "docs_suffix_max"}
KERNELS = COUNT_KERNELS | COMMON_KERNELS
HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
CSRC = os.path.join(HERE, os.pardir, "suffix_amd", "csrc")


def build_emulator():
    """`make -C tests/emu`; sfx_docs.hip (like sfx_lce.hip) is compiled as part of sfx_api.hip's translation unit and
    tests/emu/Makefile does not name it: when either is newer than the library, sfx_api.hip is declared new."""
    lib = os.path.join(EMU_DIR, "libsuffix_emu.so")
    cmd = ["make", "-s", "-j8", "-C", EMU_DIR]
    if os.path.exists(lib) and any(os.path.getmtime(os.path.join(CSRC, f)) > os.path.getmtime(lib) for f in ("sfx_docs.hip", "sfx_lce.hip")):
        cmd += ["-W", "../../suffix_amd/csrc/sfx_api.hip"]
    subprocess.check_call(cmd)
    return lib


def _u32a(x):
    return np.ascontiguousarray(x, dtype=np.uint32)


def _sync(device):
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()


# ---- the known answers -------------------------------------------------------------------------------------------------
def brute_df(da, lcp):
    """Per boundary: the interval by walking outwards while the values stay >= the boundary's, then len(set(da[lb:rb+1]))."""
    n = len(da)
    out = np.zeros(n, dtype=np.uint32)
    for p in range(n):
        v = int(lcp[p]) if p else 0
        lb, rb = 0, n - 1
        if v:
            lb = p - 1
            while lb > 0 and lcp[lb] >= v:
                lb -= 1
            rb = p
            while rb + 1 < n and lcp[rb + 1] >= v:
                rb += 1
        out[p] = len(set(da[lb:rb + 1].tolist()))
    return out


def brute_dup(da, lcp):
    """dup_prefix from the definition: PREV by a dictionary, p(r) by scanning lcp(PREV[r], r] for its last minimum."""
    n = len(da)
    hits = np.zeros(n, dtype=np.int64)
    last = {}
    for r in range(n):
        q = last.get(int(da[r]))
        if q is not None:
            seg = np.asarray(lcp[q + 1:r + 1])
            hits[q + 1 + int(np.flatnonzero(seg == seg.min())[-1])] += 1
        last[int(da[r])] = r
    return np.cumsum(hits).astype(np.uint32)


def brute_common_lens(docs):
    """len[d - 1] from a dictionary of all substrings -> the documents that hold them."""
    occ = {}
    for d, doc in enumerate(docs):
        for i in range(len(doc)):
            for j in range(i + 1, len(doc) + 1):
                occ.setdefault(doc[i:j], set()).add(d)
    ln = [0] * len(docs)
    for s, ds in occ.items():
        for k in range(len(ds)):
            ln[k] = max(ln[k], len(s))
    return ln, occ


def tie_rule_pos(sa, lcp, df, starts, n, lens):
    """pos by the header's rule, from lens (the known answer), one d at a time."""
    out = []
    doc_len = np.diff(np.append(np.asarray(starts, dtype=np.int64), n))
    for d in range(1, len(lens) + 1):
        L = lens[d - 1]
        if L == 0:
            out.append(NONE)
            continue
        hit = [p for p in range(1, n) if df[p] >= d and lcp[p] == L]
        if hit:
            out.append(int(sa[hit[0]]))
        else:
            assert d == 1
            out.append(int(starts[int(np.flatnonzero(doc_len == L)[0])]))
    return out


def expected_common(sa, lcp, df, starts, n):
    """(len, pos) by a numpy reduction over a df that the checker accepted, with the header's tie rule."""
    nd = len(starts)
    sa, lcp, df = (np.asarray(x).astype(np.int64) for x in (sa, lcp, df))
    best_len = np.zeros(nd + 2, dtype=np.int64)
    best_p = np.full(nd + 2, -1, dtype=np.int64)
    if n > 1:
        p = np.arange(1, n)
        keep = (lcp[1:] > 0) & (df[1:] >= 1) & (df[1:] <= nd)
        p = p[keep]
        order = np.lexsort((p, -lcp[p], df[p]))                          # per df: the longest first, among them the smallest p
        p = p[order]
        first = np.flatnonzero(np.r_[True, df[p][1:] != df[p][:-1]]) if p.size else np.zeros(0, dtype=np.int64)
        best_len[df[p[first]]] = lcp[p[first]]
        best_p[df[p[first]]] = p[first]
    ln, pos = np.zeros(nd, dtype=np.uint32), np.full(nd, NONE, dtype=np.uint32)
    cur_len, cur_p = 0, -1
    for d in range(nd, 0, -1):
        if best_len[d] > cur_len or (best_len[d] == cur_len and cur_len and best_p[d] < cur_p):
            cur_len, cur_p = int(best_len[d]), int(best_p[d])
        if cur_len:
            ln[d - 1], pos[d - 1] = cur_len, sa[cur_p]
    doc_len = np.diff(np.append(np.asarray(starts, dtype=np.int64), n))
    if nd and doc_len.max() > ln[0]:
        ln[0], pos[0] = doc_len.max(), int(starts[int(np.argmax(doc_len))])
    return ln, pos


# ---- the checker ---------------------------------------------------------------------------------------------------------
def build_checker(out_dir):
    exe = os.path.join(str(out_dir), "dc_check")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-o", exe, os.path.join(HERE, "dc_check.c")])
    return exe


def run_checker(exe, out_dir, da, lcp, df, dup):
    """-> (exit code, the checker's line)"""
    paths = []
    for name, arr in (("da", da), ("lcp", lcp), ("df", df), ("dup", dup)):
        p = os.path.join(str(out_dir), name + ".bin")
        _u32a(arr).tofile(p)
        paths.append(p)
    r = subprocess.run([exe, *paths], capture_output=True, text=True, timeout=300)
    return r.returncode, (r.stdout + r.stderr).strip()


def accept(exe, out_dir, da, lcp, df, dup):
    rc, line = run_checker(exe, out_dir, da, lcp, df, dup)
    assert rc == 0 and line.startswith("ok"), line


def checker_self_test(exe, out_dir):
    """The checker agrees with the brute-force answers, and names a planted fault in each array at its index."""
    rng = random.Random(3)
    for t in range(40):
        docs = _gsa.random_collection(rng, max_docs=6, max_len=30)
        g = GeneralizedSuffixTable.new_naive(docs)
        da, lcp = g.doc_array(), g.lcp_lens()
        n = len(da)
        df, dup = brute_df(da, lcp), brute_dup(da, lcp)
        accept(exe, out_dir, da, lcp, df, dup)
        if n < 2:
            continue
        x = rng.randrange(n)
        bad = df.copy()
        bad[x] += 1
        rc, line = run_checker(exe, out_dir, da, lcp, bad, dup)
        assert rc == 1 and line.startswith(f"df differs at {x}:"), line
        x = rng.randrange(n)
        bad = dup.copy()
        bad[x:] += 1                                                     # (a prefix sum that is wrong from x on)
        rc, line = run_checker(exe, out_dir, da, lcp, df, bad)
        assert rc == 1 and line.startswith(f"dup_prefix differs at {x}:"), line
        lcp2 = lcp.copy()
        lcp2[0] = 77                                                     # lcp[0] counts as 0
        accept(exe, out_dir, da, lcp2, df, dup)
    rc, line = run_checker(exe, out_dir, [0, 0], [0, 1], [1], [0])
    assert rc == 1 and line.startswith("lengths differ"), line


# ---- the raw ABI over guarded buffers ------------------------------------------------------------------------------------
def doc_counts_raw(eng, device, da, lcp, ndocs, want_df=True, want_dup=True, da_off=4, lcp_off=0, df_off=8, dup_off=12, fill=0xFF,
                   ws_bytes=None, ws_off=0, n=None):
    """-> (rc, df, dup_prefix): every array between guard bands, the workspace exactly as long as stated and pre-filled."""
    da, lcp = _u32a(da), _u32a(lcp)
    n = int(da.size) if n is None else n
    need = int(eng.lib.sfx_doc_counts_workspace_bytes(n))
    b = {"da": _buffers.inp(da, device, da_off), "lcp": _buffers.inp(lcp, device, lcp_off),
         "df": _buffers.guarded(4 * da.size, device, df_off, _buffers.out_fill(fill)),
         "dup": _buffers.guarded(4 * da.size, device, dup_off, _buffers.out_fill(fill)),
         "workspace": _buffers.guarded(need if ws_bytes is None else ws_bytes, device, ws_off, fill)}
    rc = eng.lib.sfx_doc_counts_dev(b["da"].ptr, b["lcp"].ptr, n, ndocs, b["dup"].ptr if want_dup else None, b["df"].ptr if want_df else None,
                                    b["workspace"].ptr, b["workspace"].nbytes, _buffers.stream_of(device))
    _sync(device)
    _buffers.check_all(b)
    assert np.array_equal(b["da"].host(np.uint32), da) and np.array_equal(b["lcp"].host(np.uint32), lcp), "an input was written"
    return rc, b["df"].host(np.uint32), b["dup"].host(np.uint32)


def common_raw(eng, device, sa, lcp, df, starts, fill=0xFF, offs=(4, 8, 12, 4, 12), ws_bytes=None, ws_off=0):
    """-> (rc, len, pos)"""
    sa, lcp, df = _u32a(sa), _u32a(lcp), _u32a(df)
    st = np.ascontiguousarray(starts, dtype=np.uint64)
    n, nd = int(sa.size), int(st.size)
    need = int(eng.lib.sfx_common_substrings_workspace_bytes(nd))
    b = {"sa": _buffers.inp(sa, device, offs[0]), "lcp": _buffers.inp(lcp, device, offs[1]), "df": _buffers.inp(df, device, offs[2]),
         "starts": _buffers.inp(st, device, 8), "len": _buffers.guarded(4 * nd, device, offs[3], _buffers.out_fill(fill)),
         "pos": _buffers.guarded(4 * nd, device, offs[4], _buffers.out_fill(fill)),
         "workspace": _buffers.guarded(need if ws_bytes is None else ws_bytes, device, ws_off, fill)}
    rc = eng.lib.sfx_common_substrings_dev(b["sa"].ptr, b["lcp"].ptr, b["df"].ptr, n, b["starts"].ptr, nd, b["len"].ptr, b["pos"].ptr,
                                           b["workspace"].ptr, b["workspace"].nbytes, _buffers.stream_of(device))
    _sync(device)
    _buffers.check_all(b)
    return rc, b["len"].host(np.uint32), b["pos"].host(np.uint32)


def tables(docs):
    """-> (text, sa, da, lcp, starts uint64) by the definition."""
    g = GeneralizedSuffixTable.new_naive(docs)
    return b"".join(docs), _u32a(g.table()), _u32a(g.doc_array()), _u32a(g.lcp_lens()), _gsa.doc_starts(docs).astype(np.uint64)


def check_collection(eng, device, docs, t=0, host=False):
    """One collection through both calls (the device ABI over guarded buffers, or the host route) against brute force."""
    text, sa, da, lcp, starts = tables(docs)
    n, nd = len(text), len(docs)
    fill = _buffers.FILLS[t % 3]
    if host:
        df, dup = np.full(n, 0xA5A5A5A5, dtype=np.uint32), np.full(n, 0xA5A5A5A5, dtype=np.uint32)
        rc = eng.lib.sfx_doc_counts_u32(_gsa.ptr(da), _gsa.ptr(lcp), n, nd, _gsa.ptr(dup), _gsa.ptr(df))
    else:
        offs = [(4, 0, 8, 12), (8, 4, 12, 4), (12, 8, 4, 8), (4, 12, 8, 4)][t % 4]
        rc, df, dup = doc_counts_raw(eng, device, da, lcp, nd, da_off=offs[0], lcp_off=offs[1], df_off=offs[2], dup_off=offs[3], fill=fill)
    assert rc == OK, (rc, docs)
    exp_df, exp_dup = brute_df(da, lcp), brute_dup(da, lcp)
    assert np.array_equal(df, exp_df), (docs, df.tolist(), exp_df.tolist())
    assert np.array_equal(dup, exp_dup), (docs, dup.tolist(), exp_dup.tolist())
    if n and not host and t % 4 == 0:                                    # one output at a time gives the same bytes
        rc1, df1, _ = doc_counts_raw(eng, device, da, lcp, nd, want_dup=False, fill=fill)
        rc2, _, dup2 = doc_counts_raw(eng, device, da, lcp, nd, want_df=False, fill=fill)
        assert rc1 == OK and rc2 == OK and np.array_equal(df1, exp_df) and np.array_equal(dup2, exp_dup)
    if host:
        ln, pos = np.full(nd, 0xA5A5A5A5, dtype=np.uint32), np.full(nd, 0xA5A5A5A5, dtype=np.uint32)
        rc = eng.lib.sfx_common_substrings_u32(_gsa.ptr(sa), _gsa.ptr(lcp), _gsa.ptr(exp_df), n, _gsa.ptr(starts), nd, _gsa.ptr(ln), _gsa.ptr(pos))
    else:
        rc, ln, pos = common_raw(eng, device, sa, lcp, exp_df, starts, fill=fill)
    assert rc == OK, (rc, docs)
    exp_len, occ = brute_common_lens(docs)
    assert ln.tolist() == exp_len, (docs, ln.tolist(), exp_len)
    assert pos.tolist() == tie_rule_pos(sa, lcp, exp_df, starts, n, exp_len), (docs, pos.tolist())
    for d in range(nd):                                                  # ... and the string stands there, in enough documents
        if exp_len[d]:
            s = text[int(pos[d]):int(pos[d]) + exp_len[d]]
            assert len(occ[s]) >= d + 1, (docs, d, s)
    assert all(ln[d] >= ln[d + 1] for d in range(nd - 1))
    e_len, e_pos = expected_common(sa, lcp, exp_df, starts, n)           # (the large tests' reference agrees with the dictionary)
    assert np.array_equal(e_len, ln) and np.array_equal(e_pos, pos), (docs, e_len.tolist(), e_pos.tolist(), ln.tolist(), pos.tolist())
    return 1


def small_random(eng, device, sigma, count=150, seed=41):
    """Up to 6 documents of 0 - 40 bytes over `sigma` symbols, empty ones included."""
    rng = random.Random(seed + sigma)
    done = 0
    for t in range(count):
        m = rng.randint(1, 6)
        docs = [bytes(97 + rng.randrange(sigma) for _ in range(rng.choice((0, 1, 2, 40)) if rng.random() < 0.2 else rng.randint(0, 40)))
                for _ in range(m)]
        if t % 7 == 3:
            docs[rng.randrange(m)] = b""
        if t % 9 == 4 and m > 1:
            docs[-1] = docs[0]
        done += check_collection(eng, device, docs, t, host=t % 5 == 2)
    return done


# ---- known answers ---------------------------------------------------------------------------------------------------------
def known_answers(eng, device):
    lib = eng.lib
    # one document: every df is 1, len == [n]
    text, sa, da, lcp, starts = tables([b"mississippi"])
    rc, df, dup = doc_counts_raw(eng, device, da, lcp, 1)
    assert rc == OK and (df == 1).all() and np.array_equal(dup, brute_dup(da, lcp)) and int(dup[-1]) == 10
    rc, ln, pos = common_raw(eng, device, sa, lcp, df, starts)
    assert rc == OK and ln.tolist() == [11] and pos.tolist() == [0]
    # k identical documents: every node has df == k, len[d - 1] == |D|
    for k in (2, 5):
        doc = b"abracadabra"
        text, sa, da, lcp, starts = tables([doc] * k)
        rc, df, dup = doc_counts_raw(eng, device, da, lcp, k)
        assert rc == OK and (df == k).all(), df.tolist()
        rc, ln, pos = common_raw(eng, device, sa, lcp, df, starts)
        assert rc == OK and ln.tolist() == [len(doc)] * k and all(text[int(p):int(p) + len(doc)] == doc for p in pos)
    # a^m, a^m: df == 2 on every boundary >= 1 (and at the root), len == [m, m]
    for m in (1, 7, 40):
        text, sa, da, lcp, starts = tables([b"a" * m, b"a" * m])
        rc, df, dup = doc_counts_raw(eng, device, da, lcp, 2)
        assert rc == OK and (df == 2).all() and np.array_equal(dup, brute_dup(da, lcp))
        rc, ln, pos = common_raw(eng, device, sa, lcp, df, starts)
        assert rc == OK and ln.tolist() == [m, m] and pos.tolist() == [int(sa[2 * m - 1])] * 2, (m, ln, pos)
    # no common byte: len[1] == 0, pos[1] == UINT32_MAX
    text, sa, da, lcp, starts = tables([b"abcab", b"xyzzy"])
    rc, df, dup = doc_counts_raw(eng, device, da, lcp, 2)
    rc2, ln, pos = common_raw(eng, device, sa, lcp, df, starts)
    assert rc == OK and rc2 == OK and ln.tolist() == [5, 0] and pos.tolist() == [0, NONE]
    # nothing at all
    assert lib.sfx_doc_counts_dev(None, None, 0, 0, None, None, None, 0, _buffers.stream_of(device)) == OK
    assert lib.sfx_doc_counts_u32(None, None, 0, 3, None, None) == OK
    rc, ln, pos = common_raw(eng, device, [], [], [], [0, 0, 0])
    assert rc == OK and ln.tolist() == [0, 0, 0] and pos.tolist() == [NONE] * 3
    # the public class
    docs = [b"xabcdy", b"", b"zabcdw", b"abcq", b"q"]
    g = GeneralizedSuffixTable.new_naive(docs, engine=eng)
    assert np.array_equal(g.document_counts(), brute_df(g.doc_array(), g.lcp_lens()))
    assert g.common_substring_lengths().tolist() == brute_common_lens(docs)[0] == [6, 4, 3, 0, 0]
    assert g.longest_common_substring(2) == (b"abcd", 2) and g.longest_common_substring(3) == (b"abc", 3)
    assert g.longest_common_substring() == (b"", 0) and g.longest_common_substring(5) == (b"", 0) and g.longest_common_substring(9) == (b"", 0)
    assert g.longest_common_substring(1)[0] in (docs[0], docs[2])
    res = g.query_batch([b"abc", b"q", b"abcd", b"nothing", b""])
    assert g.interval_document_frequency(res["start"], res["end"]).tolist() == res["ndocs"].tolist() == [3, 2, 2, 0, 0]
    assert g.interval_document_frequency(0, g.len()) == 4 and g.interval_document_frequency(3, 3) == 0
    with contextlib.suppress(IndexError):
        g.interval_document_frequency(0, g.len() + 1)
        raise AssertionError("an interval past the table")
    g2 = GeneralizedSuffixTable.new_naive([b"abcab", b"cabx", b"b"], engine=eng)
    assert g2.longest_common_substring() == (b"b", 3) and g2.longest_common_substring(2) == (b"cab", 2)
    empty = GeneralizedSuffixTable.new_naive([b"", b""], engine=eng)
    assert empty.document_counts().size == 0 and empty.common_substring_lengths().tolist() == [0, 0] and empty.longest_common_substring(1) == (b"", 0)
    # the torch-tensor functions
    text, sa, da, lcp, starts = tables(docs)
    t = lambda x: torch.from_numpy(_u32a(x).view(np.int32).copy()).to(device)
    df, dup = sdev.doc_counts(t(da), t(lcp), len(docs), want_prefix=True, engine=eng)
    only = sdev.doc_counts(t(da), t(lcp), len(docs), want_df=False, want_prefix=True, engine=eng)
    ln, pos = sdev.common_substrings(t(sa), t(lcp), df, torch.from_numpy(starts.astype(np.int64)).to(device), engine=eng)
    _sync(device)
    assert np.array_equal(df.cpu().numpy().view(np.uint32), brute_df(da, lcp)) and np.array_equal(dup.cpu().numpy().view(np.uint32), brute_dup(da, lcp))
    assert torch.equal(only, dup) and ln.cpu().numpy().view(np.uint32).tolist() == [6, 4, 3, 0, 0]
    assert sdev.doc_counts_workspace(len(text), device, engine=eng).numel() == lib.sfx_doc_counts_workspace_bytes(len(text))
    with contextlib.suppress(SuffixHipError):
        sdev.doc_counts(t(da), t(lcp), 2, engine=eng)
        raise AssertionError("a da entry >= ndocs was taken")


def arrays_are_made_once(eng):
    """The table keeps (df, dup_prefix) and (len, pos): the first call launches the kernels, later ones nothing."""
    docs = [_gen.english_like(1500, seed=s).tobytes() for s in (1, 2, 1)] + [b""]
    g = GeneralizedSuffixTable.new_naive(docs, engine=eng)
    first = _gsa.profile_names(eng, g.common_substring_lengths)
    assert KERNELS <= first, sorted(first)
    for call in (g.document_counts, g.common_substring_lengths, lambda: g.interval_document_frequency(5, 900)):
        assert _gsa.profile_names(eng, call) == set()
    assert g.common_substring_lengths()[1] == 1500


# ---- refusals and bounds -----------------------------------------------------------------------------------------------------
def refusals(eng, device):
    lib, st = eng.lib, _buffers.stream_of(device)
    rng = random.Random(43)
    docs = [bytes(rng.choice(b"acgt") for _ in range(k)) for k in (30, 0, 200, 30, 200, 0, 30, 200, 30)]
    text, sa, da, lcp, starts = tables(docs)
    n, nd = len(text), len(docs)
    exp_df = brute_df(da, lcp)
    for where, val in ((n // 2, nd), (0, NONE), (n - 1, nd + 5)):
        bad = da.copy()
        bad[where] = val
        rc, _, _ = doc_counts_raw(eng, device, bad, lcp, nd)             # (guard bands checked inside)
        assert rc == ERR_ARG, (rc, where, val)
        out = np.zeros(n, dtype=np.uint32)
        assert lib.sfx_doc_counts_u32(_gsa.ptr(bad), _gsa.ptr(lcp), n, nd, _gsa.ptr(out), None) == ERR_ARG
    assert doc_counts_raw(eng, device, da, lcp, 0)[0] == ERR_ARG
    assert lib.sfx_doc_counts_u32(_gsa.ptr(da), _gsa.ptr(lcp), n, 0, None, None) == ERR_ARG
    assert doc_counts_raw(eng, device, da, lcp, nd + 7)[0] == OK         # more documents than occur: fine
    need = int(lib.sfx_doc_counts_workspace_bytes(n))
    assert need > 0 and lib.sfx_doc_counts_workspace_bytes(0) == 0 and lib.sfx_doc_counts_workspace_bytes(1 << 32) == 0
    for short in (need - 1, 0):
        rc, df, dup = doc_counts_raw(eng, device, da, lcp, nd, ws_bytes=short)
        assert rc == ERR_WORKSPACE and (df == NONE).all() and (dup == NONE).all(), rc
    for ws_off in (1, 4, 8):
        rc, df, dup = doc_counts_raw(eng, device, da, lcp, nd, ws_off=ws_off)
        assert rc == ERR_ARG and (df == NONE).all(), (rc, ws_off)
    for off in (1, 2, 3):
        for kw in ({"da_off": off}, {"lcp_off": off}, {"df_off": off}, {"dup_off": off}):
            assert doc_counts_raw(eng, device, da, lcp, nd, **kw)[0] == ERR_ARG, kw
    assert doc_counts_raw(eng, device, da, lcp, nd, n=1 << 32)[0] == ERR_TOO_LARGE
    assert lib.sfx_doc_counts_u32(_gsa.ptr(da), _gsa.ptr(lcp), 1 << 32, nd, None, None) == ERR_TOO_LARGE
    d_ = _buffers.inp(da, device, 4)
    w_ = _buffers.guarded(need, device, 0, 0xFF)
    assert lib.sfx_doc_counts_dev(None, d_.ptr, n, nd, None, None, w_.ptr, need, st) == ERR_ARG
    assert lib.sfx_doc_counts_dev(d_.ptr, None, n, nd, None, None, w_.ptr, need, st) == ERR_ARG
    assert lib.sfx_doc_counts_dev(d_.ptr, d_.ptr, n, nd, None, None, None, need, st) == ERR_WORKSPACE
    assert (w_.host() == 0xFF).all()
    # the common substrings: doc_starts, ndocs, workspace, alignment
    for bad_starts in ([1] + starts.tolist()[1:], starts.tolist()[:3] + [2] + starts.tolist()[4:], starts.tolist()[:-1] + [n + 1]):
        rc, ln, pos = common_raw(eng, device, sa, lcp, exp_df, bad_starts)
        assert rc == ERR_ARG and (ln == NONE).all() and (pos == NONE).all(), (rc, bad_starts)
    need = int(lib.sfx_common_substrings_workspace_bytes(nd))
    assert 0 < need <= 8 * nd + 1024 and lib.sfx_common_substrings_workspace_bytes(0) == 0
    assert common_raw(eng, device, sa, lcp, exp_df, starts, ws_bytes=need - 1)[0] == ERR_WORKSPACE
    assert common_raw(eng, device, sa, lcp, exp_df, starts, ws_off=8)[0] == ERR_ARG
    for k in range(5):
        offs = [4, 8, 12, 4, 12]
        offs[k] = 2
        assert common_raw(eng, device, sa, lcp, exp_df, starts, offs=tuple(offs))[0] == ERR_ARG, k
    assert common_raw(eng, device, sa, lcp, exp_df, [])[0] == ERR_ARG     # ndocs == 0 with n > 0
    one = np.zeros(1, dtype=np.uint32)
    assert lib.sfx_common_substrings_u32(_gsa.ptr(sa), _gsa.ptr(lcp), _gsa.ptr(exp_df), 1 << 32, _gsa.ptr(starts), nd, _gsa.ptr(one), _gsa.ptr(one)) == ERR_TOO_LARGE
    assert lib.sfx_common_substrings_u32(_gsa.ptr(sa), _gsa.ptr(lcp), None, n, _gsa.ptr(starts), nd, _gsa.ptr(one), _gsa.ptr(one)) == ERR_ARG
    # a df that is not this collection's: entries of 0 and above ndocs are passed over, nothing leaves its arrays
    wild = exp_df.copy()
    wild[::3] = 0
    wild[1::3] = NONE
    rc, ln, pos = common_raw(eng, device, sa, lcp, wild, starts)
    assert rc == OK and ln[0] == max(len(d) for d in docs)


def corrupted_lcp(eng, device):
    """lcp is not verified: random words, UINT32_MAX everywhere, small random values -- every call returns SFX_OK, the
    guard bands stay intact (checked inside the raw calls), and dup_prefix is still what the definition gives for the
    array as stored (df is the interval search's business)."""
    rng = random.Random(44)
    nrng = np.random.default_rng(44)
    docs = [bytes(rng.choice(b"ab") for _ in range(rng.choice((0, 1, 40, 130)))) for _ in range(14)]
    text, sa, da, lcp, starts = tables(docs)
    n, nd = len(text), len(docs)
    for t, bad in enumerate((nrng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), np.full(n, NONE, dtype=np.uint32),
                             nrng.integers(0, 3, n).astype(np.uint32), nrng.integers(0, 2 * n, n).astype(np.uint32))):
        rc, df, dup = doc_counts_raw(eng, device, da, bad, nd, fill=_buffers.FILLS[t % 3], lcp_off=(0, 4, 8, 12)[t])
        assert rc == OK
        assert np.array_equal(dup, brute_dup(da, bad)), t
        rc, ln, pos = common_raw(eng, device, sa, bad, df, starts, fill=_buffers.FILLS[t % 3])
        assert rc == OK
        rc, ln, pos = common_raw(eng, device, nrng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), bad, brute_df(da, lcp), starts)
        assert rc == OK


def dirty_workspace_and_streams(eng, device):
    """The same collection over the three kinds of dirt in a workspace of exactly the stated size, outputs at every
    offset, on the current and on a side stream: the same bytes every time."""
    rng = random.Random(45)
    docs = [_gen.english_like(rng.choice((1, 300, 900)), seed=s).tobytes() for s in range(7)] + [b"", b"the same", b"the same"]
    text, sa, da, lcp, starts = tables(docs)
    nd = len(docs)
    exp_df, exp_dup = brute_df(da, lcp), brute_dup(da, lcp)
    exp_len, exp_pos = expected_common(sa, lcp, exp_df, starts, len(text))
    side = torch.cuda.Stream() if str(device).startswith("cuda") else None
    for t in range(6):
        with (torch.cuda.stream(side) if side is not None and t % 2 else contextlib.nullcontext()):
            rc, df, dup = doc_counts_raw(eng, device, da, lcp, nd, fill=_buffers.FILLS[t % 3], da_off=(4, 8, 12)[t % 3], lcp_off=(0, 4, 8, 12)[t % 4],
                                         df_off=(12, 4, 8)[t % 3], dup_off=(8, 12, 4)[t % 3])
            assert rc == OK and np.array_equal(df, exp_df) and np.array_equal(dup, exp_dup), t
            rc, ln, pos = common_raw(eng, device, sa, lcp, df, starts, fill=_buffers.FILLS[t % 3], offs=((4, 8, 12, 4, 12), (12, 4, 8, 8, 4))[t % 2])
            assert rc == OK and np.array_equal(ln, exp_len) and np.array_equal(pos, exp_pos), t


def cross_check_queries(eng, device, count=1000, seed=46):
    """The engine's existing count (the linear pass over PREV of sfx_gindex_query) against two reads of dup_prefix, for
    substrings of the collection, a third of them altered, 1 - 12 bytes."""
    rng = random.Random(seed)
    docs = [_gen.dna(rng.choice((1, 150, 400)), seed=s).tobytes() for s in range(8)] + [b"", _gen.dna(400, seed=2).tobytes()[50:300]]
    text, sa, da, lcp, starts = tables(docs)
    g = GeneralizedSuffixTable.new_naive(docs, engine=eng)
    rc, _, dup = doc_counts_raw(eng, device, da, lcp, len(docs), want_df=False)
    assert rc == OK
    qs = []
    for k in range(count):
        a = rng.randrange(len(text))
        q = bytearray(text[a:a + rng.randint(1, 12)])
        if k % 3 == 0:
            q[rng.randrange(len(q))] = rng.choice(b"acgtn")
        qs.append(bytes(q))
    res = g.query_batch(qs)
    s, e = res["start"].astype(np.int64), res["end"].astype(np.int64)
    found = e > s
    assert found.sum() > count // 2 and (~found).sum() > 10
    d = dup.astype(np.int64)
    via = np.where(found, (e - s) - (d[np.maximum(e, 1) - 1] - d[s]), 0)
    assert np.array_equal(via, res["ndocs"].astype(np.int64)), np.flatnonzero(via != res["ndocs"])[:5]
    assert np.array_equal(g.interval_document_frequency(s, e), res["ndocs"])
    return count


def launch_names(eng, device):
    docs = [_gen.dna(700, seed=s).tobytes() for s in (1, 2, 3)]
    text, sa, da, lcp, starts = tables(docs)

    def run():
        rc, df, _ = doc_counts_raw(eng, device, da, lcp, 3)
        assert rc == OK and common_raw(eng, device, sa, lcp, df, starts)[0] == OK
    names = _gsa.profile_names(eng, run)
    assert KERNELS <= names, sorted(names)
    assert {x for x in names if x.startswith("docs_")} == KERNELS, sorted(names)
    assert {"gsa_prev", "lce_levels", "gsa_scan", "tree_intervals"} <= names, sorted(names)


def size_bound(eng):
    """Hook-free: 32 n <= sfx_doc_counts_workspace_bytes(n) <= 34 n + 9 MiB (the header's bound, from the carve)."""
    assert "SFX_LCE_FAN" not in os.environ
    f = eng.lib.sfx_doc_counts_workspace_bytes
    for n in (1, 2, 31, 33, 1025, 32769, 100003, 1 << 20, (1 << 20) + 5, (1 << 24) + 1, 10 ** 8, 10 ** 9, (1 << 32) - 1):
        got = int(f(n))
        assert 32 * n <= got <= 34 * n + (9 << 20), (n, got)
    assert f(0) == 0 and f(1 << 32) == 0


# ---- synthetic arrays: PREV distances and interval ends placed by hand ---------------------------------------------------------
def synthetic(eng, device, exe, out_dir, sizes=(2, 3, 31, 32, 33, 64, 65, 1023, 1025, 2049, 4097, 5000), seed=47):
    """da / lcp that belong to no text: PREV distances of 1, of exactly a node (32, 1024) and one more or less, and of
    nearly the whole array; minima that sit on the first and last word of a node and repeat (the rightmost counts);
    sa and lcp entries above 2^31, which len / pos carry through unchanged."""
    nrng = np.random.default_rng(seed)
    for t, n in enumerate(sizes):
        lcp = (nrng.integers(0, 1 << 20, n) >> nrng.integers(0, 20, n)).astype(np.uint32) + np.uint32(2)
        for e in range(0, n, 32):                                        # equal minima at both ends of every node
            lcp[e] = 1
            lcp[min(e + 31, n - 1)] = 1
        lcp[nrng.integers(0, n, 1 + n // 40)] = 0
        if t % 3 == 0:
            lcp[n // 2:] = np.uint32(0x80000000) + lcp[n // 2:]            # values above 2^31
        nd = (2, 3, 40, n)[t % 4]
        da = nrng.integers(0, nd, n).astype(np.uint32)
        for dist in (1, 31, 32, 33, 1023, 1024, 1025, n - 1):             # a document seen at exactly these two ranks
            if dist < n and nd > 3:
                r = int(nrng.integers(dist, n))
                doc = nd + dist
                da[r - dist], da[r] = doc, doc
        nd_all = int(da.max()) + 1
        rc, df, dup = doc_counts_raw(eng, device, da, lcp, nd_all, fill=_buffers.FILLS[t % 3], lcp_off=(0, 4, 8, 12)[t % 4])
        assert rc == OK, (rc, n)
        exp = brute_dup(da, lcp)
        assert np.array_equal(dup, exp), (n, np.flatnonzero(dup != exp)[:4])
        accept(exe, out_dir, da, lcp, df, dup)
        sa = (np.uint32(0xFFFFFFFF) - nrng.permutation(n).astype(np.uint32))          # "positions" up to 2^32 - 1
        starts = np.zeros(nd_all, dtype=np.uint64)
        rc, ln, pos = common_raw(eng, device, sa, lcp, df, starts)
        assert rc == OK
        e_len, e_pos = expected_common(sa, lcp, df, starts, n)
        assert np.array_equal(ln, e_len) and np.array_equal(pos, e_pos), (n, ln[:4], e_len[:4], pos[:4], e_pos[:4])


def hooked(eng, device, exe, out_dir):
    """What a hooked child process runs (SFX_LCE_FAN, SFX_MAX_GRID): the random, known and synthetic cases again."""
    known_answers(eng, device)
    small_random(eng, device, 2, count=40, seed=51)
    small_random(eng, device, 3, count=30, seed=52)
    synthetic(eng, device, exe, out_dir, sizes=(2, 5, 33, 65, 1025, 3000))
    corrupted_lcp(eng, device)
