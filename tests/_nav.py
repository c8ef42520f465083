"""The cases of the suffix-tree navigation calls (sfx_lce_substr*, sfx_lce_lca*, sfx_lce_range_argmin*, sfx_suffix_links_*;
DESIGN.md section 28), shared by test_nav_emu.py (the emulator build, host memory) and test_gpu_nav.py
(libsuffix_hip.so, HBM).

Nothing expected comes from the calls under test.  Small texts are answered by brute force over the sorted (truncated)
suffixes -- which ranks start with the substring -- and larger ones go through the serial checker tests/nav_check.c,
which reads sa and lcp only.  The tables handed to the engine are the oracle's and, for collections, the definition's."""
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
import _lce as L
import _tree
from suffix_amd import GeneralizedSuffixTable, SuffixTable, SuffixTree
from suffix_amd import device as sdev

OK, ERR_ARG, ERR_TOO_LARGE, ERR_WORKSPACE = 0, 1, 2, 5
NONE = 0xFFFFFFFF
QUERY_KERNELS = {"nav_substr", "nav_lca", "nav_argmin"}
KERNELS = QUERY_KERNELS | {"nav_home", "nav_slink"}
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, os.pardir, "suffix_amd", "csrc")
_vp, _u64 = ctypes.c_void_p, ctypes.c_uint64
_u32a = L._u32a


def build_emulator():
    """`make -C tests/emu`; sfx_nav.hip and sfx_lce.hip are compiled as part of sfx_api.hip's translation unit and
    tests/emu/Makefile does not name the former, so when one is newer than the library sfx_api.hip is declared new."""
    lib = os.path.join(L.EMU_DIR, "libsuffix_emu.so")
    cmd = ["make", "-s", "-j8", "-C", L.EMU_DIR]
    if os.path.exists(lib) and any(os.path.getmtime(os.path.join(CSRC, f)) > os.path.getmtime(lib) for f in ("sfx_nav.hip", "sfx_lce.hip")):
        cmd += ["-W", L.CSRC_FROM_EMU + "/sfx_api.hip"]
    subprocess.check_call(cmd)
    return lib


def _sync(device):
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()


def _dev(x, device):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32).copy()).to(device)


def _host(t, device):
    _sync(device)
    return t.cpu().numpy().view(np.uint32)


# ---- the checker -----------------------------------------------------------------------------------------------------------
def build_checker(out_dir):
    so = os.path.join(str(out_dir), "libnav_check.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "nav_check.c")])
    lib = ctypes.CDLL(so)
    i64p = ctypes.POINTER(ctypes.c_int64)
    lib.nav_open.restype = _vp
    lib.nav_open.argtypes = [_vp, _vp, _u64, _vp, _u64]
    lib.nav_close.restype = None
    lib.nav_close.argtypes = [_vp]
    for name, args in (("nav_check_substr", [_vp, _vp, _vp, _u64, _vp, _vp, _vp, i64p]), ("nav_check_lca", [_vp, _vp, _vp, _u64, _vp, _vp, _vp, i64p]),
                       ("nav_check_argmin", [_vp, _vp, _vp, _u64, _vp, i64p]), ("nav_check_slink", [_vp, _u64, _vp, _vp, _vp, _vp, i64p])):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = args
    lib.nav_check_name.restype = ctypes.c_char_p
    lib.nav_check_name.argtypes = [ctypes.c_int]
    return lib


class Checker:
    """nav_check.c over one (sa, lcp[, starts]): every method -> (verdict, index of the first wrong answer or -1)."""

    def __init__(self, chk, sa, lcp, starts=None):
        self.chk, self.sa, self.lcp = chk, _u32a(sa), _u32a(lcp)
        self.starts = None if starts is None else np.ascontiguousarray(starts, dtype=np.uint64)
        self.h = chk.nav_open(_gsa.ptr(self.sa), _gsa.ptr(self.lcp), self.sa.size, _gsa.ptr(self.starts) if self.starts is not None else None,
                              0 if self.starts is None else self.starts.size)
        assert self.h, "nav_check: sa is no permutation"

    def _run(self, fn, *arrays, lead=()):
        arrays = [_u32a(x) for x in arrays]
        where = ctypes.c_int64(-2)
        rc = fn(self.h, *lead, *[_gsa.ptr(x) for x in arrays], ctypes.byref(where))
        return self.chk.nav_check_name(rc).decode(), int(where.value)

    def substr(self, pos, ln, lo, hi, depth):
        return self._run(lambda h, p, l, a, b, d, w: self.chk.nav_check_substr(h, p, l, len(pos), a, b, d, w), pos, ln, lo, hi, depth)

    def lca(self, a, b, lo, hi, depth):
        return self._run(lambda h, p, l, x, y, d, w: self.chk.nav_check_lca(h, p, l, len(a), x, y, d, w), a, b, lo, hi, depth)

    def argmin(self, lo, hi, arg):
        return self._run(lambda h, a, b, g, w: self.chk.nav_check_argmin(h, a, b, len(lo), g, w), lo, hi, arg)

    def slink(self, node_lb, node_rb, node_depth, slink):
        return self._run(lambda h, a, b, d, s, w: self.chk.nav_check_slink(h, len(node_lb), a, b, d, s, w), node_lb, node_rb, node_depth, slink)

    def close(self):
        h, self.h = self.h, None
        if h:
            self.chk.nav_close(h)


def accept(verdict, what, *show):
    name, where = verdict
    assert name == "ok", f"nav_check ({what}): {name} at {where}: {[tuple(int(x[where]) for x in show)] if where >= 0 else ''}"


def checker_self_test(chk, orc):
    """One fault per mode, each named; and the faultless lists pass."""
    text = b"abcabdabcabd__abcabe"
    n = len(text)
    sa, lcp = L.tables(orc, text)
    c = Checker(chk, sa, lcp)
    sfx = suffixes(text, sa)
    pos, ln = _u32a([0, 0, 3, 14, 5, 20, 21, 19, 0]), _u32a([2, 5, 1, 6, 0, 0, 0, 2, 21])
    good = np.array([brute_substr(sfx, lcp, text, sa, None, int(p), int(k)) for p, k in zip(pos, ln)], dtype=np.uint32).T
    assert c.substr(pos, ln, *good) == ("ok", -1)
    assert good[:, 5].tolist() == [0, n, 0] and good[:, 6].tolist() == [NONE] * 3 and good[:, 7].tolist() == [NONE] * 3
    shape = {"a rank lies outside the interval", "the left boundary is not below", "the right boundary is not below", "a boundary inside is below"}
    for q, col, delta, names in ((0, 0, 1, shape), (0, 0, -1, shape), (0, 1, 1, shape), (0, 1, -1, shape), (2, 0, -1, shape), (3, 1, 1, shape),
                                 (1, 2, 1, {"wrong depth"}), (3, 2, -1, {"wrong depth"}), (4, 1, -1, {"wrong mark"}), (6, 0, 1, {"wrong mark"}),
                                 (8, 2, 1, {"wrong mark"})):
        bad = good.copy()
        bad[col, q] = (int(bad[col, q]) + delta) & NONE
        got = c.substr(pos, ln, *bad)
        assert got[0] in names and got[1] == q, (q, col, delta, got)
    seen = set()
    for l in range(n):                                                   # every interval around "ab" but the right one, each fault by name
        for h in range(l + 1, n + 1):
            if (l, h) != (int(good[0, 0]), int(good[1, 0])):
                got = c.substr(pos[:1], ln[:1], [l], [h], good[2, :1])
                assert got[0] in shape and got[1] == 0, (l, h, got)
                seen.add(got[0])
    assert seen == shape, seen
    a, b = _u32a([0, 6, 3, 3, 13, 20]), _u32a([6, 14, 9, 3, 0, 0])
    good = np.array([brute_lca(sfx, text, sa, None, int(i), int(j)) for i, j in zip(a, b)], dtype=np.uint32).T
    assert c.lca(a, b, *good) == ("ok", -1) and good[:, 5].tolist() == [NONE] * 3
    for q, col, delta, names in ((0, 2, 1, {"wrong depth"}), (0, 1, 1, shape), (0, 0, -1, shape), (1, 0, 1, shape), (3, 1, 1, {"a rank lies outside the interval"}),
                                 (5, 2, 1, {"wrong mark"}), (4, 0, 1, {"the left boundary is not below"}), (4, 1, -1, {"the right boundary is not below"})):
        bad = good.copy()
        bad[col, q] = (int(bad[col, q]) + delta) & NONE
        got = c.lca(a, b, *bad)
        assert got[0] in names and got[1] == q, (q, col, delta, got, good[:, q])
    flat = _u32a([7, 3, 5, 3, 9, 3, 8])
    c2 = Checker(chk, np.arange(7), flat)
    assert c2.argmin([0, 2, 4, 5, 3], [7, 5, 5, 5, 8], [1, 3, 4, NONE, NONE]) == ("ok", -1)
    assert c2.argmin([0], [7], [3]) == ("a smaller index attains the minimum", 0)
    assert c2.argmin([0], [7], [2]) == ("not the minimum", 0)
    assert c2.argmin([2], [7], [1]) == ("a rank lies outside the interval", 0)
    assert c2.argmin([5], [5], [5]) == ("wrong mark", 0)
    c2.close()
    bsa, blcp = L.tables(orc, b"banana")
    cb = Checker(chk, bsa, blcp)                                         # nodes: root, "a" [0,2], "ana" [1,2], "na" [4,5]
    lb, rb, dp = [0, 0, 1, 4], [5, 2, 2, 5], [0, 1, 3, 2]
    assert cb.slink(lb, rb, dp, [NONE, 0, 3, 1]) == ("ok", -1)
    assert cb.slink(lb, rb, dp, [0, 0, 3, 1]) == ("wrong mark", 0)
    assert cb.slink(lb, rb, dp, [NONE, 1, 3, 1]) == ("the root is the target of depth 1 alone", 1)
    assert cb.slink(lb, rb, dp, [NONE, 0, 0, 1]) == ("the root is the target of depth 1 alone", 2)
    assert cb.slink(lb, rb, dp, [NONE, 0, 1, 1]) == ("the target's depth is not d - 1", 2)
    assert cb.slink(lb, rb, dp, [NONE, 0, 3, 9]) == ("wrong mark", 3)
    assert cb.slink([0, 0, 1, 4, 3], [5, 2, 2, 5, 3], [0, 1, 3, 2, 2], [NONE, 0, 4, 1, 1]) == ("the target does not hold the shortened suffix", 2)
    cb.close()
    c.close()


# ---- the known answer --------------------------------------------------------------------------------------------------------
def _isa(sa):
    return L.expected_isa(sa)


def suffixes(text, sa, starts=None):
    """The (truncated) suffixes in rank order."""
    n = len(text)
    return [text[p:L.end_of(p, n, starts)] for p in np.asarray(sa).tolist()]


def _starting_with(sfx, pat):
    hit = [r for r, s in enumerate(sfx) if s.startswith(pat)]
    assert hit and hit[-1] - hit[0] + 1 == len(hit), "the ranks of a prefix are consecutive"
    return hit[0], hit[-1] + 1


def brute_substr(sfx, lcp, text, sa, starts, pos, ln):
    n = len(text)
    if ln == 0:
        return (0, n, 0) if pos <= n else (NONE, NONE, NONE)
    if pos >= n or ln > L.end_of(pos, n, starts) - pos:
        return NONE, NONE, NONE
    lo, hi = _starting_with(sfx, text[pos:pos + ln])
    if hi - lo == 1:
        return lo, hi, L.end_of(pos, n, starts) - pos
    # the lowest node at or below the locus spells the longest common prefix of the interval's first and last suffix
    a, b = sfx[lo], sfx[hi - 1]
    d = next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), min(len(a), len(b)))
    return lo, hi, d


def brute_lca(sfx, text, sa, starts, i, j):
    n = len(text)
    if i >= n or j >= n:
        return NONE, NONE, NONE
    if i == j:
        r = int(np.flatnonzero(np.asarray(sa) == i)[0])
        return r, r + 1, L.end_of(i, n, starts) - i
    d = L.brute(text, i, j, 0, starts)
    if d == 0:
        return 0, n, 0
    lo, hi = _starting_with(sfx, text[i:i + d])
    return lo, hi, d


def brute_slinks(text, sa, nodes):
    """For every node of the table the id of the node that spells its string without the first byte."""
    lb, dp = nodes["node_lb"].tolist(), nodes["node_depth"].tolist()
    spell = [text[sa[lb[k]]:sa[lb[k]] + dp[k]] for k in range(len(lb))]
    by = {s: k for k, s in enumerate(spell)}
    assert len(by) == len(spell) and by[b""] == 0
    return _u32a([NONE if not s else by[s[1:]] for s in spell])


def query_list(n, rng, starts=None, limit=500):
    """Every (pos, len) with pos <= n + 1 and len up to one past the room where the text has at most 40 bytes, else
    `limit` drawn ones; then the specials."""
    if n <= 40:
        q = [(p, k) for p in range(n + 2) for k in range(0, max(L.end_of(p, n, starts) - p, 0) + 2 if p < n else 2)]
    else:
        q = []
        for _ in range(limit):
            p = rng.randrange(n)
            room = L.end_of(p, n, starts) - p
            q.append((p, rng.choice((1, 2, 3, room, room + 1, rng.randint(0, room), rng.randint(1, min(room, 12))))))
    q += [(n, 0), (n, 1), (n + 1, 0), (0, 0), (NONE, 0), (0, NONE), (max(n, 1) - 1, 1), (max(n, 1) - 1, 2)]
    return _u32a([x[0] for x in q]), _u32a([x[1] for x in q])


# ---- the raw ABI over guarded buffers -------------------------------------------------------------------------------------
class Nx(L.Lx):
    """_lce.Lx with the navigation calls: inputs and the three outputs between guard bands of their own."""

    def _call3(self, name, a, b, want_depth=True, out_off=4):
        a, b = _u32a(a), _u32a(b)
        nq = int(a.size)
        fn = getattr(self.eng.lib, name + ("" if self.host else "_dev"))
        if self.host:
            outs = [np.full(nq, 0xDEADBEEF, dtype=np.uint32) for _ in range(3)]
            rc = fn(self.h, _gsa.ptr(a), _gsa.ptr(b), nq, _gsa.ptr(outs[0]), _gsa.ptr(outs[1]), _gsa.ptr(outs[2]) if want_depth else None)
            assert rc == OK, rc
            return outs if want_depth else outs[:2]
        bufs = {"in0": _buffers.inp(a, self.device, 4), "in1": _buffers.inp(b, self.device, 12)}
        for k, off in zip(("lo", "hi", "depth"), (out_off, 8, 12)):
            bufs[k] = _buffers.guarded(4 * nq, self.device, off, "count")
        rc = fn(self.h, bufs["in0"].ptr, bufs["in1"].ptr, nq, bufs["lo"].ptr, bufs["hi"].ptr, bufs["depth"].ptr if want_depth else None,
                _buffers.stream_of(self.device))
        assert rc == OK, rc
        _buffers.check_all(bufs)
        _buffers.check_all(getattr(self, "bufs", {}))
        outs = [bufs[k].host(np.uint32) for k in ("lo", "hi", "depth")]
        if not want_depth:
            assert np.array_equal(bufs["depth"].host(), _buffers.guarded(4 * nq, "cpu", 12, "count").host()), "depth was written"
        return outs if want_depth else outs[:2]

    def substr(self, pos, ln, **kw):
        return self._call3("sfx_lce_substr", pos, ln, **kw)

    def lca(self, a, b, **kw):
        return self._call3("sfx_lce_lca", a, b, **kw)

    def argmin(self, lo, hi, out_off=8):
        rc, out = self._call("sfx_lce_range_argmin", [_u32a(lo), _u32a(hi)], out_off)
        assert rc == OK, rc
        return out


def links_raw(eng, device, lx, sa, nodes, ws_bytes=None, ws_fill=0xFF, ws_off=0, out_off=4, host=False, lcp=None):
    """sfx_suffix_links_dev over guarded buffers (sfx_suffix_links_u32 when host) -> (status, slink)."""
    lb, rb, dp = (_u32a(nodes[k]) for k in ("node_lb", "node_rb", "node_depth"))
    m = int(lb.size)
    if host:
        out = np.full(m, 0xDEADBEEF, dtype=np.uint32)
        rc = eng.lib.sfx_suffix_links_u32(_gsa.ptr(_u32a(sa)), _gsa.ptr(_u32a(lcp)), len(sa), m, _gsa.ptr(lb), _gsa.ptr(rb), _gsa.ptr(dp), _gsa.ptr(out))
        return rc, out
    need = int(eng.lib.sfx_suffix_links_workspace_bytes(len(sa)))
    b = {"sa": _buffers.inp(_u32a(sa), device, 8), "lb": _buffers.inp(lb, device, 4), "rb": _buffers.inp(rb, device, 12),
         "depth": _buffers.inp(dp, device, 4), "slink": _buffers.guarded(4 * m, device, out_off, "count"),
         "workspace": _buffers.guarded(need if ws_bytes is None else ws_bytes, device, ws_off, ws_fill)}
    rc = eng.lib.sfx_suffix_links_dev(lx.h, b["sa"].ptr, m, b["lb"].ptr, b["rb"].ptr, b["depth"].ptr, b["slink"].ptr, b["workspace"].ptr,
                                      b["workspace"].nbytes, _buffers.stream_of(device))
    _buffers.check_all(b)
    _buffers.check_all(getattr(lx, "bufs", {}))
    return rc, b["slink"].host(np.uint32)


def same(got, exp, what, *ctx):
    for name, g, e in zip(("lo", "hi", "depth"), got, exp):
        bad = np.flatnonzero(np.asarray(g) != np.asarray(e))
        assert bad.size == 0, (what, name, int(bad[0]), [int(x[bad[0]]) for x in ctx], int(g[bad[0]]), int(e[bad[0]]))


def check_text(eng, device, orc, text, sa, lcp, starts=None, rng=None, host=False, lcp_off=0, limit=500, tree=True):
    """One handle: every query of query_list and as many LCA pairs against brute force, argmins against numpy, and -- for
    a plain text -- every suffix link and the SuffixTree methods."""
    rng = rng or random.Random(len(text))
    n = len(text)
    sfx = suffixes(text, sa, starts)
    lx = Nx(eng, device, sa, lcp, starts, host=host, lcp_off=lcp_off)
    assert lx.rc == OK, (lx.rc, n)
    try:
        pos, ln = query_list(n, rng, starts, limit)
        exp = np.array([brute_substr(sfx, lcp, text, sa, starts, int(p), int(k)) for p, k in zip(pos, ln)], dtype=np.uint32).T
        same(lx.substr(pos, ln), exp, ("substr", n, host, text[:40], starts), pos, ln)
        same(lx.substr(pos, ln, want_depth=False), exp[:2], ("substr without depth", n), pos, ln)
        a, b = L.pair_list(n, rng, min(limit, 300)) if n else (_u32a([0, 1]), _u32a([0, 0]))
        exp = np.array([brute_lca(sfx, text, sa, starts, int(i), int(j)) for i, j in zip(a, b)], dtype=np.uint32).T
        same(lx.lca(a, b), exp, ("lca", n, host, text[:40], starts), a, b)
        lo, hi = L.edge_ranges(n, rng, extra=40)
        exp = _u32a([l + int(np.argmin(lcp[l:h])) if l < h <= n else NONE for l, h in zip(lo.tolist(), hi.tolist())])
        got = lx.argmin(lo, hi)
        assert np.array_equal(got, exp), ("argmin", n, np.flatnonzero(got != exp)[:4])
        if starts is None and n and tree:
            nodes = _tree.tree_u32(eng, text, sa, lcp)
            want = brute_slinks(text, np.asarray(sa).tolist(), nodes)
            rc, got = links_raw(eng, device, lx, sa, nodes, host=host, lcp=lcp, ws_fill=_buffers.FILLS[n % 3], out_off=(4, 8, 12)[n % 3])
            assert rc == OK and np.array_equal(got, want), ("slink", n, text[:40], got[:8], want[:8])
    finally:
        lx.close()
    return pos.size


def check_classes(eng, orc, text, rng, loci=40):
    """SuffixTree.suffix_link / .lca / .locus and the SuffixTable calls on one text against brute force."""
    n = len(text)
    sa, lcp = L.tables(orc, text)
    sfx = suffixes(text, sa)
    st = SuffixTable.from_parts(text, sa, engine=eng)
    tree = SuffixTree.from_suffix_table(st)
    nodes = tree.arrays
    spell = lambda nd: text[sa[nd.rank]:] if nd.id is None else text[sa[nodes["node_lb"][nd.id]]:sa[nodes["node_lb"][nd.id]] + int(nodes["node_depth"][nd.id])]
    internal = [nd for nd in tree.root().preorder() if nd.id is not None]
    for nd in internal:
        link = nd.suffix_link()
        if nd.is_root():
            assert link is None
        else:
            assert link.id is not None and spell(link) == spell(nd)[1:], (text, spell(nd), spell(link))
            assert link == tree.suffix_link(nd)
    if n:
        assert tree.arrays["suffix_link"].dtype == np.uint32 and tree.arrays["suffix_link"].size == len(internal)
    everything = list(tree.root().preorder())
    leaf = next((nd for nd in everything if nd.id is None), None)
    if leaf is not None:
        with contextlib.suppress(ValueError):
            leaf.suffix_link()
            raise AssertionError("a leaf has no suffix link here")
    for _ in range(loci if n else 0):
        p = rng.randrange(n)
        k = rng.randint(1, min(n - p, 8)) if rng.random() < 0.7 else rng.randint(1, n - p)
        lo, hi, d = brute_substr(sfx, lcp, text, sa, None, p, k)
        assert st.substring_interval(p, k) == (lo, hi) and st.substring_count(p, k) == hi - lo
        nd = tree.locus(p, k)
        s = spell(nd)
        assert s.startswith(text[p:p + k]) and len(s) == d, (text, p, k, s, d)
        assert (nd.id is None) == (hi - lo == 1)
        if nd.id is None:
            assert nd.rank == lo and nd in tree._node(nd.parent_id).children()
        assert len(spell(list(nd.ancestors())[1])) < k, "the locus is the HIGHEST node that starts with the substring"
        x, y = rng.choice(everything), rng.choice(everything)
        got = tree.lca(x, y)
        above_y = set(y.ancestors())
        common = [z for z in x.ancestors() if z in above_y]
        assert got == common[0], (text, spell(x), spell(y), spell(got), spell(common[0]))
    assert tree.locus(0, 0) == tree.root() and tree.locus(n, 0) == tree.root()
    with contextlib.suppress(IndexError):
        tree.locus(n, 1)
        raise AssertionError("a locus outside the text")
    if n:
        i, j = rng.randrange(n), rng.randrange(n)
        assert st.lca(i, j) == brute_lca(sfx, text, sa, None, i, j)
        l, h = sorted((rng.randrange(n), rng.randrange(n)))
        assert st.lcp_range_argmin(l, h + 1) == l + int(np.argmin(st.lcp_lens()[l:h + 1])) and st.lcp_range_argmin(h, h) == NONE


# ---- 1. known answers ------------------------------------------------------------------------------------------------------
def known_answers(eng, device, orc):
    sa, lcp = L.tables(orc, b"banana")                                   # a ana anana banana na nana
    for host in (False, True):
        lx = Nx(eng, device, sa, lcp, host=host)
        assert [x.tolist() for x in lx.substr([1, 0, 6, 5], [3, 6, 0, 2])] == [[1, 3, 0, NONE], [3, 4, 6, NONE], [3, 6, 0, NONE]]
        assert [x.tolist() for x in lx.lca([1, 1, 0, 7], [3, 1, 1, 0])] == [[1, 2, 0, NONE], [3, 3, 6, NONE], [3, 5, 0, NONE]]
        assert lx.argmin([0, 1, 4, 3, 1], [6, 4, 6, 3, 3]).tolist() == [0, 3, 4, NONE, 1]
        nodes = _tree.tree_u32(eng, b"banana", sa, lcp)
        spell = [b"banana"[sa[l]:sa[l] + d] for l, d in zip(nodes["node_lb"].tolist(), nodes["node_depth"].tolist())]
        assert sorted(spell) == [b"", b"a", b"ana", b"na"]
        rc, sl = links_raw(eng, device, lx, sa, nodes, host=host, lcp=lcp)
        assert rc == OK
        link = {spell[k]: (None if w == NONE else spell[w]) for k, w in enumerate(sl.tolist())}
        assert link == {b"": None, b"a": b"", b"ana": b"na", b"na": b"a"}, link
        lx.close()
    sa, lcp = L.tables(orc, b"aaaa")
    lx = Nx(eng, device, sa, lcp)
    nodes = _tree.tree_u32(eng, b"aaaa", sa, lcp)
    assert nodes["node_lb"].tolist()[:2] == [0, 0] and nodes["node_rb"].tolist()[:2] == [3, 3] and nodes["node_depth"].tolist()[:2] == [0, 1]
    rc, sl = links_raw(eng, device, lx, sa, nodes)
    assert rc == OK and sl.tolist() == [NONE, 0, 1, 2], sl                   # (the depth-1 node links to the root, not to itself)
    lx.close()
    # the public classes
    st = SuffixTable.from_parts(b"banana", orc.sais(b"banana"), engine=eng)
    assert st.substring_interval(1, 3) == (1, 3) and st.substring_count(1, 3) == 2 and st.lca(1, 3) == (1, 3, 3) and st.lca(2, 2) == (5, 6, 4)
    assert [x.tolist() for x in st.substring_intervals_batch([1, 5], [3, 2])] == [[1, NONE], [3, NONE], [3, NONE]]
    assert st.lcp_range_argmin(1, 4) == 3 and st.lcp_range_argmin(1, 3) == 1 and st.lcp_range_argmin_batch([4, 3], [6, 3]).tolist() == [4, NONE]
    with contextlib.suppress(IndexError):
        st.substring_interval(5, 2)
        raise AssertionError("a substring past the end")
    tree = SuffixTree.from_suffix_table(st)
    ana = tree.locus(1, 3)
    assert tree.label(ana) == b"na" and tree.label(ana.suffix_link()) == b"na" and ana.suffix_link().suffix_link() == tree.locus(5, 1)
    assert tree.locus(5, 1).suffix_link() == tree.root() and tree.root().suffix_link() is None
    assert tree.locus(0, 2).rank == 3 and tree.locus(0, 2).parent_id == 0
    assert tree.lca(tree.locus(1, 5), tree.locus(3, 3)) == ana and tree.lca(ana, tree.locus(0, 1)) == tree.root()
    unary = SuffixTree.from_suffix_table(SuffixTable.from_parts(b"aaaa", orc.sais(b"aaaa"), engine=eng))
    one = unary.locus(0, 1)
    assert one.id == 1 and one.suffix_link() == unary.root() and unary.lca(one, unary.root()) == unary.root()
    assert unary.lca(unary.locus(0, 3), unary.locus(0, 2)) == unary.locus(0, 2)
    docs = [b"abcab", b"", b"cabx", b"b"]
    g = GeneralizedSuffixTable.new_naive(docs, engine=eng)
    text, gsa, glcp, starts = L.collection_tables(docs)
    sfx = suffixes(text, gsa, starts)
    assert g.substring_interval((0, 3), 2) == brute_substr(sfx, glcp, text, gsa, starts, 3, 2)[:2] and g.substring_count((2, 1), 2) == 3
    assert g.lca((0, 0), (0, 3)) == brute_lca(sfx, text, gsa, starts, 0, 3) and g.lcp_range_argmin(0, len(text)) == 0
    with contextlib.suppress(IndexError):
        g.substring_interval((0, 3), 3)
        raise AssertionError("a substring past its document's end")
    # the torch-tensor classes
    sa, lcp = L.tables(orc, b"mississippi")
    sfx = suffixes(b"mississippi", sa)
    ix = sdev.LceDeviceIndex(_dev(sa, device), _dev(lcp, device), engine=eng)
    got = [_host(x, device).tolist() for x in ix.substr(_dev([1, 2, 11], device), _dev([4, 1, 1], device))]
    assert list(zip(*got)) == [brute_substr(sfx, lcp, b"mississippi", sa, None, p, k) for p, k in ((1, 4), (2, 1), (11, 1))]
    got = [_host(x, device).tolist() for x in ix.lca(_dev([1, 2], device), _dev([4, 2], device))]
    assert list(zip(*got)) == [brute_lca(sfx, b"mississippi", sa, None, 1, 4), brute_lca(sfx, b"mississippi", sa, None, 2, 2)]
    assert _host(ix.range_argmin(_dev([0, 5], device), _dev([11, 5], device)), device).tolist() == [0, NONE]
    nodes = _tree.tree_u32(eng, b"mississippi", sa, lcp)
    sl = sdev.suffix_links(ix, _dev(sa, device), *[_dev(nodes[k], device) for k in ("node_lb", "node_rb", "node_depth")],
                           workspace=sdev.suffix_links_workspace(11, device, eng))
    assert np.array_equal(_host(sl, device), brute_slinks(b"mississippi", sa.tolist(), nodes))
    ix.close()


def handle_is_made_once(eng, orc):
    """The table's cached handle serves the new calls: after the first one nothing but the query kernel is launched."""
    text = _gen.english_like(5000).tobytes()
    st = SuffixTable.from_parts(text, orc.sais(text), engine=eng)
    st.lce(3, 700)
    for call, kernel in ((lambda: st.substring_interval(100, 5), "nav_substr"), (lambda: st.substring_intervals_batch([1, 2], [9, 40]), "nav_substr"),
                         (lambda: st.lca(10, 4000), "nav_lca"), (lambda: st.lcp_range_argmin(10, 4000), "nav_argmin")):
        names = _gsa.profile_names(eng, call)
        assert names == {kernel}, sorted(names)
    g = GeneralizedSuffixTable.new_naive([text[:1500], b"", text[700:2900]], engine=eng)
    g.lce((0, 3), (2, 40))
    assert _gsa.profile_names(eng, lambda: g.substring_count((0, 5), 3)) == {"nav_substr"}
    assert _gsa.profile_names(eng, lambda: g.lca((0, 5), (2, 800))) == {"nav_lca"}


# ---- 2. random small texts and collections -----------------------------------------------------------------------------------
def small_random(eng, device, orc, count=152, seed=41):
    rng = random.Random(seed)
    done = 0
    for t in range(count):
        sigma = (1, 2, 3, 4)[t % 4]
        n = rng.choice((0, 1, 2, 3, 5, 17, 22, 33, 40, 64, 65, 100, 300)) if t % 3 else rng.randint(0, 300)
        text = bytes(rng.randrange(sigma) + 97 for _ in range(n))
        sa, lcp = L.tables(orc, text)
        check_text(eng, device, orc, text, sa, lcp, rng=rng, host=t % 5 == 2, lcp_off=(0, 4, 8, 12)[t % 4], limit=500)
        if t % 6 == 0:
            check_classes(eng, orc, text[:120], rng, loci=25)
        done += 1
    return done


def small_collections(eng, device, orc, count=64, seed=42):
    rng = random.Random(seed)
    done = 0
    while done < count:
        docs = _gsa.random_collection(rng, max_docs=12, max_len=20)
        if done % 3 == 0:
            docs = [b""] + docs[:4] + [b"a", b""] + docs[4:] + [b"b", b""]
        if not sum(len(d) for d in docs):
            continue
        text, sa, lcp, starts = L.collection_tables(docs)
        check_text(eng, device, orc, text, sa, lcp, starts, rng=rng, host=done % 4 == 1, lcp_off=(0, 4)[done % 2], limit=300)
        done += 1
    return done


# ---- 3. sizes at the level edges: synthetic arrays against the definition ------------------------------------------------------
def expected_bounds(lcp, r, d):
    n = len(lcp)
    if d == 0:
        return 0, n
    below = np.flatnonzero(lcp < d)
    below = below[below > 0]
    k = int(np.searchsorted(below, r, side="right"))
    return (int(below[k - 1]) if k else 0), (int(below[k]) if k < below.size else n)


def level_edges(eng, device, sizes=L.LEVEL_EDGES, seed=43, fan=32):
    """A random permutation as the table and an LCP landscape of plateaus (40 .. 59) with sparse dips, so that intervals
    span whole nodes and levels; ranks at node and level edges, lengths at the values around them.  lcp[0] holds
    0xFFFFFFFF, then 0: the same answers."""
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    for t, n in enumerate(sizes):
        sa = nrng.permutation(n).astype(np.uint32)
        lcp = nrng.integers(40, 60, n).astype(np.uint32)
        if n:
            dips = nrng.integers(0, n, 1 + n // 300)
            lcp[dips] = nrng.integers(1 if t % 2 else 0, 35, dips.size)
        ranks = sorted({r for r in [0, 1, n - 2, n - 1, n // 2] + [e + o for f in (fan, fan * fan, fan ** 3) for e in range(0, n, f) for o in (-1, 0, 1)
                                                                    if e // f < 4 or e + 4 * f > n] + [rng.randrange(max(n, 1)) for _ in range(60)]
                        if 0 <= r < n})
        pos, ln = [], []
        for r in ranks:
            room = n - int(sa[r])
            for d in {int(lcp[r]), int(lcp[r]) + 1, int(lcp[r + 1]) if r + 1 < n else 1, (int(lcp[r + 1]) if r + 1 < n else 1) + 1, 1, 2, 36, 45, 61}:
                pos.append(int(sa[r]))
                ln.append(min(max(d, 1), room))
        pos, ln = _u32a(pos), _u32a(ln)
        isa = _isa(sa)
        for first in (NONE, 0):
            if n:
                lcp[0] = first
            B = lcp.copy()
            if n:
                B[0] = 0
            exp = []
            for p, d in zip(pos.tolist(), ln.tolist()):
                lo, hi = expected_bounds(B, int(isa[p]), d)
                exp.append((lo, hi, n - p if hi - lo == 1 else int(lcp[lo + 1:hi].min())))
            exp = np.array(exp, dtype=np.uint32).reshape(-1, 3).T
            if n > 64 and t % 2:
                assert ((exp[0] == 0) & (exp[1] == n)).any(), "no query spans the whole array"
            for host, lcp_off in ((False, (0, 4, 8, 12)[t % 4]), (True, 0)) if n < 2000 else ((False, (0, 4)[t % 2]),):
                lx = Nx(eng, device, sa, lcp, host=host, lcp_off=lcp_off)
                assert lx.rc == OK, (lx.rc, n)
                same(lx.substr(pos, ln), exp, ("level edges", n, host, lcp_off, first), pos, ln)
                # LCA of the suffixes at two ranks: the minimum between them, then its interval
                a = _u32a([sa[r] for r in ranks])
                b = _u32a([sa[rng.choice(ranks)] for _ in ranks])
                want = []
                for i, j in zip(a.tolist(), b.tolist()):
                    ra, rb = sorted((int(isa[i]), int(isa[j])))
                    if ra == rb:
                        want.append((ra, ra + 1, n - i))
                    else:
                        d = int(lcp[ra + 1:rb + 1].min())
                        want.append((*expected_bounds(B, ra, d), d))
                same(lx.lca(a, b), np.array(want, dtype=np.uint32).reshape(-1, 3).T, ("level edges: lca", n, host, first), a, b)
                lo, hi = L.edge_ranges(n, rng, fan=fan, extra=60)
                want = _u32a([l + int(np.argmin(lcp[l:h])) if l < h <= n else NONE for l, h in zip(lo.tolist(), hi.tolist())])
                got = lx.argmin(lo, hi)
                assert np.array_equal(got, want), ("level edges: argmin", n, first, np.flatnonzero(got != want)[:4])
                lx.close()


# ---- 4. edge texts -----------------------------------------------------------------------------------------------------------
def unary(eng, device, orc, n=1500):
    """a^n in closed form: (pos, len) -> [len - 1, n); m = n nodes, the depth-d node links to the depth-(d - 1) node."""
    text = b"a" * n
    sa, lcp = L.tables(orc, text)
    rng = np.random.default_rng(44)
    pos = rng.integers(0, n, 400)
    ln = np.minimum(rng.integers(1, n + 1, 400), n - pos)
    for host in (False, True):
        lx = Nx(eng, device, sa, lcp, host=host)
        lo, hi, depth = lx.substr(pos, ln)
        assert np.array_equal(lo, ln - 1) and (hi == n).all(), (host, np.flatnonzero(lo != ln - 1)[:4])
        assert np.array_equal(depth, ln), "the node at the locus of a^len is a^len itself"
        nodes = _tree.tree_u32(eng, text, sa, lcp)
        assert nodes["node_lb"].size == n and nodes["node_depth"].tolist() == list(range(n))
        rc, sl = links_raw(eng, device, lx, sa, nodes, host=host, lcp=lcp)
        assert rc == OK and sl.tolist() == [NONE] + list(range(n - 1))
        lx.close()


def edge_texts(eng, device, orc, n=1500, limit=300):
    rng = random.Random(45)
    half = bytes(rng.randrange(97, 100) for _ in range(n // 2 - 1))
    for text in (L.fibonacci(n), b"x" + half + b"y" + half, b"ab" * (n // 2) + b"a"):     # (two halves that differ in their first byte only)
        sa, lcp = L.tables(orc, text)
        check_text(eng, device, orc, text, sa, lcp, rng=rng, limit=limit, lcp_off=4)
    check_classes(eng, orc, L.fibonacci(200), rng, loci=30)


# ---- 5. refusals and bounds ----------------------------------------------------------------------------------------------------
def refusals(eng, device, orc):
    text = _gen.dna(700, seed=9).tobytes()
    n = len(text)
    sa, lcp = L.tables(orc, text)
    lib, st = eng.lib, _buffers.stream_of(device)
    lx = Nx(eng, device, sa, lcp)
    nodes = _tree.tree_u32(eng, text, sa, lcp)
    m = int(nodes["node_lb"].size)
    # every NONE case of the definitions
    lo, hi, d = lx.substr([n, n, n + 1, 0, 5, n - 1, NONE, 3], [0, 1, 0, n + 1, NONE, 2, 0, n - 3])
    assert lo[:7].tolist() == [0, NONE, NONE, NONE, NONE, NONE, NONE] and hi[:7].tolist() == [n] + [NONE] * 6 and d[:7].tolist() == [0] + [NONE] * 6
    assert lo[7] != NONE
    lo, hi, d = lx.lca([n, 0, NONE, n + 1], [0, n, 0, n + 1])
    assert (lo == NONE).all() and (hi == NONE).all() and (d == NONE).all()
    assert lx.argmin([0, 5, 5, 0, n], [n + 1, 5, 4, 0, n]).tolist() == [NONE] * 5
    q = _buffers.inp(_u32a([1, 2, 3]), device, 4)
    o = _buffers.guarded(12, device, 4, 0xA5)
    for fn in (lib.sfx_lce_substr_dev, lib.sfx_lce_lca_dev):
        assert fn(None, q.ptr, q.ptr, 3, o.ptr, o.ptr, o.ptr, st) == ERR_ARG
        assert fn(lx.h, None, q.ptr, 3, o.ptr, o.ptr, o.ptr, st) == ERR_ARG and fn(lx.h, q.ptr, None, 3, o.ptr, o.ptr, o.ptr, st) == ERR_ARG
        assert fn(lx.h, q.ptr, q.ptr, 3, None, o.ptr, o.ptr, st) == ERR_ARG and fn(lx.h, q.ptr, q.ptr, 3, o.ptr, None, o.ptr, st) == ERR_ARG
        assert fn(lx.h, q.ptr, q.ptr, 3, o.ptr, o.ptr, _vp(o.ptr.value + 2), st) == ERR_ARG
        assert fn(lx.h, _vp(q.ptr.value + 1), q.ptr, 3, o.ptr, o.ptr, o.ptr, st) == ERR_ARG
        assert fn(lx.h, None, None, 0, None, None, None, st) == OK
    assert lib.sfx_lce_range_argmin_dev(None, q.ptr, q.ptr, 3, o.ptr, st) == ERR_ARG
    assert lib.sfx_lce_range_argmin_dev(lx.h, q.ptr, None, 3, o.ptr, st) == ERR_ARG
    assert lib.sfx_lce_range_argmin_dev(lx.h, q.ptr, q.ptr, 3, _vp(o.ptr.value + 3), st) == ERR_ARG
    assert lib.sfx_lce_range_argmin_dev(lx.h, None, None, 0, None, st) == OK
    hq, ho = _u32a([1, 2, 3]), np.full(3, 0xA5A5A5A5, dtype=np.uint32)
    assert lib.sfx_lce_substr(None, _gsa.ptr(hq), _gsa.ptr(hq), 3, _gsa.ptr(ho), _gsa.ptr(ho), None) == ERR_ARG
    assert lib.sfx_lce_lca(lx.h, _gsa.ptr(hq), None, 3, _gsa.ptr(ho), _gsa.ptr(ho), None) == ERR_ARG
    assert lib.sfx_lce_range_argmin(lx.h, None, _gsa.ptr(hq), 3, _gsa.ptr(ho)) == ERR_ARG
    assert lib.sfx_lce_substr(lx.h, None, None, 0, None, None, None) == OK
    assert (ho == 0xA5A5A5A5).all() and (o.host() == 0xA5).all(), "a refused call wrote"
    o.check_guards("refused")
    # suffix links: a collection handle, a short / missing / misaligned workspace, missing arrays, nothing to do
    need = int(lib.sfx_suffix_links_workspace_bytes(n))
    assert 4 * n <= need <= 4 * n + (64 << 10)
    gx = Nx(eng, device, sa, lcp, np.array([0, 5, n], dtype=np.uint64))
    assert gx.rc == OK and links_raw(eng, device, gx, sa, nodes)[0] == ERR_ARG
    gx.close()
    for short in (need - 1, 0):
        rc, sl = links_raw(eng, device, lx, sa, nodes, ws_bytes=short)
        assert rc == ERR_WORKSPACE
    assert links_raw(eng, device, lx, sa, nodes, ws_off=8)[0] == ERR_ARG and links_raw(eng, device, lx, sa, nodes, out_off=2)[0] == ERR_ARG
    w = _buffers.guarded(need, device, 0, 0xFF)
    s_ = _buffers.inp(sa, device, 4)
    nb = [_buffers.inp(_u32a(nodes[k]), device, 4) for k in ("node_lb", "node_rb", "node_depth")]
    out = _buffers.guarded(4 * m, device, 4, 0xA5)
    assert lib.sfx_suffix_links_dev(None, s_.ptr, m, nb[0].ptr, nb[1].ptr, nb[2].ptr, out.ptr, w.ptr, need, st) == ERR_ARG
    assert lib.sfx_suffix_links_dev(lx.h, None, m, nb[0].ptr, nb[1].ptr, nb[2].ptr, out.ptr, w.ptr, need, st) == ERR_ARG
    assert lib.sfx_suffix_links_dev(lx.h, s_.ptr, m, nb[0].ptr, None, nb[2].ptr, out.ptr, w.ptr, need, st) == ERR_ARG
    assert lib.sfx_suffix_links_dev(lx.h, s_.ptr, m, nb[0].ptr, nb[1].ptr, nb[2].ptr, None, w.ptr, need, st) == ERR_ARG
    assert lib.sfx_suffix_links_dev(lx.h, s_.ptr, m, nb[0].ptr, nb[1].ptr, nb[2].ptr, out.ptr, None, need, st) == ERR_WORKSPACE
    assert lib.sfx_suffix_links_dev(lx.h, None, 0, None, None, None, None, None, 0, st) == OK
    assert (out.host() == 0xA5).all(), "a refused call wrote"
    assert lib.sfx_suffix_links_u32(None, None, 0, 0, None, None, None, None) == OK
    assert lib.sfx_suffix_links_u32(_gsa.ptr(sa), _gsa.ptr(lcp), n, 0, None, None, None, None) == OK
    assert lib.sfx_suffix_links_u32(_gsa.ptr(sa), None, n, m, _gsa.ptr(hq), _gsa.ptr(hq), _gsa.ptr(hq), _gsa.ptr(ho)) == ERR_ARG
    assert lib.sfx_suffix_links_u32(_gsa.ptr(sa), _gsa.ptr(lcp), 1 << 32, m, _gsa.ptr(hq), _gsa.ptr(hq), _gsa.ptr(hq), _gsa.ptr(ho)) == ERR_TOO_LARGE
    assert lib.sfx_suffix_links_workspace_bytes(0) == 0 and lib.sfx_suffix_links_workspace_bytes(1 << 32) == 0
    lx.close()
    # the empty index
    for host in (False, True):
        e = Nx(eng, device, [], [], host=host)
        assert [x.tolist() for x in e.substr([0, 0, 1], [0, 1, 0])] == [[0, NONE, NONE], [0, NONE, NONE], [0, NONE, NONE]]
        assert [x.tolist() for x in e.lca([0], [0])] == [[NONE]] * 3 and e.argmin([0], [0]).tolist() == [NONE]
        e.close()


def workspace_bound(eng):
    f = eng.lib.sfx_suffix_links_workspace_bytes
    for n in (1, 2, 31, 33, 1025, 100003, (1 << 20) + 5, 10 ** 9, (1 << 32) - 1):
        assert 4 * n <= int(f(n)) <= 4 * n + (64 << 10), (n, int(f(n)))


def corrupted(eng, device, orc):
    """lcp is not verified and may be changed behind the handle's back; a node table may be anything: every call returns,
    writes inside its outputs, and leaves lo <= rank < hi <= n, argmins inside their ranges and links < nodes or NONE."""
    rng = random.Random(46)
    nrng = np.random.default_rng(46)
    docs = [bytes(rng.choice(b"ab") for _ in range(rng.choice((0, 1, 40, 130)))) for _ in range(14)]
    text, gsa, _, starts = L.collection_tables(docs)
    n = len(text)
    psa = _u32a(orc.sais(text))
    real = _u32a(orc.lcp_kasai(text, psa))
    nodes = _tree.tree_u32(eng, text, psa, real)
    m = int(nodes["node_lb"].size)
    pos, ln = query_list(n, rng, None, 600)
    a, b = L.pair_list(n, rng, 400)
    lo_, hi_ = L.edge_ranges(n, rng, extra=60)
    for starts_ in (None, starts):
        sa = psa if starts_ is None else gsa
        isa = _isa(sa)
        for lcp in (nrng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), np.full(n, NONE, dtype=np.uint32),
                    nrng.integers(0, 2 * n, n).astype(np.uint32), np.zeros(n, dtype=np.uint32), real):
            for changed in (False, True):
                lx = Nx(eng, device, sa, lcp, starts_, lcp_off=4)
                assert lx.rc == OK
                if changed:                                               # the borrowed level 0 no longer matches the levels above
                    lx.bufs["lcp"].load(nrng.integers(0, 200, n).astype(np.uint32))
                lo, hi, _ = lx.substr(pos, ln)
                for p, k, l, h in zip(pos.tolist(), ln.tolist(), lo.tolist(), hi.tolist()):
                    if l != NONE and k:
                        assert l <= isa[p] < h <= n, (p, k, l, h)
                lo, hi, _ = lx.lca(a, b)
                for i, j, l, h in zip(a.tolist(), b.tolist(), lo.tolist(), hi.tolist()):
                    if l != NONE:
                        assert l <= min(isa[i], isa[j]) < h <= n, (i, j, l, h)      # (the smaller rank: bounds starts from it)
                got = lx.argmin(lo_, hi_)
                for l, h, g in zip(lo_.tolist(), hi_.tolist(), got.tolist()):
                    assert (l <= g < h) if l < h <= n else g == NONE, (l, h, g)
                if starts_ is None:
                    shuffled = {k: v[nrng.permutation(m)] for k, v in nodes.items() if k in ("node_lb", "node_rb", "node_depth")}
                    wild = {"node_lb": nrng.integers(0, n + 3, m).astype(np.uint32), "node_rb": nrng.integers(0, n + 3, m).astype(np.uint32),
                            "node_depth": nrng.integers(0, 6, m).astype(np.uint32)}
                    wild["node_rb"][:4], wild["node_lb"][:4] = [n, NONE, 3, n - 1], [0, 0, 5, 0]
                    for table in (nodes, shuffled, wild):
                        rc, sl = links_raw(eng, device, lx, sa, table, ws_fill=_buffers.FILLS[m % 3])
                        assert rc == OK and ((sl < m) | (sl == NONE)).all()
                        if table is wild:
                            assert sl[0] == NONE and sl[1] == NONE and sl[2] == NONE
                lx.close()


def dirty_workspaces(eng, device, orc):
    text = _gen.near_duplicates(3000).tobytes()
    sa, lcp = L.tables(orc, text)
    nodes = _tree.tree_u32(eng, text, sa, lcp)
    want = brute_slinks(text, sa.tolist(), nodes)
    lx = Nx(eng, device, sa, lcp)
    for fill in _buffers.FILLS + (0xA5,):
        rc, sl = links_raw(eng, device, lx, sa, nodes, ws_fill=fill)               # exactly the stated size, between guard bands
        assert rc == OK and np.array_equal(sl, want), fill
    lx.close()


def streams_and_threads(eng, device, orc):
    text = _gen.english_like(4000).tobytes()
    n = len(text)
    sa, lcp = L.tables(orc, text)
    rng = random.Random(47)
    sfx = suffixes(text, sa)
    pos, ln = query_list(n, rng, None, 300)
    exp = np.array([brute_substr(sfx, lcp, text, sa, None, int(p), int(k)) for p, k in zip(pos, ln)], dtype=np.uint32).T
    nodes = _tree.tree_u32(eng, text, sa, lcp)
    want = brute_slinks(text, sa.tolist(), nodes)
    side = torch.cuda.Stream() if str(device).startswith("cuda") else None
    for t in range(2):
        with (torch.cuda.stream(side) if side is not None and t % 2 else contextlib.nullcontext()):
            lx = Nx(eng, device, sa, lcp, lcp_off=(0, 4)[t])
            same(lx.substr(pos, ln), exp, ("stream", t), pos, ln)
            rc, sl = links_raw(eng, device, lx, sa, nodes)
            assert rc == OK and np.array_equal(sl, want)
            lx.close()
    ix = sdev.LceDeviceIndex(_dev(sa, device), _dev(lcp, device), engine=eng)
    dp, dl = _dev(pos, device), _dev(ln, device)
    results, errors = [None, None], []

    def worker(j):
        try:
            for _ in range(3):
                got = ix.substr(dp, dl) if j == 0 else ix.lca(dp, dp)
                results[j] = [_host(x, device) for x in got]
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
    same(results[0], exp, "two threads")
    isa = _isa(sa)
    own = np.where(pos < n, isa[np.minimum(pos, n - 1)], NONE)
    assert np.array_equal(results[1][0], own) and np.array_equal(results[1][1], np.where(pos < n, own + 1, NONE))
    ix.close()


def launch_names(eng, device, orc):
    text = _gen.dna(3000, seed=3).tobytes()
    sa, lcp = L.tables(orc, text)
    nodes = _tree.tree_u32(eng, text, sa, lcp)
    lx = Nx(eng, device, sa, lcp)

    def queries():
        lx.substr([1, 2], [5, 9])
        lx.lca([0], [2000])
        lx.argmin([7], [900])
    names = _gsa.profile_names(eng, queries)
    assert names == QUERY_KERNELS, sorted(names)
    names = _gsa.profile_names(eng, lambda: links_raw(eng, device, lx, sa, nodes))
    assert names == {"nav_home", "nav_slink"}, sorted(names)
    lx.close()


def hooked(eng, device, orc):
    """What a hooked child process runs (SFX_LCE_FAN, SFX_MAX_GRID): the random and edge cases again over deep trees."""
    fan = int(os.environ.get("SFX_LCE_FAN", "32"))
    known_answers(eng, device, orc)
    small_random(eng, device, orc, count=30, seed=51)
    small_collections(eng, device, orc, count=10, seed=52)
    level_edges(eng, device, sizes=(0, 1, 2, 3, 4, 5, 31, 33, 64, 65, 1025, 4097, 5000), fan=fan)
    unary(eng, device, orc, n=700)
    edge_texts(eng, device, orc, n=1200, limit=150)


# ---- scale (test_gpu_nav.py) -------------------------------------------------------------------------------------------------
def scale_queries(n, sa, lcp, nq, seed, ends=None):
    """nq (pos, len): positions uniform; half of the lengths at the places an off-by-one shows -- lcp[r], lcp[r] + 1,
    lcp[r + 1], lcp[r + 1] + 1, 1, 2, end - pos --, the rest uniform in 1 .. 64; all clipped to 1 .. end - pos."""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, n, nq)
    isa = _isa(sa).astype(np.int64)
    r = isa[pos]
    room = (n if ends is None else ends[pos]) - pos
    nxt = lcp[np.minimum(r + 1, n - 1)].astype(np.int64)
    here = lcp[r].astype(np.int64)
    pick = rng.integers(0, 7, nq)
    special = np.choose(pick, [here, here + 1, nxt, nxt + 1, np.ones(nq, dtype=np.int64), np.full(nq, 2), room])
    ln = np.where(np.arange(nq) % 2 == 0, special, rng.integers(1, 65, nq))
    return _u32a(pos), _u32a(np.clip(ln, 1, room))
