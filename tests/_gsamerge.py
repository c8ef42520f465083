"""Shared cases of the GSA merge (sfx_gsa_merge_dev / _u32, sfx_gsa_extend_u32, GeneralizedSuffixTable.extend / merge):
test_gsamerge_emu.py runs them on the fiber emulator ("cpu"), test_gpu_gsamerge.py on libsuffix_hip.so ("cuda").

The expected value is never the code under test: for small collections it is GeneralizedSuffixTable.new_naive (the
definition), which also supplies the arrays of the two halves; for larger ones the one-shot sfx_build_gsa_u32 of the whole
collection, which the merge does not touch and tests/gsa_check.c vouches for."""
import contextlib
import ctypes
import os
import random
import subprocess
import threading
import time

import numpy as np
import torch

import _buffers
import _gsa
from suffix_amd import GeneralizedSuffixTable
from suffix_amd import device as sdev

OK, ERR_ARG, ERR_TOO_LARGE, ERR_WORKSPACE = 0, 1, 2, 5
ROUTE_NONE, ROUTE_MERGE, ROUTE_REBUILD = 0, 1, 2
TILE = 2048                                                             # kGmTile: output slots per workgroup
KERNELS = {"gmerge_check", "gmerge_rank", "gmerge_scatter"}
NAMES = ("sa", "da", "lcp")
HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")


def build_emulator():
    """`make -C tests/emu`; sfx_gsamerge.hip is compiled as part of sfx_api.hip's translation unit and tests/emu/Makefile does
    not name it: when it is newer than the library, sfx_api.hip is declared new."""
    lib = os.path.join(EMU_DIR, "libsuffix_emu.so")
    cmd = ["make", "-s", "-j8", "-C", EMU_DIR]
    unit = os.path.join(HERE, os.pardir, "suffix_amd", "csrc", "sfx_gsamerge.hip")
    if os.path.exists(lib) and os.path.getmtime(unit) > os.path.getmtime(lib):
        cmd += ["-W", "../../suffix_amd/csrc/sfx_api.hip"]
    subprocess.check_call(cmd)
    return lib


def _sync(device):
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()


def _arrays(g):
    return g.table(), g.doc_array(), g.lcp_lens()


def _t32(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to(device)


def _h32(t):
    return t.cpu().numpy().view(np.uint32)


class Split:
    """A collection cut behind its first k documents: the whole text and starts, and the arrays of either side alone --
    from the definition (eng None) or from the engine's one-shot build of that side."""

    def __init__(self, docs, k, eng=None, sides=None):
        self.docs, self.k = [bytes(d) for d in docs], int(k)
        self.text = b"".join(self.docs)
        self.starts = _gsa.doc_starts(self.docs).astype(np.uint64)
        self.nd = len(self.docs)
        mk = (lambda d: GeneralizedSuffixTable.new_naive(d)) if eng is None else (lambda d: GeneralizedSuffixTable(d, engine=eng))
        self.A, self.B = sides if sides is not None else (_arrays(mk(self.docs[:k])), _arrays(mk(self.docs[k:])))
        self.na, self.nb = int(self.A[0].size), int(self.B[0].size)
        self.n = self.na + self.nb
        assert self.n == len(self.text)


def expected(docs, eng=None):
    """(sa, da, lcp) of the whole collection: the definition, or with `eng` its one-shot build."""
    return _arrays(GeneralizedSuffixTable.new_naive(docs) if eng is None else GeneralizedSuffixTable(docs, engine=eng))


def same(got, exp, what, names=NAMES):
    for name, g, x in zip(names, got, exp):
        if g is None:
            continue
        g = _h32(g) if isinstance(g, torch.Tensor) else g
        assert g.size == x.size and np.array_equal(g, x), (what, name, np.flatnonzero(g != x)[:4] if g.size == x.size else (g.size, x.size))


# ---- the entry points -------------------------------------------------------------------------------------------------
def merge_dev(eng, device, c, use_da=True, want_da=True, want_lcp=True, limit=0, workspace=None):
    text = torch.from_numpy(np.frombuffer(c.text, dtype=np.uint8).copy()).to(device)
    ds = torch.from_numpy(c.starts.astype(np.int64)).to(device)
    a, b = [_t32(x, device) for x in c.A], [_t32(x, device) for x in c.B]
    r = sdev.gsa_merge(text, ds, c.k, a[0], a[2], b[0], b[2], da_a=a[1] if use_da else None, da_b=b[1] if use_da else None,
                       match_limit=limit, want_da=want_da, want_lcp=want_lcp, workspace=workspace, engine=eng)
    _sync(device)
    return r


def merge_host(eng, c, use_da=True, limit=0, fill=0xA5):
    """sfx_gsa_merge_u32 -> (status, (sa, da, lcp), longest); the outputs start as `fill` bytes."""
    out = [np.full(c.n, fill * 0x01010101, dtype=np.uint32) for _ in range(3)]
    longest = ctypes.c_uint64(77)
    t = np.frombuffer(c.text, dtype=np.uint8)
    p = _gsa.ptr
    rc = eng.lib.sfx_gsa_merge_u32(p(t), p(c.starts), c.nd, c.k, p(c.A[0]), p(c.A[1]) if use_da else None, p(c.A[2]), c.na,
                                   p(c.B[0]), p(c.B[1]) if use_da else None, p(c.B[2]), c.nb, limit, p(out[0]), p(out[1]), p(out[2]),
                                   ctypes.byref(longest))
    return rc, out, int(longest.value)


def extend_host(eng, c, limit=0, rebuild=1, use_da=True, fill=0xA5):
    """sfx_gsa_extend_u32 -> (status, (sa, da, lcp), longest, route)."""
    out = [np.full(c.n, fill * 0x01010101, dtype=np.uint32) for _ in range(3)]
    longest, route = ctypes.c_uint64(77), ctypes.c_uint32(77)
    t = np.frombuffer(c.text, dtype=np.uint8)
    p = _gsa.ptr
    rc = eng.lib.sfx_gsa_extend_u32(p(t), c.n, p(c.starts), c.nd, c.k, p(c.A[0]), p(c.A[1]) if use_da else None, p(c.A[2]), limit, rebuild,
                                    p(out[0]), p(out[1]), p(out[2]), ctypes.byref(longest), ctypes.byref(route))
    return rc, out, int(longest.value), int(route.value)


def raw(eng, device, c, use_da=True, want=(True, True), limit=0, text_off=0, in_off=0, out_offs=(0, 0, 0), fill=0xFF, ws_bytes=None,
        ws_off=0, replace=None, ndocs=None, k=None):
    """sfx_gsa_merge_dev over guarded buffers -> (status, longest, buffers).  replace: {name: array} swaps an input."""
    need = int(eng.lib.sfx_gsa_merge_workspace_bytes(c.na, c.nb))
    src = {"starts": c.starts, "sa_a": c.A[0], "da_a": c.A[1], "lcp_a": c.A[2], "sa_b": c.B[0], "da_b": c.B[1], "lcp_b": c.B[2]}
    src.update(replace or {})
    b = {"text": _buffers.text_in(c.text, device, text_off)}
    for name, arr in src.items():
        b[name] = _buffers.inp(arr, device, 8 if name == "starts" and in_off else in_off)
    for name, off in zip(NAMES, out_offs):
        b["out_" + name] = _buffers.guarded(4 * c.n, device, off, _buffers.out_fill(fill))
    b["ws"] = _buffers.guarded(need if ws_bytes is None else ws_bytes, device, ws_off, fill)
    longest = ctypes.c_uint64(77)
    da = (lambda x: b[x].ptr) if use_da else (lambda x: None)
    rc = eng.lib.sfx_gsa_merge_dev(b["text"].ptr, b["starts"].ptr, c.nd if ndocs is None else ndocs, c.k if k is None else k,
                                   b["sa_a"].ptr, da("da_a"), b["lcp_a"].ptr, c.na, b["sa_b"].ptr, da("da_b"), b["lcp_b"].ptr, c.nb, limit,
                                   b["out_sa"].ptr, b["out_da"].ptr if want[0] else None, b["out_lcp"].ptr if want[1] else None,
                                   ctypes.byref(longest), b["ws"].ptr, b["ws"].nbytes, _buffers.stream_of(device))
    _sync(device)
    return rc, int(longest.value), b


def outputs_of(b, want=(True, True)):
    return [b["out_sa"].host(np.uint32), b["out_da"].host(np.uint32) if want[0] else None, b["out_lcp"].host(np.uint32) if want[1] else None]


def untouched(b, fill=0xFF):
    for name in NAMES:
        assert (b["out_" + name].host() == fill).all(), f"a refused or failed call wrote {name}"


def true_longest(c, exp):
    """max lcp over the neighbouring pairs of the merged table that are one old and one new suffix."""
    new = exp[0].astype(np.int64) >= c.na
    seam = np.flatnonzero(new[1:] != new[:-1]) + 1
    return int(exp[2][seam].max()) if seam.size else 0


def every_route(eng, device, docs, k, exp=None, what=None, eng_sides=False):
    """One split through sfx_gsa_merge_dev (da given and NULL, outputs skipped), _u32 and sfx_gsa_extend_u32."""
    c = Split(docs, k, eng if eng_sides else None)
    exp = expected(docs) if exp is None else exp
    want_longest = true_longest(c, exp)
    for use_da in (True, False):
        *got, longest = merge_dev(eng, device, c, use_da=use_da)
        same(got, exp, (what, "dev", use_da, docs, k))
        assert longest == want_longest, (what, longest, want_longest, docs, k)
    sa, da, lcp, _ = merge_dev(eng, device, c, want_da=False, want_lcp=False)
    assert da is None and lcp is None
    same([sa], exp, (what, "sa only", docs, k))
    rc, got, longest = merge_host(eng, c)
    assert rc == OK and longest == want_longest, (what, rc, longest)
    same(got, exp, (what, "host", docs, k))
    rc, got, longest, route = extend_host(eng, c, use_da=False)
    assert (rc, route, longest) == (OK, ROUTE_MERGE, want_longest), (what, rc, route, longest)
    same(got, exp, (what, "extend", docs, k))
    return c


# ---- 1. the known answer ------------------------------------------------------------------------------------------------
KNOWN_SA, KNOWN_DA, KNOWN_LCP = [5, 8, 3, 6, 1, 0, 4, 7, 2], [0, 1, 0, 1, 0, 0, 0, 1, 0], [0, 1, 1, 3, 3, 0, 0, 2, 2]


def known_answer(eng, device):
    docs = [b"banana", b"ana"]
    exp = [np.array(x, dtype=np.uint32) for x in (KNOWN_SA, KNOWN_DA, KNOWN_LCP)]
    same(expected(docs), exp, "the definition")
    c = every_route(eng, device, docs, 1, exp, "banana + ana")
    for use_da in (True, False):
        assert merge_dev(eng, device, c, use_da=use_da)[3] == 3
    rc, longest, b = raw(eng, device, c)
    assert (rc, longest) == (OK, 3)
    same(outputs_of(b), exp, "raw")
    p = b["ws"].host(np.uint32)[64:67]                                # [flags 256 B | p ...]: the ranks among the old suffixes
    assert p.tolist() == [1, 2, 5]
    for g in (GeneralizedSuffixTable([b"banana"], engine=eng).extend([b"ana"]),
              GeneralizedSuffixTable(["banana"], engine=eng).merge(GeneralizedSuffixTable([b"ana"], engine=eng))):
        same(_arrays(g), exp, "table")
        assert g.last_extend_route == "merge" and g.num_docs() == 2 and g.document(1) == b"ana"
        assert g.positions(b"ana") == [(0, 3), (1, 0), (0, 1)] and g.documents(b"an") == [0, 1]      # fresh handles on the new arrays
    assert GeneralizedSuffixTable(["banana"], engine=eng).extend(["ana"]).document(0) == "banana"


# ---- 2. random splits ---------------------------------------------------------------------------------------------------
def random_splits(eng, device, count=300, seed=5):
    rng = random.Random(seed)
    merges = 0
    for it in range(count):
        docs = _gsa.random_collection(rng, max_docs=6, max_len=10)
        if it % 3 == 0:
            docs = [bytes(rng.choice(b"abc") for _ in range(rng.randint(0, 12))) for _ in range(rng.randint(1, 6))]
        exp = expected(docs)
        for k in range(len(docs) + 1):
            c = Split(docs, k)
            use_da, want = bool((it + k) & 1), ((it + k) % 3 != 0, (it + k) % 4 != 0)
            *got, longest = merge_dev(eng, device, c, use_da=use_da, want_da=want[0], want_lcp=want[1])
            same(got, exp, ("random", it, docs, k, use_da))
            assert (got[1] is None, got[2] is None) == (not want[0], not want[1])
            assert longest == true_longest(c, exp), (docs, k)
            merges += 1
        if it % 10 == 0:
            every_route(eng, device, docs, rng.randint(0, len(docs)), exp, ("random", it))
    return merges


# ---- 3. ties and prefixes -------------------------------------------------------------------------------------------------
TIES = [
    ([b"xy", b"b", b"xy", b"a", b"xy"], 3),                             # a copy of a document of A: old first
    ([b"a" * 40] * 10, 7),
    ([b"a" * 40] * 7 + [b"a" * 41], 7),
    ([b"abcabc", b"abcab", b"abc", b"ab"], 2),                          # new suffixes that are proper prefixes of old ones
    ([b"ab", b"abc", b"abcab", b"abcabc"], 2),                          # and the reverse
    ([b"abab", b"ba", b"\x00\x00\x00", b"\x00"], 2),                    # p = 0 for every new suffix
    ([b"abab", b"ba", b"\xff\xff\xff", b"\xff"], 2),                    # p = N for every new suffix
    ([b"a\x00b\xffa", b"\xff\x00", b"\x00\xffa\x00", b"b\xff", b"\x00"], 2),
    ([b"a\x00b\xffa", b"\xff\x00", b"\x00\xffa\x00", b"b\xff", b"\x00"], 3),
    ([b"", b"ab", b"", b"", b"ab", b""], 3),                            # empty documents on both sides of the split
    ([b"", b""], 1),
    ([b"q"], 0),
    ([b"q"], 1),
]


def ties_and_prefixes(eng, device):
    for docs, k in TIES:
        every_route(eng, device, docs, k, what="ties")
    c = Split(*TIES[0])
    sa = _h32(merge_dev(eng, device, c)[0])
    at = [int(np.flatnonzero(sa == pos)[0]) for pos in (0, 3, 6)]       # the three suffixes "xy": documents 0, 2 (old), 4 (new)
    assert at == [at[0], at[0] + 1, at[0] + 2]
    c = Split(*TIES[5])
    assert (_h32(merge_dev(eng, device, c)[0])[:4] >= 6).all()
    c = Split(*TIES[6])
    assert (_h32(merge_dev(eng, device, c)[0])[-4:] >= 6).all()


# ---- 4. around the scatter tile ---------------------------------------------------------------------------------------------
def _bits(n, seed):
    return np.random.default_rng(seed).integers(97, 99, n).astype(np.uint8).tobytes()


def _docs_of(text, step):
    return [text[i:i + step] for i in range(0, len(text), step)]


def tile_sizes(eng, device, sizes=(1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)):
    """N and M over the sizes in all pairs, a 2-symbol text in documents of 300 bytes; either side's arrays are built once."""
    sides = {(which, s): _docs_of(_bits(s, 10 * s + which), 300) for which in (0, 1) for s in sizes}
    built = {key: _arrays(GeneralizedSuffixTable(d, engine=eng)) for key, d in sides.items()}
    for na in sizes:
        for nb in sizes:
            docs = sides[0, na] + sides[1, nb]
            c = Split(docs, len(sides[0, na]), sides=(built[0, na], built[1, nb]))
            exp = expected(docs, eng)
            *got, longest = merge_dev(eng, device, c, use_da=(na + nb) % 2 == 0)
            same(got, exp, ("tile sizes", na, nb))
            assert longest == true_longest(c, exp)
    return len(sizes) ** 2


def tile_patterns(eng, device, runs=TILE + 1):
    """Strict alternation of old and new slots; `runs` new suffixes with one common p (at least one whole tile of new entries
    only); the mirror: `runs` old ranks with no new one between."""
    words = sorted(bytes([97 + i // 676, 97 + i // 26 % 26, 97 + i % 26]) + b"~" for i in range(0, 7 * (runs + 50), 7))
    order = [words[i] for i in range(0, len(words), 2)] + [words[i] for i in range(1, len(words), 2)]
    c = Split(order, (len(words) + 1) // 2, eng)
    x = expected(order, eng)
    *got, _ = merge_dev(eng, device, c)
    same(got, x, "alternation")
    new = x[0].astype(np.int64) >= c.na
    assert (new[1:] != new[:-1]).sum() > runs // 2                      # the slots do alternate
    for mirror in (False, True):
        few, many = [b"abab", b"zz"], [bytes(b"mno"[i // 3 ** s % 3] for s in range(4)) for i in range(runs // 4 + 1)]
        docs = many + few if mirror else few + many                      # every suffix of `many` lies between "bab" and "z"
        k = len(many) if mirror else len(few)
        c = Split(docs, k, eng)
        x = expected(docs, eng)
        *got, _ = merge_dev(eng, device, c, use_da=mirror)
        same(got, x, ("one common p", mirror))
        new = x[0].astype(np.int64) >= c.na
        run = np.diff(np.flatnonzero(np.concatenate([[True], new[1:] != new[:-1], [True]]))).max()
        assert run >= runs, run
        rc, _, b = raw(eng, device, c)
        p = b["ws"].host(np.uint32)[64:64 + c.nb]
        assert rc == OK and (np.bincount(p).max() >= runs) == (not mirror)


def hook_goes_through_dev_env():
    src = open(os.path.join(HERE, os.pardir, "suffix_amd", "csrc", "sfx_gsamerge.hip")).read()
    assert "getenv" not in src and 'dev_env("SFX_GM_TILE")' in src


# ---- 5. chaining ------------------------------------------------------------------------------------------------------------
def chaining(eng):
    rng = random.Random(8)
    docs = [bytes(rng.choice(b"abc") for _ in range(rng.randint(0, 40))) for _ in range(24)] + [b"", b"abcabc" * 9]
    g = GeneralizedSuffixTable(docs[:5], engine=eng)
    first = _arrays(g)
    keep = [x.copy() for x in first]
    for a, b in ((5, 6), (6, 17), (17, 26)):
        h = g.extend(docs[a:b])
        assert h.last_extend_route == "merge" and h is not g
        g = h
    same(_arrays(g), expected(docs, eng), "three extends")
    same(_arrays(g), expected(docs), "three extends against the definition")
    same(first, keep, "the old table")
    assert g.num_docs() == len(docs) and g.documents(b"abcabc") == sorted(i for i, d in enumerate(docs) if b"abcabc" in d)


# ---- 6. refusals and limits ---------------------------------------------------------------------------------------------------
def planted(stretch=25):
    """Two documents over disjoint alphabets but for one shared stretch: the longest (old, new) match is `stretch`."""
    rng = random.Random(9)
    s = bytes(rng.choice(b"xyz") for _ in range(stretch))
    a = bytes(rng.choice(b"abc") for _ in range(70)) + b"!" + s + b"?" + bytes(rng.choice(b"abc") for _ in range(30))
    b = bytes(rng.choice(b"def") for _ in range(50)) + b"#" + s + b"%" + bytes(rng.choice(b"def") for _ in range(60))
    return [a, bytes(rng.choice(b"abc") for _ in range(33)), b]


def match_limits(eng, device):
    docs = planted()
    c = Split(docs, 2)
    exp = expected(docs)
    assert true_longest(c, exp) == 25
    for limit, refused in ((24, True), (25, False), (26, False), (0, False), (1, True)):
        rc, longest, b = raw(eng, device, c, limit=limit)
        assert rc == OK and longest == (limit + 1 if refused else 25), (limit, longest)
        if refused:
            untouched(b)
        else:
            same(outputs_of(b), exp, ("limit", limit))
        _buffers.check_all(b)
        sa, _, _, longest = merge_dev(eng, device, c, limit=limit)
        assert (sa is None) == refused and longest == (limit + 1 if refused else 25)
        rc, got, longest = merge_host(eng, c, limit=limit)
        assert rc == OK and longest == (limit + 1 if refused else 25)
        if refused:
            assert all((x == 0xA5A5A5A5).all() for x in got)
        else:
            same(got, exp, ("host", limit))
        rc, got, longest, route = extend_host(eng, c, limit=limit, rebuild=0)
        assert (rc, route) == (OK, ROUTE_NONE if refused else ROUTE_MERGE) and (not refused or all((x == 0xA5A5A5A5).all() for x in got))
        rc, got, longest, route = extend_host(eng, c, limit=limit, rebuild=1)
        assert (rc, route) == (OK, ROUTE_REBUILD if refused else ROUTE_MERGE)
        same(got, exp, ("extend", limit))
        g = GeneralizedSuffixTable(docs[:2], engine=eng)
        for h in (g.extend(docs[2:], match_limit=limit), g.merge(GeneralizedSuffixTable(docs[2:], engine=eng), match_limit=limit)):
            assert h.last_extend_route == ("rebuild" if refused else "merge"), limit
            same(_arrays(h), exp, ("table", limit))


def refusals(eng, device):
    lib = eng.lib
    docs = planted()
    c = Split(docs, 2)
    need = int(lib.sfx_gsa_merge_workspace_bytes(c.na, c.nb))
    # sizes
    big = ctypes.c_uint64(5)
    for na, nb in ((1 << 32, 0), (0, 1 << 32), ((1 << 32) - 1, 1), (1 << 31, 1 << 31)):
        assert lib.sfx_gsa_merge_workspace_bytes(na, nb) == 0
        assert lib.sfx_gsa_merge_dev(None, None, 2, 1, None, None, None, na, None, None, None, nb, 0, None, None, None, ctypes.byref(big), None, 0,
                                     None) == ERR_TOO_LARGE
        assert lib.sfx_gsa_merge_u32(None, None, 2, 1, None, None, None, na, None, None, None, nb, 0, None, None, None, ctypes.byref(big)) == ERR_TOO_LARGE
    assert lib.sfx_gsa_extend_u32(None, 1 << 32, None, 2, 1, None, None, None, 0, 1, None, None, None, ctypes.byref(big),
                                  ctypes.byref(ctypes.c_uint32())) == ERR_TOO_LARGE
    for nb in (0, 1, 1000, 1 << 20, (1 << 32) - 2):
        assert 12 * nb <= lib.sfx_gsa_merge_workspace_bytes(1, nb) <= 12 * nb + (34 << 10)
    assert lib.sfx_gsa_merge_dev(None, None, 0, 0, None, None, None, 0, None, None, None, 0, 0, None, None, None, ctypes.byref(big), None, 0, None) == OK
    assert big.value == 0
    # the workspace
    for ws_bytes in (need - 1, 0):
        rc, _, b = raw(eng, device, c, ws_bytes=ws_bytes)
        assert rc == ERR_WORKSPACE
        untouched(b)
        _buffers.check_all(b)
    rc, _, b = raw(eng, device, c, ws_off=4)
    assert rc == ERR_ARG                                                  # long enough, off SFX_WORKSPACE_ALIGN
    untouched(b)
    # the split
    bad_starts = c.starts.copy()
    bad_starts[2] -= 1
    down = c.starts.copy()
    down[1] = down[2] + 1
    sb = c.B[0].copy()
    sb[5] = c.nb
    sa_ = c.A[0].copy()
    sa_[0] = c.na
    da_ = c.A[1].copy()
    da_[3] = 2
    db_ = c.B[1].copy()
    db_[3] = 1
    swapped = c.B[0].copy()
    swapped[[0, c.nb - 1]] = swapped[[c.nb - 1, 0]]
    for what, kw in (("ndocs_a > ndocs", {"k": 4}), ("the split is not at N", {"replace": {"starts": bad_starts}}),
                     ("ndocs_a names another document", {"k": 1}), ("decreasing starts", {"replace": {"starts": down}}),
                     ("sa_b out of range", {"replace": {"sa_b": sb}}), ("sa_a out of range", {"replace": {"sa_a": sa_}}),
                     ("da_a out of range", {"replace": {"da_a": da_}}), ("da_b out of range", {"replace": {"da_b": db_}}),
                     ("p decreases", {"replace": {"sa_b": swapped}}), ("no document for B's bytes", {"k": 3, "ndocs": 3})):
        rc, _, b = raw(eng, device, c, **kw)
        assert rc == ERR_ARG, (what, rc)
        untouched(b)
        _buffers.check_all(b)
    # an output inside an input
    t = torch.zeros(4 * c.n + 64, dtype=torch.int32, device=device)
    ws = sdev.gsa_merge_workspace(c.na, c.nb, device, eng)
    tx = torch.from_numpy(np.frombuffer(c.text, dtype=np.uint8).copy()).to(device)
    ds = torch.from_numpy(c.starts.astype(np.int64)).to(device)
    a, b2 = [_t32(x, device) for x in c.A], [_t32(x, device) for x in c.B]
    t[:c.na] = a[0]
    p = sdev._p
    for out in (t, ws.view(torch.int32)[16:]):
        rc = lib.sfx_gsa_merge_dev(p(tx), p(ds), 3, 2, p(t[:c.na]) if out is t else p(a[0]), p(a[1]), p(a[2]), c.na, p(b2[0]), p(b2[1]), p(b2[2]),
                                   c.nb, 0, p(out), None, None, ctypes.byref(big), p(ws), ws.numel(), _buffers.stream_of(device))
        assert rc == ERR_ARG
    _sync(device)
    assert torch.equal(t[:c.na], a[0])


def garbage(eng, device, rounds=24, seed=11):
    """In-range garbage in every input array, alone and together: any status, nothing outside the arrays is written."""
    nrng = np.random.default_rng(seed)
    docs = [bytes(nrng.integers(97, 100, int(nrng.integers(0, 90))).astype(np.uint8)) for _ in range(9)]
    c = Split(docs, 5)
    junk = {"sa_a": lambda: nrng.integers(0, c.na, c.na), "da_a": lambda: nrng.integers(0, 5, c.na), "lcp_a": lambda: nrng.integers(0, 1 << 32, c.na),
            "sa_b": lambda: nrng.integers(0, c.nb, c.nb), "da_b": lambda: nrng.integers(0, 4, c.nb), "lcp_b": lambda: nrng.integers(0, 1 << 32, c.nb)}
    names = list(junk)
    seen = set()
    for t in range(rounds):
        pick = names if t % 4 == 0 else [names[t % 6]] if t % 4 < 3 else ["da_a", "da_b", "lcp_a", "lcp_b"]
        rc, _, b = raw(eng, device, c, replace={k: junk[k]().astype(np.uint32) for k in pick}, use_da=t % 5 != 4, limit=(0, 3)[t % 2])
        assert rc in (OK, ERR_ARG), rc
        seen.add(rc)
        _buffers.check_all(b)
    assert seen == {OK, ERR_ARG}


# ---- 7. buffers -----------------------------------------------------------------------------------------------------------------
def buffers_streams_threads(eng, device):
    docs = _docs_of(_bits(TILE + 300, 21), 170) + [b""] + _docs_of(_bits(TILE // 2 + 77, 22), 90)
    k = len(_docs_of(_bits(TILE + 300, 21), 170)) + 1
    c = Split(docs, k, eng)
    exp = expected(docs, eng)
    side = torch.cuda.Stream() if str(device).startswith("cuda") else None
    for t, (text_off, u32_off, fill) in enumerate(_buffers.combos()):
        with (torch.cuda.stream(side) if side is not None and t % 2 else contextlib.nullcontext()):
            offs = [(4, 8, 12), (12, 4, 8), (8, 12, 4)][t % 3]
            rc, _, b = raw(eng, device, c, use_da=t % 2 == 0, text_off=text_off, in_off=u32_off, out_offs=offs, fill=fill)
            assert rc == OK
            same(outputs_of(b), exp, ("buffers", t))
            _buffers.check_all(b)
    errors = []

    def worker(use_da):
        try:
            stream = torch.cuda.Stream() if side is not None else None
            with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
                for _ in range(3):
                    rc, _, b = raw(eng, device, c, use_da=use_da, fill="count")
                    assert rc == OK
                    same(outputs_of(b), exp, ("thread", use_da))
                    _buffers.check_all(b)
        except BaseException as ex:                                      # noqa: BLE001 -- reported by the parent
            errors.append(ex)
    held = eng.resource_stats()
    threads = [threading.Thread(target=worker, args=(a,)) for a in (True, False)]
    concurrent = side is not None                                    # (the emulator keeps threadIdx & co. in globals: one launch at a time)
    for th in threads:
        th.start()
        if not concurrent:
            th.join()
    for th in threads:
        th.join()
    assert not errors, errors
    # a thread's pinned page and stream go back when the OS thread ends, which join() does not wait for: see them gone, so
    # that the ledger is at rest for whoever reads it next
    deadline = time.monotonic() + 10
    while any(eng.resource_stats()[k] > held[k] for k in ("pinned_allocs", "streams")) and time.monotonic() < deadline:
        time.sleep(0)
    assert all(eng.resource_stats()[k] <= held[k] for k in ("pinned_allocs", "streams")), (held, eng.resource_stats())


# ---- 8. resources ---------------------------------------------------------------------------------------------------------------
def resources_come_back(eng, device):
    docs = planted()
    c = Split(docs, 2)
    exp = expected(docs)
    assert merge_host(eng, c)[0] == OK                                   # (the calling thread's page and stream exist from here on)
    _sync(device)
    eng.release_cached_buffers()
    before = eng.resource_stats()
    allocs = before["device_allocs_total"]
    same(merge_dev(eng, device, c)[:3], exp, "dev")
    assert eng.resource_stats()["device_allocs_total"] == allocs         # the device entry allocates nothing
    for limit in (0, 3):
        assert merge_host(eng, c, limit=limit)[0] == OK
        assert extend_host(eng, c, limit=limit)[0] == OK
    GeneralizedSuffixTable(docs[:2], engine=eng).extend(docs[2:])
    eng.release_cached_buffers()
    after = eng.resource_stats()
    for k in ("device_bytes", "device_allocs", "pinned_bytes", "pinned_allocs", "streams", "events", "pooled_bytes", "pooled_buffers"):
        assert after[k] == before[k], (k, before, after)


def launch_names(eng, device):
    c = Split(planted(), 2)
    names = _gsa.profile_names(eng, lambda: merge_dev(eng, device, c))
    assert names == KERNELS, sorted(names)


def hooked(eng, device):
    """What a hooked child process runs (SFX_GM_TILE = 64 / 256 / 5, SFX_MAX_GRID=3: more tiles than workgroups, tiles that
    hold new entries only, old ones only, and every mixture)."""
    known_answer(eng, device)
    ties_and_prefixes(eng, device)
    random_splits(eng, device, count=40, seed=17)
    tile_sizes(eng, device)
    tile_patterns(eng, device)
    match_limits(eng, device)
