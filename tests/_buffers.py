"""How callers hand buffers to the `*_dev` ABI (include/suffix_hip.h: the alignment contract), shared by
test_buffers_emu.py (the emulator, host memory) and test_gpu_buffers.py (the product, HBM).

Every array an entry point WRITES -- outputs and workspace -- is carved out of a larger tensor by `guarded`: 4 KiB guard
bands on both sides that must come back untouched, the array itself at a chosen byte offset behind a 256-aligned address
and pre-filled (outputs with 0xFF: every entry must be written; workspaces with 0x00, 0xFF or a running byte counter: the
engine may rely on nothing it did not clear itself).  Every workspace is exactly `*_workspace_bytes(...)` long.  Inputs go
through the same helper, so texts sit at +1 / +3 / +8 / +15 bytes, u32 arrays at +4 / +8 / +12 behind a 16-byte boundary
and query bytes at +1.  Results are compared with the oracle (or the definition), never with another engine run alone."""
import ctypes
import random

import numpy as np
import torch

import _cases
import _gen
import _gsa
import _repeats
from suffix_amd import GeneralizedSuffixTable

GUARD = 4096
ALIGN = 256
BAND = ((np.arange(GUARD, dtype=np.uint32) * 7 + 0x5B) & 0xFF).astype(np.uint8)     # never a run of 0x00 / 0xFF
FILLS = (0x00, 0xFF, "count")
TEXT_OFFSETS = (1, 3, 8, 15)
U32_OFFSETS = (4, 8, 12)
OK, ERR_ARG, ERR_WORKSPACE = 0, 1, 5
NONE = 0xFFFFFFFF


class guarded:
    """`nbytes` bytes `offset` bytes behind a 256-aligned address inside a larger uint8 tensor on `device`, between two
    guard bands of GUARD bytes that touch the array.  fill: a byte value, "count" (0, 1, .. 255, 0, ..) or None."""

    def __init__(self, nbytes, device, offset=0, fill=0xFF):
        self.nbytes, self.offset, self.device = int(nbytes), int(offset), device
        self.raw = torch.empty(GUARD + ALIGN + self.offset + self.nbytes + GUARD, dtype=torch.uint8, device=device)
        self.begin = GUARD + (-(self.raw.data_ptr() + GUARD)) % ALIGN + self.offset
        assert (self.raw.data_ptr() + self.begin - self.offset) % ALIGN == 0
        band = torch.from_numpy(BAND).to(device)
        self.raw[self.begin - GUARD:self.begin] = band
        self.raw[self.begin + self.nbytes:self.begin + self.nbytes + GUARD] = band
        if fill is not None:
            self.fill(fill)

    def fill(self, fill):
        if fill == "count":
            reps = (self.nbytes + 255) // 256
            self.u8().copy_(torch.arange(256, dtype=torch.int32, device=self.device).to(torch.uint8).repeat(reps)[:self.nbytes])
        else:
            self.u8().fill_(int(fill))
        return self

    def load(self, arr):
        a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        assert a.size == self.nbytes
        if a.size:
            self.u8().copy_(torch.from_numpy(a.copy()))
        return self

    def u8(self):
        return self.raw[self.begin:self.begin + self.nbytes]

    def view(self, dtype):
        """The array as a tensor of `dtype` (torch.int32 for u32 arrays, torch.int64 for u64 ones)."""
        return self.u8().view(dtype)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.raw.data_ptr() + self.begin)

    def host(self, dtype=np.uint8):
        if self.raw.is_cuda:
            torch.cuda.current_stream(self.raw.device).synchronize()
        return self.u8().cpu().numpy().copy().view(dtype)

    def check_guards(self, what="array"):
        if self.raw.is_cuda:
            torch.cuda.current_stream(self.raw.device).synchronize()
        for name, lo in (("in front of", self.begin - GUARD), ("behind", self.begin + self.nbytes)):
            got = self.raw[lo:lo + GUARD].cpu().numpy()
            bad = np.flatnonzero(got != BAND)
            assert bad.size == 0, (f"{what}: the guard band {name} the array ({self.nbytes} bytes at +{self.offset}) was written: first at "
                                   f"byte {lo + int(bad[0]) - self.begin:+d} from the array's start, 0x{int(got[bad[0]]):02x} instead of "
                                   f"0x{int(BAND[bad[0]]):02x}, {bad.size} bytes in all")


def inp(arr, device, offset=0):
    """An input array at `offset`, between guard bands of its own (an input must not be written either)."""
    a = np.ascontiguousarray(arr)
    return guarded(a.nbytes, device, offset, None).load(a)


def text_in(text, device, offset=0):
    return inp(np.frombuffer(text, dtype=np.uint8), device, offset)


def stream_of(device):
    if str(device).startswith("cuda"):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return None


def out_fill(fill):
    """Outputs start as 0xFF -- or as the byte counter where the workspace does: 0xFFFFFFFF is a legitimate value of some
    outputs (parent, any, src), an entry left unwritten would hide behind it."""
    return "count" if fill == "count" else 0xFF


def check_all(bufs):
    for name, b in bufs.items():
        b.check_guards(name)


def combos(always=()):
    """(text offset, u32 offset, workspace fill): every text offset once, with the u32 offsets and the fills rotating, then
    the first of them again with the two fills it has not seen -- the same call over the three kinds of dirt."""
    out = [(to, U32_OFFSETS[i % 3], FILLS[i % 3]) for i, to in enumerate(TEXT_OFFSETS)]
    out += [(TEXT_OFFSETS[0], U32_OFFSETS[0], f) for f in FILLS[1:]]
    return list(always) + out


def alphabets(n):
    """The alphabets whose packing differs: 1, 2, 2 (3 symbols), 4, 7 and 8 bits per symbol."""
    return [("2 symbols", _gen.uniform_bytes(n, 2, 4, base=97).tobytes()), ("dna", _gen.dna(n, seed=5).tobytes()),
            ("3 symbols", _gen.uniform_bytes(n, 3, 9, base=65).tobytes()), ("16 symbols", _gen.uniform_bytes(n, 16, 9, base=65).tobytes()),
            ("english", _gen.english_like(n).tobytes()), ("utf8", _gen.utf8_mixed(n).tobytes())]


# ---- the builds -----------------------------------------------------------------------------------------------------------
def call_build_sa(eng, text, device, text_off=0, sa_off=0, fill=0xFF, ws_bytes=None, ws_off=0):
    n = len(text)
    need = int(eng.lib.sfx_sa_workspace_bytes(n))
    b = {"text": text_in(text, device, text_off), "sa": guarded(4 * n, device, sa_off, out_fill(fill)),
         "workspace": guarded(need if ws_bytes is None else ws_bytes, device, ws_off, fill)}
    rc = eng.lib.sfx_build_sa_u32_dev(b["text"].ptr, n, b["sa"].ptr, b["workspace"].ptr, b["workspace"].nbytes, stream_of(device))
    return rc, b


def build_sa_case(eng, orc, text, device, exp=None, which=None):
    """sfx_build_sa_u32_dev over combos(): the oracle's table every time, every guard band intact, the text unchanged."""
    exp = orc.sais(text) if exp is None else exp
    for text_off, sa_off, fill in (which or combos()):
        rc, b = call_build_sa(eng, text, device, text_off, sa_off, fill)
        assert rc == OK, (rc, len(text), text_off, sa_off, fill)
        got = b["sa"].host(np.uint32)
        assert np.array_equal(got, exp), (len(text), text_off, sa_off, fill, np.flatnonzero(got != exp)[:4])
        assert b["text"].host().tobytes() == text
        check_all(b)
        # the statistics of the build just made: its n, and the alphabet it saw -- a build that read presence flags or counts
        # out of the dirt of its workspace sorts a larger alphabet and may still arrive at the right table
        st = eng.build_stats()
        assert st["n"] == len(text), st
        assert st["sigma"] in (0, len(set(text))), (st, len(set(text)), fill)          # (0: the one-workgroup build keeps none)
    return exp


def call_build_sa_lcp(eng, text, device, text_off=0, sa_off=0, lcp_off=0, fill=0xFF, ws_bytes=None, ws_off=0):
    n = len(text)
    need = int(eng.lib.sfx_sa_lcp_workspace_bytes(n))
    b = {"text": text_in(text, device, text_off), "sa": guarded(4 * n, device, sa_off, out_fill(fill)),
         "lcp": guarded(4 * n, device, lcp_off, out_fill(fill)),
         "workspace": guarded(need if ws_bytes is None else ws_bytes, device, ws_off, fill)}
    rc = eng.lib.sfx_build_sa_lcp_u32_dev(b["text"].ptr, n, b["sa"].ptr, b["lcp"].ptr, b["workspace"].ptr, b["workspace"].nbytes,
                                          stream_of(device))
    return rc, b


def call_build_lcp(eng, text, sa, device, text_off=0, sa_off=0, lcp_off=0, fill=0xFF, ws_bytes=None, ws_off=0):
    n = len(text)
    need = int(eng.lib.sfx_lcp_workspace_bytes(n))
    b = {"text": text_in(text, device, text_off), "sa": inp(sa, device, sa_off), "lcp": guarded(4 * n, device, lcp_off, out_fill(fill)),
         "workspace": guarded(need if ws_bytes is None else ws_bytes, device, ws_off, fill)}
    rc = eng.lib.sfx_build_lcp_u32_dev(b["text"].ptr, n, b["sa"].ptr, b["lcp"].ptr, b["workspace"].ptr, b["workspace"].nbytes,
                                       stream_of(device))
    return rc, b


def lcp_case(eng, orc, text, device, exp=None, exp_lcp=None):
    """The one-call build and the LCP-only entry: d_lcp at +0 (the fused route: k_groups_reduce writes it and k_lcp_pending reads
    it 16 bytes at a time) and at every u32 offset (where the engine must not fuse), d_sa at another one, over the three kinds
    of dirt."""
    exp = orc.sais(text) if exp is None else exp
    if exp_lcp is None:
        exp_lcp = orc.lcp_kasai(text, exp) if len(text) > 3000 else orc.lcp_quadratic(text, exp)
    n = len(text)
    for i, lcp_off in enumerate((0,) + U32_OFFSETS):
        sa_off, text_off, fill = ((0,) + U32_OFFSETS)[(i + 2) % 4], (0, 1, 8, 15)[i], FILLS[i % 3]
        rc, b = call_build_sa_lcp(eng, text, device, text_off, sa_off, lcp_off, fill)
        assert rc == OK, (rc, n, lcp_off)
        assert np.array_equal(b["sa"].host(np.uint32), exp), ("fused SA", n, text_off, sa_off, lcp_off, fill)
        got = b["lcp"].host(np.uint32)
        assert np.array_equal(got, exp_lcp), ("fused LCP", n, text_off, sa_off, lcp_off, fill, np.flatnonzero(got != exp_lcp)[:4])
        check_all(b)
        rc, b = call_build_lcp(eng, text, exp, device, text_off, sa_off, lcp_off, fill)
        assert rc == OK, (rc, n, lcp_off)
        got = b["lcp"].host(np.uint32)
        assert np.array_equal(got, exp_lcp), ("LCP", n, text_off, sa_off, lcp_off, fill, np.flatnonzero(got != exp_lcp)[:4])
        assert np.array_equal(b["sa"].host(np.uint32), exp)
        check_all(b)
    for fill in FILLS:                                                 # the fused route over the three kinds of dirt
        rc, b = call_build_sa_lcp(eng, text, device, 1, 4, 0, fill)
        assert rc == OK and np.array_equal(b["sa"].host(np.uint32), exp) and np.array_equal(b["lcp"].host(np.uint32), exp_lcp), (n, fill)
        check_all(b)


def repeat_rich(k):
    """b"ab" * k + b"a" and planted repeats: pairs the initial sort cannot tell apart, so that pending entries exist."""
    d = _gen.dna(40 * k, seed=31).tobytes()
    return [b"ab" * k + b"a", d + d[5 * k:5 * k + 3 * k] + b"G" + d[20 * k:20 * k + k] + d[5 * k + 10:5 * k + 2 * k]]


# ---- queries --------------------------------------------------------------------------------------------------------------
def query_arrays(qs):
    off = np.zeros(len(qs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(q) for q in qs])
    return np.frombuffer(b"".join(qs) + b"\x00", dtype=np.uint8), off


def query_outputs(nq, device, fill, offs=(4, 8, 1, 12)):
    return {"start": guarded(4 * nq, device, offs[0], out_fill(fill)), "end": guarded(4 * nq, device, offs[1], out_fill(fill)),
            "found": guarded(nq, device, offs[2], out_fill(fill)), "any": guarded(4 * nq, device, offs[3], out_fill(fill))}


def check_query_results(orc, text, exp, qs, o, sa_part=None, base=0):
    """start / end / found / any of a batch against the oracle (for a slice: intervals inside the slice, 0 / 0 if empty)."""
    s, e, f, a = o["start"].host(np.uint32), o["end"].host(np.uint32), o["found"].host(), o["any"].host(np.uint32)
    ps, pe = orc.positions_batch(text, exp, *query_arrays(qs))
    for k, q in enumerate(qs):
        ws, we = int(ps[k]), int(pe[k])
        if sa_part is not None:                                         # the part of the interval inside [base, base + count)
            ws, we = max(ws, base) - base, min(we, base + len(sa_part)) - base
            if we <= ws:
                ws, we = 0, 0
        assert (int(s[k]), int(e[k])) == (ws, we), (q, int(s[k]), int(e[k]), ws, we)
        assert bool(f[k]) == (we > ws), q
        if we > ws:
            p = int(a[k])
            assert text[p:p + len(q)] == q, (q, p)
        else:
            assert int(a[k]) == NONE, q


def query_case(eng, orc, text, qs, device, exp=None):
    """sfx_query_batch_dev and the resident index over text at +1 / +15, table at +4 / +12, query bytes at +1, every output
    at an offset of its own; then one slice of the table through sfx_query_batch_range_dev and sfx_build_lcp_range_u32_dev."""
    exp = orc.sais(text) if exp is None else exp
    n, nq = len(text), len(qs)
    qb, qoff = query_arrays(qs)
    for i, fill in enumerate(FILLS):
        text_off, sa_off = (1, 15, 3)[i], U32_OFFSETS[i]
        b = {"text": text_in(text, device, text_off), "sa": inp(exp, device, sa_off), "qbytes": inp(qb, device, 1), "qoff": inp(qoff, device, 8)}
        o = query_outputs(nq, device, fill, offs=((4, 8, 1, 12), (12, 4, 3, 8), (8, 12, 0, 4))[i])
        rc = eng.lib.sfx_query_batch_dev(b["text"].ptr, n, b["sa"].ptr, b["qbytes"].ptr, b["qoff"].ptr, nq, o["start"].ptr, o["end"].ptr,
                                         o["found"].ptr, o["any"].ptr, stream_of(device))
        assert rc == OK, rc
        check_query_results(orc, text, exp, qs, o)
        check_all({**b, **o})
        # the resident index over the same (borrowed) arrays
        h = ctypes.c_void_p()
        assert eng.lib.sfx_index_create_dev(b["text"].ptr, n, b["sa"].ptr, stream_of(device), ctypes.byref(h)) == OK
        try:
            o = query_outputs(nq, device, fill, offs=((8, 12, 1, 4), (4, 8, 0, 12), (12, 4, 3, 8))[i])
            rc = eng.lib.sfx_index_query_dev(h, b["qbytes"].ptr, b["qoff"].ptr, nq, o["start"].ptr, o["end"].ptr, o["found"].ptr,
                                             o["any"].ptr, stream_of(device))
            assert rc == OK, rc
            check_query_results(orc, text, exp, qs, o)
            check_all({**b, **o})
        finally:
            if str(device).startswith("cuda"):
                torch.cuda.synchronize()
            eng.lib.sfx_index_destroy(h)
        # one slice of the table: queries and LCP against it
        lo, hi = n // 3, n - n // 4
        part = exp[lo:hi]
        bp = {"text": b["text"], "part": inp(part, device, sa_off), "qbytes": b["qbytes"], "qoff": b["qoff"]}
        o = query_outputs(nq, device, fill)
        rc = eng.lib.sfx_query_batch_range_dev(bp["text"].ptr, n, bp["part"].ptr, len(part), bp["qbytes"].ptr, bp["qoff"].ptr, nq,
                                               o["start"].ptr, o["end"].ptr, o["found"].ptr, o["any"].ptr, stream_of(device))
        assert rc == OK, rc
        check_query_results(orc, text, exp, qs, o, sa_part=part, base=lo)
        check_all({**bp, **o})
        lcp = guarded(4 * len(part), device, U32_OFFSETS[(i + 1) % 3], out_fill(fill))
        prev = int(exp[lo - 1]) if lo else NONE
        rc = eng.lib.sfx_build_lcp_range_u32_dev(bp["text"].ptr, n, bp["part"].ptr, len(part), prev, lcp.ptr, stream_of(device))
        assert rc == OK, rc
        want = (orc.lcp_kasai(text, exp) if n > 3000 else orc.lcp_quadratic(text, exp))[lo:hi].copy()
        if not lo and len(want):
            want[0] = 0
        assert np.array_equal(lcp.host(np.uint32), want), (n, i)
        lcp.check_guards("lcp_part")
        check_all(bp)


# ---- suffix-tree topology, document lookup, widening ----------------------------------------------------------------------
def intervals_case(eng, orc, text, device):
    sa = orc.sais(text)
    lcp = orc.lcp_kasai(text, sa)
    ref = orc.suffix_tree_sweep(lcp)
    n = len(text)
    names = ("lb", "rb", "node", "parent", "leaf_parent")
    for i, fill in enumerate(FILLS):
        b = {"lcp": inp(lcp, device, U32_OFFSETS[i])}
        o = {k: guarded(4 * n, device, ((0,) + U32_OFFSETS)[(i + j) % 4], out_fill(fill)) for j, k in enumerate(names)}
        ws = guarded(int(eng.lib.sfx_lcp_intervals_workspace_bytes(n)), device, 0, fill)
        rc = eng.lib.sfx_lcp_intervals_dev(b["lcp"].ptr, n, *[o[k].ptr for k in names], ws.ptr, ws.nbytes, stream_of(device))
        assert rc == OK, rc
        for k in names:
            assert np.array_equal(o[k].host(np.uint32), ref[k]), (k, n, fill)
        check_all({**b, **o, "workspace": ws})


def doc_lookup_case(eng, device, n=5000, ndocs=37, seed=3):
    rng = np.random.default_rng(seed)
    starts = np.sort(np.concatenate(([0], rng.integers(0, n, ndocs - 1)))).astype(np.uint64)     # (equal starts: empty documents)
    pos = rng.integers(0, n, 3001).astype(np.uint32)
    want_d = np.searchsorted(starts.astype(np.int64), pos.astype(np.int64), side="right") - 1
    for i, off in enumerate(U32_OFFSETS):
        b = {"pos": inp(pos, device, off), "starts": inp(starts, device, 8)}
        o = {"doc": guarded(4 * pos.size, device, U32_OFFSETS[(i + 1) % 3], 0xFF), "offset": guarded(4 * pos.size, device, U32_OFFSETS[(i + 2) % 3], 0xFF)}
        rc = eng.lib.sfx_doc_lookup_dev(b["pos"].ptr, pos.size, b["starts"].ptr, starts.size, o["doc"].ptr, o["offset"].ptr, stream_of(device))
        assert rc == OK, rc
        assert np.array_equal(o["doc"].host(np.uint32), want_d)
        assert np.array_equal(o["offset"].host(np.uint32).astype(np.int64), pos.astype(np.int64) - starts.astype(np.int64)[want_d])
        check_all({**b, **o})


def widen_case(eng, device, counts=(1, 7, 255, 256, 257, 10001)):
    rng = np.random.default_rng(4)
    for i, cnt in enumerate(counts):
        a = rng.integers(0, 1 << 32, cnt, dtype=np.uint64).astype(np.uint32)
        src = inp(a, device, ((0,) + U32_OFFSETS)[i % 4])
        dst = guarded(8 * cnt, device, (0, 8)[i % 2], 0xFF)
        assert eng.lib.sfx_widen_u32_to_u64_dev(src.ptr, cnt, dst.ptr, stream_of(device)) == OK
        assert np.array_equal(dst.host(np.uint64), a.astype(np.uint64))
        check_all({"in": src, "out": dst})


# ---- generalized suffix array ---------------------------------------------------------------------------------------------
def gsa_case(eng, docs, queries, device):
    """sfx_build_gsa_u32_dev and the resident generalized index against the definition (GeneralizedSuffixTable.new_naive,
    the naive scan of _gsa.naive_matches)."""
    text = b"".join(docs)
    n = len(text)
    starts = _gsa.doc_starts(docs).astype(np.uint64)
    naive = GeneralizedSuffixTable.new_naive(docs, engine=eng)
    want = {"sa": naive.table(), "da": naive.doc_array(), "lcp": naive.lcp_lens()}
    qb, qoff = query_arrays(queries)
    nq = len(queries)
    for i, fill in enumerate(FILLS):
        b = {"text": text_in(text, device, TEXT_OFFSETS[i]), "starts": inp(starts, device, 8)}
        o = {k: guarded(4 * n, device, U32_OFFSETS[(i + j) % 3], out_fill(fill)) for j, k in enumerate(("sa", "da", "lcp"))}
        ws = guarded(int(eng.lib.sfx_gsa_workspace_bytes(n, len(docs))), device, 0, fill)
        rc = eng.lib.sfx_build_gsa_u32_dev(b["text"].ptr, n, b["starts"].ptr, len(docs), o["sa"].ptr, o["da"].ptr, o["lcp"].ptr, ws.ptr,
                                           ws.nbytes, stream_of(device))
        assert rc == OK, rc
        for k in ("sa", "da", "lcp"):
            assert np.array_equal(o[k].host(np.uint32), want[k]), (k, fill, docs[:3])
        check_all({**b, **o, "workspace": ws})
        if not n:
            continue
        h = ctypes.c_void_p()
        assert eng.lib.sfx_gindex_create_dev(b["text"].ptr, n, b["starts"].ptr, len(docs), o["sa"].ptr, o["da"].ptr, stream_of(device),
                                             ctypes.byref(h)) == OK
        try:
            q = {"qbytes": inp(qb, device, 1), "qoff": inp(qoff, device, 8)}
            r = query_outputs(nq, device, fill)
            r["ndocs"] = guarded(4 * nq, device, U32_OFFSETS[i], out_fill(fill))
            rc = eng.lib.sfx_gindex_query_dev(h, q["qbytes"].ptr, q["qoff"].ptr, nq, r["start"].ptr, r["end"].ptr, r["found"].ptr,
                                              r["any"].ptr, r["ndocs"].ptr, stream_of(device))
            assert rc == OK, rc
            s, e, f, a, nd = (r[k].host(np.uint32 if k != "found" else np.uint8) for k in ("start", "end", "found", "any", "ndocs"))
            sa_h, da_h = want["sa"], want["da"]
            for k, qq in enumerate(queries):
                m = _gsa.naive_matches(docs, qq)
                got = sorted((int(da_h[r_]), int(sa_h[r_]) - int(starts[da_h[r_]])) for r_ in range(int(s[k]), int(e[k])))
                assert got == m, (qq, docs[:3])
                assert bool(f[k]) == bool(m) and int(nd[k]) == len({d for d, _ in m}), qq
                assert (int(a[k]) in set(sa_h[int(s[k]):int(e[k])].tolist())) if m else (int(a[k]) == NONE and (int(s[k]), int(e[k])) == (0, 0))
            check_all({**b, **o, **q, **r})
        finally:
            if str(device).startswith("cuda"):
                torch.cuda.synchronize()
            eng.lib.sfx_gindex_destroy(h)


def gsa_cases(eng, device, iters=6, seed=12, max_docs=40, max_len=24):
    rng = random.Random(seed)
    for _ in range(iters):
        docs = _gsa.random_collection(rng, max_docs=max_docs, max_len=max_len)
        if not sum(len(d) for d in docs):
            continue
        text = b"".join(docs)
        qs = [b"", text[:1], text[-2:], b"\xfe"] + _gsa.boundary_queries(docs, rng) + [text[a:a + rng.randint(1, 5)] for a in
                                                                                    (rng.randrange(len(text)) for _ in range(8))]
        gsa_case(eng, docs, qs, device)


# ---- repeat lengths and spans ---------------------------------------------------------------------------------------------
def repeats_case(eng, orc, text, device, starts=None):
    """sfx_repeat_lens_dev (three scopes, with and without witnesses) against brute force, sfx_repeat_spans_dev against the
    difference-array reference; inputs of at most 80 bytes."""
    n = len(text)
    if starts is None:
        sa = orc.sais(text)
        lcp, da = orc.lcp_quadratic(text, sa), None
        scopes = ("any", "earlier")
    else:
        docs = [text[int(a):int(b_)] for a, b_ in zip(starts, list(starts[1:]) + [n])]
        g = GeneralizedSuffixTable.new_naive(docs, engine=eng)
        sa, lcp, da = g.table(), g.lcp_lens(), g.doc_array()
        scopes = ("any", "earlier", "other_doc")
    k = 0
    for scope in scopes:
        exp = _repeats.brute_rep(text, scope, starts)
        for want_src in (True, False):
            fill = FILLS[k % 3]
            off = U32_OFFSETS[k % 3]
            k += 1
            sc = _repeats.SCOPES[scope]
            b = {"sa": inp(sa, device, off), "lcp": inp(lcp, device, U32_OFFSETS[(k + 1) % 3])}
            if scope == "other_doc":
                b["da"] = inp(da, device, U32_OFFSETS[(k + 2) % 3])
            o = {"rep": guarded(4 * n, device, U32_OFFSETS[k % 3], out_fill(fill))}
            if want_src:
                o["src"] = guarded(4 * n, device, off, out_fill(fill))
            ws = guarded(int(eng.lib.sfx_repeat_lens_workspace_bytes(n, sc)), device, 0, fill)
            rc = eng.lib.sfx_repeat_lens_dev(b["sa"].ptr, b["lcp"].ptr, b["da"].ptr if "da" in b else None, n, sc, o["rep"].ptr,
                                             o["src"].ptr if want_src else None, ws.ptr, ws.nbytes, stream_of(device))
            assert rc == OK, (rc, scope)
            rep = o["rep"].host(np.uint32)
            assert np.array_equal(rep, exp), (scope, text, fill)
            if want_src:
                _repeats.check_witnesses(text, scope, rep, o["src"].host(np.uint32), starts)
            check_all({**b, **o, "workspace": ws})
        for m in (1, 2, 3):
            for st in ((None,) if starts is None else (None, starts)):
                fill = FILLS[(k + m) % 3]
                ref = _repeats.span_reference(exp, m, st)
                cap = n // m + 1
                b = {"rep": inp(exp, device, U32_OFFSETS[m % 3])}
                if st is not None:
                    b["starts"] = inp(np.asarray(st, dtype=np.uint64), device, 8)
                o = {"begin": guarded(4 * cap, device, U32_OFFSETS[(m + 1) % 3], 0xFF), "end": guarded(4 * cap, device, U32_OFFSETS[(m + 2) % 3], 0xFF)}
                ws = guarded(int(eng.lib.sfx_repeat_spans_workspace_bytes(n)), device, 0, fill)
                count = ctypes.c_uint64(12345)
                rc = eng.lib.sfx_repeat_spans_dev(b["rep"].ptr, n, m, b["starts"].ptr if st is not None else None,
                                                  0 if st is None else len(st), o["begin"].ptr, o["end"].ptr, cap, ctypes.byref(count),
                                                  ws.ptr, ws.nbytes, stream_of(device))
                assert rc == OK, rc
                kk = int(count.value)
                bg, en = o["begin"].host(np.uint32), o["end"].host(np.uint32)
                assert kk == len(ref) and list(zip(bg[:kk].tolist(), en[:kk].tolist())) == ref, (scope, m, text, st)
                assert (bg[kk:] == NONE).all() and (en[kk:] == NONE).all()          # nothing behind the entries reported
                check_all({**b, **o, "workspace": ws})


def repeats_cases(eng, orc, device, iters=5, seed=6):
    rng = random.Random(seed)
    for t in [b"banana", b"abababa", b"a" * 33, b"mississippi" * 3]:
        repeats_case(eng, orc, t, device)
    for _ in range(iters):
        docs = [d for d in _gsa.random_collection(rng, max_docs=8, max_len=12)]
        text = b"".join(docs)[:80]
        if len(text) < 2:
            continue
        docs, left = [], text
        for ln in (len(text) // 3, 0, len(text) // 4):
            docs.append(left[:ln]); left = left[ln:]
        docs.append(left)
        repeats_case(eng, orc, text, device, starts=_gsa.doc_starts(docs))


# ---- the range build ------------------------------------------------------------------------------------------------------
def range_case(eng, orc, text, device, nranges=3):
    """_cases.range_slices with the text at every offset: k_key_hist_raw's byte path, sfx_pack_text_dev and the filter on a
    text that is not 16-byte aligned (plain and packed)."""
    exp = orc.sais(text)
    for i, off in enumerate(TEXT_OFFSETS):
        _cases.range_slices(eng, orc, text, nranges, device=device, packed=bool(i & 1), exp=exp, text_offset=off)


# ---- refusals -------------------------------------------------------------------------------------------------------------
def refusals(eng, orc, device):
    """A workspace one byte short is SFX_ERR_WORKSPACE; a misaligned workspace, u32 or u64 array is SFX_ERR_ARG -- decided on
    the host: outputs keep their fill, guard bands stay intact.  (Nothing misaligned ever reaches a kernel.)"""
    text = _gen.dna(5000, seed=9).tobytes()
    n = len(text)
    exp = orc.sais(text)
    lcp = orc.lcp_kasai(text, exp)

    def untouched(b, outs):
        for k in outs:
            assert (b[k].host() == 0xFF).all(), k
        check_all(b)

    for general in (False, True):
        ctx = _cases.general_build(eng) if general else _Null()
        with ctx:
            need = int(eng.lib.sfx_sa_workspace_bytes(n))
            rc, b = call_build_sa(eng, text, device, ws_bytes=need - 1)
            assert rc == ERR_WORKSPACE, rc
            untouched(b, ["sa"])
            for ws_off in (1, 4, 8):
                rc, b = call_build_sa(eng, text, device, ws_off=ws_off)
                assert rc == ERR_ARG, (rc, ws_off)
                untouched(b, ["sa"])
            for sa_off in (1, 2, 3):
                rc, b = call_build_sa(eng, text, device, sa_off=sa_off)
                assert rc == ERR_ARG, (rc, sa_off)
                untouched(b, ["sa"])
            need = int(eng.lib.sfx_sa_lcp_workspace_bytes(n))
            rc, b = call_build_sa_lcp(eng, text, device, ws_bytes=need - 1)
            assert rc == ERR_WORKSPACE, rc
            untouched(b, ["sa", "lcp"])
            rc, b = call_build_sa_lcp(eng, text, device, ws_off=8)
            assert rc == ERR_ARG, rc
            untouched(b, ["sa", "lcp"])
            rc, b = call_build_sa_lcp(eng, text, device, lcp_off=2)
            assert rc == ERR_ARG, rc
            untouched(b, ["sa", "lcp"])
    need = int(eng.lib.sfx_lcp_workspace_bytes(n))
    rc, b = call_build_lcp(eng, text, exp, device, ws_bytes=need - 1)
    assert rc == ERR_WORKSPACE, rc
    untouched(b, ["lcp"])
    rc, b = call_build_lcp(eng, text, exp, device, ws_off=4)
    assert rc == ERR_ARG, rc
    untouched(b, ["lcp"])
    rc, b = call_build_lcp(eng, text, exp, device, sa_off=2)
    assert rc == ERR_ARG, rc
    untouched(b, ["lcp"])
    st = stream_of(device)
    # u64 arrays: the query offsets, the document starts, the widened table, the histogram bins
    qs = [text[10:20], text[100:103], b"zz"]
    qb, qoff = query_arrays(qs)
    t, sa, q = text_in(text, device), inp(exp, device), inp(qb, device, 1)
    for off in (1, 4):
        qo = inp(qoff, device, off)
        o = query_outputs(len(qs), device, 0xFF, offs=(0, 0, 0, 0))
        assert eng.lib.sfx_query_batch_dev(t.ptr, n, sa.ptr, q.ptr, qo.ptr, len(qs), o["start"].ptr, o["end"].ptr, o["found"].ptr,
                                           o["any"].ptr, st) == ERR_ARG
        assert eng.lib.sfx_query_batch_range_dev(t.ptr, n, sa.ptr, n, q.ptr, qo.ptr, len(qs), o["start"].ptr, o["end"].ptr,
                                                 o["found"].ptr, o["any"].ptr, st) == ERR_ARG
        h = ctypes.c_void_p()
        assert eng.lib.sfx_index_create_dev(t.ptr, n, sa.ptr, st, ctypes.byref(h)) == OK
        try:
            assert eng.lib.sfx_index_query_dev(h, q.ptr, qo.ptr, len(qs), o["start"].ptr, o["end"].ptr, o["found"].ptr, o["any"].ptr,
                                               st) == ERR_ARG
        finally:
            if str(device).startswith("cuda"):
                torch.cuda.synchronize()
            eng.lib.sfx_index_destroy(h)
        untouched(o, list(o))
        wide = guarded(8 * n, device, off, 0xFF)
        assert eng.lib.sfx_widen_u32_to_u64_dev(sa.ptr, n, wide.ptr, st) == ERR_ARG
        untouched({"out": wide}, ["out"])
        bins = guarded(8 * 256, device, off, 0xFF)
        assert eng.lib.sfx_byte_histogram_dev(t.ptr, 0, n, bins.ptr, st) == ERR_ARG
        untouched({"bins": bins}, ["bins"])
        starts = inp(np.array([0, 100, 100, 3000], dtype=np.uint64), device, off)
        o = {k: guarded(4 * n, device, 0, 0xFF) for k in ("sa", "da", "lcp")}
        ws = guarded(int(eng.lib.sfx_gsa_workspace_bytes(n, 4)), device, 0, 0xFF)
        assert eng.lib.sfx_build_gsa_u32_dev(t.ptr, n, starts.ptr, 4, o["sa"].ptr, o["da"].ptr, o["lcp"].ptr, ws.ptr, ws.nbytes, st) == ERR_ARG
        assert eng.lib.sfx_doc_lookup_dev(sa.ptr, n, starts.ptr, 4, o["sa"].ptr, o["da"].ptr, st) == ERR_ARG
        untouched(o, list(o))
    # the workspaces of the other entry points: one byte short, then misaligned
    lc = inp(lcp, device)
    names = ("lb", "rb", "node", "parent", "leaf_parent")
    for short, ws_off, want in ((1, 0, ERR_WORKSPACE), (0, 8, ERR_ARG)):
        o = {k: guarded(4 * n, device, 0, 0xFF) for k in names}
        ws = guarded(int(eng.lib.sfx_lcp_intervals_workspace_bytes(n)) - short, device, ws_off, 0xFF)
        assert eng.lib.sfx_lcp_intervals_dev(lc.ptr, n, *[o[k].ptr for k in names], ws.ptr, ws.nbytes, st) == want
        untouched(o, list(o))
        ws.check_guards("workspace")
        starts = inp(np.array([0, 100, 100, 3000], dtype=np.uint64), device, 0)
        o = {k: guarded(4 * n, device, 0, 0xFF) for k in ("sa", "da", "lcp")}
        ws = guarded(int(eng.lib.sfx_gsa_workspace_bytes(n, 4)) - short, device, ws_off, 0xFF)
        assert eng.lib.sfx_build_gsa_u32_dev(t.ptr, n, starts.ptr, 4, o["sa"].ptr, o["da"].ptr, o["lcp"].ptr, ws.ptr, ws.nbytes, st) == want
        untouched(o, list(o))
        ws.check_guards("workspace")
        for scope in (0, 1):
            o = {k: guarded(4 * n, device, 0, 0xFF) for k in ("rep", "src")}
            ws = guarded(int(eng.lib.sfx_repeat_lens_workspace_bytes(n, scope)) - short, device, ws_off, 0xFF)
            assert eng.lib.sfx_repeat_lens_dev(sa.ptr, lc.ptr, None, n, scope, o["rep"].ptr, o["src"].ptr, ws.ptr, ws.nbytes, st) == want
            untouched(o, list(o))
            ws.check_guards("workspace")
        o = {k: guarded(4 * (n + 1), device, 0, 0xFF) for k in ("begin", "end")}
        ws = guarded(int(eng.lib.sfx_repeat_spans_workspace_bytes(n)) - short, device, ws_off, 0xFF)
        count = ctypes.c_uint64(0)
        assert eng.lib.sfx_repeat_spans_dev(lc.ptr, n, 1, None, 0, o["begin"].ptr, o["end"].ptr, n + 1, ctypes.byref(count), ws.ptr,
                                            ws.nbytes, st) == want
        untouched(o, list(o))
        ws.check_guards("workspace")
        bb = inp(np.bincount(np.frombuffer(text, dtype=np.uint8), minlength=256).astype(np.uint64), device)
        part = guarded(4 * n, device, 0, 0xFF)
        ws = guarded(int(eng.lib.sfx_sa_range_workspace_bytes(n, n)) - short, device, ws_off, 0xFF)
        assert eng.lib.sfx_build_sa_range_u32_dev(t.ptr, n, bb.ptr, 8, 0, 256, n, part.ptr, ctypes.byref(count), ws.ptr, ws.nbytes, st) == want
        untouched({"part": part}, ["part"])
        ws.check_guards("workspace")


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False
