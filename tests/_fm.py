"""The cases of the FM-index over the Burrows-Wheeler pair (sfx_fm_*), shared by test_fm_emu.py
(the emulator build, host memory) and test_gpu_fm.py (libsuffix_hip.so, HBM).

Nothing expected comes from the engine: the table is the oracle's (`oracle.sais`), the pair is the numpy definition of
tests/_bwt.py, the intervals are `oracle.positions_batch`'s and the lookups are the table itself."""
import contextlib
import ctypes
import os
import random
import subprocess

import numpy as np
import torch

import _buffers
import _bwt
import _gsa
from suffix_amd import FmIndex, SuffixHipError, SuffixTable
from suffix_amd import device as sdev
from suffix_amd._lib import FmInfo

OK, ERR_ARG, ERR_TOO_LARGE = 0, 1, 2
NONE = 0xFFFFFFFF
MAX_CHAIN = 1 << 20
KERNELS = {"fm_build", "fm_count", "fm_lookup"}
STEPS = (0, 1, 2, 8, 64)
OCC_STEPS = (32, 64, 128, 4096, 0)

table_of, definition, sample_count = _bwt.table_of, _bwt.definition, _bwt.sample_count
HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
CSRC_FROM_EMU = "../../suffix_amd/csrc"                                  # tests/emu/Makefile's CSRC


def build_emulator():
    """`make -C tests/emu`, with sfx_fm.hip's age taken into account: the file is compiled as part of sfx_api.hip's
    translation unit and tests/emu/Makefile does not name it, so after an edit to it alone make would keep the previous
    kernels.  Then sfx_api.hip is declared new (`make -W`), which rebuilds sfx_api.o and the library.
    -> the library's path."""
    lib = os.path.join(EMU_DIR, "libsuffix_emu.so")
    cmd = ["make", "-s", "-j8", "-C", EMU_DIR]
    fm = os.path.join(HERE, os.pardir, "suffix_amd", "csrc", "sfx_fm.hip")
    if os.path.exists(lib) and os.path.getmtime(fm) > os.path.getmtime(lib):
        cmd += ["-W", CSRC_FROM_EMU + "/sfx_api.hip"]
    subprocess.check_call(cmd)
    return lib


def expected(orc, text, sa, qs):
    """The oracle's intervals: (start, end) lists, (0, 0) wherever there is no match."""
    if not len(text) or not qs:
        return [0] * len(qs), [0] * len(qs)
    ps, pe = orc.positions_batch(text, sa, *_buffers.query_arrays(qs))
    return ps.tolist(), pe.tolist()


def _sync(device):
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()


# ---- the raw ABI over guarded buffers --------------------------------------------------------------------------------
class Handle:
    """sfx_fm_create_dev over inputs between guard bands: the transform at an odd address, the samples at +4."""

    def __init__(self, eng, device, bwt, samples, s, occ_step=0, bwt_off=1, nsamples=None, host=False):
        self.eng, self.device, self.n = eng, device, len(bwt)
        b = np.frombuffer(bytes(bwt), dtype=np.uint8)
        sm = np.ascontiguousarray(samples, dtype=np.uint32)
        ns = sm.size if nsamples is None else nsamples
        h = ctypes.c_void_p()
        if host:
            self.rc = eng.lib.sfx_fm_create(_gsa.ptr(b), self.n, _gsa.ptr(sm), ns, s, occ_step, ctypes.byref(h))
        else:
            bufs = {"bwt": _buffers.inp(b, device, bwt_off), "samples": _buffers.inp(sm, device, 4)}
            self.rc = eng.lib.sfx_fm_create_dev(bufs["bwt"].ptr, self.n, bufs["samples"].ptr, ns, s, occ_step, _buffers.stream_of(device),
                                                ctypes.byref(h))
            _buffers.check_all(bufs)
            del bufs                                                   # the handle owns its memory: the pair may go
        self.h = h if self.rc == OK else None
        assert (self.rc == OK) == bool(h), (self.rc, h)
        self.host = host

    def info(self):
        i = FmInfo()
        assert self.eng.lib.sfx_fm_info(self.h, ctypes.byref(i)) == OK
        return i.as_dict()

    def count(self, qs, q_off=1):
        """-> (rc, start list, end list); every output between guard bands, the query bytes at an odd address."""
        qb, qoff = _buffers.query_arrays(qs)
        nq = len(qs)
        if self.host:
            s, e = np.full(nq, 0xDEADBEEF, dtype=np.uint32), np.full(nq, 0xDEADBEEF, dtype=np.uint32)
            rc = self.eng.lib.sfx_fm_count(self.h, _gsa.ptr(qb), _gsa.ptr(qoff), nq, _gsa.ptr(s), _gsa.ptr(e))
            return rc, s.tolist(), e.tolist()
        b = {"qbytes": _buffers.inp(qb, self.device, q_off), "qoff": _buffers.inp(qoff, self.device, 8),
             "start": _buffers.guarded(4 * nq, self.device, 4, 0xFF), "end": _buffers.guarded(4 * nq, self.device, 12, "count")}
        rc = self.eng.lib.sfx_fm_count_dev(self.h, b["qbytes"].ptr, b["qoff"].ptr, nq, b["start"].ptr, b["end"].ptr,
                                           _buffers.stream_of(self.device))
        _buffers.check_all(b)
        return rc, b["start"].host(np.uint32).tolist(), b["end"].host(np.uint32).tolist()

    def lookup(self, ranks=None, first=0, count=None):
        """-> (rc, positions uint32); ranks None: first + j."""
        r = None if ranks is None else np.ascontiguousarray(ranks, dtype=np.uint32)
        count = int(r.size if r is not None else count)
        if self.host:
            pos = np.full(count, 0xDEADBEEF, dtype=np.uint32)
            rc = self.eng.lib.sfx_fm_lookup(self.h, _gsa.ptr(r) if r is not None else None, first, count, _gsa.ptr(pos))
            return rc, pos
        b = {"pos": _buffers.guarded(4 * count, self.device, 8, "count")}
        if r is not None:
            b["ranks"] = _buffers.inp(r, self.device, 12)
        rc = self.eng.lib.sfx_fm_lookup_dev(self.h, b["ranks"].ptr if r is not None else None, first, count, b["pos"].ptr,
                                            _buffers.stream_of(self.device))
        _buffers.check_all(b)
        return rc, b["pos"].host(np.uint32)

    def close(self):
        h, self.h = self.h, None
        if h:
            _sync(self.device)
            self.eng.lib.sfx_fm_destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def check_pair(eng, device, orc, text, sa, s, occ_step, qs, host=False, all_ranks=True, rng=None, want=None):
    """One index over the definition's pair: every interval the oracle's, every lookup the table's entry, the size
    within its bound.  -> the oracle's (start, end)."""
    n = len(text)
    wb, ws = definition(text, sa, s)
    ps, pe = want if want is not None else expected(orc, text, sa, qs)
    with Handle(eng, device, wb, ws, s, occ_step, host=host) as h:
        assert h.rc == OK, (h.rc, n, s, occ_step)
        info = h.info()
        assert info["n"] == n and info["sample_step"] == s and info["nsamples"] == ws.size, info
        assert info["sigma"] == len(set(text)), info
        if n:
            assert info["occ_step"] == occ_step or (occ_step == 0 and 64 <= info["occ_step"] <= 4096), info
            assert info["bytes"] <= int(eng.lib.sfx_fm_bytes(n, s, occ_step)), (info, n, s, occ_step)
            if occ_step == 0 and s >= 32:
                assert info["bytes"] <= n * (1 + 1 / 4 + 1 / 6 + 1 / 8) + 65536, (info, n)
        rc, gs, ge = h.count(qs, q_off=1 + 2 * (n & 1))
        assert rc == OK
        assert (gs, ge) == (ps, pe), (text[:40], s, occ_step, [(q, a, b, c, d) for q, a, b, c, d in zip(qs, gs, ge, ps, pe) if (a, b) != (c, d)][:3])
        if all_ranks:
            rc, pos = h.lookup(None, 0, n)
            assert rc == OK and np.array_equal(pos, sa), (text[:40], s, occ_step)
        rng = rng or random.Random(n * 31 + s)
        ranks = np.array([rng.randrange(n) for _ in range(min(n, 48))] + [n, n + 1, NONE], dtype=np.uint32) if n else np.array([0, 1, NONE], dtype=np.uint32)
        rng.shuffle(ranks)
        rc, pos = h.lookup(ranks)
        assert rc == OK
        want_pos = np.where(ranks < n, np.concatenate([sa, [0]])[np.minimum(ranks, n)], NONE).astype(np.uint32)
        assert np.array_equal(pos, want_pos), (text[:40], s, occ_step)
        if n > 2 and all_ranks:                                        # a stretch in the middle through first + j
            rc, pos = h.lookup(None, n // 3, n - n // 3 + 2)
            assert rc == OK and np.array_equal(pos[:-2], sa[n // 3:]) and (pos[-2:] == NONE).all()
    return ps, pe


def check_bindings(eng, device, orc, text, sa, s, qs):
    """FmDeviceIndex, FmIndex and SuffixTable.fm_index against the oracle, positions() element for element."""
    n = len(text)
    wb, ws = definition(text, sa, s)
    ps, pe = expected(orc, text, sa, qs)
    qb, qoff = _buffers.query_arrays(qs)
    dq = torch.from_numpy(qb.copy()).to(device)
    doff = torch.from_numpy(qoff.astype(np.int64)).to(device)
    ix = sdev.FmDeviceIndex(_bwt._t(wb, device), _bwt._t(ws, device, np.uint32), s, engine=eng)
    try:
        assert ix.info["n"] == n
        # the handle owns its memory: no tensor the binding keeps may share the pair's storage (a view would hold all n bytes)
        assert all(t.untyped_storage().nbytes() == 0 for t in vars(ix).values() if torch.is_tensor(t)), vars(ix)
        a, b = ix.count(dq, doff)
        _sync(device)
        assert a.cpu().numpy().view(np.uint32).tolist() == ps and b.cpu().numpy().view(np.uint32).tolist() == pe
        assert np.array_equal(ix.sa_range(0, n).cpu().numpy().view(np.uint32), sa)
        if n:
            r = torch.arange(n - 1, -1, -1, dtype=torch.int32, device=device)
            assert np.array_equal(ix.lookup(r).cpu().numpy().view(np.uint32), sa[::-1])
        off, pos = ix.locate(dq, doff)
        off, pos = off.cpu().numpy(), pos.cpu().numpy().view(np.uint32)
        assert off.tolist() == np.concatenate([[0], np.cumsum(np.array(pe) - np.array(ps))]).tolist()
        for k in range(len(qs)):
            assert np.array_equal(pos[off[k]:off[k + 1]], sa[ps[k]:pe[k]]), qs[k]
    finally:
        _sync(device)
        ix.close()
    table = SuffixTable.from_parts(text, sa, engine=eng)
    for fm in (FmIndex.from_bwt(wb.tobytes(), ws, s, engine=eng), table.fm_index(s)):
        assert fm.len() == len(fm) == n and (fm.nbytes > n) == (n > 0)
        assert fm.lookup(first=n + 5).size == 0 and fm.lookup(first=n).size == 0              # nothing behind the table
        for k, q in enumerate(qs):
            assert fm.count(q) == pe[k] - ps[k] and fm.contains(q) == (pe[k] > ps[k]), q
            assert np.array_equal(fm.positions(q), sa[ps[k]:pe[k]]), q
        fm.close()


# ---- 1. known answers ------------------------------------------------------------------------------------------------
KNOWN_COUNTS = {b"banana": {b"a": 3, b"an": 2, b"ana": 2, b"banana": 1, b"nan": 1, b"x": 0, b"": 0, b"bananab": 0},
                b"abracadabra": {b"abra": 2, b"a": 5, b"bra": 2, b"cad": 1, b"x": 0, b"": 0},
                b"mississippi": {b"ssi": 2, b"i": 4, b"issi": 2, b"p": 2, b"mississippi": 1, b"x": 0, b"": 0}}


def known_answers(eng, device, orc):
    for text, counts in KNOWN_COUNTS.items():
        sa = table_of(orc, text)
        n = len(text)
        qs = sorted({text[i:j] for i in range(n) for j in range(i + 1, n + 1)}) + [b"x", b"", text + b"b", text]
        for s in (0, 2, 4):
            ps, pe = check_pair(eng, device, orc, text, sa, s, 0, qs)
            for q, c in counts.items():
                assert pe[qs.index(q)] - ps[qs.index(q)] == c, (text, q)                # (the oracle restates the literature)
            check_pair(eng, device, orc, text, sa, s, 32, qs, host=True)
            check_bindings(eng, device, orc, text, sa, s, qs)


# ---- 2. small random texts -------------------------------------------------------------------------------------------
def patterns_of(rng, text, count=40, max_len=40, longer=True):
    """Substrings of 1-max_len bytes, substrings with one byte changed (to a byte of the text, or to one it lacks), a byte
    the text lacks and (longer) one pattern longer than the text -- on a text of one repeated byte that one takes n
    dependent steps of a single lane."""
    n = len(text)
    lack = [c for c in (0x7E, 0x00, 0xFF, 0x41, 0x80) if c not in text] or [c for c in range(256) if c not in text]
    out = [bytes([lack[0]]) if lack else text[:1] + text[:1]] + ([text + (text[:1] or b"z")] if longer else [])
    while len(out) < count:
        kind = len(out) % 20
        if not n:
            out.append(bytes(rng.randrange(256) for _ in range(rng.randint(1, 5))))
            continue
        a = rng.randrange(n)
        q = bytearray(text[a:a + rng.randint(1, max_len)])
        if kind >= 12:
            q[rng.randrange(len(q))] = (lack[rng.randrange(len(lack))] if lack and kind >= 15 else text[rng.randrange(n)])
        out.append(bytes(q))
    return out


def random_text(rng, sigma, n):
    if sigma == 256:
        return bytes(rng.randrange(256) for _ in range(n))
    return bytes(rng.choice(b"ab\x00\xff"[:sigma]) for _ in range(n))


def small_random(eng, device, orc, iters=320, seed=20261018, long_every=4, full=False):
    rng = random.Random(seed)
    present = absent = 0
    for it in range(iters):
        sigma = (1, 2, 4, 256)[it % 4]
        s = STEPS[it % 5]
        occ = OCC_STEPS[(it // 5) % 5]
        # (the emulator runs a fiber per lane: long texts now and then, and short ones where one chain is the whole text)
        # (full: the GPU, where a lane costs nothing -- every text from the whole range)
        top = 600 if full or ((it // 4) % long_every == 0 and s) else (120 if s else 60)
        n = rng.randint(0, top) if it % 9 else rng.randint(0, 3)
        text = random_text(rng, sigma, n)
        sa = table_of(orc, text)
        qs = patterns_of(rng, text)
        ps, pe = check_pair(eng, device, orc, text, sa, s, occ, qs, host=it % 8 == 3, rng=rng)
        present += sum(1 for a, b in zip(ps, pe) if b > a)
        absent += sum(1 for a, b in zip(ps, pe) if b == a)
    assert present >= 0.4 * (present + absent) and absent >= 0.2 * (present + absent), (present, absent)
    return iters


# ---- 3. edges --------------------------------------------------------------------------------------------------------
def edges(eng, device, orc, big_all_ranks=True):
    rng = np.random.default_rng(18)
    prng = random.Random(7)
    # n = 0, 1, 2; NUL and 0xFF bytes
    for text in (b"", b"a", b"\x00", b"\xff", b"ab", b"ba", b"aa", b"\x00\xff", b"\xff\x00", b"\x00\xff" * 40 + b"\x00", b"\xff" * 70):
        sa = table_of(orc, text)
        qs = [b"", b"a", b"b", b"ab", b"ba", b"aa", b"\x00", b"\xff", b"\x00\xff", b"\xff\x00", b"\xff\xff\xff", text, text + b"a"]
        for s in (0, 1, 2):
            check_pair(eng, device, orc, text, sa, s, (0, 32, 64)[s], qs)
        check_bindings(eng, device, orc, text, sa, 2, qs)
    # primary = 1 and primary = n, rows on both sides of the primary counted
    for k in (1, 2, 7, 64, 65):
        for text, primary in ((b"a" + b"b" * k, 1), (b"b" + b"a" * k, k + 1)):
            sa = table_of(orc, text)
            assert definition(text, sa, 0)[1][0] == primary
            qs = [b"a", b"b", b"ab", b"ba", b"bb", b"aa", b"abb", b"baa", b"b" * k, b"a" * k, text, text[1:], b"c"]
            for s in (0, 4):
                check_pair(eng, device, orc, text, sa, s, 32, qs)
    # n around the blocks: one less, exactly, one more, two blocks, three and one entry
    for B in (32, 64, 128, 4096):
        for n in (B - 1, B, B + 1, 2 * B, 3 * B + 1):
            sigma = (2, 4, 256)[n % 3]
            text = rng.integers(0, sigma, n).astype(np.uint8).tobytes()
            sa = table_of(orc, text)
            check_pair(eng, device, orc, text, sa, (8, 64)[n & 1], B, patterns_of(prng, text), all_ranks=big_all_ranks or B < 4096)
    # one symbol: count("a" * k) = n - k + 1; lo walks 0, 1, 2, .. through r == B / 2 and over the block's end, hi stays at n
    for B, n in ((32, 3 * 32 + 1), (64, 64), (128, 129)):
        text = b"a" * n
        sa = table_of(orc, text)
        qs = [b"a" * k for k in range(1, n + 2)]
        ps, pe = check_pair(eng, device, orc, text, sa, 8, B, qs)
        assert [b - a for a, b in zip(ps, pe)] == [n - k + 1 for k in range(1, n + 2)]
    # lo and hi in one half-block: rare patterns of a text of several blocks (intervals of one to three rows)
    text = rng.integers(97, 101, 1500).astype(np.uint8).tobytes()
    sa = table_of(orc, text)
    qs = [text[a:a + 12] for a in range(0, 1400, 37)] + [text[a:a + 5] for a in range(0, 1400, 41)]
    for B in (32, 128, 4096):
        ps, pe = check_pair(eng, device, orc, text, sa, 64, B, qs, all_ranks=False)
        assert max(b - a for a, b in zip(ps, pe)) <= 8 and min(b - a for a, b in zip(ps, pe)) >= 1
    # nq == 0; a side stream
    wb, ws = definition(text, sa, 8)
    with Handle(eng, device, wb, ws, 8) as h:
        assert h.count([])[0] == OK
        assert eng.lib.sfx_fm_count_dev(h.h, None, None, 0, None, None, _buffers.stream_of(device)) == OK
        assert eng.lib.sfx_fm_lookup_dev(h.h, None, 0, 0, None, _buffers.stream_of(device)) == OK
    side = torch.cuda.Stream() if str(device).startswith("cuda") else None
    with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
        check_pair(eng, device, orc, text, sa, 8, 0, qs)
    _sync(device)


def small_grid(eng, device, orc):
    """More teams than the grid holds (a build with hooks: SFX_MAX_GRID=3 in the environment): every team takes several
    patterns and several ranks, and every scan chunk of the build several blocks."""
    rng = np.random.default_rng(4)
    prng = random.Random(5)
    for n, sigma, B in ((700, 4, 32), (2500, 256, 64), (3 * 4096 + 1, 3, 4096), (3000, 90, 0)):
        text = rng.integers(0, sigma, n).astype(np.uint8).tobytes()
        sa = table_of(orc, text)
        qs = patterns_of(prng, text, 120)
        check_pair(eng, device, orc, text, sa, 8, B, qs)


# ---- 4. refusals and unchecked input ---------------------------------------------------------------------------------
def refusals(eng, device, orc):
    lib = eng.lib
    text = b"mississippi river banks" * 9
    n = len(text)
    sa = table_of(orc, text)
    wb, ws = definition(text, sa, 8)
    for host in (False, True):
        assert Handle(eng, device, wb, ws, 3, host=host).rc == ERR_ARG                       # a bad step
        assert Handle(eng, device, wb, ws, 12, host=host).rc == ERR_ARG
        for wrong in (ws.size - 1, ws.size + 1, 0):                                          # nsamples
            assert Handle(eng, device, wb, ws, 8, nsamples=wrong, host=host).rc == ERR_ARG
        for occ in (1, 16, 48, 8192, 1 << 31):                                               # a bad occ_step
            assert Handle(eng, device, wb, ws, 8, occ, host=host).rc == ERR_ARG
        for pos in (0, 1, ws.size - 1):                                                      # a sample outside [1, n]
            for bad in (0, n + 1, NONE):
                sm = ws.copy()
                sm[pos] = bad
                assert Handle(eng, device, wb, sm, 8, host=host).rc == ERR_ARG, (pos, bad)
        for a, b in ((0, 1), (3, ws.size - 1), (5, 6)):                                      # two equal samples
            sm = ws.copy()
            sm[a] = sm[b]
            assert Handle(eng, device, wb, sm, 8, host=host).rc == ERR_ARG, (a, b)
    h = ctypes.c_void_p()
    assert lib.sfx_fm_create_dev(None, 1 << 32, None, 1 << 29, 8, 0, None, ctypes.byref(h)) == ERR_TOO_LARGE and not h
    assert lib.sfx_fm_create(None, 1 << 32, None, 1 << 29, 8, 0, ctypes.byref(h)) == ERR_TOO_LARGE and not h
    assert int(lib.sfx_fm_bytes(0, 8, 0)) == 0 and int(lib.sfx_fm_bytes(n, 3, 0)) == 0 and int(lib.sfx_fm_bytes(n, 8, 48)) == 0
    assert int(lib.sfx_fm_bytes(1 << 32, 8, 0)) == 0 and int(lib.sfx_fm_bytes(n, 8, 0)) > n
    # misaligned samples, offsets and outputs: decided on the host
    bufs = {"bwt": _buffers.inp(wb, device, 0), "samples": _buffers.inp(ws, device, 2)}
    assert lib.sfx_fm_create_dev(bufs["bwt"].ptr, n, bufs["samples"].ptr, ws.size, 8, 0, _buffers.stream_of(device), ctypes.byref(h)) == ERR_ARG
    # n == 0: a valid empty index
    for host in (False, True):
        with Handle(eng, device, b"", np.zeros(0, dtype=np.uint32), 8, host=host) as e:
            assert e.rc == OK and e.info()["n"] == 0 and e.info()["bytes"] == 0
            assert e.count([b"", b"a", b"ab"]) == (OK, [0, 0, 0], [0, 0, 0])
            rc, pos = e.lookup(None, 0, 3)
            assert rc == OK and (pos == NONE).all()
        assert Handle(eng, device, b"", np.zeros(1, dtype=np.uint32), 8, nsamples=1, host=host).rc == ERR_ARG
    # ranks >= n
    with Handle(eng, device, wb, ws, 8) as g:
        rc, pos = g.lookup(np.array([n, n + 1, 1 << 31, NONE, 0, n - 1], dtype=np.uint32))
        assert rc == OK and pos.tolist() == [NONE] * 4 + [int(sa[0]), int(sa[n - 1])]
        rc, pos = g.lookup(None, n - 2, 5)
        assert rc == OK and pos.tolist() == [int(sa[n - 2]), int(sa[n - 1]), NONE, NONE, NONE]
        rc, pos = g.lookup(None, 1 << 40, 2)
        assert rc == OK and pos.tolist() == [NONE, NONE]
        qb, qoff = _buffers.query_arrays([b"ss"])
        q = {"qbytes": _buffers.inp(qb, device, 1), "qoff": _buffers.inp(qoff, device, 4), "out": _buffers.guarded(8, device, 0, 0xFF)}
        assert lib.sfx_fm_count_dev(g.h, q["qbytes"].ptr, q["qoff"].ptr, 1, q["out"].ptr, q["out"].ptr, _buffers.stream_of(device)) == ERR_ARG
        out2 = _buffers.guarded(8, device, 2, 0xFF)
        assert lib.sfx_fm_lookup_dev(g.h, None, 0, 1, out2.ptr, _buffers.stream_of(device)) == ERR_ARG
        assert (q["out"].host() == 0xFF).all() and (out2.host() == 0xFF).all()
    # a chain over SFX_UNBWT_MAX_CHAIN: lookup is refused on the host (nothing launched), count still works
    big = MAX_CHAIN + 1
    with Handle(eng, device, bytes(big), np.full(1, big, dtype=np.uint32), 0, 4096, bwt_off=0) as c:
        assert c.rc == OK
        got = {}
        names = _gsa.profile_names(eng, lambda: got.update(r=c.lookup(None, 0, 4)))
        assert got["r"][0] == ERR_ARG and names == set(), names
        assert c.count([b"\x00", b"\x00" * 5, b"\x01"]) == (OK, [0, 4, 0], [big, big, 0])


def mutated_pairs(eng, device, orc, pairs=50, seed=99):
    """Flipped bwt bytes, samples swapped or shifted inside [1, n]: refused at creation, or every call stays in bounds --
    intervals inside [0, n], positions < n or UINT32_MAX.  Never a crash; creation does not promise more."""
    rng = random.Random(seed)
    refused = accepted = 0
    for it in range(pairs):
        sigma = (2, 3, 4, 26)[it % 4]
        n = rng.randint(2, 150)
        text = bytes(97 + rng.randrange(sigma) for _ in range(n))
        s = (0, 1, 4, 16, 64)[it % 5]
        sa = table_of(orc, text)
        wb, ws = definition(text, sa, s)
        b, sm = wb.copy(), ws.copy()
        kind = it % 3
        if kind == 0 or sm.size < 2:
            for _ in range(rng.randint(1, 4)):
                b[rng.randrange(n)] = rng.choice([0, 255, 97, 98, 122])
        elif kind == 1:
            i, j = rng.sample(range(sm.size), 2)
            sm[i], sm[j] = sm[j], sm[i]
        else:
            sm[rng.randrange(sm.size)] = rng.randint(1, n)
        with Handle(eng, device, b, sm, s, OCC_STEPS[it % 5]) as h:
            if h.rc != OK:
                assert h.rc == ERR_ARG
                refused += 1
                continue
            accepted += 1
            qs = patterns_of(rng, text, 20) + patterns_of(rng, b.tobytes(), 10)
            rc, gs, ge = h.count(qs)
            assert rc == OK and all(0 <= a <= e <= n for a, e in zip(gs, ge)), (it, gs, ge)
            rc, pos = h.lookup(None, 0, n + 2)
            assert rc == OK and all(p < n or p == NONE for p in pos.tolist()), (it, pos)
            assert (pos[n:] == NONE).all()
    assert accepted >= pairs // 3, (refused, accepted)
    return refused, accepted


# ---- 5. size ---------------------------------------------------------------------------------------------------------
def sizes(eng, device, orc):
    """info.bytes <= sfx_fm_bytes(n, s, B) for every B, and with occ_step 0 and s >= 32 within n (1 + 1/4 + 1/6 + 1/8) +
    64 KiB: the bound the layout promises (check_pair asserts both), for alphabets of 1, 4, 90 and 256 symbols."""
    rng = np.random.default_rng(21)
    prng = random.Random(22)
    lib = eng.lib
    for sigma, want_step in ((1, 64), (4, 64), (90, 2048), (256, 4096)):
        n = 20000 + sigma
        text = rng.integers(0, sigma, n).astype(np.uint8).tobytes()
        sa = table_of(orc, text)
        for s, occ in ((32, 0), (64, 0), (256, 0), (32, 32), (64, 4096), (0, 128)):
            wb, ws = definition(text, sa, s)
            with Handle(eng, device, wb, ws, s, occ) as h:
                info = h.info()
                assert info["occ_step"] == (occ or want_step), (sigma, info)
                assert info["bytes"] <= int(lib.sfx_fm_bytes(n, s, occ)), (sigma, s, occ, info)
                if occ == 0 and s >= 32:
                    assert info["bytes"] <= n * (1 + 1 / 4 + 1 / 6 + 1 / 8) + 65536, (sigma, s, info)
                    assert info["bytes"] >= n * (1 + 4 * ((sigma + 3) // 4 * 4) / want_step + 64 / 480) + 4 * ws.size       # (every part is there)
    check_pair(eng, device, orc, text, sa, 32, 0, patterns_of(prng, text), all_ranks=False)


# ---- 6. launch names -------------------------------------------------------------------------------------------------
def launch_names(eng, device, orc):
    text = b"she sells sea shells by the sea shore" * 20
    sa = table_of(orc, text)
    names = _gsa.profile_names(eng, lambda: check_pair(eng, device, orc, text, sa, 16, 0, [b"sea", b"shells", b"zz"]))
    assert KERNELS <= names, names
