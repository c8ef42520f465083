"""The cases of the Burrows-Wheeler transform with sampled ranks and of its inverse (sfx_bwt_dev, sfx_bwt_u32,
sfx_unbwt_dev, sfx_unbwt), shared by test_bwt_emu.py (the emulator build, host memory) and
test_gpu_bwt.py (libsuffix_hip.so, HBM).

Nothing expected comes from the engine: the table is the oracle's, the transform is the definition in three numpy lines
(`definition`), and the inverse is compared with the text it started from."""
import contextlib
import ctypes
import random

import numpy as np
import torch

import _buffers
import _gsa
import suffix_amd
from suffix_amd import SuffixHipError, SuffixTable
from suffix_amd import device as sdev

OK, ERR_ARG, ERR_TOO_LARGE, ERR_WORKSPACE = 0, 1, 2, 5
MAX_CHAIN = 1 << 20
TILE = 16384                              # bytes of one bwt_rank tile in a build without hooks
KERNELS = {"bwt_gather", "bwt_rank", "unbwt_walk"}
ROUTES = ("dev", "host", "host_build", "table")

KNOWN = [(b"banana", 0, b"annbaa", [4]),
         (b"banana", 2, b"annbaa", [4, 6, 5]),
         (b"abracadabra", 4, b"ardrcaaaabb", [3, 8, 6]),
         (b"mississippi", 0, b"ipssmpissii", [5]),
         (b"a", 0, b"a", [1]),
         (b"aaaa", 2, b"aaaa", [4, 2])]


def sample_count(n, s):
    return 0 if n == 0 else (1 if s == 0 else -(-n // s))


def table_of(orc, text):
    return np.ascontiguousarray(orc.sais(text), dtype=np.uint32) if len(text) else np.zeros(0, dtype=np.uint32)


def definition(text, sa, s):
    """-> (bwt uint8, samples uint32) of the issue's definitions: L = t[sa - 1] without the entry at sa == 0, behind
    t[n-1]; samples = the rows (rank + 1) of the suffixes at 0, s, 2s, ..."""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    n = t.size
    if n == 0:
        return np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint32)
    sa = np.asarray(sa).astype(np.int64)
    L = np.concatenate([t[n - 1:], t[sa - 1][sa != 0]])
    isa = np.empty(n, dtype=np.int64)
    isa[sa] = np.arange(n)
    return L, (isa[::s] + 1 if s else isa[:1] + 1).astype(np.uint32)


def _t(a, device, dtype=np.uint8):
    a = np.ascontiguousarray(np.frombuffer(bytes(a), dtype=np.uint8) if isinstance(a, (bytes, bytearray)) else a, dtype=dtype)
    return torch.from_numpy(a.view(np.int32 if dtype == np.uint32 else dtype).copy()).to(device)


def _sync(device):
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()


def forward(eng, device, route, text, sa, s):
    """One entry point or binding -> (bwt uint8, samples uint32) on the host."""
    n = len(text)
    if route == "dev":
        b, sm = sdev.bwt(_t(text, device), _t(sa, device, np.uint32), s, engine=eng)
        _sync(device)
        return b.cpu().numpy(), sm.cpu().numpy().view(np.uint32)
    if route == "table":
        b, sm = SuffixTable.from_parts(text, sa, engine=eng).bwt(s)
        return np.frombuffer(b, dtype=np.uint8), sm
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    b, sm = np.full(n, 0xEE, dtype=np.uint8), np.full(sample_count(n, s), 0xDEADBEEF, dtype=np.uint32)
    tab = np.ascontiguousarray(sa, dtype=np.uint32)
    rc = eng.lib.sfx_bwt_u32(_gsa.ptr(t), n, _gsa.ptr(tab) if route == "host" else None, s, _gsa.ptr(b), _gsa.ptr(sm))
    assert rc == OK, (route, rc)
    return b, sm


def inverse(eng, device, route, bwt, samples, s):
    """-> the restored text (bytes), or None where the entry point refuses the pair (SFX_ERR_ARG)."""
    n = len(bwt)
    if route == "dev":
        try:
            out = sdev.unbwt(_t(bwt, device), _t(samples, device, np.uint32), s, engine=eng)
        except SuffixHipError:
            return None
        return out.cpu().numpy().tobytes()
    if route == "table":
        try:
            return suffix_amd.unbwt(bytes(bwt), samples, s, engine=eng)
        except SuffixHipError:
            return None
    b, sm = np.ascontiguousarray(bwt, dtype=np.uint8), np.ascontiguousarray(samples, dtype=np.uint32)
    out = np.full(n, 0xEE, dtype=np.uint8)
    rc = eng.lib.sfx_unbwt(_gsa.ptr(b), n, _gsa.ptr(sm), sm.size, s, _gsa.ptr(out))
    assert rc in (OK, ERR_ARG), rc
    return out.tobytes() if rc == OK else None


def check_all_routes(eng, device, text, sa, s, want=None):
    """bwt and samples equal to the definition (and to `want`) and the round trip, through every route."""
    wb, ws = definition(text, sa, s)
    if want is not None:
        assert wb.tobytes() == want[0] and ws.tolist() == list(want[1]), (text, s)
    assert ws.size == sample_count(len(text), s) == int(eng.lib.sfx_bwt_sample_count(len(text), s))
    for route in ROUTES:
        b, sm = forward(eng, device, route, text, sa, s)
        assert np.array_equal(b, wb), (route, text[:40], s)
        assert np.array_equal(sm, ws), (route, text[:40], s)
        back = inverse(eng, device, "host" if route == "host_build" else route, b, sm, s)
        assert back == bytes(text), (route, text[:40], s)


# ---- 1. known answers ------------------------------------------------------------------------------------------------
def known_answers(eng, device, orc):
    for text, s, b, sm in KNOWN:
        check_all_routes(eng, device, text, table_of(orc, text), s, (b, sm))


# ---- 2. small random texts against the definition --------------------------------------------------------------------
def small_random(eng, device, orc, iters=320, seed=20261018):
    rng = random.Random(seed)
    done = 0
    for it in range(iters):
        sigma = (1, 2, 4, 256)[it % 4]
        n = rng.randint(0, 200) if it % 9 else rng.randint(0, 3)
        text = bytes(rng.randrange(sigma) for _ in range(n)) if sigma == 256 else bytes(rng.choice(b"ab\x00\xff"[:sigma]) for _ in range(n))
        sa = table_of(orc, text)
        s = (0, 1, 2, 8, 64, 256)[it % 6]                             # 256 >= every n here
        wb, ws = definition(text, sa, s)
        dev = forward(eng, device, "dev", text, sa, s)
        host = forward(eng, device, "host_build" if it % 8 == 0 else "host", text, sa, s)      # (sa == NULL: the table is built)
        for got in (dev, host):
            assert np.array_equal(got[0], wb) and np.array_equal(got[1], ws), (text, s)
        assert inverse(eng, device, "dev", wb, ws, s) == text, (text, s)
        assert inverse(eng, device, "host", wb, ws, s) == text, (text, s)
        done += 1
    return done


# ---- raw calls over guarded buffers ----------------------------------------------------------------------------------
def raw_forward(eng, device, text, sa, s, text_off=0, bwt_off=0, sm_off=4):
    n, cnt = len(text), sample_count(len(text), s)
    b = {"text": _buffers.text_in(text, device, text_off), "sa": _buffers.inp(np.ascontiguousarray(sa, dtype=np.uint32), device, 4),
         "bwt": _buffers.guarded(n, device, bwt_off, 0xFF), "samples": _buffers.guarded(4 * cnt, device, sm_off, 0xFF)}
    rc = eng.lib.sfx_bwt_dev(b["text"].ptr, n, b["sa"].ptr, s, b["bwt"].ptr, b["samples"].ptr, _buffers.stream_of(device))
    return rc, b


def raw_inverse(eng, device, bwt, samples, s, bwt_off=0, out_off=0, fill=0xFF, ws_bytes=None, ws_off=0, nsamples=None):
    n = len(bwt)
    sm = np.ascontiguousarray(samples, dtype=np.uint32)
    need = int(eng.lib.sfx_unbwt_workspace_bytes(n))
    b = {"bwt": _buffers.inp(np.frombuffer(bytes(bwt), dtype=np.uint8), device, bwt_off), "samples": _buffers.inp(sm, device, 4),
         "out": _buffers.guarded(n, device, out_off, 0xFF),
         "workspace": _buffers.guarded(need if ws_bytes is None else ws_bytes, device, ws_off, fill)}
    rc = eng.lib.sfx_unbwt_dev(b["bwt"].ptr, n, b["samples"].ptr, sm.size if nsamples is None else nsamples, s, b["out"].ptr,
                               b["workspace"].ptr, b["workspace"].nbytes, _buffers.stream_of(device))
    return rc, b


def guarded_round_trip(eng, device, text, sa, s, offs=(0, 0, 0, 0), fill=0xFF):
    """Forward and inverse over guarded buffers at the given (text, bwt, inverse-input, output) byte offsets; every
    result against the definition / the text, every guard band intact, the workspace exactly as long as stated."""
    wb, ws = definition(text, sa, s)
    rc, f = raw_forward(eng, device, text, sa, s, offs[0], offs[1])
    assert rc == OK, (rc, len(text), s)
    assert np.array_equal(f["bwt"].host(), wb) and np.array_equal(f["samples"].host(np.uint32), ws), (len(text), s, offs)
    _buffers.check_all(f)
    rc, i = raw_inverse(eng, device, wb, ws, s, offs[2], offs[3], fill)
    assert rc == OK, (rc, len(text), s)
    assert i["out"].host().tobytes() == bytes(text), (len(text), s, offs)
    _buffers.check_all(i)


# ---- 3. edges --------------------------------------------------------------------------------------------------------
def edge_texts():
    out = [b"", b"a", b"\x00", b"\xff", b"ab", b"ba", b"aa", b"\x00\xff", b"\xff\x00"]
    for k in (1, 2, 7, 64, 65):
        out += [b"a" + b"b" * k, b"b" + b"a" * k, b"z" * k]
    out += [bytes(range(256)), bytes(range(255, -1, -1)), bytes(range(256)) * 3, b"\x00" * 70, b"\xff" * 70, b"\x00\xff" * 40 + b"\x00"]
    return out


def edges(eng, device, orc):
    for text in edge_texts():
        sa = table_of(orc, text)
        n = len(text)
        for s in (0, 1, 2, 64):
            check_all_routes(eng, device, text, sa, s)
        if n:
            _, sm = definition(text, sa, 0)
            if text[:1] == b"a" and text[1:] == b"b" * (n - 1) and n > 1:
                assert sm[0] == 1                                     # primary = 1
            if text[:1] == b"b" and text[1:] == b"a" * (n - 1) and n > 1:
                assert sm[0] == n                                     # primary = n
    # n one less than, equal to and one more than a multiple of s
    rng = np.random.default_rng(5)
    for s in (8, 64):
        for n in (3 * s - 1, 3 * s, 3 * s + 1):
            text = rng.integers(97, 100, n).astype(np.uint8).tobytes()
            check_all_routes(eng, device, text, table_of(orc, text), s)
    # around one bwt_rank tile and around three; text, bwt and output at odd addresses; exact workspaces, dirty
    k = 0
    for n in (TILE - 1, TILE, TILE + 1, 3 * TILE - 1, 3 * TILE, 3 * TILE + 1):
        sigma = (256, 1, 4)[k % 3]
        text = rng.integers(0, sigma, n).astype(np.uint8).tobytes()
        sa = table_of(orc, text)
        for fill in (("count", 0xFF) if k == 0 else (0xFF,)):
            guarded_round_trip(eng, device, text, sa, (64, 256, 1024)[k % 3], ((1, 3, 1, 3), (3, 1, 15, 1), (15, 7, 3, 5))[k % 3], fill)
        k += 1
    # small ones at every output alignment (the walk stores four bytes at a time where the address allows)
    text = rng.integers(97, 101, 333).astype(np.uint8).tobytes()
    sa = table_of(orc, text)
    for off in range(8):
        for s in (0, 1, 2, 8, 512):
            guarded_round_trip(eng, device, text, sa, s, (off, off ^ 1, 7 - off, off), (0x00, 0xFF, "count")[off % 3])
    # a side stream
    side = torch.cuda.Stream() if str(device).startswith("cuda") else None
    with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
        guarded_round_trip(eng, device, text, sa, 8, (1, 1, 1, 1))
        text2 = rng.integers(0, 256, TILE + 77).astype(np.uint8).tobytes()
        guarded_round_trip(eng, device, text2, table_of(orc, text2), 64, (3, 5, 7, 9))
    _sync(device)


# ---- 4. refusals and integrity ---------------------------------------------------------------------------------------
def refusals(eng, device, orc):
    text = b"mississippi river banks" * 9
    n = len(text)
    sa = table_of(orc, text)
    wb, ws = definition(text, sa, 8)
    lib = eng.lib
    assert int(lib.sfx_bwt_sample_count(n, 3)) == 0 and int(lib.sfx_bwt_sample_count(0, 8)) == 0
    assert int(lib.sfx_bwt_sample_count(n, 0)) == 1 and int(lib.sfx_bwt_sample_count(17, 16)) == 2
    assert int(lib.sfx_unbwt_workspace_bytes(0)) == 0
    # a step that is no power of two
    rc, b = raw_forward(eng, device, text, sa, 3)
    assert rc == ERR_ARG and (b["bwt"].host() == 0xFF).all()
    rc, b = raw_inverse(eng, device, wb, ws, 3)
    assert rc == ERR_ARG
    t = np.frombuffer(text, dtype=np.uint8)
    o8, o32 = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint32)
    assert lib.sfx_bwt_u32(_gsa.ptr(t), n, _gsa.ptr(sa), 12, _gsa.ptr(o8), _gsa.ptr(o32)) == ERR_ARG
    assert lib.sfx_unbwt(_gsa.ptr(wb), n, _gsa.ptr(ws), ws.size, 12, _gsa.ptr(o8)) == ERR_ARG
    # n beyond u32, n == 0
    assert lib.sfx_bwt_dev(None, 1 << 32, None, 8, None, None, None) == ERR_TOO_LARGE
    assert lib.sfx_unbwt_dev(None, 1 << 32, None, 1 << 29, 8, None, None, 0, None) == ERR_TOO_LARGE
    assert lib.sfx_bwt_dev(None, 0, None, 8, None, None, None) == OK
    assert lib.sfx_unbwt_dev(None, 0, None, 0, 8, None, None, 0, None) == OK
    assert lib.sfx_unbwt_dev(None, 0, None, 1, 8, None, None, 0, None) == ERR_ARG
    # wrong nsamples
    for wrong in (ws.size - 1, ws.size + 1, 0):
        rc, b = raw_inverse(eng, device, wb, ws, 8, nsamples=wrong)
        assert rc == ERR_ARG and (b["out"].host() == 0xFF).all(), wrong
    assert lib.sfx_unbwt(_gsa.ptr(wb), n, _gsa.ptr(ws), ws.size - 1, 8, _gsa.ptr(o8)) == ERR_ARG
    # a sample of 0 and one of n + 1, at the front, inside and at the end
    for pos in (0, 1, ws.size - 1):
        for bad in (0, n + 1, 0xFFFFFFFF):
            sm = ws.copy()
            sm[pos] = bad
            rc, b = raw_inverse(eng, device, wb, sm, 8)
            assert rc == ERR_ARG, (pos, bad)
            _buffers.check_all(b)
            assert inverse(eng, device, "host", wb, sm, 8) is None
    # output overlapping the transform
    need = int(lib.sfx_unbwt_workspace_bytes(n))
    buf = _buffers.guarded(2 * n, device, 0, 0x41)
    smp = _buffers.inp(ws, device, 4)
    wsb = _buffers.guarded(need, device, 0, 0xFF)
    base = buf.ptr.value
    for delta in (0, 1, n - 1, -(n - 1)):
        src = base + (n - 1 if delta < 0 else 0)
        rc = lib.sfx_unbwt_dev(ctypes.c_void_p(src), n, smp.ptr, ws.size, 8, ctypes.c_void_p(src + delta), wsb.ptr, need, _buffers.stream_of(device))
        assert rc == ERR_ARG, delta
    assert (buf.host() == 0x41).all()
    # workspace too short, missing, misaligned
    rc, b = raw_inverse(eng, device, wb, ws, 8, ws_bytes=need - 1)
    assert rc == ERR_WORKSPACE and (b["out"].host() == 0xFF).all()
    _buffers.check_all(b)
    rc = lib.sfx_unbwt_dev(b["bwt"].ptr, n, b["samples"].ptr, ws.size, 8, b["out"].ptr, None, 0, _buffers.stream_of(device))
    assert rc == ERR_WORKSPACE
    rc, b = raw_inverse(eng, device, wb, ws, 8, ws_bytes=need + 16, ws_off=4)
    assert rc == ERR_ARG and (b["out"].host() == 0xFF).all()
    # misaligned samples
    rc, b = raw_forward(eng, device, text, sa, 8, sm_off=2)
    assert rc == ERR_ARG and (b["bwt"].host() == 0xFF).all()
    # a chain over SFX_UNBWT_MAX_CHAIN: refused on the host, nothing launched, nothing written
    big = MAX_CHAIN + 1
    zeros = bytes(big)
    for s, cnt in ((0, 1), (MAX_CHAIN * 2, 1)):
        got = {}
        names = _gsa.profile_names(eng, lambda: got.update(r=raw_inverse(eng, device, zeros, np.full(cnt, big, dtype=np.uint32), s)))
        rc, b = got["r"]
        assert rc == ERR_ARG and names == set(), (s, names)
        assert (b["out"].host() == 0xFF).all() and (b["workspace"].host() == 0xFF).all()
    o = np.zeros(big, dtype=np.uint8)
    one = np.full(1, big, dtype=np.uint32)
    o2 = np.zeros(big, dtype=np.uint8)
    assert lib.sfx_unbwt(_gsa.ptr(o), big, _gsa.ptr(one), 1, 0, _gsa.ptr(o2)) == ERR_ARG
    # ... and MAX_CHAIN itself is within the contract (all one byte: primary = n)
    assert inverse(eng, device, "dev", bytes(MAX_CHAIN), np.full(1, MAX_CHAIN, dtype=np.uint32), 0) == bytes(MAX_CHAIN)


def integrity(eng, device, orc, pairs=50, seed=99):
    """One flipped bwt byte or one changed sample: SFX_ERR_ARG, or a text whose transform IS the mutated pair."""
    rng = random.Random(seed)
    refused = accepted = 0
    for it in range(pairs):
        sigma = (2, 3, 4, 26)[it % 4]
        n = rng.randint(2, 150)
        text = bytes(97 + rng.randrange(sigma) for _ in range(n))
        s = (0, 1, 4, 16, 64)[it % 5]
        wb, ws = definition(text, table_of(orc, text), s)
        b, sm = wb.copy(), ws.copy()
        if it % 2:
            k = rng.randrange(sm.size)
            sm[k] = rng.choice([v for v in range(1, n + 1) if v != sm[k]])
        else:
            k = rng.randrange(n)
            b[k] = rng.choice([c for c in set(text) | {0, 255} if c != b[k]])
        for route in ("dev", "host"):
            back = inverse(eng, device, route, b, sm, s)
            if back is None:
                refused += 1
                continue
            accepted += 1
            vb, vs = definition(back, table_of(orc, back), s)
            assert np.array_equal(vb, b) and np.array_equal(vs, sm), (text, s, it)
    assert refused >= pairs                                             # (most single changes break the cycle)
    return refused, accepted


def bad_tables(eng, device, orc):
    """The forward table is unchecked: one without a zero entry and one with two read and write nothing out of bounds."""
    rng = np.random.default_rng(11)
    for n in (1, 2, 9, 300, TILE + 3):
        text = rng.integers(97, 100, n).astype(np.uint8).tobytes()
        sa = table_of(orc, text)
        zero = int(np.flatnonzero(sa == 0)[0])
        none, two = sa.copy(), sa.copy()
        none[zero] = n - 1
        two[(zero + 1) % n] = 0
        hi = np.full(n, n - 1, dtype=np.uint32)
        for tab in (none, two, hi, np.zeros(n, dtype=np.uint32)):
            for s in (0, 1, 8):
                rc, b = raw_forward(eng, device, text, tab, s, 1, 1)
                assert rc == OK
                _buffers.check_all(b)


# ---- 5. no host fallback ---------------------------------------------------------------------------------------------
def launch_names(eng, device, orc):
    text = b"she sells sea shells by the sea shore" * 20
    sa = table_of(orc, text)
    eng.profile(True)
    eng.profile_reset()
    try:
        b, sm = forward(eng, device, "dev", text, sa, 16)
        assert inverse(eng, device, "dev", b, sm, 16) == text
        rep = {r["name"]: r["launches"] for r in eng.profile_report()}
    finally:
        eng.profile(False)
    for name in KERNELS:
        assert rep.get(name, 0) >= 1, (name, rep)


# ---- small tiles (a build with hooks: SFX_BWT_TILE=256 SFX_MAX_GRID=3 in the environment) -----------------------------
def small_tiles(eng, device, orc, tile=256):
    """Texts of 1 .. 40 tiles: every workgroup takes several tiles and the per-symbol scan several tiles per chunk."""
    rng = np.random.default_rng(3)
    for n in (tile - 1, tile, tile + 1, 3 * tile - 1, 3 * tile, 3 * tile + 1, 10 * tile + 5, 40 * tile + 129):
        for sigma in (1, 2, 256):
            text = rng.integers(0, sigma, n).astype(np.uint8).tobytes()
            sa = table_of(orc, text)
            if n >= 10 * tile:                                        # 1 KiB of counts per 256-byte tile: the hook is on
                assert int(eng.lib.sfx_unbwt_workspace_bytes(n)) >= 7 * n
            guarded_round_trip(eng, device, text, sa, 64, (1, 3, 5, 7), "count")
