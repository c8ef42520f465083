"""The cases of the LZ77 factorization and its decoder (sfx_lz_parse_dev, sfx_lz_decode_dev, sfx_lz77_u32, sfx_unlz;
DESIGN.md section 19), shared by test_lz_emu.py (the emulator build, host memory) and test_gpu_lz.py (libsuffix_hip.so,
HBM).

Nothing expected comes from the engine: the longest-previous-factor array is the brute force of _repeats (or `lpf`, a
bytes.find loop that is itself held against that brute force), the parse is the definition as a plain loop
(`reference`), witnesses are checked as properties (src < begin, equal bytes), and the decoder is compared with the
text the parse started from or with a serial decode."""
import ctypes
import os
import random
import subprocess

import numpy as np
import torch

import _buffers
import _gen
import _gsa
import _repeats
import suffix_amd
from suffix_amd import SuffixHipError, SuffixTable
from suffix_amd import device as sdev

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
CSRC_FROM_EMU = "../../suffix_amd/csrc"
OK, ERR_ARG, ERR_TOO_LARGE, ERR_WORKSPACE = 0, 1, 2, 5
NONE = 0xFFFFFFFF
MIN_LENS = (1, 2, 3, 8, 1000)
ROUTES = ("dev", "host", "host_build", "table")
PARSE_KERNELS = {"lz_exit", "lz_walk_groups", "lz_walk_tiles", "lz_count", "lz_emit"}
DECODE_KERNELS = {"unlz_scan", "unlz_origin", "unlz_jump", "unlz_fill"}


def build_emulator():
    """`make -C tests/emu`, with sfx_lz.hip's age taken into account: the file is compiled as part of sfx_api.hip's
    translation unit and tests/emu/Makefile does not name it, so after an edit to it alone make would keep the previous
    kernels.  Then sfx_api.hip is declared new (`make -W`), which rebuilds sfx_api.o and the library.
    -> the library's path."""
    lib = os.path.join(EMU_DIR, "libsuffix_emu.so")
    cmd = ["make", "-s", "-j8", "-C", EMU_DIR]
    lz = os.path.join(HERE, os.pardir, "suffix_amd", "csrc", "sfx_lz.hip")
    if os.path.exists(lib) and os.path.getmtime(lz) > os.path.getmtime(lib):
        cmd += ["-W", CSRC_FROM_EMU + "/sfx_api.hip"]
    subprocess.check_call(cmd)
    return lib


# ---- the definition --------------------------------------------------------------------------------------------------
def lpf(text):
    """The longest-previous-factor array by bytes.find: L grows while text[p : p + L + 1] also starts before p
    (LPF[p] >= LPF[p - 1] - 1, so L never restarts from 0).  Engine-independent; `test_lpf_helper` holds it against
    _repeats.brute_rep."""
    text, n = bytes(text), len(text)
    out = np.zeros(n, dtype=np.uint32)
    L = 0
    for p in range(n):
        L = max(L - 1, 0)
        while p + L < n and text.find(text[p:p + L + 1], 0, p + L) != -1:
            L += 1
        out[p] = L
    return out


def next_of(rep, min_len):
    n = len(rep)
    r = np.minimum(np.asarray(rep, dtype=np.int64), n - np.arange(n))
    return np.arange(n) + np.where(r >= min_len, r, 1)


def reference(rep, min_len):
    """The phrases by the definition: -> (begin list, len list, copy flags)."""
    n = len(rep)
    begin, ln, copy = [], [], []
    p = 0
    while p < n:
        r = min(int(rep[p]), n - p)
        c = r >= min_len
        begin.append(p)
        ln.append(r if c else 1)
        copy.append(c)
        p += ln[-1]
    return begin, ln, copy


def serial_decode(ln, src, lit):
    out = bytearray()
    for l, s, c in zip(ln, src, lit):
        if s == NONE:
            out.append(c)
        else:
            for i in range(l):
                out.append(out[s + i])
    return bytes(out)


def check_phrases(text, rep, min_len, begin, ln, src, lit, what=""):
    """(begin, len) equal to the definition's; a literal is (1, NONE, its byte); a copy has lit 0, src < begin and len
    equal bytes -- which src is the engine's choice."""
    text = bytes(text)
    wb, wl, wc = reference(rep, min_len)
    assert [int(x) for x in ln] == wl, (what, min_len, text[:40], list(ln)[:12], wl[:12])
    if begin is not None:
        assert [int(x) for x in begin] == wb, (what, min_len, text[:40])
    for k, (b, l, c) in enumerate(zip(wb, wl, wc)):
        s = int(src[k])
        if c:
            assert s < b and text[s:s + l] == text[b:b + l], (what, "witness", k, b, l, s)
            assert lit is None or int(lit[k]) == 0, (what, "copy lit", k)
        else:
            assert s == NONE and (lit is None or int(lit[k]) == text[b]), (what, "literal", k, b, s)


# ---- routes ----------------------------------------------------------------------------------------------------------
def _t(a, device, dtype=np.int32):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(dtype).copy()).to(device)


def _h(t, dtype):
    return t.cpu().numpy().view(dtype) if t is not None else None


def table_of(orc, text):
    if not len(text):
        return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32)
    sa = np.ascontiguousarray(orc.sais(text), dtype=np.uint32)
    return sa, np.ascontiguousarray(orc.lcp_kasai(text, sa), dtype=np.uint32)


def parse(eng, device, route, text, sa, lcp, min_len):
    """-> (begin, len, src, lit) numpy arrays by one of the four routes."""
    text, n = bytes(text), len(text)
    t = np.frombuffer(text, dtype=np.uint8)
    if route == "dev":
        rep, src = sdev.repeat_lens(_t(sa, device), _t(lcp, device), "earlier", want_src=True, engine=eng)
        b, l, s, c = sdev.lz_parse(rep, src, _t(t, device, np.uint8), min_len=min_len, engine=eng)
        return _h(b, np.uint32), _h(l, np.uint32), _h(s, np.uint32), _h(c, np.uint8)
    if route == "table":
        f = SuffixTable.from_parts(text, sa, engine=eng).lz77(min_len)     # (the oracle's table: nothing is built)
        assert f.n == n and len(f) == f.len.size
        return f.begin, f.len, f.src, f.lit
    outs = [np.full(n, 0xDEADBEEF, dtype=np.uint32) for _ in range(3)] + [np.full(n, 0xEE, dtype=np.uint8)]
    count = ctypes.c_uint64(0)
    given = route == "host"
    rc = eng.lib.sfx_lz77_u32(_gsa.ptr(t), n, _gsa.ptr(sa) if given else None, _gsa.ptr(lcp) if given else None, min_len,
                              *[_gsa.ptr(a) for a in outs], n, ctypes.byref(count))
    assert rc == OK, (rc, route, n)
    z = int(count.value)
    for a in outs:
        assert (a[z:] == (0xDEADBEEF if a.dtype == np.uint32 else 0xEE)).all(), (route, "written past z")
    return tuple(a[:z] for a in outs)


def decode(eng, device, route, ln, src, lit, n):
    if route == "dev":
        out = sdev.lz_decode(_t(ln, device), _t(src, device), _t(lit, device, np.uint8), engine=eng)
        return bytes(_h(out, np.uint8))
    if route == "table":
        return suffix_amd.unlz(ln, src, lit, engine=eng)
    out = np.full(n, 0xEE, dtype=np.uint8)
    rc = eng.lib.sfx_unlz(_gsa.ptr(np.ascontiguousarray(ln)), _gsa.ptr(np.ascontiguousarray(src)), _gsa.ptr(np.ascontiguousarray(lit)),
                          len(ln), n, _gsa.ptr(out))
    assert rc == OK, (rc, route, n)
    return out.tobytes()


def check_all_routes(eng, device, orc, text, min_lens=MIN_LENS, rep=None, routes=ROUTES):
    text = bytes(text)
    sa, lcp = table_of(orc, text)
    rep = lpf(text) if rep is None else rep
    for m in min_lens:
        for route in routes:
            b, l, s, c = parse(eng, device, route, text, sa, lcp, m)
            check_phrases(text, rep, m, b, l, s, c, route)
            assert decode(eng, device, route, l, s, c, len(text)) == text, (route, m, text[:40])


# ---- 1. known answers, small random texts ----------------------------------------------------------------------------
def known_answers(eng, device, orc):
    for text, m, want in [(b"a", 1, [(0, 1, None)]), (b"aaaa", 1, [(0, 1, None), (1, 3, 0)]),
                          (b"abababab", 1, [(0, 1, None), (1, 1, None), (2, 6, 0)])]:
        f = SuffixTable(text, engine=eng).lz77(m)
        assert list(f) == want and f.decode() == text, (text, list(f))
    assert bytes(SuffixTable(b"aaaa", engine=eng).lz77().lit) == b"a\x00"
    for text in (b"banana", b"abracadabra", b"mississippi"):
        rep = _repeats.brute_rep(text, "earlier")
        assert np.array_equal(rep, lpf(text))
        check_all_routes(eng, device, orc, text, (1, 2, 3), rep)
    # banana at min_len 1: b, a, n, "ana" from 1; at 3 the same; mississippi at 1: m i s s "issi" p p i -> counted by hand
    assert [l for _, l, _ in SuffixTable(b"banana", engine=eng).lz77(1)] == [1, 1, 1, 3]
    assert [l for _, l, _ in SuffixTable(b"mississippi", engine=eng).lz77(1)] == [1, 1, 1, 1, 4, 1, 1, 1]
    assert [l for _, l, _ in SuffixTable(b"mississippi", engine=eng).lz77(2)] == [1, 1, 1, 1, 4, 1, 1, 1]
    assert [l for _, l, _ in SuffixTable(b"abracadabra", engine=eng).lz77(2)] == [1, 1, 1, 1, 1, 1, 1, 4]


def random_texts(iters, seed=20261019, max_len=600):
    """Texts of 0 .. max_len bytes over 1, 2, 4 and 256 symbols, every second one with its first half doubled."""
    rng = random.Random(seed)
    for i in range(iters):
        sigma = (1, 2, 4, 256)[i % 4]
        alpha = bytes(rng.sample(range(256), sigma))
        n = rng.randint(0, max_len)
        if (i // 4) % 2:
            h = bytes(rng.choice(alpha) for _ in range(n // 2))
            t = h + h + bytes(rng.choice(alpha) for _ in range(n - 2 * len(h)))
        else:
            t = bytes(rng.choice(alpha) for _ in range(n))
        yield t


def small_random(eng, device, orc, iters=300, seed=20261019):
    """Every text at two of the min_len values (they rotate) on the routes that take the oracle's table; every fifth text
    also on the route that builds the table itself (0.2 s per build on the emulator)."""
    done = 0
    for i, t in enumerate(random_texts(iters, seed)):
        check_all_routes(eng, device, orc, t, (MIN_LENS[i % 5], MIN_LENS[(i + 2) % 5]), routes=("dev", "host", "table"))
        if i % 5 == 0:
            check_all_routes(eng, device, orc, t, (MIN_LENS[(i // 5) % 5],), routes=("host_build",))
        done += 1
    return done


# ---- raw calls over guarded buffers ----------------------------------------------------------------------------------
def raw_parse(eng, device, rep, src, text, min_len, capacity=None, offs=(4, 8, 1), out_offs=(4, 8, 12, 3), fill=0xFF, ws_bytes=None,
              ws_off=0, want_begin=True, stream=None, n=None):
    """sfx_lz_parse_dev over guarded buffers -> (rc, z, buffers).  capacity None: n."""
    n = len(rep) if n is None else n
    cap = n if capacity is None else capacity
    need = int(eng.lib.sfx_lz_parse_workspace_bytes(n))
    b = {"rep": _buffers.inp(np.ascontiguousarray(rep, dtype=np.uint32), device, offs[0]),
         "src": _buffers.inp(np.ascontiguousarray(src, dtype=np.uint32), device, offs[1]),
         "begin": _buffers.guarded(4 * cap, device, out_offs[0], 0xFF), "len": _buffers.guarded(4 * cap, device, out_offs[1], 0xFF),
         "psrc": _buffers.guarded(4 * cap, device, out_offs[2], 0xFF), "lit": _buffers.guarded(cap, device, out_offs[3], 0xFF),
         "workspace": _buffers.guarded(need if ws_bytes is None else ws_bytes, device, ws_off, fill)}
    if text is not None:
        b["text"] = _buffers.text_in(bytes(text), device, offs[2])
    count = ctypes.c_uint64(0xDEAD)
    rc = eng.lib.sfx_lz_parse_dev(b["rep"].ptr, b["src"].ptr, b["text"].ptr if text is not None else None, n, min_len,
                                  b["begin"].ptr if want_begin else None, b["len"].ptr, b["psrc"].ptr, b["lit"].ptr, cap,
                                  ctypes.byref(count), b["workspace"].ptr, b["workspace"].nbytes,
                                  stream if stream is not None else _buffers.stream_of(device))
    return rc, int(count.value), b


def raw_decode(eng, device, ln, src, lit, n, offs=(4, 8, 1), out_off=0, fill=0xFF, ws_bytes=None, ws_off=0, stream=None):
    z = len(ln)
    need = int(eng.lib.sfx_lz_decode_workspace_bytes(n, z))
    b = {"len": _buffers.inp(np.ascontiguousarray(ln, dtype=np.uint32), device, offs[0]),
         "src": _buffers.inp(np.ascontiguousarray(src, dtype=np.uint32), device, offs[1]),
         "lit": _buffers.inp(np.ascontiguousarray(lit, dtype=np.uint8), device, offs[2]),
         "out": _buffers.guarded(n, device, out_off, 0xFF),
         "workspace": _buffers.guarded(need if ws_bytes is None else ws_bytes, device, ws_off, fill)}
    rc = eng.lib.sfx_lz_decode_dev(b["len"].ptr, b["src"].ptr, b["lit"].ptr, z, n, b["out"].ptr, b["workspace"].ptr,
                                   b["workspace"].nbytes, stream if stream is not None else _buffers.stream_of(device))
    return rc, b


def guarded_round_trip(eng, device, text, rep, src, min_len, offs=(4, 8, 1), out_offs=(4, 8, 12, 3), fill=0xFF, capacity=None,
                       ref=None, stream=None):
    """Parse and decode over guarded buffers, the workspaces exactly as long as stated: the phrases against the
    definition over `ref` (default: rep), nothing written past min(z, capacity), every guard band intact."""
    text = bytes(text)
    n = len(text)
    rc, z, p = raw_parse(eng, device, rep, src, text, min_len, capacity, offs, out_offs, fill, stream=stream)
    assert rc == OK, (rc, n, min_len)
    wb, wl, _ = reference(rep if ref is None else ref, min_len)
    assert z == len(wb), (z, len(wb), n, min_len)
    cap = n if capacity is None else capacity
    k = min(z, cap)
    got = [p[name].host(np.uint32 if name != "lit" else np.uint8) for name in ("begin", "len", "psrc", "lit")]
    for g in got:
        assert (g[k:] == (NONE if g.dtype == np.uint32 else 0xFF)).all(), ("written past the phrases", n, min_len, cap)
    if k == z:
        check_phrases(text, rep if ref is None else ref, min_len, *[g[:z] for g in got], what="guarded")
    else:
        assert got[0][:k].tolist() == wb[:k] and got[1][:k].tolist() == wl[:k], (n, min_len, cap)
    _buffers.check_all(p)
    if k == z and n:
        rc, d = raw_decode(eng, device, got[1][:z], got[2][:z], got[3][:z], n, offs, out_offs[3], fill, stream=stream)
        assert rc == OK, (rc, n, min_len)
        assert d["out"].host().tobytes() == text, (n, min_len, offs)
        _buffers.check_all(d)
    return z


def earlier(eng, orc, text):
    """The engine's EARLIER arrays of a small text, held against the definition first (src is the engine's choice)."""
    sa, lcp = table_of(orc, text)
    rep, src = _repeats.repeat_lens(eng, sa, lcp, "earlier")
    assert np.array_equal(rep, lpf(text))
    return np.array(rep, dtype=np.uint32), np.array(src, dtype=np.uint32)


# ---- 2. edges --------------------------------------------------------------------------------------------------------
def edge_texts():
    out = [b"a", b"\x00", b"\xff", b"ab", b"aa", b"\x00\xff", b"\x00\x00\xff\xff\x00\x00\xff\xff", b"\xff" * 9]
    out += [_gen.english_like(300).tobytes(), _buffers.repeat_rich(3)[1][:500], _gen.fibonacci_string(12)[:233]]
    return out


def edges(eng, device, orc):
    # n = 0 on every route: z = 0, nothing read or written
    for route in ROUTES:
        b, l, s, c = parse(eng, device, route, b"", *table_of(orc, b""), 1)
        assert len(l) == 0 and decode(eng, device, route, l, s, c, 0) == b""
    count = ctypes.c_uint64(7)
    assert eng.lib.sfx_lz_parse_dev(None, None, None, 0, 1, None, None, None, None, 0, ctypes.byref(count), None, 0, None) == OK
    assert count.value == 0 and eng.lib.sfx_lz_decode_dev(None, None, None, 0, 0, None, None, 0, None) == OK
    for i, t in enumerate(edge_texts()):
        check_all_routes(eng, device, orc, t, (1, 2, 8))
        rep, src = earlier(eng, orc, t)
        to, uo, fill = _buffers.combos()[i % 6]
        z = guarded_round_trip(eng, device, t, rep, src, 1 + i % 3, offs=(uo, U32(uo), to), out_offs=(uo, U32(uo), 4, to), fill=fill)
        for cap in {0, z - 1, z}:                                   # capacity 0, z - 1, z: nothing written past it
            if cap >= 0:
                guarded_round_trip(eng, device, t, rep, src, 1 + i % 3, capacity=cap, fill=_buffers.FILLS[(i + 1) % 3])
        # no text: no lit; no begin wanted: none written
        rc, z2, p = raw_parse(eng, device, rep, src, None, 1, want_begin=False)
        assert rc == OK and z2 == len(reference(rep, 1)[0])
        assert (p["lit"].host() == 0xFF).all() and (p["begin"].host() == 0xFF).all()
        _buffers.check_all(p)
    if str(device).startswith("cuda"):                              # a side stream
        t = _gen.english_like(5000).tobytes()
        rep, src = earlier(eng, orc, t)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            guarded_round_trip(eng, device, t, rep, src, 2, stream=ctypes.c_void_p(side.cuda_stream))
        side.synchronize()


def U32(o):
    return _buffers.U32_OFFSETS[(_buffers.U32_OFFSETS.index(o) + 1) % 3]


# ---- 3. refusals -----------------------------------------------------------------------------------------------------
def refusals(eng, device, orc):
    t = _gen.english_like(400).tobytes()
    n = len(t)
    rep, src = earlier(eng, orc, t)
    lib = eng.lib
    assert raw_parse(eng, device, rep, src, t, 0)[0] == ERR_ARG                                   # min_len 0
    assert raw_parse(eng, device, rep, src, t, 1, capacity=0, n=1 << 32)[0] == ERR_TOO_LARGE
    need = int(lib.sfx_lz_parse_workspace_bytes(n))
    assert 0 < need <= 9 * n + (64 << 10)
    assert raw_parse(eng, device, rep, src, t, 1, ws_bytes=need - 1)[0] == ERR_WORKSPACE
    rc, _, p = raw_parse(eng, device, rep, src, t, 1, ws_bytes=need + 16, ws_off=4)               # off SFX_WORKSPACE_ALIGN
    assert rc == ERR_ARG and (p["len"].host() == 0xFF).all()
    assert raw_parse(eng, device, rep, src, t, 1, offs=(2, 8, 1))[0] == ERR_ARG                    # a u32 array off 4 bytes
    assert raw_parse(eng, device, rep, src, t, 1, out_offs=(4, 6, 12, 3))[0] == ERR_ARG
    count = ctypes.c_uint64(0)
    b = _buffers.inp(rep, device, 4)
    assert lib.sfx_lz_parse_dev(b.ptr, b.ptr, None, n, 1, None, None, None, None, n, ctypes.byref(count), None, 0, None) == ERR_ARG
    assert lib.sfx_lz_parse_dev(b.ptr, b.ptr, None, n, 1, None, None, None, None, 0, None, None, 0, None) == ERR_ARG
    assert lib.sfx_lz77_u32(None, n, None, None, 0, None, None, None, None, 0, ctypes.byref(count)) == ERR_ARG
    assert lib.sfx_lz77_u32(None, 1 << 32, None, None, 1, None, None, None, None, 0, ctypes.byref(count)) == ERR_TOO_LARGE
    assert lib.sfx_lz77_u32(None, 0, None, None, 1, None, None, None, None, 0, ctypes.byref(count)) == OK and count.value == 0
    # decode
    f = SuffixTable(t, engine=eng).lz77(1)
    ln, sr, lt, z = f.len, f.src, f.lit, len(f)
    need = int(lib.sfx_lz_decode_workspace_bytes(n, z))
    assert 0 < need <= 5 * n + 8 * z + (64 << 10)
    assert raw_decode(eng, device, ln, sr, lt, n, ws_bytes=need - 1)[0] == ERR_WORKSPACE
    rc, d = raw_decode(eng, device, ln, sr, lt, n, ws_bytes=need + 16, ws_off=4)
    assert rc == ERR_ARG and (d["out"].host() == 0xFF).all()
    assert raw_decode(eng, device, ln, sr, lt, n, offs=(2, 8, 1))[0] == ERR_ARG
    assert lib.sfx_lz_decode_dev(None, None, None, 1, 1 << 32, None, None, 0, None) == ERR_TOO_LARGE
    assert lib.sfx_unlz(None, None, None, 1, 1 << 32, None) == ERR_TOO_LARGE
    assert lib.sfx_unlz(None, None, None, 0, 0, None) == OK
    # the output overlapping an input: the literal bytes' own buffer, and the tail of the lengths
    big = _buffers.guarded(max(n, 4 * z) + 16, device, 0, 0x00)
    ws = _buffers.guarded(need, device, 0, 0xFF)
    li, si, ci = _buffers.inp(ln, device, 4), _buffers.inp(sr, device, 4), _buffers.inp(lt, device, 1)
    st = _buffers.stream_of(device)
    assert lib.sfx_lz_decode_dev(li.ptr, si.ptr, ci.ptr, z, n, ci.ptr, ws.ptr, need, st) == ERR_ARG
    assert lib.sfx_lz_decode_dev(li.ptr, si.ptr, ci.ptr, z, n, ctypes.c_void_p(li.ptr.value + 4 * z - 1), ws.ptr, need, st) == ERR_ARG
    assert lib.sfx_lz_decode_dev(li.ptr, si.ptr, ci.ptr, z, n, big.ptr, ws.ptr, need, st) == OK
    assert big.host()[:n].tobytes() == t
    for x in (li, si, ci, ws, big):
        x.check_guards()
    try:
        suffix_amd.unlz([1, 1], [NONE, 1], b"a\x00", engine=eng)
        raise AssertionError("a forward copy was decoded")
    except SuffixHipError:
        pass
    try:
        SuffixTable(t, engine=eng).lz77(0)
        raise AssertionError("min_len 0 was accepted")
    except ValueError:
        pass


# ---- 4. unchecked input ----------------------------------------------------------------------------------------------
def unchecked_parse(eng, device, iters=50, seed=77):
    """Random arrays that are no LPF arrays: refused iff some rep[p] > n - p or a chain copy has src >= its begin;
    otherwise exactly the definition's phrases.  Guard bands intact either way."""
    rng = random.Random(seed)
    refused = accepted = nonmono = 0
    for i in range(iters):
        n = rng.randint(1, 400)
        text = bytes(rng.randrange(256) for _ in range(n))
        bad_rep, bad_src = i % 3 == 1, i % 3 == 2
        rep = np.array([rng.randint(0, min(n - p, 12)) if rng.random() < 0.7 else rng.randint(0, n - p) for p in range(n)], dtype=np.uint32)
        src = np.array([rng.randrange(p) if p else NONE for p in range(n)], dtype=np.uint32)
        rep[0] = 0
        m = rng.choice((1, 2, 3, 8))
        if bad_rep:
            for p in rng.sample(range(n), min(n, 3)):
                rep[p] = n - p + rng.choice((1, 2, 1 << 31, NONE - (n - p)))
        wb, wl, wc = reference(rep, m)
        if bad_src:
            for k in rng.sample(range(len(wb)), min(len(wb), 4)):
                src[wb[k]] = rng.choice((wb[k], wb[k] + 1, n, NONE))
        # positions off the chain may hold anything
        on = set(wb)
        for p in range(n):
            if p not in on and rng.random() < 0.3:
                src[p] = rng.choice((p, n + 5, NONE))
        want_bad = bool((rep.astype(np.int64) > n - np.arange(n)).any()) or any(c and int(src[b]) >= b for b, c in zip(wb, wc))
        rc, z, p = raw_parse(eng, device, rep, src, text, m, fill=_buffers.FILLS[i % 3])
        assert rc == (ERR_ARG if want_bad else OK), (i, rc, want_bad, n, m)
        _buffers.check_all(p)
        if want_bad:
            refused += 1
            continue
        accepted += 1
        nonmono += bool((np.diff(next_of(rep, m)) < 0).any())
        assert z == len(wb)
        assert p["begin"].host(np.uint32)[:z].tolist() == wb and p["len"].host(np.uint32)[:z].tolist() == wl
        ps, lt = p["psrc"].host(np.uint32)[:z], p["lit"].host()[:z]
        for k, (b, c) in enumerate(zip(wb, wc)):
            assert (int(ps[k]), int(lt[k])) == ((int(src[b]), 0) if c else (NONE, text[b])), (i, k)
    assert refused >= iters // 3 and accepted >= iters // 4 and nonmono >= 5, (refused, accepted, nonmono)


def unchecked_decode(eng, device, iters=50, seed=78):
    """Phrase lists nobody parsed: valid ones (random lengths, any earlier source) decode like the serial loop; a zero
    length, a forward or self source, a wrong sum or a literal of 2 bytes is refused with the output untouched."""
    rng = random.Random(seed)
    for i in range(iters):
        z = rng.randint(1, 120)
        ln, sr, lt, b = [], [], [], 0
        for k in range(z):
            if b == 0 or rng.random() < 0.3:
                ln.append(1), sr.append(NONE), lt.append(rng.randrange(256))
            else:
                ln.append(rng.randint(1, min(3 * b, 300) if rng.random() < 0.2 else 9)), sr.append(rng.randrange(b)), lt.append(rng.randrange(256))
            b += ln[-1]
        n = b
        kind = i % 6
        k = rng.randrange(z)
        copies = [j for j in range(z) if sr[j] != NONE]
        begins = np.concatenate(([0], np.cumsum(ln)))[:-1].tolist()
        if kind == 1:
            ln[k] = 0
            n -= begins[k + 1] - begins[k] if k + 1 < z else n - begins[k]
        elif kind == 2 and copies:
            j = rng.choice(copies)
            sr[j] = begins[j] + rng.choice((0, 1, 1000))
        elif kind == 3:
            n += rng.choice((-1, 1, 7))
        elif kind == 4:
            lits = [j for j in range(z) if sr[j] == NONE]
            j = rng.choice(lits)
            ln[j] = 2
            n += 1
        elif kind == 5:
            sr[0] = 0                                              # the first phrase as a copy: no source is earlier
        bad = kind in (1, 3, 4, 5) or (kind == 2 and copies)
        if n <= 0:
            continue
        rc, d = raw_decode(eng, device, ln, sr, lt, n, fill=_buffers.FILLS[i % 3])
        _buffers.check_all(d)
        if bad:
            assert rc == ERR_ARG, (i, kind, rc)
            assert (d["out"].host() == 0xFF).all(), (i, kind, "the output of a refused list was written")
        else:
            assert rc == OK, (i, kind, rc)
            assert d["out"].host().tobytes() == serial_decode(ln, sr, lt), (i, z, n)


# ---- 5. collections --------------------------------------------------------------------------------------------------
def collection(eng, device, iters=12, seed=5):
    """The EARLIER arrays of a generalized table (truncated suffixes): no phrase crosses a document start, the phrases
    are the definition's over the brute force, decode restores the concatenation."""
    rng = random.Random(seed)
    for _ in range(iters):
        docs = [_repeats.random_text(rng, 14) for _ in range(5)]
        docs[rng.randrange(5)] = docs[rng.randrange(5)]             # one document twice: copies want to run across
        text = b"".join(docs)
        if not text:
            continue
        starts = _gsa.doc_starts(docs)
        g = suffix_amd.GeneralizedSuffixTable(docs, engine=eng)
        rep, src = g.repeat_lens("earlier", with_source=True)
        want = _repeats.brute_rep(text, "earlier", starts)
        assert np.array_equal(rep, want)
        for m in (1, 2, 3):
            z = guarded_round_trip(eng, device, text, rep, src, m, ref=want)
            wb, wl, _ = reference(want, m)
            inner = set(int(s) for s in starts[:len(docs)]) - {0}
            for b, l in zip(wb, wl):
                assert not any(b < s < b + l for s in inner), (docs, m, b, l)
            assert z == len(wb)


# ---- 6. launch names -------------------------------------------------------------------------------------------------
def launch_names(eng, device, orc):
    t = _gen.english_like(3000).tobytes()
    rep, src = earlier(eng, orc, t)
    names = _gsa.profile_names(eng, lambda: guarded_round_trip(eng, device, t, rep, src, 1))
    assert PARSE_KERNELS <= names and DECODE_KERNELS <= names, names
    assert not {x for x in names if x.startswith(("lz_", "unlz_"))} - PARSE_KERNELS - DECODE_KERNELS - {"lz_hop"}, names


# ---- 7. small tiles (a process with SFX_LZ_TILE / SFX_LZ_LEVELS set) ---------------------------------------------------
def small_tiles(eng, device, orc, tile=8, levels=2):
    group = tile << levels
    rng = random.Random(11)
    ab = lambda n, sigma=2: bytes(rng.choice(b"abcd"[:sigma]) for _ in range(n))
    texts = [ab(n, 2 + n % 2) for n in (tile - 1, tile, tile + 1, group - 1, group, group + 1, 3 * group + 1)]
    x = ab(2 * group + 9, 4)
    xx = x + x + ab(20, 4)
    texts += [xx, b"a" * (3 * group + 5), _gen.fibonacci_string(11)[:144], b"ab" * 40 + b"c"]
    for t in texts:
        check_all_routes(eng, device, orc, t, (1, 3))
        rep, src = earlier(eng, orc, t)
        for m in (1, 3, 8):
            guarded_round_trip(eng, device, t, rep, src, m, fill="count")
    wb, wl, _ = reference(lpf(xx), 1)
    assert any((b + l) // group >= b // group + 2 and b + l < len(xx) for b, l in zip(wb, wl))      # one phrase skips a whole group
    assert reference(lpf(b"a" * (3 * group + 5)), 1)[1] == [1, 3 * group + 4]      # decode depth n - 1
    # next() that is not monotone at min_len = 3
    seen = 0
    for t in random_texts(40, seed=3, max_len=150):
        rep = lpf(t)
        if len(t) > 1 and (np.diff(next_of(rep, 3)) < 0).any():
            seen += 1
            check_all_routes(eng, device, orc, t, (3,), rep)
    assert seen >= 5, seen
    unchecked_parse(eng, device, 30, seed=79)
    unchecked_decode(eng, device, 30, seed=80)
    collection(eng, device, 4, seed=6)


# ---- the serial checker ----------------------------------------------------------------------------------------------
def build_checker(out_dir):
    """tests/lz_check.c -> an executable."""
    exe = os.path.join(str(out_dir), "lz_check")
    subprocess.check_call(["cc", "-O2", "-std=c99", "-o", exe, os.path.join(HERE, "lz_check.c")])
    return exe


def run_checker(exe, out_dir, text, rep, min_len, ln, src, lit):
    """-> the checker's line ("ok z=... literals=... longest=..." or the first fault)."""
    paths = []
    for name, arr, dt in (("text", np.frombuffer(text, dtype=np.uint8) if isinstance(text, bytes) else text, np.uint8), ("rep", rep, np.uint32),
                          ("len", ln, np.uint32), ("src", src, np.uint32), ("lit", lit, np.uint8)):
        p = os.path.join(str(out_dir), "lz_" + name + ".bin")
        np.ascontiguousarray(arr, dtype=dt).tofile(p)
        paths.append(p)
    r = subprocess.run([exe, str(min_len), *paths], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip()


def checker_self_test(exe, out_dir):
    """The checker accepts the definition's parse of a small text and names a fault in each kind of damage."""
    t = b"abracadabra_abracadabra"
    rep = _repeats.brute_rep(t, "earlier")
    for m in (1, 3):
        wb, wl, wc = reference(rep, m)
        src = [bytes(t).find(t[b:b + l]) if c else NONE for b, l, c in zip(wb, wl, wc)]
        lit = [0 if c else t[b] for b, c in zip(wb, wc)]
        line = run_checker(exe, out_dir, t, rep, m, wl, src, lit)
        assert line == f"ok z={len(wb)} literals={wc.count(False)} longest={max(wl)}", line
        for damage in ("len", "src", "lit", "short"):
            l2, s2, c2 = list(wl), list(src), list(lit)
            k = wc.index(True)
            if damage == "len":
                l2[k] -= 1
            elif damage == "src":
                s2[k] = wb[k]
            elif damage == "lit":
                c2[0] ^= 1
            else:
                l2, s2, c2 = l2[:-1], s2[:-1], c2[:-1]
            assert run_checker(exe, out_dir, t, rep, m, l2, s2, c2).startswith("fault"), damage
