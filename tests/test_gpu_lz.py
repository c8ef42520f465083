"""The LZ77 factorization and its decoder on the MI355X (sfx_lz_parse_dev, sfx_lz_decode_dev, sfx_lz77_u32, sfx_unlz): the
emulator's cases (tests/_lz.py) through the product library, then texts of 2^22 + 5 bytes -- four groups of 2^20
positions and a ragged tile -- whose longest-previous-factor array tests/rep_check.c has accepted, checked phrase by
phrase by tests/lz_check.c and decoded back on the device."""
import ctypes
import random
import re

import numpy as np
import pytest
import torch

import _gen
import _lz as Z
import _repeats as R
from suffix_amd import device as sdev

pytestmark = pytest.mark.gpu
N = (1 << 22) + 5


@pytest.fixture(scope="module")
def eng():
    import suffix_amd
    e = suffix_amd.default_engine()
    e.require_device()                      # fail loudly: no CPU fallback
    assert e.path.endswith("libsuffix_hip.so")
    return e


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    d = tmp_path_factory.mktemp("lz_check")
    return R.build_checker(d), Z.build_checker(d)


def test_known_answers(eng, oracle):
    Z.known_answers(eng, "cuda", oracle)


def test_small_random_texts_every_route(eng, oracle):
    assert Z.small_random(eng, "cuda", oracle, iters=100) >= 100


def test_edges_guard_bands_side_stream_capacity(eng, oracle):
    Z.edges(eng, "cuda", oracle)


def test_refusals(eng, oracle):
    Z.refusals(eng, "cuda", oracle)


def test_unchecked_input_stays_in_bounds(eng):
    Z.unchecked_parse(eng, "cuda")
    Z.unchecked_decode(eng, "cuda")


def test_small_collections(eng):
    Z.collection(eng, "cuda")


def test_launch_names(eng, oracle):
    Z.launch_names(eng, "cuda", oracle)


# ---- scale -----------------------------------------------------------------------------------------------------------
def _text(kind, n):
    if kind == "english":
        return _gen.english_like(n)
    if kind == "dna":
        return _gen.dna(n)
    if kind == "bytes":
        return _gen.uniform_bytes(n, 256, 7)
    if kind == "near_duplicates":
        return _gen.near_duplicates(n, ndocs=2)                       # 1 MiB documents: every one comes round twice
    if kind == "fibonacci":
        return np.frombuffer(_gen.fibonacci_string(32), dtype=np.uint8)[:n].copy()
    assert kind == "one_byte"
    return np.full(n, 0x61, dtype=np.uint8)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _earlier(eng, oracle, checkers, tmp_path, t):
    """The oracle's table and LCP, the engine's EARLIER arrays over them, accepted by rep_check before anything uses
    them as the reference.  -> (text tensor, rep tensor, src tensor, rep on the host)"""
    text = t.tobytes()
    sa, lcp = Z.table_of(oracle, text)
    dsa, dlcp = torch.from_numpy(sa.view(np.int32)).cuda(), torch.from_numpy(lcp.view(np.int32)).cuda()
    rep, src = sdev.repeat_lens(dsa, dlcp, scope="earlier", want_src=True, engine=eng)
    rep_h = _u32(rep)
    res = R.run_checker(checkers[0], tmp_path, text, [], sa, lcp, None, "earlier", rep_h, _u32(src))
    assert res.startswith("ok"), res
    return torch.from_numpy(t).cuda(), rep, src, rep_h


def _parse_and_check(eng, checkers, tmp_path, t, dt, rep, src, rep_h, m, ws=None):
    b, l, s, c = sdev.lz_parse(rep, src, dt, min_len=m, workspace=ws, engine=eng)
    res = Z.run_checker(checkers[1], tmp_path, t, rep_h, m, _u32(l), _u32(s), c.cpu().numpy())
    assert res.startswith("ok"), (m, res)
    z, literals, longest = (int(x) for x in re.match(r"ok z=(\d+) literals=(\d+) longest=(\d+)", res).groups())
    assert z == l.numel() == b.numel()                                       # the checker's own count
    assert torch.equal(b.to(torch.int64) & 0xFFFFFFFF, torch.cumsum(l.to(torch.int64) & 0xFFFFFFFF, 0) - (l.to(torch.int64) & 0xFFFFFFFF))
    back = sdev.lz_decode(l, s, c, n=t.size, engine=eng)
    assert torch.equal(back, dt), m
    return z, literals, longest


@pytest.mark.parametrize("kind", ["english", "dna", "bytes", "near_duplicates", "fibonacci", "one_byte"])
def test_scale(eng, oracle, checkers, tmp_path, kind):
    t = _text(kind, N)
    assert t.size == N
    dt, rep, src, rep_h = _earlier(eng, oracle, checkers, tmp_path, t)
    ws = sdev.lz_parse_workspace(N, "cuda", engine=eng)
    assert ws.numel() <= 9 * N + (64 << 10)
    counts = {}
    for m in (1, 8):
        ws.fill_(0xFF)
        counts[m] = _parse_and_check(eng, checkers, tmp_path, t, dt, rep, src, rep_h, m, ws)
    print(kind, counts)
    assert counts[1][0] <= counts[8][0]
    if kind == "one_byte":
        assert counts[1] == (2, 1, N - 1) and counts[8] == (2, 1, N - 1)     # a literal and one copy of n - 1 bytes: depth n - 1
    if kind == "bytes":
        assert counts[8][0] >= N - 64                                        # (next to) all literals


def test_dense_exits_and_a_phrase_that_skips_groups(eng, oracle, checkers, tmp_path):
    """X + X of 2^21 bytes each: every position of the second half has next = n, so each of a tile's positions leaves it for
    good, and the chain takes one phrase of about 2^21 bytes across two groups."""
    x = _gen.english_like(1 << 21)
    t = np.concatenate([x, x])
    dt, rep, src, rep_h = _earlier(eng, oracle, checkers, tmp_path, t)
    z, literals, longest = _parse_and_check(eng, checkers, tmp_path, t, dt, rep, src, rep_h, 1)
    assert longest >= (1 << 21) - 64, longest


def test_all_literals(eng, oracle, checkers, tmp_path):
    """min_len 1000 on English-like text: (nearly) every phrase a literal, the emit path at its widest."""
    t = _gen.english_like(N)
    dt, rep, src, rep_h = _earlier(eng, oracle, checkers, tmp_path, t)
    z, literals, longest = _parse_and_check(eng, checkers, tmp_path, t, dt, rep, src, rep_h, 1000)
    assert z >= N - (N >> 6) and literals >= z - (z >> 10), (z, literals, longest)


def test_collection(eng, checkers, tmp_path):
    """2^22 bytes cut into documents: the EARLIER arrays of the generalized table, accepted by rep_check; no phrase
    crosses a document start and the decode is exact."""
    rng = random.Random(2)
    n = 1 << 22
    t = _gen.english_like(n, seed=80)
    text = t.tobytes()
    starts, p = [0], 0
    while True:
        p += rng.randint(5000, 15000)
        if p >= n:
            break
        starts.append(p)
    starts = np.array(starts, dtype=np.int64)
    dt = torch.from_numpy(t).cuda()
    sa, da, lcp = sdev.build_gsa(dt, torch.from_numpy(starts).cuda(), engine=eng)
    rep, src = sdev.repeat_lens(sa, lcp, scope="earlier", da=da, want_src=True, engine=eng)
    rep_h = _u32(rep)
    res = R.run_checker(checkers[0], tmp_path, text, starts, _u32(sa), _u32(lcp), _u32(da), "earlier", rep_h, _u32(src))
    assert res.startswith("ok"), res
    for m in (1, 8):
        b, l, s, c = sdev.lz_parse(rep, src, dt, min_len=m, engine=eng)
        res = Z.run_checker(checkers[1], tmp_path, t, rep_h, m, _u32(l), _u32(s), c.cpu().numpy())
        assert res.startswith("ok"), (m, res)
        bh, lh = _u32(b).astype(np.int64), _u32(l).astype(np.int64)
        k = np.searchsorted(bh, starts[1:], side="left")                      # every start is some phrase's begin
        assert np.array_equal(bh[k], starts[1:]), m
        assert torch.equal(sdev.lz_decode(l, s, c, engine=eng), dt), m


def test_capacity_below_z_at_scale(eng, oracle, checkers, tmp_path):
    t = _gen.dna(1 << 20)
    dt, rep, src, rep_h = _earlier(eng, oracle, checkers, tmp_path, t)
    wb, wl, _ = Z.reference(rep_h, 1)
    z = len(wb)
    for cap in (0, 1, z // 2, z - 1):
        Z.guarded_round_trip(eng, "cuda", t.tobytes(), rep_h, _u32(src), 1, capacity=cap)
