"""The FM-index over the Burrows-Wheeler pair on the MI355X (sfx_fm_create*, sfx_fm_count*, sfx_fm_lookup*): the
emulator's cases (tests/_fm.py), then texts of 2^20 + 5 bytes -- 257 blocks at occ_step 4096, 16385 at 64, a partial last
block -- against the oracle's table and intervals."""
import random

import numpy as np
import pytest
import torch

import _buffers
import _fm as F
import _gen
from suffix_amd import device as sdev

pytestmark = pytest.mark.gpu
N = (1 << 20) + 5
CONFIGS = ((32, 0), (256, 64), (64, 4096))                # (sample_step, occ_step)
LOCATE_MAX = 1 << 22                                      # positions one locate call may return here


@pytest.fixture(scope="module")
def eng():
    import suffix_amd
    e = suffix_amd.default_engine()
    e.require_device()                      # fail loudly: no CPU fallback
    assert e.path.endswith("libsuffix_hip.so")
    return e


def test_known_answers(eng, oracle):
    F.known_answers(eng, "cuda", oracle)


def test_small_random_texts_vs_oracle(eng, oracle):
    assert F.small_random(eng, "cuda", oracle, full=True) >= 300


def test_edges(eng, oracle):
    F.edges(eng, "cuda", oracle)


def test_refusals(eng, oracle):
    F.refusals(eng, "cuda", oracle)


def test_mutated_pairs_stay_in_bounds(eng, oracle):
    F.mutated_pairs(eng, "cuda", oracle)


def test_size_bounds(eng, oracle):
    F.sizes(eng, "cuda", oracle)


def test_launch_names(eng, oracle):
    F.launch_names(eng, "cuda", oracle)


# ---- scale -----------------------------------------------------------------------------------------------------------
def _text(kind, n):
    if kind == "english":
        return _gen.english_like(n)
    if kind == "dna":
        return _gen.dna(n)
    if kind == "bytes":
        return _gen.uniform_bytes(n, 256, 7)
    if kind == "near_duplicates":
        return _gen.near_duplicates(n, ndocs=2)
    if kind == "fibonacci":
        return np.frombuffer(_gen.fibonacci_string(32), dtype=np.uint8)[:n].copy()
    assert kind == "one_byte"
    return np.full(n, 0x61, dtype=np.uint8)


def _table(eng, oracle, t):
    dt = torch.from_numpy(t).cuda()
    dsa = sdev.build_sa(dt, engine=eng)
    torch.cuda.synchronize()
    sa = dsa.cpu().numpy().view(np.uint32)
    assert np.array_equal(sa, oracle.sais(t.tobytes()))                # the engine's table IS the oracle's, first
    return dt, dsa, sa


@pytest.mark.parametrize("kind", ["english", "dna", "bytes", "near_duplicates", "fibonacci", "one_byte"])
def test_scale(eng, oracle, kind):
    """2^16 patterns of 1-64 bytes and a few of 1000, drawn as for the small texts, against oracle.positions_batch;
    sa_range(0, n) against the whole table at sample_step 32; locate of 256 patterns against the table's slices (on a
    text where 256 intervals hold more than LOCATE_MAX positions -- one byte repeated -- as many patterns as fit)."""
    t = _text(kind, N)
    assert t.size == N
    text = t.tobytes()
    dt, dsa, sa = _table(eng, oracle, t)
    rng = random.Random(N + len(kind))
    # (drawn as for the small texts, the pattern one byte longer than the text included -- except on the one repeated
    # byte, where it is 2^20 dependent steps of one lane, three seconds per index; the small texts cover it there)
    qs = F.patterns_of(rng, text, 1 << 16, max_len=64, longer=kind != "one_byte") + [text[a:a + 1000] for a in (0, 12345, N - 1000, N // 2)]
    qb, qoff = _buffers.query_arrays(qs)
    ps, pe = oracle.positions_batch(text, sa, qb, qoff)
    cnt = pe.astype(np.int64) - ps
    assert (cnt > 0).sum() >= 0.4 * len(qs) and (cnt == 0).sum() >= 0.2 * len(qs)
    dq, doff = torch.from_numpy(qb.copy()).cuda(), torch.from_numpy(qoff.astype(np.int64)).cuda()
    # the patterns of the locate: the first 256 with at most 2^14 occurrences each, else the last few within LOCATE_MAX
    pick = np.flatnonzero(cnt <= (1 << 14))[:256]
    if pick.size < 256:
        pick = np.arange(len(qs) - 4, len(qs))
        pick = pick[np.cumsum(cnt[pick]) <= LOCATE_MAX]
        assert pick.size >= 2
    lb, loff = _buffers.query_arrays([qs[k] for k in pick])
    dlb, dloff = torch.from_numpy(lb.copy()).cuda(), torch.from_numpy(loff.astype(np.int64)).cuda()
    for s, occ in CONFIGS:
        b, sm = sdev.bwt(dt, dsa, s, engine=eng)
        ix = sdev.FmDeviceIndex(b, sm, s, occ, engine=eng)
        del b, sm                                                      # the handle owns its memory
        try:
            info = ix.info
            assert info["n"] == N and info["bytes"] <= int(eng.lib.sfx_fm_bytes(N, s, occ)), info
            if occ == 0:
                assert info["bytes"] <= N * (1 + 1 / 4 + 1 / 6 + 1 / 8) + 65536, info
            else:
                assert info["occ_step"] == occ and (N + occ - 1) // occ == {64: 16385, 4096: 257}[occ]
            gs, ge = ix.count(dq, doff)
            torch.cuda.synchronize()
            gs, ge = gs.cpu().numpy().view(np.uint32), ge.cpu().numpy().view(np.uint32)
            bad = np.flatnonzero((gs != ps) | (ge != pe))
            assert bad.size == 0, (kind, s, occ, bad[:4], [qs[k] for k in bad[:2]])
            if s == 32:
                assert np.array_equal(ix.sa_range(0, N).cpu().numpy().view(np.uint32), sa), (kind, s, occ)
            off, pos = ix.locate(dlb, dloff)
            off, pos = off.cpu().numpy(), pos.cpu().numpy().view(np.uint32)
            assert off.tolist() == np.concatenate([[0], np.cumsum(cnt[pick])]).tolist()
            for j, k in enumerate(pick):
                assert np.array_equal(pos[off[j]:off[j + 1]], sa[ps[k]:pe[k]]), (kind, s, occ, qs[k][:20])
        finally:
            torch.cuda.synchronize()
            ix.close()


def test_index_does_not_keep_the_pair(eng, oracle):
    """The handle owns its HBM: once the pair is deleted torch holds n + 4 n / s bytes less, with the index alive."""
    n = 1 << 24
    dt = torch.from_numpy(_gen.dna(n)).cuda()
    dsa = sdev.build_sa(dt, engine=eng)
    b, sm = sdev.bwt(dt, dsa, 64, engine=eng)
    torch.cuda.synchronize()
    ix = sdev.FmDeviceIndex(b, sm, 64, engine=eng)
    try:
        before = torch.cuda.memory_allocated()
        held = b.numel() + 4 * sm.numel()
        del b, sm
        after = torch.cuda.memory_allocated()
        print(f"allocated by torch: {before} with the pair, {after} without it; the pair is {held} bytes")
        assert before - after >= held, (before, after, held)
        qb = torch.from_numpy(np.frombuffer(b"ACGTACGT", dtype=np.uint8).copy()).cuda()
        s_, e_ = ix.count(qb, torch.tensor([0, 8], dtype=torch.int64, device="cuda"))
        want = oracle.positions(dt.cpu().numpy().tobytes(), dsa.cpu().numpy().view(np.uint32), b"ACGTACGT")
        assert (int(s_[0]) & 0xFFFFFFFF, int(e_[0]) & 0xFFFFFFFF) == want
    finally:
        torch.cuda.synchronize()
        ix.close()


def test_scale_one_chain(eng, oracle):
    """sample_step 0: every lookup walks back to the primary row, up to 2^18 steps; 64 ranks."""
    n = 1 << 18
    t = _gen.english_like(n)
    dt, dsa, sa = _table(eng, oracle, t)
    b, sm = sdev.bwt(dt, dsa, 0, engine=eng)
    ix = sdev.FmDeviceIndex(b, sm, 0, engine=eng)
    try:
        ranks = np.concatenate([[0, n - 1, int(np.flatnonzero(sa == 0)[0]), int(np.flatnonzero(sa == n - 1)[0])],
                                np.random.default_rng(3).integers(0, n, 60)]).astype(np.uint32)
        got = ix.lookup(torch.from_numpy(ranks.view(np.int32).copy()).cuda())
        assert np.array_equal(got.cpu().numpy().view(np.uint32), sa[ranks])
    finally:
        torch.cuda.synchronize()
        ix.close()
