"""The Burrows-Wheeler transform with sampled ranks and its inverse on the MI355X (sfx_bwt_dev, sfx_bwt_u32,
sfx_unbwt_dev, sfx_unbwt): the emulator's cases (tests/_bwt.py), then texts of 2^22 + 5 bytes -- 257 tiles of bwt_rank,
a partial last one, up to 65536 concurrent walks -- against the oracle's table and the definition."""
import numpy as np
import pytest
import torch

import _bwt as B
import _gen
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


def test_known_answers(eng, oracle):
    B.known_answers(eng, "cuda", oracle)


def test_small_random_texts_vs_definition(eng, oracle):
    assert B.small_random(eng, "cuda", oracle) >= 300


def test_edges(eng, oracle):
    B.edges(eng, "cuda", oracle)


def test_refusals(eng, oracle):
    B.refusals(eng, "cuda", oracle)


def test_integrity_of_mutated_pairs(eng, oracle):
    B.integrity(eng, "cuda", oracle)


def test_unchecked_tables_stay_in_bounds(eng, oracle):
    B.bad_tables(eng, "cuda", oracle)


def test_launch_names(eng, oracle):
    B.launch_names(eng, "cuda", oracle)


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


def _table(eng, oracle, t):
    dt = torch.from_numpy(t).cuda()
    dsa = sdev.build_sa(dt, engine=eng)
    torch.cuda.synchronize()
    sa = dsa.cpu().numpy().view(np.uint32)
    assert np.array_equal(sa, oracle.sais(t.tobytes()))                # the engine's table IS the oracle's, first
    return dt, dsa, sa


@pytest.mark.parametrize("kind", ["english", "dna", "bytes", "near_duplicates", "fibonacci", "one_byte"])
def test_scale(eng, oracle, kind):
    t = _text(kind, N)
    assert t.size == N
    dt, dsa, sa = _table(eng, oracle, t)
    ws = sdev.unbwt_workspace(N, "cuda", engine=eng)
    for s in (64, 256, 1 << 20):
        wb, wsm = B.definition(t.tobytes(), sa, s)
        b, sm = sdev.bwt(dt, dsa, s, engine=eng)
        torch.cuda.synchronize()
        assert np.array_equal(b.cpu().numpy(), wb), (kind, s)
        assert np.array_equal(sm.cpu().numpy().view(np.uint32), wsm), (kind, s)
        ws.fill_(0xFF)
        back = sdev.unbwt(b, sm, s, workspace=ws, engine=eng)
        assert torch.equal(back, dt), (kind, s)


def test_scale_one_chain(eng, oracle):
    """sample_step 0 is one serial chain: 2^18 steps."""
    n = 1 << 18
    t = _gen.english_like(n)
    dt, dsa, sa = _table(eng, oracle, t)
    wb, wsm = B.definition(t.tobytes(), sa, 0)
    b, sm = sdev.bwt(dt, dsa, 0, engine=eng)
    torch.cuda.synchronize()
    assert np.array_equal(b.cpu().numpy(), wb) and np.array_equal(sm.cpu().numpy().view(np.uint32), wsm)
    assert torch.equal(sdev.unbwt(b, sm, 0, engine=eng), dt)
