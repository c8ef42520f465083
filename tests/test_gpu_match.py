"""Matching statistics of a query text on the MI355X (sfx_match_stats_dev, sfx_index_match_stats*,
sfx_gindex_match_stats*): the emulator's cases (tests/_match.py), then 2^18 query positions against 2^22 indexed bytes --
the product's index with a full directory and key tree, every lane-divergence pattern -- verified by the serial checker
tests/ms_check.c and against the rebuild route to the same numbers: the generalized suffix array over {T, Q} and its
other-document repeat lengths."""
import random

import numpy as np
import pytest
import torch

import _gen
import _gsa
import _match as M
import _repeats
from suffix_amd import GeneralizedSuffixTable, SuffixTable
from suffix_amd import device as sdev

pytestmark = pytest.mark.gpu
N, QM, CAP = 1 << 22, 1 << 18, 50


@pytest.fixture(scope="module")
def eng():
    import suffix_amd
    e = suffix_amd.default_engine()
    e.require_device()                      # fail loudly: no CPU fallback
    assert e.path.endswith("libsuffix_hip.so")
    return e


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return M.build_checker(tmp_path_factory.mktemp("ms_check"))


def test_known_answer(eng, checker):
    M.known_answer(eng, "cuda", checker)


def test_small_random_pairs_vs_brute_force(eng, checker):
    assert M.small_random_pairs(eng, "cuda", checker) >= 150


def test_small_random_collections_vs_brute_force(eng, checker):
    assert M.small_random_collections(eng, "cuda", checker) >= 60


def test_edges(eng, checker, oracle):
    M.edges(eng, "cuda", checker, oracle)


def test_directory_texts(eng, checker, oracle):
    M.directory_texts(eng, "cuda", checker, oracle)


def test_buffers_and_streams(eng, checker, oracle):
    M.buffers_and_streams(eng, "cuda", checker, oracle)


def test_index_route_threshold_and_launch_names(eng, checker, oracle):
    M.index_route_threshold(eng, "cuda", checker, oracle)



# ---- scale -----------------------------------------------------------------------------------------------------------
def _mixture(text, other, noise, rng, starts=None):
    """QM bytes: half slices of the text with about every 200th byte changed (with `starts`: every fourth slice laid
    across a document end), a quarter unrelated text of the same kind, a quarter noise."""
    t = np.frombuffer(text, dtype=np.uint8)
    parts, piece = [], 4096
    for k in range(QM // 2 // piece):
        a = rng.randrange(len(text) - piece)
        if starts is not None and k % 4 == 0:
            a = max(0, int(starts[rng.randrange(1, len(starts))]) - rng.randint(1, piece - 1))
        parts.append(t[a:a + piece].copy())
    half = np.concatenate(parts)
    flip = np.flatnonzero(np.random.default_rng(rng.randrange(1 << 30)).random(half.size) < 1 / 200)
    half[flip] = other[flip % other.size]                              # (a byte of the same alphabet; may be the same one)
    q = np.concatenate([half, other[:QM // 4], noise[:QM // 4]])
    assert q.size == QM
    return q


def _routes(eng, checker, text, sa_host, q, index, dt, dsa, starts=None):
    """Uncapped and capped at CAP: the index route equals the undirected route, the checker accepts, the capped len is
    min(uncapped, CAP).  -> the uncapped len."""
    dq = torch.from_numpy(q).cuda()
    lens = {}
    for cap in (0, CAP):
        a = [M._host(x) for x in index.match_stats(dq, max_len=cap, want_src=True, want_interval=True)]
        if starts is None:
            b = [M._host(x) for x in sdev.match_stats(dt, dsa, dq, max_len=cap, want_src=True, want_interval=True, engine=eng)]
            assert M.same(a, b), cap
        only = M._host(index.match_stats(dq, max_len=cap))
        assert np.array_equal(only, a[0]), cap
        M.accept(checker, text, sa_host, q, cap, a, starts)
        lens[cap] = a[0]
    assert np.array_equal(lens[CAP], np.minimum(lens[0], CAP))
    assert int(lens[0].astype(np.int64).sum()) < 10 ** 8
    return lens[0]


def _rebuild_route(eng, text, q, starts):
    """The parent commit's route to the same numbers: the GSA over the documents of T plus Q as one more, then the
    other-document repeat lengths; the tail belongs to Q."""
    n = len(text)
    both = torch.from_numpy(np.concatenate([np.frombuffer(text, dtype=np.uint8), q])).cuda()
    ds = torch.from_numpy(np.concatenate([np.asarray(starts, dtype=np.int64), [n]])).cuda()
    sa, da, lcp = sdev.build_gsa(both, ds, engine=eng)
    rep = sdev.repeat_lens(sa, lcp, "other_doc", da=da, engine=eng)
    torch.cuda.synchronize()
    return M._host(rep)[n:]


@pytest.mark.parametrize("kind", ["english", "dna"])
def test_scale_plain(eng, checker, oracle, kind):
    rng = random.Random(17)
    if kind == "english":
        text = _gen.english_like(N).tobytes()
        other, noise = _gen.english_like(QM, seed=99), _gen.uniform_bytes(QM, 256, 5)
    else:
        text = _gen.dna(N).tobytes()
        other, noise = _gen.dna(QM, seed=99), _gen.uniform_bytes(QM, 4, 5)
        noise = np.frombuffer(b"ACGT", dtype=np.uint8)[noise % 4]
    q = _mixture(text, other, noise, rng)
    if kind == "dna":
        q[np.flatnonzero(np.random.default_rng(3).random(QM) < 1 / 300)] = ord("N")        # len = 0 entries
    dt = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    dsa = sdev.build_sa(dt, engine=eng)
    torch.cuda.synchronize()
    sa = M._host(dsa)
    assert np.array_equal(sa, oracle.sais(text))
    ix = sdev.DeviceIndex(dt, dsa, engine=eng)
    un = _routes(eng, checker, text, sa, q, ix, dt, dsa)
    torch.cuda.synchronize()
    ix.close()
    if kind == "dna":
        assert (un == 0).sum() >= 100
    assert np.array_equal(un, _rebuild_route(eng, text, q, [0]))
    st = SuffixTable.from_parts(text, sa, engine=eng)
    assert st.shared_spans(q, CAP) == _repeats.span_reference(un, CAP)


def test_scale_collection(eng, checker, tmp_path):
    from test_gpu_gsa import _cut
    rng = random.Random(23)
    text = _gen.english_like(N).tobytes()
    starts = _cut(text, rng, 5000, 15000)
    q = _mixture(text, _gen.english_like(QM, seed=99), _gen.uniform_bytes(QM, 256, 5), rng, starts)
    dt = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    ds = torch.from_numpy(starts).cuda()
    dsa, dda, dlcp = sdev.build_gsa(dt, ds, engine=eng)
    torch.cuda.synchronize()
    sa, da, lcp = (M._host(x) for x in (dsa, dda, dlcp))
    out = _gsa.run_checker(_gsa.build_checker(tmp_path), tmp_path, text, starts, sa, da, lcp)
    assert out.startswith("ok"), out
    gx = sdev.GeneralizedDeviceIndex(dt, ds, dsa, dda, engine=eng)
    un = _routes(eng, checker, text, sa, q, gx, dt, dsa, starts)
    torch.cuda.synchronize()
    gx.close()
    plain = M._host(sdev.match_stats(dt, sdev.build_sa(dt, engine=eng), torch.from_numpy(q).cuda(), engine=eng))
    assert (un <= plain).all() and (un < plain).sum() >= 100                # matches stop at the ends of documents
    assert np.array_equal(un, _rebuild_route(eng, text, q, starts))
    s = [int(x) for x in starts] + [N]
    g = GeneralizedSuffixTable([text[s[k]:s[k + 1]] for k in range(len(starts))], engine=eng, _arrays=(sa, da, lcp))
    assert g.shared_spans(q, CAP) == _repeats.span_reference(un, CAP)
