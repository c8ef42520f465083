"""Maximal exact matches of a query text on the MI355X (sfx_mems_dev, sfx_index_mems*, sfx_gindex_mems*): the emulator's
cases (tests/_mem.py) through the product library with the runs around the real tile of 2048 pairs, then 2^18 query bytes
against 2^22 indexed ones -- millions of pairs, more tiles than workgroups -- verified by the serial checker
tests/mem_check.c and the two pair-count identities, with the counts of the table below computed independently (hashed
k-grams on a CPU); a collection, a refusal at 3.6 * 10^9 pairs, and pair offsets beyond 2^32."""
import random

import numpy as np
import pytest
import torch

import _buffers
import _gen
import _gsa
import _mem as E
from suffix_amd import device as sdev

pytestmark = pytest.mark.gpu
N, QM, LIMIT = 1 << 22, 1 << 18, 1 << 28

# text, L -> P, Z = P_L - P_(L+1), the largest interval
EXPECTED = {
    ("english", 12): (14265403, 6441853, 11517),
    ("english", 20): (224112, 38359, 372),
    ("dna", 8): (16903257, 12580923, 99),
    ("dna", 12): (190752, 49834, 6),
    ("near_duplicates", 16): (496392, 95830, 790),
}


@pytest.fixture(scope="module")
def eng():
    import suffix_amd
    e = suffix_amd.default_engine()
    e.require_device()                      # fail loudly: no CPU fallback
    assert e.path.endswith("libsuffix_hip.so")
    return e


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return E.build_checker(tmp_path_factory.mktemp("mem_check"))


def test_known_answers(eng):
    E.known_answers(eng, "cuda")


def test_small_random_pairs_vs_brute_force(eng, checker):
    assert E.small_random_pairs(eng, "cuda", checker) >= 150


def test_small_random_collections_vs_brute_force(eng, checker):
    assert E.small_random_collections(eng, "cuda", checker) >= 60


def test_edges(eng, checker, oracle):
    E.edges(eng, "cuda", checker, oracle)


def test_runs_around_the_tile_size(eng):
    E.runs(eng, "cuda", E.TILE)


def test_buffers_and_streams(eng, checker, oracle):
    E.buffers_and_streams(eng, "cuda", checker, oracle)


def test_refusals_and_workspace_bound(eng, oracle):
    E.refusals(eng, "cuda", oracle)
    E.workspace_bound(eng)


def test_launch_names(eng, oracle):
    E.launch_names(eng, "cuda", oracle)


# ---- scale -----------------------------------------------------------------------------------------------------------
def _texts(kind):
    """-> (text bytes, query array) by the recipe of the matching-statistics scale test, random.Random(17) fresh per text."""
    rng = random.Random(17)
    if kind == "english":
        text, other, noise = _gen.english_like(N), _gen.english_like(QM, seed=99), _gen.uniform_bytes(QM, 256, 5)
    elif kind == "dna":
        text, other = _gen.dna(N), _gen.dna(QM, seed=99)
        noise = np.frombuffer(b"ACGT", dtype=np.uint8)[_gen.uniform_bytes(QM, 4, 5) % 4]
    else:
        text, other, noise = _gen.near_duplicates(N), _gen.near_duplicates(QM, seed=99), _gen.uniform_bytes(QM, 256, 5)
    text = text.tobytes()
    return text, E.mixture(text, other, noise, rng, QM)


_plain = {}


def _indexed(eng, oracle, kind):
    """The text on the device with its table (checked against the oracle once) and its index; kept for the module."""
    if kind not in _plain:
        text, q = _texts(kind)
        dt = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
        dsa = sdev.build_sa(dt, engine=eng)
        torch.cuda.synchronize()
        sa = E._host(dsa)
        assert np.array_equal(sa, oracle.sais(text))
        _plain[kind] = (text, q, sa, dt, dsa, sdev.DeviceIndex(dt, dsa, engine=eng))
    return _plain[kind]


def _lists(index, dq, L):
    out = []
    for unique in (False, True):
        got = index.mems(dq, L, unique=unique, max_pairs=LIMIT)
        torch.cuda.synchronize()
        out.append((E._host(got[0]), E._host(got[1]), E._host(got[2]), got[3]))
    return out


@pytest.mark.parametrize("kind,L", sorted(EXPECTED))
def test_scale_plain(eng, checker, oracle, kind, L):
    text, q, sa, dt, dsa, ix = _indexed(eng, oracle, kind)
    dq = torch.from_numpy(q).cuda()
    full, uniq = _lists(ix, dq, L)
    p, z, widest = E.verify(eng, "cuda", checker, text, sa, q, L, full, uniq, index=ix)
    assert 0 < uniq[0].size < z
    assert (p, z, widest) == EXPECTED[kind, L]
    if (kind, L) == ("english", 20):                                      # the undirected entry: identical bytes
        other = sdev.mems(dt, dsa, dq, L, max_pairs=LIMIT, engine=eng)
        torch.cuda.synchronize()
        assert other[3] == p and all(np.array_equal(E._host(other[k]), full[k]) for k in range(3))


def _keys(res):
    return (res[0].astype(np.uint64) << np.uint64(40)) | (res[1].astype(np.uint64) << np.uint64(16)) | res[2].astype(np.uint64)


def test_scale_collection(eng, checker, oracle, tmp_path):
    L = 12
    rng = random.Random(17)
    text = _gen.english_like(N).tobytes()
    starts = E.cut(text, rng, 5000, 15000)
    q = E.mixture(text, _gen.english_like(QM, seed=99), _gen.uniform_bytes(QM, 256, 5), rng, QM, starts)
    dt = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    ds = torch.from_numpy(starts).cuda()
    dsa, dda, dlcp = sdev.build_gsa(dt, ds, engine=eng)
    torch.cuda.synchronize()
    sa, da, lcp = (E._host(x) for x in (dsa, dda, dlcp))
    out = _gsa.run_checker(_gsa.build_checker(tmp_path), tmp_path, text, starts, sa, da, lcp)
    assert out.startswith("ok"), out
    gx = sdev.GeneralizedDeviceIndex(dt, ds, dsa, dda, engine=eng)
    dq = torch.from_numpy(q).cuda()
    full, uniq = _lists(gx, dq, L)
    p, z, _ = E.verify(eng, "cuda", checker, text, sa, q, L, full, uniq, starts=starts, da=da, index=gx)
    assert z > 10 ** 6 and int(full[2].max()) <= 15000
    # the plain table of the same text: matches there run across document ends
    psa = sdev.build_sa(dt, engine=eng)
    plain = sdev.mems(dt, psa, dq, L, max_pairs=LIMIT, engine=eng)
    torch.cuda.synchronize()
    a, b = _keys(full), _keys([E._host(x) for x in plain[:3]])
    differ = np.setdiff1d(a, b).size + np.setdiff1d(b, a).size
    print(f"collection: pairs {p}, Z {z}; the plain table's Z {b.size}; {differ} triples differ")
    assert differ >= 100
    torch.cuda.synchronize()
    gx.close()


def test_refusal_at_scale(eng, oracle):
    """english, L = 2: 3.6 * 10^9 pairs against a limit of 2^30: the count is reported, nothing is written."""
    text, q, sa, dt, dsa, ix = _indexed(eng, oracle, "english")
    dq = torch.from_numpy(q).cuda()
    wsb = int(eng.lib.sfx_mems_workspace_bytes(QM, 1 << 30))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    bufs = [_buffers.guarded(4 * 4096, "cuda", 4, 0xA5) for _ in range(3)]
    pairs, count = E._u64(0), E._u64(77)
    rc = eng.lib.sfx_index_mems_dev(ix._h, sdev._p(dq), QM, 2, 0, 1 << 30, *[b.ptr for b in bufs], 4096, E.ctypes.byref(pairs),
                                    E.ctypes.byref(count), sdev._p(ws), wsb, _buffers.stream_of("cuda"))
    assert (rc, pairs.value, count.value) == (E.OK, 3578551087, 0), (rc, pairs.value, count.value)
    for b in bufs:
        assert (b.host() == 0xA5).all()
        b.check_guards("refused")
    with pytest.raises(E.SuffixHipError, match="3578551087"):
        ix.mems(dq, 2, max_pairs=1 << 30, workspace=ws)


def test_pair_offsets_beyond_2_to_32(eng):
    """T = a^(2^17), Q = a^(2^15 + 1), L = 1: P = 2^32 + 2^17 pairs, Z = m + n - 1 matches in closed form."""
    n, m = 1 << 17, (1 << 15) + 1
    dt = torch.full((n,), 97, dtype=torch.uint8, device="cuda")
    dq = torch.full((m,), 97, dtype=torch.uint8, device="cuda")
    dsa = torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda")
    got = sdev.mems(dt, dsa, dq, 1, max_pairs=1 << 33, engine=eng)
    torch.cuda.synchronize()
    assert got[3] == (1 << 32) + (1 << 17) and got[0].numel() == m + n - 1 == 163840
    p = np.arange(n - 1, -1, -1, dtype=np.int64)
    i = np.arange(1, m, dtype=np.int64)
    want = (np.concatenate([np.zeros(n, dtype=np.int64), i]), np.concatenate([p, np.zeros(m - 1, dtype=np.int64)]),
            np.concatenate([np.minimum(m, n - p), np.minimum(m - i, n)]))
    for k in range(3):
        assert np.array_equal(E._host(got[k]).astype(np.int64), want[k]), k
    assert E.triples([E._host(x)[:5] for x in got[:3]]) == E.run_closed_form(n, m, 1)[:5]
