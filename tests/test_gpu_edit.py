"""k-error pattern search on the MI355X (sfx_edit_dev, sfx_index_edit*, sfx_gindex_edit*): the emulator's cases
(tests/_edit.py) through the product library with the closed forms around the real tile of 2048 candidates, then 2^10
patterns of 24 .. 64 bytes against 2^20 + 5 indexed bytes, half of them planted with insertions, deletions and
substitutions -- every quadruple verified by the serial checker tests/ed_check.c, a complete sweep of the text for 128 of
the patterns, the planted origins, and the counts C, H and Z of the table below, computed independently on a CPU
(_edit.scale_counts: the oracle's search over the oracle's table, every window by a full table, Sellers' recurrence over
the whole text); a collection, a refusal at more than 2^32 hits, and candidate offsets beyond 2^32."""
import random

import numpy as np
import pytest
import torch

import _buffers
import _edit as E
import _gen
import _gsa
import _mem
from suffix_amd import device as sdev

pytestmark = pytest.mark.gpu
N, NQ, LIMIT, HLIMIT = (1 << 20) + 5, 1 << 10, 1 << 28, 1 << 26

# text, k -> C, H, Z (E.scale_counts on a CPU)
EXPECTED = {
    ("english", 1): (778, 1049, 702),
    ("english", 3): (132767, 4988, 1723),
    ("dna", 1): (655, 1144, 771),
    ("dna", 3): (92515, 5601, 1934),
    ("near_duplicates", 1): (1799, 1045, 700),
    ("near_duplicates", 3): (137206, 4957, 1718),
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
    return E.build_checker(tmp_path_factory.mktemp("ed_check"))


def test_known_answers(eng):
    E.known_answers(eng, "cuda")


def test_small_random_texts_vs_brute_force(eng, checker):
    assert E.small_random_texts(eng, "cuda", checker) >= 150


def test_small_random_collections_vs_brute_force(eng, checker):
    assert E.small_random_collections(eng, "cuda", checker) >= 60


def test_edges(eng, checker, oracle):
    E.edges(eng, "cuda", checker, oracle)


def test_closed_forms_around_the_tile_size(eng):
    E.closed_forms(eng, "cuda", (2047, 2048, 2049, 4096 + 17, 1 << 16))


def test_buffers_and_streams(eng, checker, oracle):
    E.buffers_and_streams(eng, "cuda", checker, oracle)


def test_refusals_and_workspace_bound(eng, oracle):
    E.refusals(eng, "cuda", oracle)
    E.workspace_bound(eng)


def test_foreign_table_stays_in_bounds(eng):
    E.foreign_table(eng, "cuda")


def test_launch_names(eng, oracle):
    E.launch_names(eng, "cuda", oracle)


# ---- scale -----------------------------------------------------------------------------------------------------------
def scale_text(kind):
    gen = {"english": _gen.english_like, "dna": _gen.dna, "near_duplicates": _gen.near_duplicates}[kind]
    return gen(N).tobytes()


def scale_case(kind, k):
    """-> (text, patterns, origins): random.Random(26 + k) fresh per case."""
    text = scale_text(kind)
    pats, origins = E.scale_patterns(random.Random(26 + k), text, k, NQ)
    return text, pats, origins


_plain = {}


def _indexed(eng, oracle, kind):
    """The text on the device with its table (checked against the oracle once) and its index; kept for the module."""
    if kind not in _plain:
        text = scale_text(kind)
        dt = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
        dsa = sdev.build_sa(dt, engine=eng)
        torch.cuda.synchronize()
        sa = _mem._host(dsa)
        assert np.array_equal(sa, oracle.sais(text))
        _plain[kind] = (text, sa, dt, dsa, sdev.DeviceIndex(dt, dsa, engine=eng))
    return _plain[kind]


def _host(got):
    torch.cuda.synchronize()
    return E.host(got)


def _device_patterns(pats):
    qb, qoff = E.pack(pats)
    return torch.from_numpy(qb.copy()).cuda(), torch.from_numpy(qoff.astype(np.int64)).cuda()


SWEEP = [1 if j % 8 == 0 else 0 for j in range(NQ)]                          # 128 patterns, all of them planted ones


@pytest.mark.parametrize("kind,k", sorted(EXPECTED))
def test_scale_plain(eng, checker, oracle, kind, k):
    text, sa, dt, dsa, ix = _indexed(eng, oracle, kind)
    _, pats, origins = scale_case(kind, k)
    dq, doff = _device_patterns(pats)
    res = _host(ix.edit_search(dq, doff, k, max_candidates=LIMIT, max_hits=HLIMIT))
    assert sum(SWEEP) == 128 and len(origins) == NQ // 2 and sum(1 for o in origins if o[3] <= k) >= 100
    E.accept(checker, text, None, pats, k, res, SWEEP)
    assert E.check_origins(origins, res, k) >= 100
    print(f"edit: {kind} k {k}: C {res[5]}, H {res[6]}, Z {res[1].size}, tiles {-(-res[5] // E.TILE)}")
    assert (res[5], res[6], res[1].size) == EXPECTED[kind, k]
    if (kind, k) == ("english", 1):                                        # the undirected entry: identical bytes
        other = _host(sdev.edit_search(dt, dsa, dq, doff, k, max_candidates=LIMIT, max_hits=HLIMIT, engine=eng))
        assert other[5:] == res[5:] and all(np.array_equal(other[c], res[c]) for c in range(5))


def test_scale_collection(eng, checker, tmp_path):
    k = 3
    text = scale_text("english")
    starts = _mem.cut(text, random.Random(17), 5000, 15000)
    assert len(starts) >= 100
    _, pats, origins = scale_case("english", k)
    for i, s in enumerate(starts[1:65]):                                    # 64 more, laid across a document end
        pats[2 * i + 1] = text[int(s) - 20:int(s) + 20]
    dt = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    ds = torch.from_numpy(starts).cuda()
    dsa, dda, dlcp = sdev.build_gsa(dt, ds, engine=eng)
    torch.cuda.synchronize()
    sa, da, lcp = (_mem._host(x) for x in (dsa, dda, dlcp))
    out = _gsa.run_checker(_gsa.build_checker(tmp_path), tmp_path, text, starts, sa, da, lcp)
    assert out.startswith("ok"), out
    gx = sdev.GeneralizedDeviceIndex(dt, ds, dsa, dda, engine=eng)
    dq, doff = _device_patterns(pats)
    res = _host(gx.edit_search(dq, doff, k, max_candidates=LIMIT, max_hits=HLIMIT))
    sweep = [1 if j % 8 == 0 or (j % 2 == 1 and j < 128) else 0 for j in range(NQ)]
    E.accept(checker, text, starts, pats, k, res, sweep)                   # (no occurrence passes a document end: the checker's rule)
    _, hi = _mem._doc_bounds(len(text), starts)
    inside = [o for o in origins if o[2] <= hi[o[1]]]
    assert E.check_origins(inside, res, k) >= 100
    # the plain table of the same text: there the patterns laid across a document end are found whole
    psa = sdev.build_sa(dt, engine=eng)
    plain = _host(sdev.edit_search(dt, psa, dq, doff, k, max_candidates=LIMIT, max_hits=HLIMIT, engine=eng))
    across = 0
    for i, s in enumerate(starts[1:65]):
        j, e = 2 * i + 1, int(s) + 20
        here = res[3][int(res[0][j]):int(res[0][j + 1])].tolist()
        there = plain[3][int(plain[0][j]):int(plain[0][j + 1])].tolist()
        assert e in there and e not in here, (j, e)
        across += 1
    print(f"collection: C {res[5]}, H {res[6]}, Z {res[1].size}; the plain table's C {plain[5]}, H {plain[6]}, Z {plain[1].size}")
    assert across == 64 and plain[1].size > res[1].size
    torch.cuda.synchronize()
    gx.close()


def _run_of_a(n):
    return (torch.full((n,), 97, dtype=torch.uint8, device="cuda"), torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda"))


def test_refusal_beyond_2_to_32_hits(eng):
    """T = a^(2^22), 2^9 patterns a^32, k = 1: 2^10 pieces a^16 with 2^22 - 15 places each, C = 2^10 (2^22 - 15) just below
    2^32.  A candidate of piece 0 at q has L = 0 and the ends qe + 15, 16, 17 that the text still holds: 3 for the n - 32
    places q <= n - 33, then 2, 1 and 0.  One of piece 1 has L = max(0, 16 - q) and the ends qe, qe + 1 within what is left
    of k: 1 at q = 15, 2 for the n - 32 places 16 .. n - 17, 1 at q = n - 16 (qe = n).  5 (n - 31) hits per pattern, far
    above 2^32 in all: the count is reported, nothing is written."""
    n, nq = 1 << 22, 1 << 9
    per = lambda n: 5 * (n - 31)
    small = E.expected_counts(b"a" * 50, None, [b"a" * 32], 1, np.arange(49, -1, -1))
    assert small == (2 * 35, per(50), 20), small
    dt, dsa = _run_of_a(n)
    dq, doff = _device_patterns([b"a" * 32] * nq)
    C, H = 2 * nq * (n - 15), nq * per(n)
    assert C == 4294951936 and H == 10737338880 > (1 << 32)
    wsb = int(eng.lib.sfx_edit_workspace_bytes(nq, 1, 1 << 33, 1 << 20))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    bufs = [_buffers.guarded(4 * 4096, "cuda", 4, 0xA5) for _ in range(3)] + [_buffers.guarded(4096, "cuda", 1, 0xA5),
                                                                              _buffers.guarded(8 * (nq + 1), "cuda", 8, 0xA5)]
    cands, hits, count = E._u64(0), E._u64(0), E._u64(77)
    rc = eng.lib.sfx_edit_dev(sdev._p(dt), n, sdev._p(dsa), sdev._p(dq), sdev._p(doff), nq, 1, 1 << 33, 1 << 20, *[b.ptr for b in bufs[:4]], 4096,
                              bufs[4].ptr, E.ctypes.byref(cands), E.ctypes.byref(hits), E.ctypes.byref(count), sdev._p(ws), wsb,
                              _buffers.stream_of("cuda"))
    assert (rc, cands.value, hits.value, count.value) == (E.OK, C, H, 0), (rc, cands.value, hits.value, H, count.value)
    for b in bufs:
        assert (b.host() == 0xA5).all()
        b.check_guards("refused")


def test_candidate_offsets_beyond_2_to_32(eng):
    """T = a^N c^32 with N = 2^22, 2^11 patterns a^16 b^16 and then c^32, k = 1.  Piece 0 of every a^16 b^16 has N - 15
    places, none of which extends (b^16 against a's or c's is 15 edits away): 2^11 (N - 15) > 2^32 candidates without a
    hit.  The candidates of c^32 lie behind them: its occurrences are the ends n - 1 (c^31, one c short) and n."""
    N, nq = 1 << 22, (1 << 11) + 1
    n = N + 32
    dt = torch.cat([torch.full((N,), 97, dtype=torch.uint8), torch.full((32,), 99, dtype=torch.uint8)]).cuda()
    # the table: a^i c^32 sorts before a^(i-1) c^32, so the a-suffixes ascend by position; the c-suffixes shortest first
    dsa = torch.cat([torch.arange(0, N, dtype=torch.int64), torch.arange(n - 1, N - 1, -1, dtype=torch.int64)]).to(torch.int32).cuda()
    small = (b"a" * 40 + b"c" * 32)
    assert np.array_equal(E.naive_table(small), np.concatenate([np.arange(40), np.arange(71, 39, -1)]).astype(np.uint32))
    assert E.brute(small, None, [b"a" * 16 + b"b" * 16, b"c" * 32], 1) == ([(1, 40, 71, 1), (1, 40, 72, 0)], [0, 0, 2])
    dq, doff = _device_patterns([b"a" * 16 + b"b" * 16] * (nq - 1) + [b"c" * 32])
    got = _host(sdev.edit_search(dt, dsa, dq, doff, 1, max_candidates=1 << 34, max_hits=1 << 20, capacity=16, engine=eng))
    assert got[5] == (nq - 1) * (N - 15) + 2 * 17 > 1 << 32
    assert E.quads(got) == [(nq - 1, N, n - 1, 1), (nq - 1, N, n, 0)]
    assert got[0].tolist() == [0] * nq + [2]
