"""k-mismatch pattern search on the MI355X (sfx_hamming_dev, sfx_index_hamming*, sfx_gindex_hamming*): the emulator's
cases (tests/_hamming.py) through the product library with the closed forms around the real tile of 2048 candidates, then
2^12 patterns against 2^22 + 5 indexed bytes -- more tiles than workgroups -- verified by the serial checker
tests/hm_check.c (every triple; full window counts for the 512 patterns planted from the text), the planted origins, the
rank order through the oracle's inverse table, and the counts of the table below, computed independently on a CPU
(_hamming.expected_counts: the oracle's search over the oracle's table, the windows compared in numpy); a collection, a
refusal at 3.4 * 10^10 candidates, and candidate offsets beyond 2^32."""
import random

import numpy as np
import pytest
import torch

import _buffers
import _gen
import _gsa
import _hamming as H
import _mem
from suffix_amd import device as sdev

pytestmark = pytest.mark.gpu
N, NQ, LIMIT = (1 << 22) + 5, 1 << 12, 1 << 28

# text, k -> C, Z, the largest piece interval (H.expected_counts on a CPU)
EXPECTED = {
    ("english", 1): (47207, 296, 12233),
    ("english", 3): (2589536, 1183, 24538),
    ("dna", 1): (2914, 390, 10),
    ("dna", 3): (5783286, 585, 4294),
    ("near_duplicates", 1): (16508, 289, 2908),
    ("near_duplicates", 3): (2827125, 479, 25195),
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
    return H.build_checker(tmp_path_factory.mktemp("hm_check"))


def test_known_answers(eng):
    H.known_answers(eng, "cuda")


def test_small_random_texts_vs_brute_force(eng, checker):
    assert H.small_random_texts(eng, "cuda", checker) >= 150


def test_small_random_collections_vs_brute_force(eng, checker):
    assert H.small_random_collections(eng, "cuda", checker) >= 60


def test_edges(eng, checker, oracle):
    H.edges(eng, "cuda", checker, oracle)


def test_closed_forms_around_the_tile_size(eng):
    H.closed_forms(eng, "cuda", (2047, 2048, 2049, 4096 + 17, 1 << 16))


def test_buffers_and_streams(eng, checker, oracle):
    H.buffers_and_streams(eng, "cuda", checker, oracle)


def test_refusals_and_workspace_bound(eng, oracle):
    H.refusals(eng, "cuda", oracle)
    H.workspace_bound(eng)


def test_foreign_table_stays_in_bounds(eng):
    H.foreign_table(eng, "cuda")


def test_launch_names(eng, oracle):
    H.launch_names(eng, "cuda", oracle)


# ---- scale -----------------------------------------------------------------------------------------------------------
def scale_text(kind):
    gen = {"english": _gen.english_like, "dna": _gen.dna, "near_duplicates": _gen.near_duplicates}[kind]
    return gen(N).tobytes()


def scale_case(kind, k, starts=None):
    """-> (text, patterns, origins): random.Random(17 + k) fresh per case."""
    text = scale_text(kind)
    pats, origins = H.scale_patterns(random.Random(17 + k), text, k, NQ, starts=starts)
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
    return (got[0].cpu().numpy().view(np.uint64), got[1].cpu().numpy().view(np.uint32), got[2].cpu().numpy().view(np.uint32),
            got[3].cpu().numpy(), got[4])


def _device_patterns(pats):
    qb, qoff = H.pack(pats)
    return torch.from_numpy(qb.copy()).cuda(), torch.from_numpy(qoff.astype(np.int64)).cuda()


@pytest.mark.parametrize("kind,k", sorted(EXPECTED))
def test_scale_plain(eng, checker, oracle, kind, k):
    text, sa, dt, dsa, ix = _indexed(eng, oracle, kind)
    _, pats, origins = scale_case(kind, k)
    dq, doff = _device_patterns(pats)
    res = _host(ix.hamming(dq, doff, k, max_candidates=LIMIT))
    complete = [1 if j % 8 == 0 else 0 for j in range(NQ)]                 # every pattern planted from the text: 512 full counts
    assert sum(complete) >= 256 and all(complete[j] for j, _, _ in origins) and len(origins) >= 100
    H.accept(checker, text, None, pats, k, res, complete)
    H.check_origins(origins, res)
    H.check_rank_order(text, sa, pats, k, res)
    widest = int(np.diff(H.piece_intervals(ix, pats, k)).max())
    print(f"hamming: {kind} k {k}: C {res[4]}, Z {res[1].size}, largest piece interval {widest}, tiles {-(-res[4] // H.TILE)}")
    assert (res[4], res[1].size, widest) == EXPECTED[kind, k]
    if (kind, k) == ("english", 1):                                        # the undirected entry: identical bytes
        other = _host(sdev.hamming(dt, dsa, dq, doff, k, max_candidates=LIMIT, engine=eng))
        assert other[4] == res[4] and all(np.array_equal(other[c], res[c]) for c in range(4))


def test_scale_cases_have_more_tiles_than_workgroups():
    assert max(c for c, _, _ in EXPECTED.values()) > 2048 * H.TILE


def test_scale_collection(eng, checker, tmp_path):
    k = 3
    text = scale_text("english")
    starts = _mem.cut(text, random.Random(17), 5000, 15000)
    assert len(starts) >= 400
    _, pats, origins = scale_case("english", k, starts)
    dt = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    ds = torch.from_numpy(starts).cuda()
    dsa, dda, dlcp = sdev.build_gsa(dt, ds, engine=eng)
    torch.cuda.synchronize()
    sa, da, lcp = (_mem._host(x) for x in (dsa, dda, dlcp))
    out = _gsa.run_checker(_gsa.build_checker(tmp_path), tmp_path, text, starts, sa, da, lcp)
    assert out.startswith("ok"), out
    gx = sdev.GeneralizedDeviceIndex(dt, ds, dsa, dda, engine=eng)
    dq, doff = _device_patterns(pats)
    res = _host(gx.hamming(dq, doff, k, max_candidates=LIMIT))
    complete = [1 if j % 8 == 0 else 0 for j in range(NQ)]
    H.accept(checker, text, starts, pats, k, res, complete)                # (no window passes a document end: the checker's rule)
    # the planted origins that lie inside one document are found; those laid across an end are not
    _, hi = _mem._doc_bounds(len(text), starts)
    inside = [(j, a, d) for j, a, d in origins if a + len(pats[j]) <= hi[a]]
    across = [(j, a, d) for j, a, d in origins if a + len(pats[j]) > hi[a]]
    assert len(inside) >= 100 and len(across) >= 10
    H.check_origins(inside, res)
    for j, a, _ in across:
        assert a not in res[2][int(res[0][j]):int(res[0][j + 1])].tolist(), (j, a)
    # the plain table of the same text: windows there run across document ends
    psa = sdev.build_sa(dt, engine=eng)
    plain = _host(sdev.hamming(dt, psa, dq, doff, k, max_candidates=LIMIT, engine=eng))
    per_g, per_p = np.diff(res[0].astype(np.int64)), np.diff(plain[0].astype(np.int64))
    print(f"collection: C {res[4]}, Z {res[1].size}; the plain table's C {plain[4]}, Z {plain[1].size}; "
          f"{int((per_g != per_p).sum())} patterns differ")
    assert (per_p >= per_g).all() and int((per_g != per_p).sum()) >= 10
    torch.cuda.synchronize()
    gx.close()


def _run_of_a(n):
    return (torch.full((n,), 97, dtype=torch.uint8, device="cuda"), torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda"))


def test_refusal_at_scale(eng):
    """T = a^(2^22), 2^12 patterns a^32, k = 1: 2^13 pieces with 2^22 - 15 hits each against a limit of 2^28: the count is
    reported, nothing is written."""
    n, nq = 1 << 22, 1 << 12
    dt, dsa = _run_of_a(n)
    dq, doff = _device_patterns([b"a" * 32] * nq)
    C = 2 * nq * (n - 15)
    assert C == 34359615488
    wsb = int(eng.lib.sfx_hamming_workspace_bytes(nq, 1, LIMIT))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    bufs = [_buffers.guarded(4 * 4096, "cuda", 4, 0xA5), _buffers.guarded(4 * 4096, "cuda", 4, 0xA5), _buffers.guarded(4096, "cuda", 1, 0xA5),
            _buffers.guarded(8 * (nq + 1), "cuda", 8, 0xA5)]
    cands, count = H._u64(0), H._u64(77)
    rc = eng.lib.sfx_hamming_dev(sdev._p(dt), n, sdev._p(dsa), sdev._p(dq), sdev._p(doff), nq, 1, LIMIT, *[b.ptr for b in bufs[:3]], 4096,
                                 bufs[3].ptr, H.ctypes.byref(cands), H.ctypes.byref(count), sdev._p(ws), wsb, _buffers.stream_of("cuda"))
    assert (rc, cands.value, count.value) == (H.OK, C, 0), (rc, cands.value, count.value)
    for b in bufs:
        assert (b.host() == 0xA5).all()
        b.check_guards("refused")
    with pytest.raises(H.SuffixHipError, match=str(C)):
        sdev.hamming(dt, dsa, dq, doff, 1, max_candidates=LIMIT, workspace=ws, engine=eng)


def test_candidate_offsets_beyond_2_to_32(eng):
    """T = a^(2^22), 2^11 patterns a^32, k = 0, room for 2^16 triples: C = Z = 2^11 (2^22 - 31) > 2^32, first[j] =
    j (2^22 - 31), and the written triples in closed form (the table of a^n holds the shortest suffix first)."""
    n, nq, cap = 1 << 22, 1 << 11, 1 << 16
    dt, dsa = _run_of_a(n)
    dq, doff = _device_patterns([b"a" * 32] * nq)
    per = n - 31
    got = _host(sdev.hamming(dt, dsa, dq, doff, 0, max_candidates=1 << 34, capacity=cap, engine=eng))
    assert got[4] == nq * per > 1 << 32
    assert np.array_equal(got[0], np.arange(nq + 1, dtype=np.uint64) * np.uint64(per))           # (first[nq] = Z, beyond the room)
    assert got[1].size == cap and not got[1].any() and not got[3].any()
    assert np.array_equal(got[2].astype(np.int64), n - 32 - np.arange(cap, dtype=np.int64))
