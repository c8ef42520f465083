"""The LCE index on the MI355X (sfx_inverse_table_*, sfx_lce_*): the emulator's cases (tests/_lce.py) through the product
library, a tree of five levels, then 2^22 + 5 indexed bytes of four kinds of text with 2^20 pairs each and 0, 1 and 5
mismatches -- every pair verified by the serial checker tests/lce_check.c, which reads the text only --, a Fibonacci
string and one repeated byte (closed form), a collection whose extensions must stop at document ends, 2^16 range minima
and the whole inverse table.  The tables are the oracle's; the collection's is the engine's generalized build once the
serial checker tests/gsa_check.c has accepted it against the text (and the LCE checker needs no table at all)."""
import random

import numpy as np
import pytest
import torch

import _gen
import _gsa
import _lce as L
from suffix_amd import device as sdev

pytestmark = pytest.mark.gpu
N, NQ = (1 << 22) + 5, 1 << 20
KS = (0, 1, 5)
NONE = L.NONE


@pytest.fixture(scope="module")
def eng():
    import suffix_amd
    e = suffix_amd.default_engine()
    e.require_device()                      # fail loudly: no CPU fallback
    assert e.path.endswith("libsuffix_hip.so")
    return e


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    return L.build_checker(tmp_path_factory.mktemp("lce_check"))


def test_known_answers(eng, oracle):
    L.known_answers(eng, "cuda", oracle)


def test_the_tables_handle_is_made_once(eng, oracle):
    L.handle_is_made_once(eng, oracle)


def test_small_random_texts_vs_brute(eng, oracle):
    assert L.small_random(eng, "cuda", oracle) >= 150


def test_small_random_collections_vs_brute(eng):
    assert L.small_collections(eng, "cuda") >= 60


def test_sizes_at_the_level_edges(eng):
    L.level_edges(eng, "cuda")


def test_five_levels_the_top_one_with_two_entries(eng):
    """n = 2^20 + 5 at the shipped fan of 32: 32769 / 1025 / 33 / 2 words above the array."""
    n = (1 << 20) + 5
    assert int(eng.lib.sfx_lce_bytes(n)) == 4 * (n + 27) + 4 * (32800 + 1056 + 64 + 32)
    L.level_edges(eng, "cuda", sizes=(n,))


def test_edge_texts(eng, oracle):
    L.edge_texts(eng, "cuda", oracle)


def test_refusals_and_size_bound(eng, oracle):
    L.refusals(eng, "cuda", oracle)
    L.size_bound(eng)


def test_corrupted_lcp_stays_in_bounds(eng, oracle):
    L.corrupted_lcp(eng, "cuda", oracle)


def test_streams_and_threads(eng, oracle):
    L.streams_and_threads(eng, "cuda", oracle)


def test_launch_names(eng, oracle):
    L.launch_names(eng, "cuda", oracle)


# ---- scale -----------------------------------------------------------------------------------------------------------
TEXTS = {
    "english": lambda: _gen.english_like(N),
    "dna": lambda: _gen.dna(N),
    "uniform": lambda: _gen.uniform_bytes(N, 256, 7),
    "near_duplicates": lambda: _gen.near_duplicates(N),
    "fibonacci": lambda: np.frombuffer(L.fibonacci(N), dtype=np.uint8),
    "run": lambda: np.full(N, 0x61, dtype=np.uint8),
}
_cache = {}


def _tables(oracle, kind):
    """(text bytes, sa, lcp) of one kind of text, the oracle's, computed once and left unchanged."""
    if kind not in _cache:
        text = np.ascontiguousarray(TEXTS[kind](), dtype=np.uint8).tobytes()
        assert len(text) == N
        sa = oracle.sais(text)
        _cache[kind] = (text, L._u32a(sa), L._u32a(oracle.lcp_kasai(text, sa)))
    return _cache[kind]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32).copy()).to("cuda")


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("kind", ["english", "dna", "uniform", "near_duplicates"])
def test_scale_every_pair_through_the_checker(eng, oracle, chk, kind):
    text, sa, lcp = _tables(oracle, kind)
    a, b = L.scale_pairs(N, sa, NQ, seed=len(kind))
    assert a.size == NQ
    ix = sdev.LceDeviceIndex(_dev(sa), _dev(lcp), engine=eng)
    assert ix.nbytes <= 4 * N + N // 7 + (64 << 10)
    da, db = _dev(a), _dev(b)
    longest = {}
    for k in KS:
        got = _host(ix.lce(da, db, mismatches=k))
        L.accept_pairs(chk, text, None, a, b, k, got)                   # all 2^20 pairs, nothing left out
        longest[k] = int(got[got != NONE].max())
    print(f"{kind}: longest extension by mismatches {longest}")
    ix.close()


@pytest.mark.parametrize("kind", ["fibonacci", "run"])
def test_scale_long_extensions(eng, oracle, chk, kind):
    """Extensions up to n long: 2^12 pairs through the checker; for the repeated byte all 2^20 against n - max(i, j)."""
    text, sa, lcp = _tables(oracle, kind)
    a, b = L.scale_pairs(N, sa, NQ, seed=3)
    ix = sdev.LceDeviceIndex(_dev(sa), _dev(lcp), engine=eng)
    da, db = _dev(a), _dev(b)
    pick = np.random.default_rng(4).choice(NQ, 1 << 12, replace=False)
    for k in KS:
        got = _host(ix.lce(da, db, mismatches=k))
        L.accept_pairs(chk, text, None, a[pick], b[pick], k, got[pick])
        if kind == "run":
            m = np.maximum(a, b).astype(np.int64)
            exp = np.where(m > N, NONE, N - m).astype(np.uint32)
            assert np.array_equal(got, exp), (k, np.flatnonzero(got != exp)[:4])
    ix.close()


def test_scale_collection_never_passes_a_document_end(eng, oracle, chk, tmp_path):
    """Documents of 5000 to 15000 bytes cut from the near-duplicates text: pairs inside one document, across two, and at
    last bytes of documents; every length checked against the document ends by the checker.  A plain index over the same
    bytes must answer differently somewhere."""
    text, psa, plcp = _tables(oracle, "near_duplicates")
    rng = random.Random(8)
    starts, p = [0], 0
    while True:
        p += rng.randint(5000, 15000)
        if p >= N:
            break
        starts.append(p)
        if rng.random() < 0.02:
            starts.append(p)                                             # an empty document
    starts = np.array(starts, dtype=np.int64)
    dt, ds = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to("cuda"), torch.from_numpy(starts).to("cuda")
    gsa, gda, glcp = sdev.build_gsa(dt, ds, engine=eng)
    # no oracle builds a table of this size for a collection: the engine's is accepted by the serial checker
    # tests/gsa_check.c (order, document array and in-document LCP against the text) before anything rests on it
    verdict = _gsa.run_checker(_gsa.build_checker(tmp_path), tmp_path, text, starts, *[_host(x) for x in (gsa, gda, glcp)])
    assert verdict.startswith("ok"), verdict
    ix = sdev.LceDeviceIndex(gsa, glcp, doc_starts=ds, engine=eng)
    plain = sdev.LceDeviceIndex(_dev(psa), _dev(plcp), engine=eng)
    nrng = np.random.default_rng(9)
    q = NQ // 4
    ends = np.concatenate((starts[1:], [N]))
    d = nrng.integers(0, starts.size, q)
    nonempty = ends > starts
    d = d[nonempty[d]]
    d = np.concatenate((d, d[:q - d.size]))
    one_a = starts[d] + (nrng.random(q) * (ends[d] - starts[d])).astype(np.int64)
    one_b = starts[d] + (nrng.random(q) * (ends[d] - starts[d])).astype(np.int64)
    last = ends[d] - 1                                                   # a document's last byte
    rn = nrng.integers(0, N - 1, NQ - 3 * q)    # neighbours in the PLAIN table share long stretches, many across a document end
    a = np.concatenate((one_a, nrng.integers(0, N, q), last, psa[rn].astype(np.int64)))
    b = np.concatenate((one_b, nrng.integers(0, N, q), nrng.integers(0, N, q), psa[rn + 1].astype(np.int64)))
    a, b = L._u32a(a), L._u32a(b)
    da, db = _dev(a), _dev(b)
    for k in KS:
        got = _host(ix.lce(da, db, mismatches=k))
        L.accept_pairs(chk, text, starts.astype(np.uint64), a, b, k, got)
        other = _host(plain.lce(da, db, mismatches=k))
        assert (other >= got).all()
        differ = int((other != got).sum())
        print(f"collection of {starts.size} documents, {k} mismatches: {differ} of {NQ} pairs stop at a document end")
        assert differ >= 1
    ix.close()
    plain.close()


def test_scale_range_minima_ranks_and_inverse_table(eng, oracle, chk):
    text, sa, lcp = _tables(oracle, "english")
    rng = np.random.default_rng(11)
    nr = 1 << 16
    lo = rng.integers(0, N, nr)
    ln = rng.integers(1, 1 << 16, nr)
    ln[:nr // 2] = rng.integers(1, 4096, nr // 2)                      # half shorter than 4096
    ln[nr // 2:nr // 2 + 256] = rng.integers(N // 2 + 1, N + 1, 256)    # 256 longer than n / 2
    lo[nr // 2:nr // 2 + 256] = rng.integers(0, N // 2 - 4, 256)
    hi = np.minimum(lo + ln, N + 1)                                     # (hi = n + 1 now and then: the empty mark)
    lo[-8:], hi[-8:] = [0, 0, N, N - 1, 5, 32, 31, 33], [N, N + 1, N, N, 5, 64, 65, 1 << 20]
    dsa, dlcp = _dev(sa), _dev(lcp)
    ix = sdev.LceDeviceIndex(dsa, dlcp, engine=eng)
    L.accept_min(chk, lcp, lo, hi, _host(ix.range_min(_dev(L._u32a(lo)), _dev(L._u32a(hi)))))
    pos = L._u32a(np.concatenate((rng.integers(0, N, nr - 4), [0, N - 1, N, N + 1])))
    isa = L.expected_isa(sa)
    want = np.where(pos < N, isa[np.minimum(pos, N - 1)], NONE).astype(np.uint32)
    assert np.array_equal(_host(ix.rank_of(_dev(pos))), want)
    ix.close()
    got = _host(sdev.inverse_table(dsa, engine=eng))
    L.accept_isa(chk, sa, got)
    assert np.array_equal(got, isa)
