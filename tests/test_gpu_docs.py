"""The document counts and the k-common substrings on the MI355X: the emulator's cases on libsuffix_hip.so, then
collections of 2^20 + 5 bytes (four levels of either min-tree, many scan tiles, an odd tail) built by sdev.build_gsa,
with df and dup_prefix held to the serial checker tests/dc_check.c and len / pos to a numpy reduction over the df the
checker accepted (tests/_docs.py: expected_common)."""
import random

import numpy as np
import pytest
import torch

import _docs as D
import _gen
import _gsa
from suffix_amd import device as sdev

pytestmark = pytest.mark.gpu
N = (1 << 20) + 5


@pytest.fixture(scope="module")
def eng():
    import suffix_amd
    e = suffix_amd.default_engine()
    e.require_device()                      # fail loudly: no CPU fallback
    assert e.path.endswith("libsuffix_hip.so")
    return e


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    return D.build_checker(tmp_path_factory.mktemp("dc_check"))


# ---- the emulator's cases ------------------------------------------------------------------------------------------------
def test_known_answers(eng):
    D.known_answers(eng, "cuda")


def test_the_tables_arrays_are_made_once(eng):
    D.arrays_are_made_once(eng)


@pytest.mark.parametrize("sigma", [2, 3])
def test_small_random_collections_vs_brute_force(eng, sigma):
    assert D.small_random(eng, "cuda", sigma) >= 150


def test_refusals(eng):
    D.refusals(eng, "cuda")


def test_corrupted_lcp_stays_in_bounds(eng):
    D.corrupted_lcp(eng, "cuda")


def test_dirty_workspace_offsets_and_streams(eng):
    D.dirty_workspace_and_streams(eng, "cuda")


def test_pattern_counts_agree_with_the_gindex_query(eng):
    assert D.cross_check_queries(eng, "cuda") >= 1000


def test_launch_names(eng):
    D.launch_names(eng, "cuda")


def test_workspace_bound(eng):
    D.size_bound(eng)


def test_synthetic_arrays_with_placed_prev_distances_and_high_values(eng, chk, tmp_path):
    D.synthetic(eng, "cuda", chk, tmp_path)


# ---- 2^20 + 5 bytes ------------------------------------------------------------------------------------------------------
def _cut(text, rng, lo, hi):
    """Document starts lo .. hi bytes apart, one in a hundred followed by an empty document (as test_gpu_gsa._cut)."""
    starts, p = [0], 0
    while True:
        p += rng.randint(lo, hi)
        if p >= len(text):
            break
        starts.append(p)
        if rng.random() < 0.01:
            starts.append(p)
    return np.array(starts, dtype=np.int64)


def _run(eng, chk, tmp_path, text, starts):
    """build_gsa -> doc_counts -> common_substrings on the device; the checker and the numpy reduction on the host.
    -> (sa, da, lcp, df, dup, len, pos) as uint32 arrays."""
    n, nd = len(text), len(starts)
    t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    ds = torch.from_numpy(np.asarray(starts, dtype=np.int64)).cuda()
    sa, da, lcp = sdev.build_gsa(t, ds, engine=eng)
    df, dup = sdev.doc_counts(da, lcp, nd, want_prefix=True, engine=eng)
    ln, pos = sdev.common_substrings(sa, lcp, df, ds, engine=eng)
    torch.cuda.synchronize()
    h = [x.cpu().numpy().view(np.uint32) for x in (sa, da, lcp, df, dup, ln, pos)]
    D.accept(chk, tmp_path, h[1], h[2], h[3], h[4])
    e_len, e_pos = D.expected_common(h[0], h[2], h[3], starts, n)
    assert np.array_equal(h[5], e_len), np.flatnonzero(h[5] != e_len)[:5]
    assert np.array_equal(h[6], e_pos), np.flatnonzero(h[6] != e_pos)[:5]
    assert (np.diff(h[5].astype(np.int64)) <= 0).all()
    for d in {0, 1, nd // 2, nd - 1}:                                    # the string stands where pos says, inside one document
        if h[5][d]:
            p, L = int(h[6][d]), int(h[5][d])
            k = int(np.searchsorted(np.asarray(starts), p, side="right")) - 1
            assert p + L <= (int(starts[k + 1]) if k + 1 < nd else n), (d, p, L)
    return h


def _common_to_all(docs, cap):
    """The longest substring of docs[0] present in every other document: bisection on the length with Python sets of
    k-mers.  cap: an upper bound that must not be attained."""
    def present(L):
        if L == 0:
            return True
        if any(len(d) < L for d in docs):
            return False
        alive = {docs[0][i:i + L] for i in range(len(docs[0]) - L + 1)}
        for d in docs[1:]:
            alive &= {d[i:i + L] for i in range(len(d) - L + 1)}
            if not alive:
                return False
        return True
    assert not present(cap)
    lo, hi = 0, cap                                                      # present(lo), not present(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if present(mid):
            lo = mid
        else:
            hi = mid
    return lo


def test_english_documents_with_empty_ones(eng, chk, tmp_path):
    text = _gen.english_like(N).tobytes()
    starts = _cut(text, random.Random(1), 5000, 15000)
    starts = np.sort(np.concatenate([starts, starts[[0, 3, 40]], [starts[-1]]]))       # empty documents: in front, inside, before the last one
    assert (np.diff(starts) == 0).sum() >= 4
    h = _run(eng, chk, tmp_path, text, starts)
    assert h[5][0] == np.diff(np.append(starts, N)).max()


def test_dna_as_two_documents(eng, chk, tmp_path):
    text = _gen.dna(N, seed=12).tobytes()
    starts = np.array([0, 1 << 19], dtype=np.int64)
    h = _run(eng, chk, tmp_path, text, starts)
    assert int(h[5][1]) == _common_to_all([text[:1 << 19], text[1 << 19:]], 32)


def test_dna_as_4096_short_documents(eng, chk, tmp_path):
    """The hot-address case: nearly every p(r) is one of a few hundred shallow boundaries."""
    text = _gen.dna(N, seed=13).tobytes()
    starts = np.arange(0, N, 256, dtype=np.int64)                         # 4096 documents of 256 bytes and one of 5
    h = _run(eng, chk, tmp_path, text, starts)
    docs = [text[int(a):int(b)] for a, b in zip(starts, np.append(starts[1:], N))]
    assert int(h[5][len(starts) - 1]) == _common_to_all(docs, 6)
    assert int(h[5][4095]) >= int(h[5][4096])


def test_near_duplicates_in_64k_documents(eng, chk, tmp_path):
    text = _gen.near_duplicates(N).tobytes()
    _run(eng, chk, tmp_path, text, np.arange(0, N, 1 << 16, dtype=np.int64))


def test_sixteen_copies_and_an_altered_one(eng, chk, tmp_path):
    doc = _gen.english_like(1 << 16, seed=5).tobytes()
    altered = bytearray(doc)
    altered[40000] ^= 1
    docs = [doc] * 9 + [bytes(altered)] + [doc] * 7
    h = _run(eng, chk, tmp_path, b"".join(docs), _gsa.doc_starts(docs))
    assert h[5][:16].tolist() == [1 << 16] * 16 and int(h[5][16]) == 40000       # the altered copy shares its first 40000 bytes


def test_fibonacci_string_cut_in_three(eng, chk, tmp_path):
    k = 2
    while len(_gen.fibonacci_string(k)) < N:
        k += 1
    text = bytes(_gen.fibonacci_string(k)[:N])
    _run(eng, chk, tmp_path, text, np.array([0, N // 3, 2 * N // 3 + 1], dtype=np.int64))


def test_two_runs_of_one_byte_closed_form(eng, chk, tmp_path):
    """a^m, a^m with m = 2^19: a chain of depth m.  Ranks alternate between the documents by length, PREV[r] = r - 2, the
    last minimum of lcp(r - 2, r] is at r for even r and at r - 1 for odd r: dup_prefix[x] = 2 (x // 2)."""
    m = 1 << 19
    h = _run(eng, chk, tmp_path, b"a" * (2 * m), np.array([0, m], dtype=np.int64))
    assert (h[3] == 2).all()
    assert np.array_equal(h[4], 2 * (np.arange(2 * m, dtype=np.uint32) // 2))
    assert h[5].tolist() == [m, m] and h[6].tolist() == [int(h[0][2 * m - 1])] * 2
