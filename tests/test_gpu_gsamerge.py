"""The GSA merge on the MI355X: the emulator's cases on libsuffix_hip.so, then collections of 2^20 + 5 bytes whose two
sides and whole are built by sdev.build_gsa -- the merged arrays must equal the one-shot build's in sa, da and lcp -- and
tests/gsa_check.c over one merged result."""
import random

import numpy as np
import pytest
import torch

import _gen
import _gsa
import _gsamerge as M
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


# ---- the emulator's cases ------------------------------------------------------------------------------------------------
def test_known_answer_through_every_entry_point(eng):
    M.known_answer(eng, "cuda")


def test_300_random_collections_at_every_split_vs_the_definition(eng):
    assert M.random_splits(eng, "cuda") >= 900


def test_ties_and_prefixes(eng):
    M.ties_and_prefixes(eng, "cuda")


def test_sizes_around_the_scatter_tile(eng):
    assert M.tile_sizes(eng, "cuda") == 25


def test_alternation_and_whole_tiles_of_one_side(eng):
    M.tile_patterns(eng, "cuda")


def test_three_extends_equal_one_build(eng):
    M.chaining(eng)


def test_match_limit_below_at_and_above_the_longest_match(eng):
    M.match_limits(eng, "cuda")


def test_refusals(eng):
    M.refusals(eng, "cuda")


def test_garbage_stays_inside_the_guard_bands(eng):
    M.garbage(eng, "cuda")


def test_offsets_dirty_workspace_streams_and_threads(eng):
    M.buffers_streams_threads(eng, "cuda")


def test_resources_come_back(eng):
    M.resources_come_back(eng, "cuda")


# ---- 2^20 + 5 bytes ------------------------------------------------------------------------------------------------------
def _cut(text, rng, lo, hi):
    """Document starts lo .. hi bytes apart, one in a hundred followed by an empty document (as test_gpu_doclist._cut)."""
    starts, p = [0], 0
    while True:
        p += rng.randint(lo, hi)
        if p >= len(text):
            break
        starts.append(p)
        if rng.random() < 0.01:
            starts.append(p)
    return np.array(starts, dtype=np.int64)


def _merge_vs_one_shot(eng, text, starts, k, limit=0, check=None):
    """Both sides and the whole by sdev.build_gsa; -> (merged or None, longest).  The profile of the merge names its three
    launches and none of the build's."""
    starts = np.asarray(starts, dtype=np.int64)
    n, na = len(text), int(starts[k]) if k < len(starts) else len(text)
    t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    ds = torch.from_numpy(starts).cuda()
    whole = sdev.build_gsa(t, ds, engine=eng)
    a = sdev.build_gsa(t[:na], ds[:k].contiguous(), engine=eng)
    b = sdev.build_gsa(t[na:], (ds[k:] - na).contiguous(), engine=eng)
    ws = sdev.gsa_merge_workspace(na, n - na, "cuda", eng)
    assert ws.numel() <= 12 * (n - na) + (34 << 10)
    out = {}

    def run():
        out["r"] = sdev.gsa_merge(t, ds, k, a[0], a[2], b[0], b[2], da_a=a[1], da_b=b[1], match_limit=limit, workspace=ws, engine=eng)
        torch.cuda.synchronize()
    names = _gsa.profile_names(eng, run)
    sa, da, lcp, longest = out["r"]
    assert names == (M.KERNELS if sa is not None else M.KERNELS - {"gmerge_scatter"}), sorted(names)      # (a refusal writes nothing)
    assert not any(x.startswith("gsa_") for x in names)
    if sa is None:
        return None, longest
    for name, got, exp in zip(M.NAMES, (sa, da, lcp), whole):
        assert torch.equal(got, exp), (name, k, torch.nonzero(got != exp)[:4].flatten().tolist())
    sa2, da2, lcp2, _ = sdev.gsa_merge(t, ds, k, a[0], a[2], b[0], b[2], engine=eng)          # the documents from doc_starts
    assert torch.equal(sa2, whole[0]) and torch.equal(da2, whole[1]) and torch.equal(lcp2, whole[2])
    if check is not None:
        exe, tmp = check
        line = _gsa.run_checker(exe, tmp, text, starts, *(x.cpu().numpy().view(np.uint32) for x in (sa, da, lcp)))
        assert line.startswith("ok"), line
    return (sa, da, lcp), longest


def test_english_documents_with_empty_ones(eng, tmp_path):
    text = _gen.english_like(N).tobytes()
    starts = _cut(text, random.Random(1), 5000, 15000)
    starts = np.sort(np.concatenate([starts, starts[[0, 3, 40]], [starts[-1]]]))       # empty documents: in front, inside, before the last one
    nd = len(starts)
    check = (_gsa.build_checker(tmp_path), tmp_path)
    assert starts[1] == 0 and starts[2] > 0
    for k in (nd * 9 // 10, nd // 2, 2, 1):                             # 90 / 10, 50 / 50, one document with bytes / the rest, an empty A
        merged, longest = _merge_vs_one_shot(eng, text, starts, k, check=check if k == nd // 2 else None)
        assert merged is not None and (0 < longest <= 15000 if k > 1 else longest == 0), (k, longest)


def test_dna_as_4097_short_documents(eng):
    merged, longest = _merge_vs_one_shot(eng, _gen.dna(N, seed=13).tobytes(), np.arange(0, N, 256, dtype=np.int64), 2048)
    assert merged is not None and 8 <= longest <= 256


def test_near_duplicates_with_the_last_64k_document_added(eng):
    starts = np.arange(0, N, 1 << 16, dtype=np.int64)
    merged, longest = _merge_vs_one_shot(eng, _gen.near_duplicates(N).tobytes(), starts, len(starts) - 1)
    assert merged is not None


def test_a_sixteenth_copy_of_a_64k_document(eng):
    doc = _gen.english_like(1 << 16, seed=5).tobytes()
    altered = bytearray(doc)
    altered[40000] ^= 1
    docs = [doc] * 9 + [bytes(altered)] + [doc] * 7
    text, starts = b"".join(docs), _gsa.doc_starts(docs)
    merged, longest = _merge_vs_one_shot(eng, text, starts, 16)
    assert merged is not None and longest == 65536
    merged, longest = _merge_vs_one_shot(eng, text, starts, 16, limit=1000)
    assert merged is None and longest == 1001
