"""The document listing on the MI355X: the emulator's cases on libsuffix_hip.so, then collections of 2^20 + 5 bytes built
by sdev.build_gsa -- 2^12 sampled patterns of 1 - 12 bytes, 2^12 lcp-interval nodes and [0, n) per collection, both orders,
top_k 0 and 10, every occ_cut setting -- and a closed-form batch whose interval lengths sum past 2^32.  Expected values are
numpy's over the da array the build wrote (tests/_doclist.py)."""
import random

import numpy as np
import pytest
import torch

import _doclist as L
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


# ---- the emulator's cases ------------------------------------------------------------------------------------------------
def test_known_answers(eng):
    L.known_answers(eng, "cuda")


@pytest.mark.parametrize("sigma", [2, 3])
def test_small_random_collections_every_pattern_and_node(eng, sigma):
    assert L.small_random(eng, "cuda", sigma) >= 150


def test_synthetic_document_arrays(eng):
    assert L.synthetic(eng, "cuda") > 60


def test_the_profile_names_the_routes(eng):
    L.routes_are_named(eng, "cuda")


def test_list_sizes_agree_with_the_engines_document_counts(eng):
    assert L.cross_check_queries(eng, "cuda") >= 1000


def test_the_tables_handle_is_made_once(eng):
    L.the_handle_is_made_once(eng)


def test_refusals_and_limits(eng):
    L.refusals(eng, "cuda")


def test_size_formulas(eng):
    L.size_formulas(eng)


def test_dirty_workspace_offsets_streams_and_threads(eng):
    L.dirty_workspace_streams_and_threads(eng, "cuda")


def test_resources_come_back(eng):
    L.resources_come_back(eng, "cuda")


# ---- 2^20 + 5 bytes ------------------------------------------------------------------------------------------------------
def _cut(text, rng, lo, hi):
    """Document starts lo .. hi bytes apart, one in a hundred followed by an empty document (as test_gpu_docs._cut)."""
    starts, p = [0], 0
    while True:
        p += rng.randint(lo, hi)
        if p >= len(text):
            break
        starts.append(p)
        if rng.random() < 0.01:
            starts.append(p)
    return np.array(starts, dtype=np.int64)


def _expected(da, nd, s, e, order, top_k):
    """expected_batch for many intervals at once: one sort of (interval, document) pairs over the concatenated ranks."""
    lens = (e - s).astype(np.int64)
    j = np.repeat(np.arange(s.size, dtype=np.int64), lens)
    r = np.arange(lens.sum(), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens) + np.repeat(s.astype(np.int64), lens)
    key, tf = np.unique(j * nd + da[r].astype(np.int64), return_counts=True)
    jj, dd = key // nd, key % nd
    if order == L.BY_TF:
        idx = np.lexsort((dd, -tf, jj))
        jj, dd, tf = jj[idx], dd[idx], tf[idx]
    full = np.bincount(jj, minlength=s.size)
    ffirst = np.cumsum(full) - full
    place = np.arange(jj.size) - ffirst[jj]
    keep = place < top_k if top_k else np.ones(jj.size, dtype=bool)
    first = np.zeros(s.size + 1, dtype=np.uint64)
    first[1:] = np.cumsum(np.minimum(full, top_k) if top_k else full)
    return dd[keep].astype(np.uint32), tf[keep].astype(np.uint32), first, int(full.sum())


def _collection(eng, text, starts, seed):
    """build_gsa, then patterns + nodes + [0, n) through DocListDeviceIndex.list under every occ_cut."""
    n, nd = len(text), len(starts)
    rng = np.random.default_rng(seed)
    t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    ds = torch.from_numpy(np.asarray(starts, dtype=np.int64)).cuda()
    sa, da, lcp = sdev.build_gsa(t, ds, engine=eng)
    gx = sdev.GeneralizedDeviceIndex(t, ds, sa, da, engine=eng)
    pos, ln = rng.integers(0, n, 1 << 12), rng.integers(1, 13, 1 << 12)
    qs = [text[int(p):int(p) + int(k)] for p, k in zip(pos, ln)]
    qoff = np.zeros(len(qs) + 1, dtype=np.int64)
    qoff[1:] = np.cumsum([len(q) for q in qs])
    qb = torch.from_numpy(np.frombuffer(b"".join(qs), dtype=np.uint8).copy()).cuda()
    ps, pe, _, _, pnd = gx.query(qb, torch.from_numpy(qoff).cuda())
    iv = sdev.lcp_intervals(lcp, engine=eng)
    lb, rb = iv["lb"], iv["rb"]
    torch.cuda.synchronize()
    da_h = da.cpu().numpy().view(np.uint32)
    pick = rng.integers(1, n, 1 << 12)
    s = np.concatenate([ps.cpu().numpy().view(np.uint32), lb.cpu().numpy().view(np.uint32)[pick], [0]]).astype(np.int64)
    e = np.concatenate([pe.cpu().numpy().view(np.uint32), rb.cpu().numpy().view(np.uint32)[pick].astype(np.int64) + 1, [n]]).astype(np.int64)
    # (a sampled pattern that crosses a document boundary may occur nowhere: its interval is empty)
    assert ((e - s)[:1 << 12] > 0).sum() > 3800 and (s <= e).all() and (e <= n).all()
    exp = {(o, k): _expected(da_h, nd, s, e, o, k) for o in (L.BY_DOC, L.BY_TF) for k in (0, 10)}
    sizes = np.diff(exp[L.BY_DOC, 0][2].astype(np.int64))
    assert np.array_equal(sizes[:1 << 12], pnd.cpu().numpy().view(np.uint32))          # |D_j| = the search's own count
    st, en = (torch.from_numpy(x.astype(np.uint32).view(np.int32)).cuda() for x in (s, e))
    for cut in L.CUTS:
        dx = sdev.DocListDeviceIndex(da, ds, occ_cut=cut, engine=eng)
        try:
            for (order, k), (xd, xt, xf, xz) in exp.items():
                doc, tf, first, listed = dx.list(st, en, order=("doc", "tf")[order], top_k=k)
                torch.cuda.synchronize()
                assert listed == xz and np.array_equal(first.cpu().numpy().view(np.uint64), xf), (cut, order, k)
                got_d, got_t = doc.cpu().numpy().view(np.uint32), tf.cpu().numpy().view(np.uint32)
                assert np.array_equal(got_d, xd), (cut, order, k, np.flatnonzero(got_d != xd)[:4] if got_d.size == xd.size else (got_d.size, xd.size))
                assert np.array_equal(got_t, xt), (cut, order, k)
        finally:
            dx.close()
    gx.close()


def test_english_documents_with_empty_ones(eng):
    text = _gen.english_like(N).tobytes()
    starts = _cut(text, random.Random(1), 5000, 15000)
    starts = np.sort(np.concatenate([starts, starts[[0, 3, 40]], [starts[-1]]]))       # empty documents: in front, inside, before the last one
    _collection(eng, text, starts, 1)


def test_dna_as_two_documents(eng):
    _collection(eng, _gen.dna(N, seed=12).tobytes(), np.array([0, 1 << 19], dtype=np.int64), 2)


def test_dna_as_4097_short_documents(eng):
    _collection(eng, _gen.dna(N, seed=13).tobytes(), np.arange(0, N, 256, dtype=np.int64), 3)


def test_near_duplicates_in_64k_documents(eng):
    _collection(eng, _gen.near_duplicates(N).tobytes(), np.arange(0, N, 1 << 16, dtype=np.int64), 4)


def test_sixteen_copies_and_an_altered_one(eng):
    doc = _gen.english_like(1 << 16, seed=5).tobytes()
    altered = bytearray(doc)
    altered[40000] ^= 1
    docs = [doc] * 9 + [bytes(altered)] + [doc] * 7
    _collection(eng, b"".join(docs), _gsa.doc_starts(docs), 5)


@pytest.mark.parametrize("cut", [1 << 60, 1])
def test_interval_lengths_that_sum_past_2_to_32(eng, cut):
    """2^15 + 1 copies of [0, n) on a synthetic da of 2^17 + 5 ranks: every list is (the non-empty documents, their
    lengths), first is j * their number.  Route A is forced once and route B once."""
    n, nd, nq = (1 << 17) + 5, 300, (1 << 15) + 1
    da = np.random.default_rng(7).integers(0, nd, n).astype(np.uint32)
    da[da == 5] = 6
    da[da == nd - 1] = 0                                                 # documents 5 and nd - 1 are empty
    docs, lens = np.unique(da, return_counts=True)
    assert nq * n > 1 << 32 and docs.size == nd - 2
    dx = sdev.DocListDeviceIndex(torch.from_numpy(da.view(np.int32)).cuda(), torch.from_numpy(L.starts_of(da, nd).astype(np.int64)).cuda(),
                                 occ_cut=cut, engine=eng)
    try:
        s = torch.zeros(nq, dtype=torch.int32, device="cuda")
        e = torch.full((nq,), n, dtype=torch.int32, device="cuda")
        ws = dx.workspace(nq, nq * docs.size)
        out = {}

        def run():
            out["r"] = dx.list(s, e, order="doc", list_limit=nq * docs.size, workspace=ws)
            torch.cuda.synchronize()
        names = {x for x in _gsa.profile_names(eng, run) if x.startswith("doclist_")}
        assert (L.ROUTE_B if cut == 1 else L.ROUTE_A) <= names and not (L.ROUTE_A if cut == 1 else L.ROUTE_B) & names, sorted(names)
        doc, tf, first, listed = out["r"]
        assert listed == nq * docs.size
        assert torch.equal(first, torch.arange(nq + 1, dtype=torch.int64, device="cuda") * docs.size)
        assert torch.equal(doc.view(nq, docs.size), torch.from_numpy(docs.astype(np.int32)).cuda().expand(nq, -1))
        assert torch.equal(tf.view(nq, docs.size), torch.from_numpy(lens.astype(np.int32)).cuda().expand(nq, -1))
    finally:
        dx.close()
