"""The generalized suffix array on the MI355X: the emulator's cases at larger scale, then collections of 2^25 bytes
(the product's large-input routes) verified by an engine-independent checker (tests/gsa_check.c), and 10^5 batched
queries against scans of the documents."""
import contextlib
import random

import numpy as np
import pytest
import torch

import _cases
import _gen
import _gsa
from suffix_amd import GeneralizedSuffixTable
from suffix_amd import device as sdev

pytestmark = pytest.mark.gpu
BIG = 1 << 25


@pytest.fixture(scope="module")
def eng():
    import suffix_amd
    e = suffix_amd.default_engine()
    e.require_device()                      # fail loudly: no CPU fallback
    assert e.path.endswith("libsuffix_hip.so")
    return e


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _gsa.build_checker(tmp_path_factory.mktemp("gsa_check"))


def test_random_collections_vs_definition(eng):
    rng = random.Random(4242)
    for i in range(300):
        docs = _gsa.random_collection(rng, max_len=40)
        with _cases.general_build(eng) if i % 2 else contextlib.nullcontext():
            g = _gsa.check_against_naive(eng, docs)
        if i % 10 == 0:
            _gsa.check_queries(eng, g, docs, [b"", b"a", b"ab", b"\x00\xff"] + docs[:2] + _gsa.boundary_queries(docs, rng))


def test_single_document_is_the_plain_table(eng):
    text = _gen.english_like(300_000, seed=11).tobytes()
    names = _gsa.profile_names(eng, lambda: _gsa.single_doc_matches_plain(eng, text))
    assert "gsa_fixup_sort" not in names


def _cut(text, rng, lo, hi):
    starts, p = [0], 0
    while True:
        p += rng.randint(lo, hi)
        if p >= len(text):
            break
        starts.append(p)
        if rng.random() < 0.01:
            starts.append(p)                                                  # an empty document
    return np.array(starts, dtype=np.int64)


def _build_and_check(eng, checker, text, starts, tmp_path):
    t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    ds = torch.from_numpy(starts).cuda()
    sa, da, lcp = sdev.build_gsa(t, ds, engine=eng)
    torch.cuda.synchronize()
    h = [x.cpu().numpy().view(np.uint32) for x in (sa, da, lcp)]
    out = _gsa.run_checker(checker, tmp_path, text, starts, *h)
    assert out.startswith("ok"), out
    return t, ds, sa, da, h


def test_english_collection_and_queries(eng, checker, tmp_path):
    rng = random.Random(1)
    text = _gen.english_like(BIG).tobytes()
    starts = _cut(text, rng, 5000, 15000)
    t, ds, sa, da, h = _build_and_check(eng, checker, text, starts, tmp_path)
    # 10^5 queries: substrings of the text (some across document ends), half with a changed last byte
    nq = 100_000
    qr = np.random.default_rng(3)
    pos = qr.integers(0, len(text) - 20, nq)
    lens = qr.integers(1, 17, nq)
    qs = [bytearray(text[p:p + k]) for p, k in zip(pos.tolist(), lens.tolist())]
    for i in range(nq // 2, nq):
        qs[i][-1] = (qs[i][-1] + 1) % 256
    qs = [bytes(q) for q in qs]
    qs[:6] = [b"", b"e", b"the ", b"\x00", text[int(starts[5]) - 2:int(starts[5]) + 2], text[int(starts[7]):int(starts[8])]]
    qoff = np.zeros(nq + 1, dtype=np.int64)
    qoff[1:] = np.cumsum([len(q) for q in qs])
    qb = torch.from_numpy(np.frombuffer(b"".join(qs), dtype=np.uint8).copy()).cuda()
    ix = sdev.GeneralizedDeviceIndex(t, ds, sa, da, engine=eng)
    s_, e_, f_, a_, n_ = (x.cpu().numpy().view(np.uint32) if x.dtype == torch.int32 else x.cpu().numpy()
                          for x in ix.query(qb, torch.from_numpy(qoff).cuda()))
    ix.close()
    gsa, gda = h[0], h[1]
    ref = _ScanReference(text, starts)
    sample = list(range(6)) + qr.choice(nq, 150, replace=False).tolist()
    for k in sample:
        q = qs[k]
        hits, hdocs = ref.matches(q)
        s, e = int(s_[k]), int(e_[k])
        assert np.array_equal(np.sort(gsa[s:e]), hits), (k, q)
        assert bool(f_[k]) == (hits.size > 0), (k, q)
        if hits.size:
            assert ref.contains(hits, int(a_[k])), (k, q)
        else:
            assert (s, e) == (0, 0), (k, q)
        docs = np.unique(hdocs)
        assert int(n_[k]) == docs.size and np.array_equal(np.unique(gda[s:e]), docs), (k, q)


class _ScanReference:
    """Occurrences of a query inside single documents, by vectorised scans of the text (no engine involved): the
    positions of every byte value are grouped once; a query's candidates are those of its first byte, filtered by
    each further byte, then by the end of the document they start in."""

    def __init__(self, text, starts):
        self.t = np.frombuffer(text, dtype=np.uint8)
        self.order = np.argsort(self.t, kind="stable")                    # positions, grouped by byte, ascending
        self.bstart = np.searchsorted(self.t[self.order], np.arange(257))
        self.starts = np.asarray(starts, dtype=np.int64)
        self.ends = np.append(self.starts[1:], self.t.size)

    def matches(self, q):
        """-> (sorted positions, their documents) of the in-document occurrences of q."""
        if not q:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        cand = self.order[self.bstart[q[0]]:self.bstart[q[0] + 1]].astype(np.int64)
        cand = cand[cand <= self.t.size - len(q)]
        for j in range(1, len(q)):
            cand = cand[self.t[cand + j] == q[j]]
        d = np.searchsorted(self.starts, cand, side="right") - 1
        keep = cand + len(q) <= self.ends[d]
        return cand[keep], d[keep]

    @staticmethod
    def contains(sorted_hits, p):
        i = int(np.searchsorted(sorted_hits, p))
        return i < sorted_hits.size and int(sorted_hits[i]) == p


def test_near_duplicate_collection(eng, checker, tmp_path):
    text = _gen.near_duplicates(BIG).tobytes()
    starts = np.arange(0, BIG, 1 << 20, dtype=np.int64)
    _build_and_check(eng, checker, text, starts, tmp_path)


def test_mostly_affected_collection_takes_the_fixup_sort(eng, checker, tmp_path):
    base = _gen.english_like(1 << 19, seed=77).tobytes()
    docs = [base] * 64
    docs += [base[:1000], base[:-1] + b"!", base[12345:]]
    starts = _gsa.doc_starts(docs)
    text = b"".join(docs)
    names = _gsa.profile_names(eng, lambda: _build_and_check(eng, checker, text, starts, tmp_path))
    assert {"gsa_fixup_sort", "gsa_merge", "gsa_lcp"} <= names, sorted(names)
