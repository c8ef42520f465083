"""Repeat lengths and repeated spans on the MI355X: the emulator's random cases at larger scale, then inputs of up to 2^22
bytes (many tiles, every pyramid level, long range minima, long runs of one document) verified by the serial sweeps of
tests/rep_check.c and by the numpy span reference of tests/_repeats.py."""
import random

import numpy as np
import pytest
import torch

import _gen
import _gsa
import _repeats as R
from suffix_amd import GeneralizedSuffixTable, SuffixTable
from suffix_amd import device as sdev

pytestmark = pytest.mark.gpu
N = 1 << 22


@pytest.fixture(scope="module")
def eng():
    import suffix_amd
    e = suffix_amd.default_engine()
    e.require_device()                      # fail loudly: no CPU fallback
    assert e.path.endswith("libsuffix_hip.so")
    return e


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return R.build_checker(tmp_path_factory.mktemp("rep_check"))


def test_random_texts_vs_brute_force(eng):
    rng = random.Random(4243)
    for _ in range(300):
        text = R.random_text(rng)
        st, lcp = SuffixTable.new_with_lcp(text, engine=eng)
        R.check_small(eng, text, st.table(), lcp, ("any", "earlier"))


def test_random_collections_vs_brute_force(eng):
    rng = random.Random(4244)
    done = 0
    while done < 300:
        docs = _gsa.random_collection(rng, max_docs=12, max_len=14)
        text = b"".join(docs)
        if len(text) > 80:
            continue
        done += 1
        g = GeneralizedSuffixTable(docs, engine=eng)
        R.check_small(eng, text, g.table(), g.lcp_lens(), ("any", "earlier", "other_doc"), starts=_gsa.doc_starts(docs), da=g.doc_array())


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _verify(eng, checker, tmp_path, text, starts, scopes, min_lens=(1, 8, 50)):
    """Builds the arrays on the device, then per scope: rep + src through rep_check, spans (with the document starts of a
    collection) against the numpy reference.  -> {scope: (rep, spans at the last min_len)}"""
    t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    if starts is None:
        sa, lcp = sdev.build_sa_lcp(t, engine=eng)
        da = ds = None
    else:
        ds = torch.from_numpy(np.asarray(starts, dtype=np.int64)).cuda()
        sa, da, lcp = sdev.build_gsa(t, ds, engine=eng)
    inputs = R.write_inputs(tmp_path, text, [] if starts is None else starts, _u32(sa), _u32(lcp), None if da is None else _u32(da))
    out = {}
    for scope in scopes:
        rep, src = sdev.repeat_lens(sa, lcp, scope=scope, da=da, want_src=True, engine=eng)
        rep_h = _u32(rep)
        res = R.check_with(checker, inputs, tmp_path, scope, rep_h, _u32(src))
        assert res.startswith("ok"), (scope, res)
        assert torch.equal(sdev.repeat_lens(sa, lcp, scope=scope, da=da, engine=eng), rep)          # (without witnesses)
        for m in min_lens:
            got = sdev.repeat_spans(rep, m, doc_starts=ds, engine=eng)
            exp = R.span_reference(rep_h, m, starts)
            assert got.shape == (len(exp), 2) and np.array_equal(_u32(got.reshape(-1)).reshape(-1, 2), np.array(exp, dtype=np.uint32).reshape(-1, 2)), (scope, m)
        out[scope] = (rep_h, exp)
    return out


def test_english_plain(eng, checker, tmp_path):
    text = _gen.english_like(N).tobytes()
    out = _verify(eng, checker, tmp_path, text, None, ("any", "earlier"), min_lens=(1, 8, 50, 1 << 23))
    assert out["any"][1] == [] and out["earlier"][1] == []                 # nothing is 2^23 bytes long
    assert (out["earlier"][0] <= out["any"][0]).all()


def test_near_duplicates_have_long_range_minima(eng, checker, tmp_path):
    text = _gen.near_duplicates(N, ndocs=1).tobytes()                     # one 1 MiB document and three altered copies
    out = _verify(eng, checker, tmp_path, text, None, ("any", "earlier"))
    assert int(out["earlier"][0].max()) > 400                              # (a substituted byte about every 400)
    assert not out["earlier"][0][:1 << 20].max() > 400 and out["any"][0][:1 << 20].max() > 400


def test_unary_text(eng, checker, tmp_path):
    n = 1 << 20
    out = _verify(eng, checker, tmp_path, b"a" * n, None, ("any", "earlier"), min_lens=(8,))
    rep = out["earlier"][0]
    assert rep[0] == 0 and np.array_equal(rep[1:], n - np.arange(1, n, dtype=np.int64))
    assert out["earlier"][1] == [(1, n)] and out["any"][1] == [(0, n)]


def test_doubled_text(eng, checker, tmp_path):
    k = 1 << 17
    r = np.random.default_rng(6).integers(0, 256, k, dtype=np.uint8).tobytes()
    out = _verify(eng, checker, tmp_path, r + r, None, ("any", "earlier"), min_lens=(8,))
    assert out["earlier"][1] == [(k, 2 * k)] and out["any"][1] == [(0, 2 * k)]


@pytest.mark.parametrize("n", [262143, 262144, 262145])
def test_fan_cubed(eng, checker, tmp_path, n):
    text = _gen.english_like(n, seed=n).tobytes()
    _verify(eng, checker, tmp_path, text, None, ("any", "earlier"), min_lens=(1, 8))


def test_copies_of_one_document(eng, checker, tmp_path):
    base = _gen.english_like(1 << 15, seed=78).tobytes()
    docs = [base] * 64 + [base[:1000], base[:-1] + b"!", base[12345:]]
    text, starts = b"".join(docs), _gsa.doc_starts(docs)
    out = _verify(eng, checker, tmp_path, text, starts, ("any", "earlier", "other_doc"), min_lens=(8, 50))
    rep = out["other_doc"][0]
    assert np.count_nonzero(rep >= 50) > 0.99 * len(text)
    assert [(b, e) for b, e in out["other_doc"][1]][:2] == [(0, 1 << 15), (1 << 15, 2 << 15)]


def test_long_runs_of_one_document(eng, checker, tmp_path):
    big = _gen.english_like(1 << 20, seed=79).tobytes()
    docs = [big] + [big[a:a + 100] for a in (0, 77_777, 400_000, 999_000, (1 << 20) - 100)]
    text, starts = b"".join(docs), _gsa.doc_starts(docs)
    out = _verify(eng, checker, tmp_path, text, starts, ("earlier", "other_doc"), min_lens=(1, 50))
    rep = out["other_doc"][0]
    assert (rep[1 << 20:].reshape(5, 100) == 100 - np.arange(100)).all()
    assert out["other_doc"][1] == sorted([(a, a + 100) for a in (0, 77_777, 400_000, 999_000, (1 << 20) - 100)] +
                                         [((1 << 20) + 100 * i, (1 << 20) + 100 * (i + 1)) for i in range(5)])


def test_collection_of_cut_documents(eng, checker, tmp_path):
    rng = random.Random(2)
    text = _gen.english_like(N, seed=80).tobytes()
    starts, p = [0], 0
    while True:
        p += rng.randint(5000, 15000)
        if p >= len(text):
            break
        starts.append(p)
        if rng.random() < 0.02:
            starts.append(p)                                                  # an empty document
    _verify(eng, checker, tmp_path, text, np.array(starts, dtype=np.int64), ("any", "earlier", "other_doc"))


def test_host_side_mirrors(eng):
    text = _gen.english_like(20_000, seed=81).tobytes()
    st = SuffixTable(text + text[:5000], engine=eng)
    rep, src = st.repeat_lens("earlier", with_source=True)
    assert rep[20_000] == 5000 and src[20_000] == 0
    assert (20_000, 25_000) in st.repeated_spans(100, "earlier") and st.repeated_spans(100) != st.repeated_spans(100, "earlier")
    docs = [text[:3000], b"", text[1000:2000], "zebra"]
    g = GeneralizedSuffixTable(docs, engine=eng)
    rep = g.repeat_lens("other_doc")
    assert rep[3000] == 1000 and rep[1000] == 1000 and rep[0] < 1000
    assert g.repeated_spans(1000, "other_doc") == [(0, 1000, 2000), (2, 0, 1000)]
    assert np.array_equal(g.repeat_lens("any"), R.repeat_lens(eng, g.table(), g.lcp_lens(), "any", want_src=False)[0])
