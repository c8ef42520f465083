"""The tie route of the hybrid initial sort on repeat-rich texts of 2^25 .. 2^28 suffixes, where the product takes it.

The texts (tests/_ties.py) leave stretches of tied slots that k_tie_direct cannot finish -- long ones, ones across 64- and
4096-slot windows, short ones equal beyond its depth, X + X tying nearly every slot -- so the leftover path (k_tie_heads,
k_tie_list, the small-groups pass, refine) runs at the sizes of the headline build.  For every text: the SA against the oracle,
the kernels the route runs, every tie bit of the LDS sort through build_stats (the witness's count of tied slots), the LCP
through the separate and the fused entry, and a bound on the tie kernels' time that only a serial walk would break.  The
oracle runs once per text; nothing is written into the tree."""
import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process, see suffix_amd/_lib.py)

import _cases
import _ties

pytestmark = pytest.mark.gpu

TIE_KERNEL_MS = 20.0        # per build; uniform 100 MB of DNA: tie_direct 0.039 ms -- only a serial walk comes near this


@pytest.fixture(scope="module")
def eng():
    import suffix_amd
    e = suffix_amd.default_engine()
    e.require_device()
    assert e.path.endswith("libsuffix_hip.so")
    return e


_ORACLE = {}


def _texts():
    t = dict(_ties.gpu_texts())
    t["planted_dna_big"] = (lambda: _ties.planted_dna(_ties.M_BIG), _ties.M_BIG)
    return t


@pytest.fixture(scope="module")
def case(oracle):
    """name -> (text, sa, lcp), the oracle's arrays computed once per text and dropped when the next text is asked for."""
    def get(name):
        if name not in _ORACLE:
            _ORACLE.clear()
            text = _texts()[name][0]()
            raw = text.tobytes()
            sa = oracle.sais(raw)
            _ORACLE[name] = (text, sa, oracle.lcp_kasai(raw, sa))
        return _ORACLE[name]
    yield get
    _ORACLE.clear()


def _build_profiled(eng, d_text):
    from suffix_amd import device as sdev
    eng.profile(True)
    eng.profile_reset()
    sa = sdev.build_sa(d_text)
    torch.cuda.synchronize()
    rep = {r["name"]: r for r in eng.profile_report()}
    eng.profile(False)
    return sa, rep, eng.build_stats()


@pytest.mark.parametrize("name", ["planted_dna", "doubled_dna", "binary", "sigma16", "planted_dna_big"])
def test_tie_route_sa_lcp(eng, case, name):
    from suffix_amd import device as sdev
    text, exp, want = case(name)
    m = len(text)
    d_text = torch.from_numpy(text).cuda()
    sa, rep, st = _build_profiled(eng, d_text)
    assert np.array_equal(sa.cpu().numpy().view(np.uint32), exp), name
    assert st["key_bits"] == 32, st
    for k in ("radix_hist16_text", "bucket_sort_ties", "tie_direct", "tie_heads", "tie_list"):
        assert k in rep, (name, k, sorted(rep))
    assert "oversize_gather" not in rep, sorted(rep)
    if name == "planted_dna_big":
        # (the SA-order witness would take several GB of host memory here: the entry test from the text alone)
        assert _ties.route_preconditions(text)["ok"]
    else:
        w = _ties.witness(text, exp, want)
        if w["small_groups_pay"]:
            assert "small_groups" in rep, (name, w["kept"], w["groups"], sorted(rep))
        # every tie bit the LDS sort wrote (the driver sets the field from k_tie_direct's count and nothing after it does)
        assert st["active_after_initial"] == w["tied"], (name, st["active_after_initial"], w["tied"])
    # a serial walk over a long stretch (one lane for ~m / 5 slots on X + X) is the only way to come near this
    t_direct = rep["tie_direct"]["total_ms"]
    t_list = rep["tie_list"]["total_ms"] + rep.get("tie_list_count", {"total_ms": 0.0})["total_ms"]
    print(f"\n{name}: m={m} tie_direct {t_direct:.3f} ms, tie_list_count + tie_list {t_list:.3f} ms, tie_heads "
          f"{rep['tie_heads']['total_ms']:.3f} ms")
    assert t_direct <= TIE_KERNEL_MS and t_list <= TIE_KERNEL_MS, (name, t_direct, t_list)
    del sa
    lcp = sdev.build_lcp(d_text, torch.from_numpy(exp.view(np.int32)).cuda())
    assert np.array_equal(lcp.cpu().numpy().view(np.uint32), want), name
    del lcp
    sa2, lcp2 = sdev.build_sa_lcp(d_text)
    assert np.array_equal(sa2.cpu().numpy().view(np.uint32), exp), name
    assert np.array_equal(lcp2.cpu().numpy().view(np.uint32), want), name
    del sa2, lcp2, d_text
    torch.cuda.empty_cache()


@pytest.mark.parametrize("nranges", [1, 3])
def test_tie_route_range_slices(eng, oracle, nranges):
    """Slices of the range-partitioned build through sfx_build_sa_range_u32_dev on planted DNA with only the repeats a slice can
    finish on its own (blocks of 24 and 40 symbols in 2 .. 3000 copies: longer ones stall its text-only rounds): no slice falls
    back to the whole array.  One rank is the whole key space (the text-fed route of the full build, leftovers and all); three
    ranks make slices of ~2^23.4 suffixes, below the route's 2^25, which keep the four-pass sort."""
    text = _ties.planted_dna(_ties.M_PLANTED, slices=True).tobytes()
    eng.profile(True)
    eng.profile_reset()
    fell_back = _cases.range_slices(eng, oracle, text, nranges, device="cuda")
    names = {r["name"] for r in eng.profile_report()}
    eng.profile(False)
    assert fell_back == 0, fell_back
    if nranges == 1:
        assert "tie_heads" in names and "tie_list" in names, sorted(names)
    torch.cuda.empty_cache()
