"""The texts of tests/test_gpu_tie_route.py reach the edges of the hybrid route's tie path that they are meant to reach.

Each text is generated at its GPU size and modelled by tests/_ties.witness from the oracle's SA and LCP alone (no engine): the
route's entry test passes, the stretches of tied slots fall into every length class, long ones cross 64- and 4096-slot
boundaries, short ones are undecided at k_tie_direct's depth, X + X ties nearly everything.  A CPU test: it keeps the
generators from drifting away from what the GPU cases rely on."""
import numpy as np
import pytest

import _ties
from _ties import M_BIG, gpu_texts


@pytest.fixture(scope="module")
def witnessed(oracle):
    out = {}
    for name, (gen, m) in gpu_texts().items():
        text = gen()
        assert len(text) == m
        raw = text.tobytes()
        sa = oracle.sais(raw)
        w = _ties.witness(text, sa, oracle.lcp_kasai(raw, sa))
        out[name] = (_ties.route_preconditions(text), w)
    return out


@pytest.mark.parametrize("name", ["planted_dna", "doubled_dna", "binary", "sigma16"])
def test_route_preconditions_and_keys(witnessed, name):
    pre, w = witnessed[name]
    assert pre["ok"], pre
    assert w["symbols_per_key"] * w["bits"] == 32 and w["key_symbols"] == w["symbols_per_key"] + 1, w["bits"]
    assert w["kept"] > 0, "the text leaves nothing for the leftover path"


def test_planted_dna_reaches_every_edge(witnessed):
    pre, w = witnessed["planted_dna"]
    classes = _ties.length_classes(w)
    assert all(v > 0 for v in classes.values()), classes
    # long stretches across a wave's 64 slots (one lane's word pair) and across 4096 (one wave's window of k_tie_direct)
    assert _ties.crossing(w, 64) >= 24 and _ties.crossing(w, 4096) >= 24, (_ties.crossing(w, 64), _ties.crossing(w, 4096))
    short_undecided = int((w["undecided"] & (w["lens"] <= _ties.RUN_MAX)).sum())
    assert short_undecided >= 24, short_undecided
    assert w["small_groups_pay"], (w["kept"], w["groups"])


def test_doubled_dna_ties_nearly_everything(witnessed):
    pre, w = witnessed["doubled_dna"]
    m = w["m"]
    # (only the ~32 suffixes that start within one key of the end of either copy have no partner: they cut the array into a few
    # dozen stretches, the longest of them ~0.2 m)
    assert w["tied"] >= m - 64, (w["tied"], m)
    assert int(w["lens"].max()) >= m // 8, int(w["lens"].max())
    assert w["small_groups_pay"] and w["kept"] == w["tied"], (w["kept"], w["groups"])      # (runs of two, nearly all of them)


@pytest.mark.parametrize("name", ["binary", "sigma16"])
def test_small_alphabets_leave_long_and_deep_stretches(witnessed, name):
    pre, w = witnessed[name]
    lens = w["lens"]
    assert int((lens > _ties.RUN_MAX).sum()) >= 24 and int((w["undecided"] & (lens <= _ties.RUN_MAX)).sum()) >= 24
    assert _ties.crossing(w, 64) >= 24


def test_big_planted_dna_keeps_the_route():
    """At 240,000,003 suffixes (most waves of k_tie_direct take two passes of its grid-stride loop) the entry test still passes:
    no sub-bucket above 16384 suffixes and at most 1/64 of them in sub-buckets above 4096.  From the text alone."""
    text = _ties.planted_dna(M_BIG)
    pre = _ties.route_preconditions(text)
    assert pre["ok"] and pre["slow"] > 0, pre
    assert np.count_nonzero(text[-40:] == ord("A")) == 40
