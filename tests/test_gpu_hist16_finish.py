"""k_hist16_finish on the MI355X (run with -m gpu): the sub-bucket starts, cursors, digit totals and statistics that the column
stage and the last column leave behind, at n = M_HYBRID = 2^25 + 4099, the smallest size the product takes the hybrid route at.

Two texts, both checked on the CPU beforehand:
  - 14 of 16 symbols uniform, the lowest and the highest once each as the last two bytes: columns 0 and 31 of the 32 columns of
    2048 sub-buckets are empty, columns 1 and 30 hold one suffix each (the column totals' scan meets zeros at both ends); the
    route is taken to its end (hybrid_ties) and the table is the oracle's;
  - DNA drawn with geometric weights 1 : 1/2 : 1/4 : 1/8: the largest sub-bucket holds 220 209 suffixes and 15 797 701 suffixes
    sit in sub-buckets above 4096 -- spread over the sweep's ~228 workgroups about 1000 per stretch, so no 16-bit counter wraps
    and the route gives way by its statistics (words 0, 1 and 4); the four-pass sort then takes its digit totals from totals_lo /
    totals_hi (radix_window_from_hist16), and the table is the oracle's.
The texts lie between guard bands (tests/_buffers.py)."""
import numpy as np
import pytest

import _buffers
import _routes

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = _routes.M_HYBRID


@pytest.fixture(scope="module")
def eng():
    import suffix_amd
    e = suffix_amd.default_engine()
    e.require_device()                      # fail loudly: no CPU fallback
    assert e.path.endswith("libsuffix_hip.so")
    return e


def _build(eng, text):
    eng.profile(True)
    eng.profile_reset()
    rc, b = _buffers.call_build_sa(eng, text, DEV, text_off=0, sa_off=0, fill=0xFF)
    got = b["sa"].host(np.uint32)
    names = set(r["name"] for r in eng.profile_report())
    eng.profile(False)
    assert rc == _buffers.OK, rc
    assert b["text"].host().tobytes() == text
    _buffers.check_all(b)
    return got, names


def test_empty_first_and_last_column(eng, oracle):
    t = _routes.uniform(N, 14, 1201) + np.uint8(1)
    t[N - 2] = 40
    t[N - 1] = 55
    text = t.tobytes()
    p = _routes.predict(text)
    assert (p["sigma"], p["bits"], p["key"], p["sort"]) == (16, 4, "k32", "hybrid"), p
    got, names = _build(eng, text)
    assert {"radix_hist16_text", "radix_hist16_finish"} <= names, sorted(names)
    assert _routes.sort_route_of(names) == "hybrid_ties", sorted(names)
    exp = oracle.sais(text)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:4]


def test_skewed_dna_gives_way_by_the_statistics(eng, oracle):
    text = _routes.skewed(N, 4, 1301, 0.5).tobytes()
    p = _routes.predict(text)
    assert (p["bits"], p["key"], p["sort"]) == (2, "k32", "hybrid"), p
    got, names = _build(eng, text)
    assert {"radix_hist16_text", "radix_hist16_finish", "radix_window_from_hist16"} <= names, sorted(names)
    assert _routes.sort_route_of(names) == "passes", sorted(names)
    exp = oracle.sais(text)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:4]
