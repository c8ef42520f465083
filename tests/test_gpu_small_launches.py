"""The small launches of the hybrid build on the MI355X (run with -m gpu; round 10): the alphabet stage inside k_byte_presence
(slots, sharded tickets, the LUT and the posted flag words from its last workgroup), k_hist16_finish's sums by write-through
stores instead of atomics, and the counter lines of the tie kernels, zeroed by the histogram sweep and again by k_tie_totals.

At n = M_HYBRID = 2^25 + 4099, the smallest size the product takes the hybrid route at, between guard bands and with a
workspace filled with 0xFF (tests/_buffers.py):
  - a uniform 4-bit text and a uniform 2-bit text: the oracle's table, twice into the same buffers, which are filled with 0xFF
    again in between -- whatever must be zero on entry is zeroed inside the build;
  - DNA drawn with geometric weights: the route gives way by its statistics and the four-pass sort finishes the table.
No make_lut launch on any of them.
And texts of 20 000 bytes whose alphabet has 2 symbols, all 256, or includes 0x00 and 0xFF: the first and the last bit of the
posted flag words, on whichever route the texts take; the build's statistics must name the alphabet's size."""
import numpy as np
import pytest

import _buffers
import _gen
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


def _build_twice(eng, text, exp):
    """The same call twice into the same guarded buffers, 0xFF over workspace and output before each; -> profiled names."""
    eng.profile(True)
    eng.profile_reset()
    rc, b = _buffers.call_build_sa(eng, text, DEV, text_off=0, sa_off=0, fill=0xFF)
    for again in (0, 1):
        if again:
            b["workspace"].fill(0xFF)
            b["sa"].fill(0xFF)
            rc = eng.lib.sfx_build_sa_u32_dev(b["text"].ptr, len(text), b["sa"].ptr, b["workspace"].ptr, b["workspace"].nbytes, _buffers.stream_of(DEV))
        assert rc == _buffers.OK, (again, rc)
        got = b["sa"].host(np.uint32)
        assert np.array_equal(got, exp), (again, np.flatnonzero(got != exp)[:4])
        _buffers.check_all(b)
        assert eng.build_stats()["sigma"] == len(set(text[:1 << 16])), (again, eng.build_stats())
    assert b["text"].host().tobytes() == text
    names = set(r["name"] for r in eng.profile_report())
    eng.profile(False)
    return names


@pytest.mark.parametrize("sigma", [16, 4])
def test_uniform_text_twice_into_dirty_buffers(eng, oracle, sigma):
    text = (_routes.uniform(N, sigma, 1400 + sigma) + np.uint8(1)).tobytes()
    p = _routes.predict(text)
    assert (p["sigma"], p["key"], p["sort"]) == (sigma, "k32", "hybrid"), p
    names = _build_twice(eng, text, oracle.sais(text))
    assert {"radix_hist16_text", "radix_hist16_finish", "byte_presence", "tie_totals"} <= names and "make_lut" not in names, sorted(names)
    assert _routes.sort_route_of(names) == "hybrid_ties", sorted(names)


def test_skewed_dna_gives_way_by_the_statistics(eng, oracle):
    text = _routes.skewed(N, 4, 1501, 0.5).tobytes()
    p = _routes.predict(text)
    assert (p["bits"], p["key"], p["sort"]) == (2, "k32", "hybrid"), p
    eng.profile(True)
    eng.profile_reset()
    rc, b = _buffers.call_build_sa(eng, text, DEV, text_off=0, sa_off=0, fill=0xFF)
    got = b["sa"].host(np.uint32)
    names = set(r["name"] for r in eng.profile_report())
    eng.profile(False)
    assert rc == _buffers.OK, rc
    _buffers.check_all(b)
    assert {"radix_hist16_text", "radix_hist16_finish", "radix_window_from_hist16"} <= names and "make_lut" not in names, sorted(names)
    assert _routes.sort_route_of(names) == "passes", sorted(names)
    exp = oracle.sais(text)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:4]


def _both_ends(n):
    t = _gen.uniform_bytes(n, 16, 907, base=0).copy()
    t[t == 15] = 0xFF
    return t.tobytes()


@pytest.mark.parametrize("name,make", [("2 symbols", lambda n: _gen.uniform_bytes(n, 2, 4, base=97).tobytes()),
                                       ("256 symbols", lambda n: _gen.uniform_bytes(n, 256, 5, base=0).tobytes()),
                                       ("0x00 and 0xFF", _both_ends)])
def test_posted_alphabet_of_small_texts(eng, oracle, name, make):
    text = make(20000)
    assert len(text) > _routes.TINY_MAX                 # (past the one-workgroup build: the alphabet stage runs)
    if name == "256 symbols":
        assert len(set(text)) == 256
    if name == "0x00 and 0xFF":
        assert 0x00 in text and 0xFF in text
    # (build_sa_case: the oracle's table, guard bands intact, the statistics' sigma = the text's)
    _buffers.build_sa_case(eng, oracle, text, DEV, which=[(0, 0, 0xFF), (1, 4, "count")])
