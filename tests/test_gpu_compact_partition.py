"""The compact-staging text-fed partition pass (k_partition_text) on the MI355X (run with -m gpu), at the smallest sizes the
product takes the hybrid route at.

Uniform texts of 1, 2, 4 and 8 bits per symbol (32, 16, 8 and 4 symbols per packed word: every instantiation the product
launches) at n = 2^25 + T + 4099 -- the last tile of T positions is short and ends inside a packed word, and a stretch holds
more than one tile -- and at n = 2^25 + T, where the last tile is exactly full and the loader reads the words behind the text's
very last positions.  The text is an input between guard bands (tests/_buffers.py): its last byte is the last byte before the
band.  The table is compared with the oracle's; the 2-bit texts also go through the one-call entry and its LCP array."""
import numpy as np
import pytest

import _buffers
import _routes

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = 16384                     # positions per tile of k_partition_text (kCompactKPT = 32 per thread x 512 threads)
SIZES = ((1 << 25) + TILE + 4099, (1 << 25) + TILE)


@pytest.fixture(scope="module")
def eng():
    import suffix_amd
    e = suffix_amd.default_engine()
    e.require_device()                      # fail loudly: no CPU fallback
    assert e.path.endswith("libsuffix_hip.so")
    return e


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bits", [1, 2, 4, 8])
def test_compact_partition_smallest_hybrid_sizes(eng, oracle, bits, n):
    text = _routes.uniform(n, 1 << bits, 1900 + bits).tobytes()
    p = _routes.predict(text)
    assert (p["bits"], p["sort"], p["key"]) == (bits, "hybrid", "k32"), p
    exp = oracle.sais(text)
    eng.profile(True)
    eng.profile_reset()
    rc, b = _buffers.call_build_sa(eng, text, DEV, text_off=0, sa_off=0, fill=0xFF)
    got = b["sa"].host(np.uint32)
    names = set(r["name"] for r in eng.profile_report())
    eng.profile(False)
    assert rc == _buffers.OK, rc
    assert _routes.sort_route_of(names) == "hybrid_ties" and "radix_scatter_text_u32" in names, sorted(names)
    assert np.array_equal(got, exp), (bits, n, np.flatnonzero(got != exp)[:4])
    assert b["text"].host().tobytes() == text
    _buffers.check_all(b)
    del b, got
    if bits == 2:
        rc, b = _buffers.call_build_sa_lcp(eng, text, DEV, text_off=0, sa_off=0, lcp_off=0, fill=0xFF)
        assert rc == _buffers.OK, rc
        assert np.array_equal(b["sa"].host(np.uint32), exp), ("one-call SA", n)
        assert np.array_equal(b["lcp"].host(np.uint32), oracle.lcp_kasai(text, exp)), ("one-call LCP", n)
        _buffers.check_all(b)
