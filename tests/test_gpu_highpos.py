"""Every structure built on the suffix array at text positions and ranks above 2^31, on the MI355X through the product
library: the cases of tests/_highpos.py (proven on the CPU by test_highpos_emu.py) at two placements of the tail,

    A   n = 2^31 + 35 539, pad_len = 2^31 - 30 000: positions on both sides of 2^31, ranks >= 2^31 in the high block;
    B   n = 2^32 - 1, the largest accepted length: positions up to 2^32 - 2, where every p + len or p + 8 near the end
        wraps in 32 bits.

One module-scoped fixture per placement holds text, SA and LCP on the device and is torn down before the next.  A never
skips; B skips only where torch.cuda.mem_get_info() shows less free memory than a step needs, and says both numbers."""
import pytest
import torch

import _highpos as HP
from suffix_amd import device as sdev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import suffix_amd
    e = suffix_amd.default_engine()
    e.require_device()                      # fail loudly: no CPU fallback
    assert e.path.endswith("libsuffix_hip.so")
    return e


@pytest.fixture(scope="module", params=["A", "B"])
def fx(request, eng, oracle):
    f = HP.HighText(eng, "cuda", oracle, HP.PLACEMENTS[request.param], may_skip=request.param == "B")
    assert f.n == {"A": (1 << 31) + 35539, "B": (1 << 32) - 1}[request.param]
    yield f
    f.close()


def test_builds(eng, fx):
    import bench
    HP.check_builds(eng, "cuda", fx, verify=lambda text, sa: bench.verify_sa_chunked(torch, sdev, text, sa))


def test_inverse_table(eng, fx):
    HP.check_inverse(eng, "cuda", fx)


def test_exact_search(eng, fx):
    HP.check_search(eng, "cuda", fx)


def test_matching_statistics(eng, fx):
    HP.check_match_stats(eng, "cuda", fx)


def test_mems(eng, fx):
    HP.check_mems(eng, "cuda", fx)


def test_k_mismatch_search(eng, fx):
    HP.check_hamming(eng, "cuda", fx)


def test_bwt_and_fm_index(eng, fx):
    HP.check_bwt_fm(eng, "cuda", fx)


def test_lce_index(eng, fx):
    HP.check_lce(eng, "cuda", fx)


def test_repeat_lengths(eng, fx):
    HP.check_repeats(eng, "cuda", fx)


def test_lz77(eng, fx):
    HP.check_lz(eng, "cuda", fx)


def test_lcp_intervals(eng, fx):
    HP.check_intervals(eng, "cuda", fx)


A_ONLY = pytest.mark.parametrize("fx", ["A"], indirect=True)


@A_ONLY
def test_collection(eng, fx):
    HP.check_collection(eng, "cuda", fx)


@A_ONLY
def test_host_wrappers(eng, fx):
    HP.check_host(eng, "cuda", fx)
