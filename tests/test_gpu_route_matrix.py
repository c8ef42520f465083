"""The route matrix on an MI355X: every case of tests/_routes.py through the product library -- the suffix array and both LCP
arrays against the oracle, build_stats() and the kernels' profile names against the declared (symbol width, key, sort route, LCP
route) cell, `active_after_initial` against the witness.  The sizes are the smallest at which the hook-free library takes the
cell (2^25 + 4099 bytes for the hybrid route, the flip points of the key rule themselves, 2^20 + 7 for the direct LCP pass), so
the GPU work of a case is milliseconds and the wall time is the CPU oracle's: the arrays of the cases of 2^23 bytes and more are
computed ahead by up to 8 threads and dropped as their case ends.  The 1-, 2- and 4-bit cells of the hybrid route's tie mode are
the texts of test_gpu_tie_route.py and run there."""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process, see suffix_amd/_lib.py)

import _routes

pytestmark = pytest.mark.gpu

TIE_KERNEL_MS = 20.0            # test_gpu_tie_route.py's bound, as it stands: only a serial walk comes near it
AHEAD_MIN = 1 << 23
GPU_CASES = sorted((c for c in _routes.CASES if not c.where.startswith("tests/")), key=lambda c: c.n)


@pytest.fixture(scope="module")
def eng():
    import suffix_amd
    e = suffix_amd.default_engine()
    e.require_device()
    assert e.path.endswith("libsuffix_hip.so")
    return e


@pytest.fixture(scope="module")
def ahead(oracle):
    """case -> (text, sa, lcp) of the oracle for the cases of 2^23 bytes and more, started together in ascending size (the oracle
    is C behind ctypes: the threads run side by side); a case takes its arrays out, so they go when it ends."""
    def work(case):
        text = np.ascontiguousarray(case.make())
        sa = oracle.sais(text)
        return text, sa, oracle.lcp_kasai(text, sa)
    pool = ThreadPoolExecutor(max_workers=8)
    pending = {c.name: pool.submit(work, c) for c in GPU_CASES if c.n >= AHEAD_MIN}

    def take(case):
        fut = pending.pop(case.name, None)
        return fut.result() if fut is not None else None
    yield take
    for fut in pending.values():
        fut.cancel()
    pool.shutdown(wait=True)


@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: c.name)
def test_gpu_takes_the_declared_cell(eng, oracle, ahead, case):
    t0 = time.time()
    arrays = ahead(case)
    t1 = time.time()
    rep, st, w = _routes.check_case(eng, oracle, case, "cuda", arrays=arrays)
    del arrays
    sort = case.cell[2]
    if sort.startswith("hybrid"):
        assert st["key_bits"] == 32 and "radix_hist16_text" in rep, (st, sorted(rep))
    if sort == "hybrid_ties":
        # what test_tie_route_sa_lcp holds its texts to
        for k in ("bucket_sort_ties", "tie_direct"):
            assert k in rep, (case.name, k, sorted(rep))
        assert "oversize_gather" not in rep and "bucket_sort_lds" not in rep, sorted(rep)
        if w["kept"]:
            assert "tie_heads" in rep and "tie_list" in rep, (case.name, w["kept"], sorted(rep))
        if w["small_groups_pay"]:
            assert "small_groups" in rep, (case.name, w["kept"], w["groups"], sorted(rep))
        t_direct = rep["tie_direct"]["total_ms"]
        t_list = rep.get("tie_list", {"total_ms": 0.0})["total_ms"] + rep.get("tie_list_count", {"total_ms": 0.0})["total_ms"]
        print(f"\n{case.name}: tied {w['tied']} kept {w['kept']} tie_direct {t_direct:.3f} ms, tie_list_count + tie_list {t_list:.3f} ms")
        assert t_direct <= TIE_KERNEL_MS and t_list <= TIE_KERNEL_MS, (case.name, t_direct, t_list)
    if sort == "hybrid_keys":
        for k in ("bucket_sort_lds", "oversize_gather", "oversize_return", "groups_reduce"):
            assert k in rep, (case.name, k, sorted(rep))
        assert "tie_direct" not in rep and "bucket_sort_ties" not in rep, sorted(rep)
    print(f"\n{case.name}: n={case.n} cell={case.cell} waited {t1 - t0:.1f} s for the oracle, checked in {time.time() - t1:.1f} s")
    torch.cuda.empty_cache()
