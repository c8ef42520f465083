"""CPU tests of the maximal repetitions and the Lyndon array (sfx_runs_*, sfx_lyndon_array_*): the product's kernels
compiled against the fiber emulator (tests/emu), checked against the definition (`brute`), a stack over the oracle's
inverse table and the serial checker tests/runs_check.c.  The cases are tests/_runs.py's, shared with test_gpu_runs.py."""
import os
import re
import subprocess
import sys

import pytest

import _runs as R
from suffix_amd import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "emu")


@pytest.fixture(scope="module")
def emu():
    return Engine(R.build_emulator())


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    return R.build_checker(tmp_path_factory.mktemp("runs_check"))


def test_checker_refuses_one_fault_per_kind(chk):
    R.checker_self_test(chk)


def test_known_answers(emu, oracle):
    R.known_answers(emu, "cpu", oracle)


def test_small_random_texts_vs_brute(emu, oracle):
    assert R.small_random(emu, "cpu", oracle) >= 300


def test_edge_texts(emu, oracle):
    R.edge_texts(emu, "cpu", oracle)


def test_filters(emu, oracle):
    R.filters(emu, "cpu", oracle)


def test_capacity(emu, oracle):
    R.capacities(emu, "cpu", oracle)


def test_buffers_and_streams(emu, oracle):
    R.buffers_and_streams(emu, "cpu", oracle)


def test_dev_route_allocates_nothing(emu, oracle):
    R.no_allocations(emu, "cpu", oracle, lambda: emu.resource_stats()["device_allocs_total"])


def test_size_bound(emu):
    R.size_bound(emu)


def test_launch_names(emu, oracle):
    R.launch_names(emu, "cpu", oracle)


def test_refusals(emu, oracle):
    R.refusals(emu, "cpu", oracle)


def test_corrupted_lcp_stays_in_bounds(emu, oracle):
    R.corrupted_lcp(emu, "cpu", oracle)


def test_every_runs_kernel_maps_to_its_launch_name():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import pmc_summary
    src = open(os.path.join(ROOT, "suffix_amd", "csrc", "sfx_runs.hip")).read()
    kernels = set(re.findall(r"__global__[^;{]*?\b(k_runs_[a-z0-9_]+)\s*\(", src, flags=re.S))
    assert len(kernels) == 9, sorted(kernels)
    for k in sorted(kernels):
        assert k[2:] in R.KERNELS, k
        assert pmc_summary.profile_name(f"sfx::{k}(sfx::LceView, unsigned int const*, ...)") == k[2:], k


def test_checker_and_brute_agree_with_the_engine_on_a_larger_text(emu, oracle, chk):
    import _gen
    text = _gen.uniform_bytes(6000, 2, 11, base=97).tobytes()
    sa, lcp = R.tables(oracle, text)
    rc, z, got, _ = R.call_runs(emu, "cpu", text, sa, lcp)
    assert rc == R.OK and z == len(got)
    assert R.accept(chk, text, got, len(text) // 2) == z
    assert 0.35 * len(text) <= z <= 0.5 * len(text), z                # (random bits: about 0.42 n runs)


SCRIPT = """
import sys
sys.path[:0] = [{root!r}, {here!r}]
import oracle
import _runs as R
from suffix_amd import Engine
oracle.build()
R.hooked(Engine({lib!r}), "cpu", oracle)
print("OK")
"""


@pytest.mark.parametrize("tile,room", [("64", "5"), ("256", "0"), ("128", "100000")])
def test_small_tiles_and_a_short_open_list_in_a_hooked_process(emu, tmp_path, tile, room):
    """SFX_MAX_GRID=3 (more tiles and candidates than the grid holds), SFX_LCE_FAN=2 (a few thousand entries have a dozen
    levels), SFX_RUNS_TILE / SFX_RUNS_LIST (tiles of 64 to 256 words; an open list of 5 entries, of none, and one that holds
    everything): the random and edge cases again, the overflow path on texts of a few thousand bytes."""
    script = tmp_path / "hooked.py"
    script.write_text(SCRIPT.format(root=ROOT, here=HERE, lib=os.path.join(EMU_DIR, "libsuffix_emu.so")))
    env = dict(os.environ, SFX_MAX_GRID="3", SFX_LCE_FAN="2", SFX_RUNS_TILE=tile, SFX_RUNS_LIST=room)
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-2000:], r.stderr[-4000:])
