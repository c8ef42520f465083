"""CPU tests of the FM-index over the Burrows-Wheeler pair (sfx_fm_create*, sfx_fm_count*, sfx_fm_lookup*): the product's
kernels compiled against the fiber emulator (tests/emu), checked against the oracle's table and intervals.  The cases
are tests/_fm.py's, shared with test_gpu_fm.py."""
import os
import subprocess
import sys

import pytest

import _fm as F
from suffix_amd import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "emu")


@pytest.fixture(scope="module")
def emu():
    return Engine(F.build_emulator())


def test_known_answers(emu, oracle):
    F.known_answers(emu, "cpu", oracle)


def test_small_random_texts_vs_oracle(emu, oracle):
    assert F.small_random(emu, "cpu", oracle) >= 300


def test_edges(emu, oracle):
    F.edges(emu, "cpu", oracle, big_all_ranks=False)


def test_refusals(emu, oracle):
    F.refusals(emu, "cpu", oracle)


def test_mutated_pairs_stay_in_bounds(emu, oracle):
    F.mutated_pairs(emu, "cpu", oracle)


def test_size_bounds(emu, oracle):
    F.sizes(emu, "cpu", oracle)


def test_launch_names(emu, oracle):
    F.launch_names(emu, "cpu", oracle)


def test_every_fm_kernel_maps_to_its_launch_name():
    import re
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import pmc_summary
    src = open(os.path.join(ROOT, "suffix_amd", "csrc", "sfx_fm.hip")).read()
    kernels = set(re.findall(r"__global__[^;{]*?\b(k_fm_[a-z0-9_]+)\s*\(", src, flags=re.S))
    assert len(kernels) >= 9, sorted(kernels)
    for k in sorted(kernels):
        want = {"k_fm_count": "fm_count", "k_fm_lookup": "fm_lookup"}.get(k, "fm_build")
        assert pmc_summary.profile_name(f"void sfx::{k}<4>(sfx::FmView, ...)") == want, k


SCRIPT = """
import sys
sys.path[:0] = [{root!r}, {here!r}]
import oracle
import _fm as F
from suffix_amd import Engine
oracle.build()
F.small_grid(Engine({lib!r}), "cpu", oracle)
print("OK")
"""


def test_small_grid_in_a_hooked_process(emu, tmp_path):
    """SFX_MAX_GRID=3 (read once per process): more teams than the grid holds, several blocks per scan chunk."""
    script = tmp_path / "small_grid.py"
    script.write_text(SCRIPT.format(root=ROOT, here=HERE, lib=os.path.join(EMU_DIR, "libsuffix_emu.so")))
    env = dict(os.environ, SFX_MAX_GRID="3")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-2000:], r.stderr[-4000:])
