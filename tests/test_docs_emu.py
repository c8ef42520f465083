"""CPU tests of the document counts and the k-common substrings (sfx_doc_counts_*, sfx_common_substrings_*): the
product's kernels compiled against the fiber emulator (tests/emu), checked against brute force over small collections
and the serial checker tests/dc_check.c.  The cases are tests/_docs.py's, shared with test_gpu_docs.py."""
import os
import re
import subprocess
import sys

import pytest

import _docs as D
from suffix_amd import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "emu")


@pytest.fixture(scope="module")
def emu():
    return Engine(D.build_emulator())


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    return D.build_checker(tmp_path_factory.mktemp("dc_check"))


def test_checker_names_a_planted_fault_in_each_array(chk, tmp_path):
    D.checker_self_test(chk, tmp_path)


def test_known_answers(emu):
    D.known_answers(emu, "cpu")


def test_the_tables_arrays_are_made_once(emu):
    D.arrays_are_made_once(emu)


@pytest.mark.parametrize("sigma", [2, 3])
def test_small_random_collections_vs_brute_force(emu, sigma):
    assert D.small_random(emu, "cpu", sigma) >= 150


def test_refusals(emu):
    D.refusals(emu, "cpu")


def test_corrupted_lcp_stays_in_bounds(emu):
    D.corrupted_lcp(emu, "cpu")


def test_dirty_workspace_offsets_and_streams(emu):
    D.dirty_workspace_and_streams(emu, "cpu")


def test_pattern_counts_agree_with_the_gindex_query(emu):
    assert D.cross_check_queries(emu, "cpu") >= 1000


def test_launch_names(emu):
    D.launch_names(emu, "cpu")


def test_workspace_bound(emu):
    D.size_bound(emu)


def test_synthetic_arrays_with_placed_prev_distances_and_high_values(emu, chk, tmp_path):
    D.synthetic(emu, "cpu", chk, tmp_path)


def test_every_docs_kernel_maps_to_its_launch_name():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import pmc_summary
    src = open(os.path.join(ROOT, "suffix_amd", "csrc", "sfx_docs.hip")).read()
    kernels = set(re.findall(r"__global__[^;{]*?\b(k_docs_[a-z0-9_]+)\s*\(", src, flags=re.S))
    assert len(kernels) == len(D.KERNELS), sorted(kernels)
    launched = set(re.findall(r'SFX_LAUNCH\("(docs_[a-z0-9_]+)"', src))
    assert launched == D.KERNELS, sorted(launched)
    for k in sorted(kernels):
        assert k[2:] in D.KERNELS, k
        assert pmc_summary.profile_name(f"sfx::{k}(sfx::DocsTree, unsigned int const*, ...)") == k[2:], k


SCRIPT = """
import sys
sys.path[:0] = [{root!r}, {here!r}]
import _docs as D
from suffix_amd import Engine
D.hooked(Engine({lib!r}), "cpu", {chk!r}, {out!r})
print("OK")
"""


@pytest.mark.parametrize("fan", ["2", "4"])
def test_deep_trees_in_a_hooked_process(emu, chk, tmp_path, fan):
    """SFX_LCE_FAN=2 / 4 (a few thousand entries have 6 to 12 levels), SFX_MAX_GRID=3 (more ranks than the grid holds):
    the known, random, synthetic and corrupted cases again."""
    script = tmp_path / "hooked.py"
    script.write_text(SCRIPT.format(root=ROOT, here=HERE, lib=os.path.join(EMU_DIR, "libsuffix_emu.so"), chk=chk, out=str(tmp_path)))
    env = dict(os.environ, SFX_LCE_FAN=fan, SFX_MAX_GRID="3")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-2000:], r.stderr[-4000:])
