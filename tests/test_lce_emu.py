"""CPU tests of the LCE index (sfx_inverse_table_*, sfx_lce_*): the product's kernels compiled against the fiber emulator
(tests/emu), checked against plain byte comparison and the serial checker tests/lce_check.c.  The cases are
tests/_lce.py's, shared with test_gpu_lce.py."""
import os
import re
import subprocess
import sys

import pytest

import _lce as L
from suffix_amd import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "emu")


@pytest.fixture(scope="module")
def emu():
    return Engine(L.build_emulator())


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    return L.build_checker(tmp_path_factory.mktemp("lce_check"))


def test_checker_names_one_fault_per_mode(chk):
    L.checker_self_test(chk)


def test_known_answers(emu, oracle):
    L.known_answers(emu, "cpu", oracle)


def test_the_tables_handle_is_made_once(emu, oracle):
    L.handle_is_made_once(emu, oracle)


def test_small_random_texts_vs_brute(emu, oracle):
    assert L.small_random(emu, "cpu", oracle) >= 150


def test_small_random_collections_vs_brute(emu):
    assert L.small_collections(emu, "cpu") >= 60


def test_sizes_at_the_level_edges(emu):
    L.level_edges(emu, "cpu")


def test_edge_texts(emu, oracle):
    L.edge_texts(emu, "cpu", oracle)


def test_refusals(emu, oracle):
    L.refusals(emu, "cpu", oracle)


def test_corrupted_lcp_stays_in_bounds(emu, oracle):
    L.corrupted_lcp(emu, "cpu", oracle)


def test_streams_and_threads(emu, oracle):
    L.streams_and_threads(emu, "cpu", oracle)


def test_size_bound(emu):
    L.size_bound(emu)


def test_launch_names(emu, oracle):
    L.launch_names(emu, "cpu", oracle)


def test_every_lce_kernel_maps_to_its_launch_name():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import pmc_summary
    src = open(os.path.join(ROOT, "suffix_amd", "csrc", "sfx_lce.hip")).read()
    kernels = set(re.findall(r"__global__[^;{]*?\b(k_lce_[a-z0-9_]+)\s*\(", src, flags=re.S))
    assert len(kernels) >= 8, sorted(kernels)
    for k in sorted(kernels):
        want = {"k_lce_scatter_pairs": "lce_scatter"}.get(k, k[2:])
        assert want in L.KERNELS, k
        assert pmc_summary.profile_name(f"sfx::{k}(sfx::LceView, unsigned int const*, ...)") == want, k


def test_checker_agrees_with_brute_on_a_larger_text(emu, oracle, chk):
    """Both known answers on one input: the engine's lengths pass the checker and equal `brute`."""
    import random
    import _gen
    text = _gen.near_duplicates(6000).tobytes()
    sa, lcp = L.tables(oracle, text)
    L.check_text(emu, "cpu", text, sa, lcp, rng=random.Random(5), limit=300, chk=chk)
    L.check_text(emu, "cpu", text, sa, lcp, rng=random.Random(5), limit=300)
    lx = L.Lx(emu, "cpu", sa, lcp)
    lo, hi = L.edge_ranges(len(text), random.Random(6))
    L.accept_min(chk, lcp, lo, hi, lx.range_min(lo, hi))
    lx.close()
    rc, isa = L.inverse_table_raw(emu, "cpu", sa)
    assert rc == 0
    L.accept_isa(chk, sa, isa)


SCRIPT = """
import sys
sys.path[:0] = [{root!r}, {here!r}]
import oracle
import _lce as L
from suffix_amd import Engine
oracle.build()
L.hooked(Engine({lib!r}), "cpu", oracle)
print("OK")
"""


@pytest.mark.parametrize("variant", ["lane", "team", "pyramid"])
@pytest.mark.parametrize("fan", ["2", "4"])
def test_deep_trees_in_a_hooked_process(emu, tmp_path, fan, variant):
    """SFX_LCE_FAN=2 / 4 (a few thousand entries have 6 to 12 levels), SFX_MAX_GRID=3 (more queries and words than the grid
    holds), SFX_PARTITION_MIN=1000 (the partitioned scatter from 1000 entries on), once per SFX_LCE_VARIANT (one lane per
    query, 32 lanes per query, the 64-ary pyramid of sfx_tree.hip): the random and edge cases again."""
    script = tmp_path / "hooked.py"
    script.write_text(SCRIPT.format(root=ROOT, here=HERE, lib=os.path.join(EMU_DIR, "libsuffix_emu.so")))
    env = dict(os.environ, SFX_LCE_FAN=fan, SFX_MAX_GRID="3", SFX_PARTITION_MIN="1000", SFX_LCE_VARIANT=variant)
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-2000:], r.stderr[-4000:])
