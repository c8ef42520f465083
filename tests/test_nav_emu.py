"""CPU tests of the suffix-tree navigation calls (sfx_lce_substr*, sfx_lce_lca*, sfx_lce_range_argmin*, sfx_suffix_links_*):
the product's kernels compiled against the fiber emulator (tests/emu), checked against brute force over the sorted
suffixes and the serial checker tests/nav_check.c.  The cases are tests/_nav.py's, shared with test_gpu_nav.py."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import _gen
import _lce as L
import _nav as N
import _tree
from suffix_amd import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def emu():
    return Engine(N.build_emulator())


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    return N.build_checker(tmp_path_factory.mktemp("nav_check"))


def test_checker_names_one_fault_per_mode(chk, oracle):
    N.checker_self_test(chk, oracle)


def test_known_answers(emu, oracle):
    N.known_answers(emu, "cpu", oracle)


def test_the_tables_handle_serves_the_new_calls(emu, oracle):
    N.handle_is_made_once(emu, oracle)


def test_small_random_texts_vs_brute(emu, oracle):
    assert N.small_random(emu, "cpu", oracle) >= 150


def test_small_random_collections_vs_brute(emu, oracle):
    assert N.small_collections(emu, "cpu", oracle) >= 60


def test_sizes_at_the_level_edges(emu):
    N.level_edges(emu, "cpu")


def test_unary_text_in_closed_form(emu, oracle):
    N.unary(emu, "cpu", oracle)


def test_edge_texts(emu, oracle):
    N.edge_texts(emu, "cpu", oracle)


def test_refusals(emu, oracle):
    N.refusals(emu, "cpu", oracle)
    N.workspace_bound(emu)


def test_corrupted_arrays_stay_in_bounds(emu, oracle):
    N.corrupted(emu, "cpu", oracle)


def test_dirty_workspaces_of_the_stated_size(emu, oracle):
    N.dirty_workspaces(emu, "cpu", oracle)


def test_streams_and_threads(emu, oracle):
    N.streams_and_threads(emu, "cpu", oracle)


def test_launch_names(emu, oracle):
    N.launch_names(emu, "cpu", oracle)


def test_every_nav_kernel_maps_to_its_launch_name():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import pmc_summary
    src = open(os.path.join(ROOT, "suffix_amd", "csrc", "sfx_nav.hip")).read()
    kernels = set(re.findall(r"__global__[^;{]*?\b(k_[a-z0-9_]+)\s*\(", src, flags=re.S))
    assert kernels == {"k_" + k for k in N.KERNELS}, sorted(kernels)
    for k in sorted(kernels):
        assert pmc_summary.profile_name(f"sfx::{k}(sfx::LceView, unsigned int const*, ...)") == k[2:], k


def test_checker_agrees_with_brute_on_a_larger_text(emu, oracle, chk):
    """Both known answers on one input: the engine's answers pass the checker and equal brute force."""
    text = _gen.near_duplicates(5000).tobytes()
    n = len(text)
    sa, lcp = L.tables(oracle, text)
    rng = random.Random(5)
    N.check_text(emu, "cpu", oracle, text, sa, lcp, rng=rng, limit=200)
    c = N.Checker(chk, sa, lcp)
    lx = N.Nx(emu, "cpu", sa, lcp)
    pos, ln = N.scale_queries(n, sa, lcp, 3000, seed=6)
    N.accept(c.substr(pos, ln, *lx.substr(pos, ln)), "substr", pos, ln)
    a, b = L.pair_list(n, rng, 2000)
    N.accept(c.lca(a, b, *lx.lca(a, b)), "lca", a, b)
    lo, hi = L.edge_ranges(n, rng)
    N.accept(c.argmin(lo, hi, lx.argmin(lo, hi)), "argmin", lo, hi)
    nodes = _tree.tree_u32(emu, text, sa, lcp)
    rc, sl = N.links_raw(emu, "cpu", lx, sa, nodes)
    assert rc == 0
    N.accept(c.slink(nodes["node_lb"], nodes["node_rb"], nodes["node_depth"], sl), "slink", nodes["node_lb"], nodes["node_depth"], sl)
    assert np.array_equal(sl, N.brute_slinks(text, sa.tolist(), nodes))
    lx.close()
    c.close()


SCRIPT = """
import sys
sys.path[:0] = [{root!r}, {here!r}]
import oracle
import _nav as N
from suffix_amd import Engine
oracle.build()
N.hooked(Engine({lib!r}), "cpu", oracle)
print("OK")
"""


@pytest.mark.parametrize("fan", ["2", "4"])
def test_deep_trees_in_a_hooked_process(emu, tmp_path, fan):
    """SFX_LCE_FAN=2 / 4 (a few thousand entries have 6 to 12 levels) and SFX_MAX_GRID=3 (more queries than the grid
    holds): the random and edge cases again."""
    script = tmp_path / "hooked.py"
    script.write_text(SCRIPT.format(root=ROOT, here=HERE, lib=os.path.join(L.EMU_DIR, "libsuffix_emu.so")))
    env = dict(os.environ, SFX_LCE_FAN=fan, SFX_MAX_GRID="3")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-2000:], r.stderr[-4000:])
