"""CPU tests of the GSA merge (sfx_gsa_merge_dev / _u32, sfx_gsa_extend_u32, GeneralizedSuffixTable.extend / merge): the
product's kernels compiled against the fiber emulator (tests/emu), checked against the definition
(GeneralizedSuffixTable.new_naive) and the one-shot build.  The cases are tests/_gsamerge.py's, shared with
test_gpu_gsamerge.py."""
import os
import re
import subprocess
import sys

import pytest

import _gsamerge as M
from suffix_amd import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "emu")


@pytest.fixture(scope="module")
def emu():
    return Engine(M.build_emulator())


def test_known_answer_through_every_entry_point(emu):
    M.known_answer(emu, "cpu")


def test_300_random_collections_at_every_split_vs_the_definition(emu):
    assert M.random_splits(emu, "cpu") >= 900


def test_ties_and_prefixes(emu):
    M.ties_and_prefixes(emu, "cpu")


def test_sizes_around_the_scatter_tile(emu):
    assert M.tile_sizes(emu, "cpu") == 25


def test_alternation_and_whole_tiles_of_one_side(emu):
    M.tile_patterns(emu, "cpu")


def test_three_extends_equal_one_build(emu):
    M.chaining(emu)


def test_match_limit_below_at_and_above_the_longest_match(emu):
    M.match_limits(emu, "cpu")


def test_refusals(emu):
    M.refusals(emu, "cpu")


def test_garbage_stays_inside_the_guard_bands(emu):
    M.garbage(emu, "cpu")


def test_offsets_dirty_workspace_streams_and_threads(emu):
    M.buffers_streams_threads(emu, "cpu")


def test_resources_come_back(emu):
    M.resources_come_back(emu, "cpu")


def test_launch_names(emu):
    M.launch_names(emu, "cpu")


def test_every_gm_kernel_maps_to_its_launch_name():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import pmc_summary
    src = open(os.path.join(ROOT, "suffix_amd", "csrc", "sfx_gsamerge.hip")).read()
    kernels = set(re.findall(r"__global__[^;{]*?\b(k_gm_[a-z0-9_]+)\s*\(", src, flags=re.S))
    launches = re.findall(r'SFX_LAUNCH\("([a-z_]+)",[^;]*?\b(k_gm_[a-z0-9_]+),', src, flags=re.S)
    assert len(kernels) == 4 and {k for _, k in launches} == kernels, (sorted(kernels), launches)
    assert {name for name, _ in launches} == M.KERNELS
    for name, k in launches:
        assert pmc_summary.profile_name(f"void sfx::{k}(sfx::GmIn, ...)") == name, k


def test_hook_free_library_reads_no_environment():
    """The hook of this feature goes through dev_env, which a build without SFX_DEV_HOOKS compiles to nothing."""
    M.hook_goes_through_dev_env()


SCRIPT = """
import sys
sys.path[:0] = [{root!r}, {here!r}]
import _gsamerge as M
from suffix_amd import Engine
M.hooked(Engine({lib!r}), "cpu")
print("OK")
"""


@pytest.mark.parametrize("tile", ["64", "256", "5"])
def test_small_tiles_in_a_hooked_process(emu, tmp_path, tile):
    """SFX_GM_TILE=64 / 256 / 5 with SFX_MAX_GRID=3 (the grid cap is read once per process): more tiles than workgroups, so
    a workgroup's LDS marks are cleared and reused, and tiles of new entries only, old ones only and every mixture."""
    script = tmp_path / "small_tiles.py"
    script.write_text(SCRIPT.format(root=ROOT, here=HERE, lib=os.path.join(EMU_DIR, "libsuffix_emu.so")))
    env = dict(os.environ, SFX_GM_TILE=tile, SFX_MAX_GRID="3")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-2000:], r.stderr[-4000:])
