"""CPU tests of the maximal exact matches of a query text (sfx_mems_dev, sfx_index_mems*, sfx_gindex_mems*): the
product's kernels compiled against the fiber emulator (tests/emu), checked against the definition as a plain double loop,
by the serial checker tests/mem_check.c and by the two pair-count identities.  The cases are tests/_mem.py's, shared with
test_gpu_mem.py."""
import os
import re
import subprocess
import sys

import pytest

import _mem as E
from suffix_amd import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "emu")


@pytest.fixture(scope="module")
def emu():
    return Engine(E.build_emulator())


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return E.build_checker(tmp_path_factory.mktemp("mem_check"))


def test_brute_force_on_hand_worked_cases():
    for text, query, L, unique, want in E.HAND:
        assert E.brute(text, query, L, unique=unique) == want, (text, query, L, unique)
    assert E.run_closed_form(3, 2, 1) == E.brute(b"aaa", b"aa", 1)
    assert E.run_closed_form(7, 9, 2) == E.brute(b"a" * 7, b"a" * 9, 2)
    assert E.run_closed_form(7, 9, 2, True) == E.brute(b"a" * 7, b"a" * 9, 2, unique=True)
    assert E.run_closed_form(9, 4, 3, True) == E.brute(b"a" * 9, b"a" * 4, 3, unique=True) == []


def test_checker_names_faults(checker):
    assert E.checker_self_test(checker) >= 6


def test_known_answers(emu):
    E.known_answers(emu, "cpu")


def test_small_random_pairs_vs_brute_force(emu, checker):
    assert E.small_random_pairs(emu, "cpu", checker) >= 150


def test_small_random_collections_vs_brute_force(emu, checker):
    assert E.small_random_collections(emu, "cpu", checker) >= 60


def test_edges(emu, checker, oracle):
    E.edges(emu, "cpu", checker, oracle)


def test_runs_at_the_real_tile_size(emu):
    """K = 2048 on the emulator: among the shapes a tile of 2048 single-pair positions, eight times the threads."""
    E.runs(emu, "cpu", E.TILE, routes=("dev",))


def test_buffers_and_streams(emu, checker, oracle):
    E.buffers_and_streams(emu, "cpu", checker, oracle)


def test_refusals(emu, oracle):
    E.refusals(emu, "cpu", oracle)


def test_workspace_bound(emu):
    E.workspace_bound(emu)


def test_launch_names(emu, oracle):
    E.launch_names(emu, "cpu", oracle)


def test_every_mem_kernel_maps_to_its_launch_name():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import pmc_summary
    src = open(os.path.join(ROOT, "suffix_amd", "csrc", "sfx_mem.hip")).read()
    kernels = set(re.findall(r"__global__[^;{]*?\b(k_mem_[a-z0-9_]+)\s*\(", src, flags=re.S))
    launches = dict(re.findall(r'SFX_LAUNCH\("([a-z_]+)",[^;]*?\b(k_mem_[a-z0-9_]+)(?:<[a-z]+>)?,', src, flags=re.S))
    assert len(kernels) == 3 and set(launches.values()) == kernels, (sorted(kernels), launches)
    for name, k in launches.items():
        assert name.startswith("mem_")
        assert pmc_summary.profile_name(f"void sfx::{k}(sfx::MemIn, ...)") == name, k


SCRIPT = """
import sys
sys.path[:0] = [{root!r}, {here!r}]
import oracle
import _mem as E
from suffix_amd import Engine
oracle.build()
eng = Engine({lib!r})
E.runs(eng, "cpu", 8)
E.known_answers(eng, "cpu")
chk = E.build_checker({tmp!r})
E.small_random_pairs(eng, "cpu", chk, iters=40)
E.small_random_collections(eng, "cpu", chk, iters=20)
E.edges(eng, "cpu", chk, oracle)
print("OK")
"""


@pytest.mark.parametrize("bisect", ["0", "1"])
def test_small_tiles_in_a_hooked_process(emu, tmp_path, bisect):
    """SFX_MEM_TILE=8 SFX_MAX_GRID=3 (read once per process): tiles of 8 pairs, more tiles than workgroups, positions that
    span many tiles; once more with every slot bisecting for its position (SFX_MEM_BISECT=1, the measured baseline)."""
    script = tmp_path / "small_tiles.py"
    script.write_text(SCRIPT.format(root=ROOT, here=HERE, lib=os.path.join(EMU_DIR, "libsuffix_emu.so"), tmp=str(tmp_path)))
    env = dict(os.environ, SFX_MEM_TILE="8", SFX_MAX_GRID="3", SFX_MEM_BISECT=bisect)
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-2000:], r.stderr[-4000:])
