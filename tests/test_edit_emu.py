"""CPU tests of the k-error pattern search (sfx_edit_dev, sfx_index_edit*, sfx_gindex_edit*): the product's kernels
compiled against the fiber emulator (tests/emu), checked against Sellers' recurrence (tests/_edit.py: brute) and by the
serial checker tests/ed_check.c.  The cases are tests/_edit.py's, shared with test_gpu_edit.py."""
import os
import re
import subprocess
import sys

import pytest

import _edit as E
from suffix_amd import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "emu")


@pytest.fixture(scope="module")
def emu():
    return Engine(E.build_emulator())


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return E.build_checker(tmp_path_factory.mktemp("ed_check"))


def test_brute_force_on_hand_worked_cases():
    E.hand_worked()
    assert E.ed(b"kitten", b"sitting") == 3 and E.ed(b"", b"abc") == 3 and E.ed(b"abc", b"abc") == 0
    # the recurrence against the definition itself: every end, the least distance over all begins, the largest begin
    for text, starts, pats, k in E.HAND:
        got, first = E.brute(text, starts, pats, k)
        want = []
        for j, p in enumerate(pats):
            for lo, hi in E._documents(len(text), starts):
                for e in range(lo, hi + 1):
                    d, s = min((E.ed(p, text[s:e]), -s) for s in range(lo, e + 1))
                    if d <= k:
                        want.append((j, -s, e, d))
        assert got == sorted(want, key=lambda x: (x[0], x[2])) and first[-1] == len(want), (text, pats, k)


def test_checker_names_faults(checker):
    assert E.checker_self_test(checker) >= 8


def test_known_answers(emu):
    E.known_answers(emu, "cpu")


def test_small_random_texts_vs_brute_force(emu, checker):
    assert E.small_random_texts(emu, "cpu", checker) >= 150


def test_small_random_collections_vs_brute_force(emu, checker):
    assert E.small_random_collections(emu, "cpu", checker) >= 60


def test_edges(emu, checker, oracle):
    E.edges(emu, "cpu", checker, oracle)


def test_closed_forms_around_the_real_tile_size(emu):
    """K = 2048 on the emulator: the candidates of a^32 at k = 1, 2 (n - 15), lie just below, at and above one and two tiles."""
    E.closed_forms(emu, "cpu", (1039, 1040, 2047, 2048 + 17), routes=("dev", "index_dev"))


def test_buffers_and_streams(emu, checker, oracle):
    E.buffers_and_streams(emu, "cpu", checker, oracle)


def test_refusals(emu, oracle):
    E.refusals(emu, "cpu", oracle)


def test_foreign_table_stays_in_bounds(emu):
    E.foreign_table(emu, "cpu")


def test_workspace_bound(emu):
    E.workspace_bound(emu)


def test_launch_names(emu, oracle):
    E.launch_names(emu, "cpu", oracle)


def test_every_ed_kernel_maps_to_its_launch_name():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import pmc_summary
    src = open(os.path.join(ROOT, "suffix_amd", "csrc", "sfx_edit.hip")).read()
    kernels = set(re.findall(r"__global__[^;{]*?\b(k_ed_[a-z0-9_]+)\s*\(", src, flags=re.S))
    launches = dict(re.findall(r'SFX_LAUNCH\("([a-z_]+)",[^;]*?\b(k_ed_[a-z0-9_]+)(?:<[a-z]+>)?,', src, flags=re.S))
    assert len(kernels) == 7 and set(launches.values()) == kernels, (sorted(kernels), launches)
    assert set(launches) == {k for k in E.KERNELS if k.startswith("ed_")}
    for name, k in launches.items():
        assert pmc_summary.profile_name(f"void sfx::{k}(sfx::EdIn, ...)") == name, k


def test_hook_free_library_reads_no_environment():
    """The hook of this feature goes through dev_env, which a build without SFX_DEV_HOOKS compiles to nothing."""
    src = open(os.path.join(ROOT, "suffix_amd", "csrc", "sfx_edit.hip")).read()
    assert "getenv" not in src and 'dev_env("SFX_ED_TILE")' in src


SCRIPT = """
import sys
sys.path[:0] = [{root!r}, {here!r}]
import oracle
import _edit as E
from suffix_amd import Engine
oracle.build()
eng = Engine({lib!r})
E.closed_forms(eng, "cpu", (37, 40, 41, 97))
E.known_answers(eng, "cpu")
chk = E.build_checker({tmp!r})
E.small_random_texts(eng, "cpu", chk, iters=40)
E.small_random_collections(eng, "cpu", chk, iters=20)
E.edges(eng, "cpu", chk, oracle)
print("OK")
"""


@pytest.mark.parametrize("tile", ["64", "256", "5"])
def test_small_tiles_in_a_hooked_process(emu, tmp_path, tile):
    """SFX_ED_TILE=64 / 256 / 5 with SFX_MAX_GRID=3 (the grid cap is read once per process): more tiles than workgroups,
    pieces that span many tiles, tiles that hold the end of one pattern and the start of the next, and hits of one
    (pattern, end) spread over several workgroups of the merge."""
    script = tmp_path / "small_tiles.py"
    script.write_text(SCRIPT.format(root=ROOT, here=HERE, lib=os.path.join(EMU_DIR, "libsuffix_emu.so"), tmp=str(tmp_path)))
    env = dict(os.environ, SFX_ED_TILE=tile, SFX_MAX_GRID="3")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-2000:], r.stderr[-4000:])
