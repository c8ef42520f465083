"""CPU tests of the k-mismatch pattern search (sfx_hamming_dev, sfx_index_hamming*, sfx_gindex_hamming*): the product's
kernels compiled against the fiber emulator (tests/emu), checked against the definition as a double loop and by the
serial checker tests/hm_check.c.  The cases are tests/_hamming.py's, shared with test_gpu_hamming.py."""
import os
import re
import subprocess
import sys

import pytest

import _hamming as H
from suffix_amd import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "emu")


@pytest.fixture(scope="module")
def emu():
    return Engine(H.build_emulator())


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return H.build_checker(tmp_path_factory.mktemp("hm_check"))


def test_brute_force_on_hand_worked_cases():
    for text, pats, k, want in H.HAND:
        assert H.brute(text, None, pats, k, H.naive_table(text))[0] == want, (text, pats, k)
    # the cut: consecutive pieces, the last one ends at m; empty pieces when m < k + 1
    assert H.cuts(32, 1) == [0, 16, 32] and H.cuts(3, 1) == [0, 1, 3] and H.cuts(2, 3) == [0, 0, 1, 1, 2] and H.cuts(10, 2) == [0, 3, 6, 10]
    # a pattern of at most k bytes occurs at every window that has room, in every document long enough
    got, first = H.brute(b"abcde", [0, 2, 2, 3], [b"zz", b"z"], 2, [0, 1, 2, 3, 4])
    assert [x[:2] for x in got] == [(0, 0), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4)] and first == [0, 2, 7]


def test_checker_names_faults(checker):
    assert H.checker_self_test(checker) >= 10


def test_known_answers(emu):
    H.known_answers(emu, "cpu")


def test_small_random_texts_vs_brute_force(emu, checker):
    assert H.small_random_texts(emu, "cpu", checker) >= 150


def test_small_random_collections_vs_brute_force(emu, checker):
    assert H.small_random_collections(emu, "cpu", checker) >= 60


def test_edges(emu, checker, oracle):
    H.edges(emu, "cpu", checker, oracle)


def test_closed_forms_around_the_real_tile_size(emu):
    """K = 2048 on the emulator: C = 2 (n - 15) lies just below, at and above one and two tiles; 2^16 bytes give 64 tiles."""
    H.closed_forms(emu, "cpu", (2047, 2048, 2049, 4096 + 17, 1 << 16), routes=("dev", "index_dev"))


def test_buffers_and_streams(emu, checker, oracle):
    H.buffers_and_streams(emu, "cpu", checker, oracle)


def test_refusals(emu, oracle):
    H.refusals(emu, "cpu", oracle)


def test_foreign_table_stays_in_bounds(emu):
    H.foreign_table(emu, "cpu")


def test_workspace_bound(emu):
    H.workspace_bound(emu)


def test_launch_names(emu, oracle):
    H.launch_names(emu, "cpu", oracle)


def test_every_hm_kernel_maps_to_its_launch_name():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import pmc_summary
    src = open(os.path.join(ROOT, "suffix_amd", "csrc", "sfx_hamming.hip")).read()
    kernels = set(re.findall(r"__global__[^;{]*?\b(k_hm_[a-z0-9_]+)\s*\(", src, flags=re.S))
    launches = dict(re.findall(r'SFX_LAUNCH\("([a-z_]+)",[^;]*?\b(k_hm_[a-z0-9_]+)(?:<[a-z]+>)?,', src, flags=re.S))
    assert len(kernels) == 6 and set(launches.values()) == kernels, (sorted(kernels), launches)
    assert set(launches) == H.KERNELS
    for name, k in launches.items():
        assert pmc_summary.profile_name(f"void sfx::{k}(sfx::HmIn, ...)") == name, k


def test_hook_free_library_reads_no_environment():
    """The hooks of this feature go through dev_env, which a build without SFX_DEV_HOOKS compiles to nothing."""
    src = open(os.path.join(ROOT, "suffix_amd", "csrc", "sfx_hamming.hip")).read()
    assert "getenv" not in src and 'dev_env("SFX_HM_TILE")' in src


SCRIPT = """
import sys
sys.path[:0] = [{root!r}, {here!r}]
import oracle
import _hamming as H
from suffix_amd import Engine
oracle.build()
eng = Engine({lib!r})
H.closed_forms(eng, "cpu", (37, 40, 41, 97))
H.known_answers(eng, "cpu")
chk = H.build_checker({tmp!r})
H.small_random_texts(eng, "cpu", chk, iters=40)
H.small_random_collections(eng, "cpu", chk, iters=20)
H.edges(eng, "cpu", chk, oracle)
print("OK")
"""


@pytest.mark.parametrize("tile", ["5", "8"])
def test_small_tiles_in_a_hooked_process(emu, tmp_path, tile):
    """SFX_HM_TILE=5 / 8 with SFX_MAX_GRID=3 (the grid cap is read once per process): tiles of a few candidates, more tiles
    than workgroups, pieces that span many tiles, tiles that hold the end of one pattern and the start of the next."""
    script = tmp_path / "small_tiles.py"
    script.write_text(SCRIPT.format(root=ROOT, here=HERE, lib=os.path.join(EMU_DIR, "libsuffix_emu.so"), tmp=str(tmp_path)))
    env = dict(os.environ, SFX_HM_TILE=tile, SFX_MAX_GRID="3")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-2000:], r.stderr[-4000:])
