"""CPU tests of the Burrows-Wheeler transform with sampled ranks and of its inverse (sfx_bwt_dev, sfx_bwt_u32,
sfx_unbwt_dev, sfx_unbwt): the product's kernels compiled against the fiber emulator (tests/emu), checked against the
oracle's table and the definition.  The cases are tests/_bwt.py's, shared with test_gpu_bwt.py."""
import os
import subprocess
import sys

import pytest

import _bwt as B
from suffix_amd import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "emu")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU_DIR])
    return Engine(os.path.join(EMU_DIR, "libsuffix_emu.so"))


def test_known_answers(emu, oracle):
    B.known_answers(emu, "cpu", oracle)


def test_definition_restates_the_known_answers(oracle):
    for text, s, b, sm in B.KNOWN:
        wb, ws = B.definition(text, B.table_of(oracle, text), s)
        assert wb.tobytes() == b and ws.tolist() == sm


def test_small_random_texts_vs_definition(emu, oracle):
    assert B.small_random(emu, "cpu", oracle) >= 300


def test_edges(emu, oracle):
    B.edges(emu, "cpu", oracle)


def test_refusals(emu, oracle):
    B.refusals(emu, "cpu", oracle)


def test_integrity_of_mutated_pairs(emu, oracle):
    B.integrity(emu, "cpu", oracle)


def test_unchecked_tables_stay_in_bounds(emu, oracle):
    B.bad_tables(emu, "cpu", oracle)


def test_launch_names(emu, oracle):
    B.launch_names(emu, "cpu", oracle)


SCRIPT = """
import sys
sys.path[:0] = [{root!r}, {here!r}]
import oracle
import _bwt as B
from suffix_amd import Engine
oracle.build()
B.small_tiles(Engine({lib!r}), "cpu", oracle)
print("OK")
"""


def test_small_tiles_in_a_hooked_process(emu, tmp_path):
    """SFX_BWT_TILE=256 SFX_MAX_GRID=3 (read once per process): a workgroup ranks several tiles, a scan chunk holds
    several tiles, and the last tile is partial."""
    script = tmp_path / "small_tiles.py"
    script.write_text(SCRIPT.format(root=ROOT, here=HERE, lib=os.path.join(EMU_DIR, "libsuffix_emu.so")))
    env = dict(os.environ, SFX_BWT_TILE="256", SFX_MAX_GRID="3")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-2000:], r.stderr[-4000:])
