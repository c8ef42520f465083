"""CPU tests of the LZ77 factorization and its decoder (sfx_lz_parse_dev, sfx_lz_decode_dev, sfx_lz77_u32, sfx_unlz): the
product's kernels compiled against the fiber emulator (tests/emu), checked against the definition as a plain loop over a
brute-force longest-previous-factor array.  The cases are tests/_lz.py's, shared with test_gpu_lz.py."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import _lz as Z
import _repeats
from suffix_amd import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "emu")


@pytest.fixture(scope="module")
def emu():
    return Engine(Z.build_emulator())


def test_lpf_helper_vs_brute_force():
    rng = random.Random(4)
    for _ in range(150):
        t = _repeats.random_text(rng, 70)
        assert np.array_equal(Z.lpf(t), _repeats.brute_rep(t, "earlier")), t


def test_checker_names_faults(tmp_path):
    Z.checker_self_test(Z.build_checker(tmp_path), tmp_path)


def test_known_answers(emu, oracle):
    Z.known_answers(emu, "cpu", oracle)


def test_small_random_texts_every_route(emu, oracle):
    assert Z.small_random(emu, "cpu", oracle) >= 300


def test_edges(emu, oracle):
    Z.edges(emu, "cpu", oracle)


def test_refusals(emu, oracle):
    Z.refusals(emu, "cpu", oracle)


def test_unchecked_arrays_are_refused_or_parsed_by_the_definition(emu):
    Z.unchecked_parse(emu, "cpu")


def test_unchecked_phrase_lists_are_refused_or_decoded(emu):
    Z.unchecked_decode(emu, "cpu")


def test_collection_phrases_end_at_document_ends(emu):
    Z.collection(emu, "cpu")


def test_launch_names(emu, oracle):
    Z.launch_names(emu, "cpu", oracle)


def test_every_lz_kernel_maps_to_its_launch_name():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import pmc_summary
    src = open(os.path.join(ROOT, "suffix_amd", "csrc", "sfx_lz.hip")).read()
    kernels = set(re.findall(r"__global__[^;{]*?\b(k_lz_[a-z0-9_]+)\s*\(", src, flags=re.S))
    launches = dict(re.findall(r'SFX_LAUNCH\("([a-z_]+)",[^;]*?\b(k_lz_[a-z0-9_]+),', src, flags=re.S))
    assert len(kernels) == 10 and set(launches.values()) == kernels, (sorted(kernels), launches)
    for name, k in launches.items():
        assert name.startswith(("lz_", "unlz_"))
        assert pmc_summary.profile_name(f"void sfx::{k}(unsigned int const*, ...)") == name, k


SCRIPT = """
import sys
sys.path[:0] = [{root!r}, {here!r}]
import oracle
import _lz as Z
from suffix_amd import Engine
oracle.build()
Z.small_tiles(Engine({lib!r}), "cpu", oracle)
print("OK")
"""


def test_small_tiles_in_a_hooked_process(emu, tmp_path):
    """SFX_LZ_TILE=8 SFX_LZ_LEVELS=2 SFX_MAX_GRID=3 SFX_LZ_ROUNDS_CHECK=1 (read once per process): tiles of 8 positions,
    groups of 32, more tiles than workgroups, the decoder's flag read back every round."""
    script = tmp_path / "small_tiles.py"
    script.write_text(SCRIPT.format(root=ROOT, here=HERE, lib=os.path.join(EMU_DIR, "libsuffix_emu.so")))
    env = dict(os.environ, SFX_LZ_TILE="8", SFX_LZ_LEVELS="2", SFX_MAX_GRID="3", SFX_LZ_ROUNDS_CHECK="1")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-2000:], r.stderr[-4000:])
