"""CPU tests of the matching statistics of a query text (sfx_match_stats_dev, sfx_index_match_stats*,
sfx_gindex_match_stats*): the product's kernels compiled against the fiber emulator (tests/emu), checked against the
definition by brute force and by the serial checker tests/ms_check.c.  The cases are tests/_match.py's, shared with
test_gpu_match.py."""
import os
import subprocess

import pytest

import _match as M
from suffix_amd import Engine

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU_DIR])
    return Engine(os.path.join(EMU_DIR, "libsuffix_emu.so"))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return M.build_checker(tmp_path_factory.mktemp("ms_check"))


def test_known_answer(emu, checker):
    M.known_answer(emu, "cpu", checker)


def test_small_random_pairs_vs_brute_force(emu, checker):
    # the checker's self-test rides along: a checker that accepts everything cannot pass
    assert M.small_random_pairs(emu, "cpu", checker) >= 150


def test_small_random_collections_vs_brute_force(emu, checker):
    assert M.small_random_collections(emu, "cpu", checker) >= 60


def test_edges(emu, checker, oracle):
    M.edges(emu, "cpu", checker, oracle)


def test_directory_texts(emu, checker, oracle):
    M.directory_texts(emu, "cpu", checker, oracle)


def test_buffers_and_streams(emu, checker, oracle):
    M.buffers_and_streams(emu, "cpu", checker, oracle)


def test_index_route_threshold_and_launch_names(emu, checker, oracle):
    M.index_route_threshold(emu, "cpu", checker, oracle)
