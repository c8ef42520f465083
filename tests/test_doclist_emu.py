"""CPU tests of the document listing (sfx_doclist_*): the product's kernels compiled against the fiber emulator
(tests/emu), checked against numpy over small collections and synthetic document arrays.  The cases are
tests/_doclist.py's, shared with test_gpu_doclist.py."""
import os
import re
import subprocess
import sys

import pytest

import _doclist as L
from suffix_amd import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "emu")


@pytest.fixture(scope="module")
def emu():
    return Engine(L.build_emulator())


def test_known_answers(emu):
    L.known_answers(emu, "cpu")


@pytest.mark.parametrize("sigma", [2, 3])
def test_small_random_collections_every_pattern_and_node(emu, sigma):
    assert L.small_random(emu, "cpu", sigma) >= 150


def test_synthetic_document_arrays(emu):
    assert L.synthetic(emu, "cpu") > 60


def test_the_profile_names_the_routes(emu):
    L.routes_are_named(emu, "cpu")


def test_list_sizes_agree_with_the_engines_document_counts(emu):
    assert L.cross_check_queries(emu, "cpu") >= 1000


def test_the_tables_handle_is_made_once(emu):
    L.the_handle_is_made_once(emu)


def test_refusals_and_limits(emu):
    L.refusals(emu, "cpu")


def test_size_formulas(emu):
    L.size_formulas(emu)


def test_dirty_workspace_offsets_streams_and_threads(emu):
    L.dirty_workspace_streams_and_threads(emu, "cpu")


def test_resources_come_back(emu):
    L.resources_come_back(emu, "cpu")


def test_every_doclist_kernel_maps_to_its_launch_name():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import pmc_summary
    src = open(os.path.join(ROOT, "suffix_amd", "csrc", "sfx_doclist.hip")).read()
    kernels = set(re.findall(r"__global__[^;{]*?\b(k_dl_[a-z0-9_]+)\s*\(", src, flags=re.S))
    launched = set(re.findall(r'SFX_LAUNCH\("(doclist_[a-z0-9_]+)"', src))
    assert launched == L.KERNELS, sorted(launched ^ L.KERNELS)
    assert {"doclist_" + k[5:] for k in kernels} == {x for x in L.KERNELS if not x.endswith("_docs")}, sorted(kernels)
    for sym, name in (("k_dl_count<true>(sfx::DlIn, unsigned long long*)", "doclist_count_docs"), ("k_dl_count<false>(sfx::DlIn)", "doclist_count"),
                      ("k_dl_emit<true>(sfx::DlIn)", "doclist_emit_docs"), ("k_dl_emit<false>(sfx::DlIn)", "doclist_emit")):
        assert pmc_summary.profile_name("void sfx::" + sym) == name, sym
    for k in sorted(kernels - {"k_dl_count", "k_dl_emit"}):
        assert pmc_summary.profile_name(f"sfx::{k}(sfx::DlView, unsigned int const*, ...)") == "doclist_" + k[5:], k


SCRIPT = """
import sys
sys.path[:0] = [{root!r}, {here!r}]
import _doclist as L
from suffix_amd import Engine
L.hooked(Engine({lib!r}), "cpu")
print("OK")
"""


@pytest.mark.parametrize("split", ["0", "1"])
def test_small_grid_and_the_two_sort_key_in_a_hooked_process(emu, tmp_path, split):
    """SFX_MAX_GRID=3 (more tiles than workgroups: the running offset crosses tiles) and SFX_DOCLIST_SPLIT=1 (the BY_TF
    key in two stable sorts, as for fields wider than 64 bits): the known, random and synthetic cases again."""
    script = tmp_path / "hooked.py"
    script.write_text(SCRIPT.format(root=ROOT, here=HERE, lib=os.path.join(EMU_DIR, "libsuffix_emu.so")))
    env = dict(os.environ, SFX_DOCLIST_SPLIT=split, SFX_MAX_GRID="3")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-2000:], r.stderr[-4000:])
