"""CPU run of tests/_buffers.py: the `*_dev` entry points of the emulator build (the product's .hip sources compiled
unchanged against tests/emu) over offset, dirty and guarded buffers, at sizes a fiber emulator can afford -- every offset
and every fill pattern of the GPU run (test_gpu_buffers.py) kept.  The same cases run under the emulator's AddressSanitizer
build by hand (SUFFIX_EMU_LIB=<path of that build's libsuffix_emu.so>, with the sanitizer's runtime preloaded as
tests/asan_check.py describes), where a guard band is not needed to see an overrun."""
import os
import subprocess

import numpy as np
import pytest

import _buffers
import _cases
import _gen
from suffix_amd import Engine

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU_DIR])
    return Engine(os.environ.get("SUFFIX_EMU_LIB") or os.path.join(EMU_DIR, "libsuffix_emu.so"))


def test_guard_helper_sees_a_damaged_byte_and_names_it():
    g = _buffers.guarded(100, "cpu", offset=3, fill="count")
    assert (g.raw.data_ptr() + g.begin - 3) % 256 == 0 and g.host().tolist() == [i % 256 for i in range(100)]
    g.check_guards()
    g.raw[g.begin + 100 + 17] ^= 1
    with pytest.raises(AssertionError, match=r"behind the array .*byte \+117 from"):
        g.check_guards()
    g.raw[g.begin + 100 + 17] ^= 1
    g.raw[g.begin - 1] = 0
    with pytest.raises(AssertionError, match=r"in front of the array .*byte -1 from"):
        g.check_guards()


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 31, 4097, 16384])
def test_one_workgroup_build_offsets_and_dirt(emu, oracle, n):
    """The 16-byte LDS fill of sfx_tiny.hip and its `i + 16 <= n` edge, for aligned and unaligned texts."""
    text = _gen.dna(n, seed=40 + n).tobytes() if n != 4097 else _gen.english_like(n).tobytes()
    which = _buffers.combos(always=[(0, 0, 0xFF)]) if n < 4097 else [(0, 0, 0xFF)] + _buffers.combos()[:4]
    _buffers.build_sa_case(emu, oracle, text, "cpu", which=which)
    emu.profile(True); emu.profile_reset()
    _buffers.build_sa_case(emu, oracle, text, "cpu", which=[(3, 4, "count")])
    names = {r["name"] for r in emu.profile_report()}
    emu.profile(False)
    assert ("tiny_sa" in names) == (n >= 2), sorted(names)


@pytest.mark.parametrize("n", [17, 4097, 16385])
def test_general_build_offsets_and_dirt(emu, oracle, n):
    """The general build on texts of every packing (1, 2, 2, 4, 7, 8 bits): an unaligned text takes the LDS-staged pack
    kernel, the byte path of the presence scan, and still gives the oracle's table."""
    with _cases.general_build(emu):
        for i, (name, text) in enumerate(_buffers.alphabets(n)):
            which = _buffers.combos() if n == 4097 else [_buffers.combos()[(i + k) % 6] for k in range(2)]
            _buffers.build_sa_case(emu, oracle, text, "cpu", which=which)


def test_general_build_count_histogram_unaligned(emu, oracle):
    """70 001 bytes, more than 16 symbols: the count histogram (head up to the first 16-byte boundary, vectors, tail) and,
    for the UTF-8 text, the bigram counts of the context codes' pilot, on texts at +1 / +15."""
    for i, text in enumerate((_gen.english_like(70_001).tobytes(), _gen.utf8_mixed(70_001).tobytes())):
        emu.profile(True); emu.profile_reset()
        _buffers.build_sa_case(emu, oracle, text, "cpu", which=[((1, 15)[i], (4, 12)[i], ("count", 0xFF)[i])])
        names = {r["name"] for r in emu.profile_report()}
        emu.profile(False)
        assert "byte_hist" in names and "tiny_sa" not in names, sorted(names)


@pytest.mark.parametrize("n", [4096, 4097, 4103])                       # n mod 8 = 0, 1, 7
def test_lcp_offsets_and_dirt(emu, oracle, n):
    with _cases.general_build(emu):
        _buffers.lcp_case(emu, oracle, _gen.dna(n, seed=n).tobytes(), "cpu")
    _buffers.lcp_case(emu, oracle, _gen.english_like(n).tobytes(), "cpu")


def test_lcp_pending_pairs_at_every_offset(emu, oracle):
    emu.profile(True); emu.profile_reset()
    with _cases.general_build(emu):
        for text in _buffers.repeat_rich(80):
            _buffers.lcp_case(emu, oracle, text, "cpu")
    names = {r["name"] for r in emu.profile_report()}
    emu.profile(False)
    assert "lcp_pending" in names, sorted(names)                      # (pending pairs existed, and the aligned calls fused)


def test_queries_index_and_slices(emu, oracle):
    rng = np.random.default_rng(5)
    for text in (_gen.dna(3000, seed=5).tobytes() + b"AAAA", _gen.english_like(2500).tobytes(),
                 b"\xff" * 40 + b"\x00" * 40 + b"\xff" * 17 + b"\x00" * 9 + b"\xff" * 16 + b"\x00" * 25 + b"\xff" * 24):
        _buffers.query_case(emu, oracle, text, _cases.directory_query_list(text, rng, random_count=60), "cpu")


def test_suffix_tree_doc_lookup_widen(emu, oracle):
    for text in (b"banana", _gen.dna(2000, seed=3).tobytes(), b"ab" * 300 + b"a", _gen.english_like(1501).tobytes()):
        _buffers.intervals_case(emu, oracle, text, "cpu")
    _buffers.doc_lookup_case(emu, "cpu")
    _buffers.widen_case(emu, "cpu")


def test_generalized_build_and_index(emu):
    _buffers.gsa_cases(emu, "cpu", iters=4)


def test_repeat_lens_and_spans(emu, oracle):
    _buffers.repeats_cases(emu, oracle, "cpu", iters=4)


def test_range_build_unaligned_text(emu, oracle):
    _buffers.range_case(emu, oracle, _gen.dna(3001, seed=8).tobytes(), "cpu")
    _buffers.range_case(emu, oracle, _gen.english_like(2503).tobytes(), "cpu", nranges=2)


def test_refusals_leave_everything_untouched(emu, oracle):
    _buffers.refusals(emu, oracle, "cpu")
