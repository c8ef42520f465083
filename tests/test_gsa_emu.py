"""CPU tests of the generalized suffix array (sfx_build_gsa_u32*, sfx_gindex_*): the product's kernels compiled
against the fiber emulator (tests/emu), checked against GeneralizedSuffixTable.new_naive -- the definition -- and
against naive scans of the documents."""
import contextlib
import os
import random
import subprocess

import numpy as np
import pytest

import _cases
import _gen
import _gsa
from suffix_amd import Engine, GeneralizedSuffixTable

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU_DIR])
    return Engine(os.path.join(EMU_DIR, "libsuffix_emu.so"))


@pytest.mark.parametrize("general", [False, True])
def test_random_collections_vs_definition(emu, general):
    rng = random.Random(20261016 + general)
    with _cases.general_build(emu) if general else contextlib.nullcontext():
        for _ in range(120):
            docs = _gsa.random_collection(rng)
            g = _gsa.check_against_naive(emu, docs)
            assert g.num_docs() == len(docs) and g.len() == sum(len(d) for d in docs)


def test_identical_documents_order_by_document_not_text_that_follows(emu):
    # D2's "xy" is followed by "a", D0's by "b": the plain suffix array puts D2's copy first, the GSA must not
    docs = [b"xy", b"b", b"xy", b"a", b"xy"]
    g = _gsa.check_against_naive(emu, docs)
    xy = [r for r in range(g.len()) if g.suffix_bytes(r) == b"xy"]
    assert [g.position(r) for r in xy] == [(0, 0), (2, 0), (4, 0)]
    assert g.lcp_lens()[xy[1]] == 2 and g.lcp_lens()[xy[2]] == 2
    _gsa.check_against_naive(emu, [b"\x00\xff", b"\xff", b"\x00\xff", b"\x00", b"", b"\x00\xff"])
    _gsa.check_against_naive(emu, [b"a" * 40] * 7)


def test_single_document_is_the_plain_table_and_sorts_nothing(emu):
    for text in (b"banana", _gen.dna(3000, seed=9).tobytes(), b"\x00\xff" * 500):
        names = _gsa.profile_names(emu, lambda: _gsa.single_doc_matches_plain(emu, text))
        assert "gsa_affected" in names and "gsa_fixup_sort" not in names, sorted(names)
    with _cases.general_build(emu):
        _gsa.single_doc_matches_plain(emu, _gen.english_like(5000).tobytes())


def test_duplicates_take_the_fixup_sort(emu):
    names = _gsa.profile_names(emu, lambda: _gsa.check_against_naive(emu, [b"abcab", b"zz", b"abcab", b"ab"]))
    assert {"gsa_fixup_sort", "gsa_merge", "gsa_lcp", "gsa_doc_array"} <= names, sorted(names)


@pytest.mark.parametrize("general", [False, True])
def test_collections_above_the_single_workgroup_limit(emu, general):
    rng = random.Random(77 + general)
    words = _gen.english_like(12000, seed=5).tobytes()
    docs = []
    while sum(len(d) for d in docs) < 18000:
        a = rng.randrange(len(words) - 200)
        docs.append(words[a:a + rng.randint(0, 200)])
    docs += [docs[3], docs[7][:50], docs[3]]
    rng.shuffle(docs)
    with _cases.general_build(emu) if general else contextlib.nullcontext():
        g = _gsa.check_against_naive(emu, docs)
    _gsa.check_queries(emu, g, docs, [docs[0], docs[5][10:20], b"the", b"e", b" ", b"\x00"] + _gsa.boundary_queries(docs, rng, 10))


def test_queries_vs_naive_scan(emu):
    rng = random.Random(5)
    for _ in range(40):
        docs = _gsa.random_collection(rng, max_docs=20)
        g = GeneralizedSuffixTable(docs, engine=emu)
        text = b"".join(docs)
        qs = [b"", b"z", b"\x01", text[:3]] + [d for d in docs[:3]] + _gsa.boundary_queries(docs, rng)
        for _ in range(6):
            if text:
                a = rng.randrange(len(text))
                qs.append(text[a:a + rng.randint(1, 5)])
        _gsa.check_queries(emu, g, docs, qs)


def test_cross_boundary_strings_are_not_found(emu):
    docs = ["hello", "world", "", "lower", "hell"]
    g = GeneralizedSuffixTable(docs, engine=emu)
    # the concatenation is "helloworldlowerhell": these occur only across document ends
    for q in ("owo", "dl", "rhe", "ldlo", "helloworld"):
        assert not g.contains(q) and g.positions(q) == [] and g.document_frequency(q) == 0, q
    assert g.positions("lo") == [(0, 3), (3, 0)]                          # table order: "lo" (truncated) before "lower"
    assert g.documents("l") == [0, 1, 3, 4] and g.document_frequency("l") == 4
    assert g.documents("hell") == [0, 4] and g.any_position("world") == (1, 0)
    assert g.any_position("") is None and not g.contains("") and g.positions("") == []
    assert g.document(2) == "" and g.document(1) == "world" and g.num_docs() == 5
    assert [g.suffix(r) for r in range(3)] == sorted(s for d in docs for s in (d[o:] for o in range(len(d))))[:3]


def test_error_statuses(emu):
    lib = emu.lib
    t = np.frombuffer(b"abcdef", dtype=np.uint8)
    sa, da, lcp = (np.zeros(6, dtype=np.uint32) for _ in range(3))
    P = _gsa.ptr
    ws = np.zeros(int(lib.sfx_gsa_workspace_bytes(6, 2)), dtype=np.uint8)

    def dev(starts, n=6, nd=None, wsb=None):
        s = np.asarray(starts, dtype=np.uint64)
        return lib.sfx_build_gsa_u32_dev(P(t), n, P(s), s.size if nd is None else nd, P(sa), P(da), P(lcp), P(ws),
                                         ws.size if wsb is None else wsb, None)
    assert dev([0, 3]) == 0
    assert dev([0, 4, 3]) == 1                                              # decreasing
    assert dev([1, 3]) == 1                                                 # [0] != 0
    assert dev([0, 7]) == 1                                                 # past n
    assert dev([0, 3], nd=0) == 1                                           # no documents, n > 0
    assert dev([0, 3], wsb=16) == 5                                         # workspace
    assert dev([0, 3], n=0) == 0                                            # n == 0
    assert lib.sfx_build_gsa_u32(None, 1 << 32, None, 1, None, None, None) == 2
    assert lib.sfx_build_gsa_u32(None, 0, None, 0, None, None, None) == 0
    s = np.array([0, 6, 6], dtype=np.uint64)                                # trailing empty documents are fine
    assert lib.sfx_build_gsa_u32(P(t), 6, P(s), 3, P(sa), P(da), P(lcp)) == 0
    assert sa.tolist() == list(range(6)) and not da.any()
    # the index checks its arrays: an entry outside the document DA names is refused
    import ctypes
    h = ctypes.c_void_p()
    s2 = np.array([0, 3], dtype=np.uint64)
    assert lib.sfx_build_gsa_u32(P(t), 6, P(s2), 2, P(sa), P(da), P(lcp)) == 0
    assert lib.sfx_gindex_create(P(t), 6, P(s2), 2, P(sa), P(da), ctypes.byref(h)) == 0
    lib.sfx_gindex_destroy(h)
    bad_da = da.copy()
    bad_da[0] ^= 1
    assert lib.sfx_gindex_create(P(t), 6, P(s2), 2, P(sa), P(bad_da), ctypes.byref(h)) == 1 and not h.value
    with pytest.raises(OverflowError):
        emu.check(2, "x")


def test_device_index_checks_its_query_arguments(emu):
    import torch

    from suffix_amd import device as sdev
    docs = [b"abc", b"", b"bca"]
    t = torch.frombuffer(bytearray(b"".join(docs)), dtype=torch.uint8)
    ds = torch.tensor([0, 3, 3], dtype=torch.int64)
    sa, da, _ = sdev.build_gsa(t, ds, engine=emu)
    ix = sdev.GeneralizedDeviceIndex(t, ds, sa, da, engine=emu)
    qb = torch.frombuffer(bytearray(b"bccb"), dtype=torch.uint8)          # "cb" only across documents
    s, e, f, a, nd = ix.query(qb, torch.tensor([0, 2, 4], dtype=torch.int64))
    assert (e - s).tolist() == [2, 0] and nd.tolist() == [2, 0] and f.tolist() == [1, 0]
    with pytest.raises(TypeError):
        ix.query(qb, torch.tensor([0, 2, 4], dtype=torch.int32))              # would be read as u64 offsets
    with pytest.raises(TypeError):
        ix.query(qb.to(torch.int32), torch.tensor([0, 2, 4], dtype=torch.int64))
    with pytest.raises(TypeError):
        ix.query(qb, torch.tensor([0, 9, 2, 4], dtype=torch.int64)[::2])      # not contiguous
    ix.close()


def test_every_gsa_kernel_maps_to_its_launch_name():
    """scripts/pmc_summary.py names rocprofv3 symbols by their longest listed prefix: every k_gsa_* kernel must come out
    under the name its SFX_LAUNCH uses."""
    import re
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "scripts"))
    import pmc_summary
    src = open(os.path.join(root, "suffix_amd", "csrc", "sfx_tree.hip")).read()
    kernels = set(re.findall(r"__global__[^;{]*?\b(k_gsa_[a-z0-9_]+)\s*\(", src, flags=re.S))
    launched = dict((k, name) for name, k in re.findall(r'SFX_LAUNCH\("(gsa_[a-z_]+)",[^,]*,\s*(k_gsa_[a-z0-9_]+)', src))
    assert kernels and kernels <= set(launched), sorted(kernels - set(launched))
    for k in sorted(kernels):
        sym = f"void sfx::{k}<unsigned int>(unsigned int const*)" if k.startswith("k_gsa_scan_") else f"sfx::{k}(...)"
        assert pmc_summary.profile_name(sym) == launched[k], (k, pmc_summary.profile_name(sym), launched[k])
