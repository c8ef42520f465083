"""CPU tests of the repeat-length arrays and repeated-span reports (sfx_repeat_lens_*, sfx_repeat_spans_*): the product's
kernels compiled against the fiber emulator (tests/emu), checked against the definition by brute force, against the serial
sweeps of tests/rep_check.c, and against a span reference that uses another method than the engine (tests/_repeats.py)."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import _gen
import _gsa
import _repeats as R
from suffix_amd import Engine, GeneralizedSuffixTable, SuffixTable

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU_DIR])
    return Engine(os.path.join(EMU_DIR, "libsuffix_emu.so"))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return R.build_checker(tmp_path_factory.mktemp("rep_check"))


def _plain(emu, text):
    st, lcp = SuffixTable.new_with_lcp(text, engine=emu)
    return st.table(), lcp


def test_banana(emu):
    sa, lcp = _plain(emu, b"banana")
    rep, src = R.repeat_lens(emu, sa, lcp, "any")
    assert rep.tolist() == [0, 3, 2, 3, 2, 1]
    assert R.repeat_spans(emu, rep, 2) == ([(1, 6)], 1)
    rep, src = R.repeat_lens(emu, sa, lcp, "earlier")
    assert rep.tolist() == [0, 0, 0, 3, 2, 1] and src.tolist()[:5] == [R.NONE, R.NONE, R.NONE, 1, 2] and src[5] in (1, 3)
    assert R.repeat_spans(emu, rep, 2) == ([(3, 6)], 1)
    assert R.repeat_spans(emu, rep, 4) == ([], 0)
    st = SuffixTable("banana", engine=emu)
    assert st.repeat_lens().tolist() == [0, 3, 2, 3, 2, 1] and st.repeated_spans(2) == [(1, 6)]
    assert st.repeat_lens("earlier").tolist() == [0, 0, 0, 3, 2, 1] and st.repeated_spans(2, "earlier") == [(3, 6)]
    rep, src = st.repeat_lens("earlier", with_source=True)
    R.check_witnesses(b"banana", "earlier", rep, src)
    with pytest.raises(ValueError):
        st.repeat_lens("other_doc")
    with pytest.raises(ValueError):
        st.repeated_spans(0)


def test_random_texts_vs_brute_force(emu):
    rng = random.Random(20261017)
    for _ in range(200):
        text = R.random_text(rng)
        sa, lcp = _plain(emu, text)
        R.check_small(emu, text, sa, lcp, ("any", "earlier"))


def test_random_collections_vs_brute_force(emu):
    rng = random.Random(20261018)
    done = 0
    while done < 120:
        docs = _gsa.random_collection(rng, max_docs=12, max_len=14)
        text = b"".join(docs)
        if len(text) > 80:
            continue
        done += 1
        g = GeneralizedSuffixTable(docs, engine=emu)
        starts = _gsa.doc_starts(docs)
        R.check_small(emu, text, g.table(), g.lcp_lens(), ("any", "earlier", "other_doc"), starts=starts, da=g.doc_array())
        # the host-side mirror: (document, begin, end) triples of the same runs
        rep = g.repeat_lens("other_doc")
        exp = R.span_reference(rep, 2, starts)
        d = R.doc_of(starts, max(len(text), 1))
        assert g.repeated_spans(2, "other_doc") == [(int(d[b]), b - int(starts[d[b]]), e - int(starts[d[b]])) for b, e in exp]


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097])
def test_edge_sizes(emu, checker, tmp_path, n):
    """The pyramid fan, the fan squared and the LDS tile, each with a neighbour on either side: every scope against the
    serial sweeps, spans against the reference."""
    text = np.random.default_rng(n).integers(97, 100, n, dtype=np.uint8).tobytes()
    sa, lcp = _plain(emu, text)
    for scope in ("any", "earlier"):
        rep, src = R.repeat_lens(emu, sa, lcp, scope)
        assert R.run_checker(checker, tmp_path, text, [], sa, lcp, None, scope, rep, src).startswith("ok"), scope
        for m in (1, 3, 7):
            assert R.repeat_spans(emu, rep, m)[0] == R.span_reference(rep, m)
    cuts = sorted([0, n // 3, n // 3, (2 * n) // 3, n - n // 64]) if n else [0]          # (an empty document among them)
    docs = [text[a:b] for a, b in zip(cuts, cuts[1:] + [n])]
    g = GeneralizedSuffixTable(docs, engine=emu)
    starts = _gsa.doc_starts(docs)
    for scope in ("any", "earlier", "other_doc"):
        rep, src = R.repeat_lens(emu, g.table(), g.lcp_lens(), scope, da=g.doc_array())
        out = R.run_checker(checker, tmp_path, text, starts, g.table(), g.lcp_lens(), g.doc_array(), scope, rep, src)
        assert out.startswith("ok"), (scope, out)
        for m in (1, 3):
            assert R.repeat_spans(emu, rep, m, starts)[0] == R.span_reference(rep, m, starts)


def test_unary_text_has_no_earlier_rank_below(emu):
    """"a" x 5000: the suffix array is descending, so no rank has an earlier position at a lower rank, and every search to
    the left leaves its tile for the global pyramid to report "none"."""
    for n in (5000, 7000):                                   # (7000: more such ranks than the list of open searches holds)
        sa, lcp = _plain(emu, b"a" * n)
        assert sa.tolist() == list(range(n - 1, -1, -1))
        rep, src = R.repeat_lens(emu, sa, lcp, "earlier")
        assert rep[0] == 0 and src[0] == R.NONE
        assert np.array_equal(rep[1:], n - np.arange(1, n)) and (src[1:] < np.arange(1, n)).all()      # (every earlier position is a witness)
        rep, _ = R.repeat_lens(emu, sa, lcp, "any")
        assert np.array_equal(rep, np.minimum(n - np.arange(n), n - 1))
        assert R.repeat_spans(emu, rep, 8) == ([(0, n)], 1)

def test_doubled_text_spans_cross_many_scan_chunks(emu, checker, tmp_path):
    r = np.random.default_rng(5).integers(0, 256, 9000, dtype=np.uint8).tobytes()
    text = r + r
    sa, lcp = _plain(emu, text)
    rep, src = R.repeat_lens(emu, sa, lcp, "earlier")
    assert R.run_checker(checker, tmp_path, text, [], sa, lcp, None, "earlier", rep, src).startswith("ok")
    assert R.repeat_spans(emu, rep, 8) == ([(9000, 18000)], 1)
    rep, src = R.repeat_lens(emu, sa, lcp, "any")
    assert R.run_checker(checker, tmp_path, text, [], sa, lcp, None, "any", rep, src).startswith("ok")
    assert R.repeat_spans(emu, rep, 8) == ([(0, 18000)], 1)


def test_identical_documents_in_other_doc_scope(emu):
    d = _gen.english_like(700, seed=3).tobytes()
    g = GeneralizedSuffixTable([d, d], engine=emu)
    rep, src = R.repeat_lens(emu, g.table(), g.lcp_lens(), "other_doc", da=g.doc_array())
    assert np.array_equal(rep, np.tile(700 - np.arange(700), 2))
    R.check_witnesses(d + d, "other_doc", rep, src, [0, 700])
    assert R.repeat_spans(emu, rep, 5) == ([(0, 1400)], 1)
    assert R.repeat_spans(emu, rep, 5, [0, 700]) == ([(0, 700), (700, 1400)], 2)
    assert g.repeated_spans(5, "other_doc") == [(0, 0, 700), (1, 0, 700)]


def test_single_document_in_other_doc_scope_runs_no_search(emu):
    text = _gen.english_like(3000, seed=4).tobytes()
    g = GeneralizedSuffixTable([text], engine=emu)
    out = {}
    names = _gsa.profile_names(emu, lambda: out.update(r=R.repeat_lens(emu, g.table(), g.lcp_lens(), "other_doc", da=g.doc_array())))
    rep, src = out["r"]
    assert not rep.any() and (src == R.NONE).all()
    assert "rep_doc_runs" in names and not names & {"rep_other_doc", "rep_pyramid", "rep_earlier", "rep_earlier_open"}, sorted(names)
    assert R.repeat_spans(emu, rep, 1) == ([], 0)
    # (with two documents the search kernel does run)
    g2 = GeneralizedSuffixTable([text[:1500], text[1500:]], engine=emu)
    names = _gsa.profile_names(emu, lambda: R.repeat_lens(emu, g2.table(), g2.lcp_lens(), "other_doc", da=g2.doc_array()))
    assert {"rep_doc_runs", "rep_pyramid", "rep_other_doc"} <= names, sorted(names)


def test_capacity_below_the_count(emu):
    text = _gen.english_like(6000, seed=8).tobytes()
    sa, lcp = _plain(emu, text)
    rep, _ = R.repeat_lens(emu, sa, lcp, "earlier")
    exp = R.span_reference(rep, 6)
    assert len(exp) > 40
    for cap in (0, 1, 17, len(exp) - 1, len(exp), len(exp) + 5):
        got, count = R.repeat_spans(emu, rep, 6, capacity=cap)                # (checks the canary behind the capacity)
        assert count == len(exp) and got == exp[:cap], cap


def test_error_statuses(emu):
    lib = emu.lib
    P = R.ptr
    sa, lcp = _plain(emu, b"abcabcab")
    n = 8
    da = np.zeros(n, dtype=np.uint32)
    rep, src = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    ws = np.zeros(int(max(lib.sfx_repeat_lens_workspace_bytes(n, s) for s in (0, 1, 2))), dtype=np.uint8)

    def lens(scope, sa=sa, da=None, n=n, wsb=None):
        return lib.sfx_repeat_lens_dev(P(sa), P(lcp), P(da), n, scope, P(rep), P(src), P(ws), ws.size if wsb is None else wsb, None)
    assert [lens(0), lens(1), lens(2, da=da)] == [0, 0, 0]
    assert lens(3) == 1 and lens(-1) == 1                                   # unknown scope
    assert lens(2) == 1                                                     # OTHER_DOC without DA
    assert lens(1, wsb=64) == 5 and lens(2, da=da, wsb=64) == 5             # workspace
    assert lens(1, n=0) == 0 and lens(2, da=da, n=0) == 0                   # n == 0
    assert lens(0, n=1 << 32) == 2
    for bad in ([0, 1, 2, 3, 4, 5, 6, 8], [7, 7, 7, 7, 0xFFFFFFFF, 7, 7, 7]):   # an entry >= n; the second: no permutation
        b = np.array(bad, dtype=np.uint32)
        assert [lens(0, sa=b), lens(1, sa=b), lens(2, sa=b, da=np.arange(n, dtype=np.uint32))] == [1, 1, 1], bad
    dup = np.array([3, 3, 3, 0, 0, 1, 1, 1], dtype=np.uint32)                   # in range, no permutation: runs, writes in bounds
    assert [lens(0, sa=dup), lens(1, sa=dup), lens(2, sa=dup, da=da)] == [0, 0, 0]
    assert lib.sfx_repeat_lens_workspace_bytes(n, 7) == 0
    assert lib.sfx_repeat_lens_u32(P(sa), P(lcp), None, n, 5, P(rep), None) == 1
    assert lib.sfx_repeat_lens_u32(P(sa), P(lcp), None, n, 2, P(rep), None) == 1
    assert lib.sfx_repeat_lens_u32(None, None, None, 0, 1, None, None) == 0

    begin, end = np.zeros(n + 1, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
    wss = np.zeros(int(lib.sfx_repeat_spans_workspace_bytes(n)), dtype=np.uint8)
    count = ctypes.c_uint64(99)

    def spans(min_len=1, starts=None, n=n, wsb=None, nd=None):
        s = None if starts is None else np.asarray(starts, dtype=np.uint64)
        return lib.sfx_repeat_spans_dev(P(rep), n, min_len, P(s), (0 if s is None else s.size) if nd is None else nd, P(begin),
                                        P(end), n + 1, ctypes.byref(count), P(wss), wss.size if wsb is None else wsb, None)
    assert spans() == 0 and spans(starts=[0, 3, 3, 8]) == 0
    assert spans(min_len=0) == 1                                            # min_len == 0
    assert spans(starts=[0, 4, 3]) == 1 and spans(starts=[1, 3]) == 1 and spans(starts=[0, 9]) == 1      # bad doc_starts
    assert spans(starts=[0, 3], nd=0) == 1
    assert spans(wsb=16) == 5                                               # workspace
    count.value = 99
    assert spans(n=0) == 0 and count.value == 0                             # n == 0
    assert lib.sfx_repeat_spans_u32(P(rep), n, 0, None, 0, P(begin), P(end), n + 1, ctypes.byref(count)) == 1
    count.value = 99
    assert lib.sfx_repeat_spans_u32(None, 0, 1, None, 0, None, None, 0, ctypes.byref(count)) == 0 and count.value == 0


def test_device_module_checks_its_arguments(emu):
    import torch

    from suffix_amd import device as sdev
    docs = [b"abcab", b"", b"bcabc"]
    t = torch.frombuffer(bytearray(b"".join(docs)), dtype=torch.uint8)
    ds = torch.tensor([0, 5, 5], dtype=torch.int64)
    sa, da, lcp = sdev.build_gsa(t, ds, engine=emu)
    text, starts = b"".join(docs), [0, 5, 5]
    for scope in ("any", "earlier", "other_doc"):
        rep, src = sdev.repeat_lens(sa, lcp, scope=scope, da=da, want_src=True, engine=emu)
        rep_h = rep.numpy().view(np.uint32)
        assert np.array_equal(rep_h, R.brute_rep(text, scope, starts)), scope
        R.check_witnesses(text, scope, rep_h, src.numpy().view(np.uint32), starts)
        spans = sdev.repeat_spans(rep, 2, doc_starts=ds, engine=emu)
        assert spans.shape[1] == 2 and [tuple(x) for x in spans.tolist()] == R.span_reference(rep_h, 2, starts)
    assert sdev.repeat_spans(sdev.repeat_lens(sa, lcp, engine=emu), 1000, engine=emu).shape == (0, 2)
    with pytest.raises(ValueError):
        sdev.repeat_lens(sa, lcp, scope="other_doc", engine=emu)              # needs da
    with pytest.raises(ValueError):
        sdev.repeat_lens(sa, lcp, scope="later", engine=emu)
    with pytest.raises(TypeError):
        sdev.repeat_lens(sa.to(torch.int64), lcp, engine=emu)
    with pytest.raises(TypeError):
        sdev.repeat_lens(sa, torch.cat((lcp, lcp))[::2], engine=emu)          # not contiguous
    with pytest.raises(ValueError):
        sdev.repeat_lens(sa, lcp[:-1].clone(), engine=emu)
    with pytest.raises(ValueError):
        sdev.repeat_spans(sa, 0, engine=emu)
    with pytest.raises(TypeError):
        sdev.repeat_spans(sa, 2, doc_starts=ds.to(torch.int32), engine=emu)


def test_every_rep_kernel_maps_to_its_launch_name():
    """scripts/pmc_summary.py names rocprofv3 symbols by their longest listed prefix: every k_rep_* kernel must come out
    under the name its SFX_LAUNCH uses."""
    import re
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "scripts"))
    import pmc_summary
    src = open(os.path.join(root, "suffix_amd", "csrc", "sfx_tree.hip")).read()
    kernels = set(re.findall(r"__global__[^;{]*?\b(k_rep_[a-z0-9_]+)\s*\(", src, flags=re.S))
    launched = dict((k, name) for name, k in re.findall(r'SFX_LAUNCH\("(rep_[a-z_]+)",[^,]*,\s*(k_rep_[a-z0-9_]+)', src))
    assert len(kernels) >= 10 and kernels <= set(launched), sorted(kernels - set(launched))
    for k in sorted(kernels):
        assert pmc_summary.profile_name(f"sfx::{k}(...)") == launched[k], (k, pmc_summary.profile_name(f"sfx::{k}(...)"), launched[k])
    assert not any(k.startswith("k_gsa_") for k in kernels)
