"""CPU tests of the suffix-tree node table (sfx_suffix_tree_*) and of the `SuffixTree` mirror: the product's kernels compiled
against the fiber emulator (tests/emu), checked against a restatement of the reference's `to_suffix_tree` (tests/_tree.py)
and, on larger texts, against the serial stack sweep of tests/tree_check.c."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import _gen
import _tree as T
from suffix_amd import Engine, SuffixTable, SuffixTree

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
NONE = T.NONE


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU_DIR])
    return Engine(os.path.join(EMU_DIR, "libsuffix_emu.so"))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return T.build_checker(tmp_path_factory.mktemp("tree_check"))


def _plain(oracle, text):
    sa = oracle.sais(text)
    return sa, oracle.lcp_kasai(text, sa)


def _debug_form(text, root):
    """Debug for SuffixTree (lib.rs:230-255) over the restatement's nodes."""
    out = ["", "-----------------------------------------", "SUFFIX TREE", "text: " + text.decode()]
    stack = [(root, 0)]
    while stack:
        node, d = stack.pop()
        out.append("ROOT" if node.parent is None else " " * (2 * d) + str(list(text[node.start:node.end])))
        stack.extend((node.children[k], d + 1) for k in sorted(node.children, reverse=True))
    return "\n".join(out + ["-----------------------------------------"]) + "\n"


def test_banana_known_answer(emu, oracle):
    """sa = 5 3 1 0 4 2, lcp = 0 1 3 0 0 2.  Nodes "a", "ana" and "na" each end a suffix (terminals 5, 3, 4): T = 3 and
    C = n - 1 + m - T = 6 -- root 3 children, "a" 1, "ana" 1, "na" 1.  (The issue's listing of the nodes says the same; its
    summary line "T = 2, C = 7" contradicts that listing and the reference's sweep, which the restatement reproduces.)"""
    text = b"banana"
    sa, lcp = _plain(oracle, text)
    assert sa.tolist() == [5, 3, 1, 0, 4, 2] and lcp.tolist() == [0, 1, 3, 0, 0, 2]
    a = T.tree_u32(emu, text, sa, lcp)
    assert a["node_lb"].tolist() == [0, 0, 1, 4] and a["node_rb"].tolist() == [5, 2, 2, 5]
    assert a["node_depth"].tolist() == [0, 1, 3, 2] and a["node_parent"].tolist() == [NONE, 0, 1, 0]
    assert a["node_terminal"].tolist() == [NONE, 5, 3, 4]
    assert a["child_off"].tolist() == [0, 3, 4, 5, 6]
    # the root: node "a" at ranks 0-2, leaf rank 3 "banana", node "na" at ranks 4-5; bytes a b n
    assert a["child_lb"].tolist()[:3] == [0, 3, 4] and a["child_node"].tolist()[:3] == [1, NONE, 3]
    assert bytes(a["child_byte"][:3]) == b"abn"
    # "a": node "ana" and nothing else; "ana": leaf rank 2, byte n; "na": leaf rank 5
    assert (a["child_lb"][3], a["child_node"][3]) == (1, 2)
    assert (a["child_lb"][4], a["child_node"][4], a["child_byte"][4]) == (2, NONE, ord("n"))
    assert (a["child_lb"][5], a["child_node"][5]) == (5, NONE)
    assert a["leaf_parent"].tolist() == [1, 2, 2, 0, 3, 3]
    m, t, c = 4, int((a["node_terminal"] != NONE).sum()), a["child_lb"].size
    assert (a["node_lb"].size, t, c) == (4, 3, 6) and c == len(text) - 1 + m - t
    ref = T.reference_tree(text, sa, lcp)
    assert T.canonical_from_arrays(text, sa, a) == T.canonical(text, ref)
    st = SuffixTree.new("banana", engine=emu)
    assert list(st.root().suffix_indices()) == [5, 3, 1, 0, 4, 2]
    assert sum(1 for _ in st.root().leaves()) == 6
    assert repr(st) == _debug_form(text, ref)
    assert repr(st) == ("\n-----------------------------------------\nSUFFIX TREE\ntext: banana\nROOT\n  [97]\n    [110, 97]\n"
                        "      [110, 97]\n  [98, 97, 110, 97, 110, 97]\n  [110, 97]\n    [110, 97]\n"
                        "-----------------------------------------\n")
    assert st.text() == "banana" and st.label(st.root()) == b""
    kids = st.root().children()
    assert [st.label(k) for k in kids] == [b"a", b"banana", b"na"]
    assert [k.len() for k in kids] == [1, 6, 2] and [k.depth() for k in kids] == [1, 1, 1]
    assert [k.suffixes() for k in kids] == [[5], [0], [4]] and st.root().suffixes() == [6]
    deep = kids[0].children()[0].children()[0]
    assert st.label(deep) == b"na" and deep.depth() == 3 and deep.suffixes() == [1] and deep.children() == []
    assert [x.id for x in deep.ancestors()] == [None, 2, 1, 0] and list(deep.ancestors())[-1] == st.root()
    assert list(kids[0].suffix_indices()) == [5, 3, 1] and [st.label(x) for x in kids[2].preorder()] == [b"na", b"na"]


def _texts():
    rng = random.Random(20261017)
    out = []
    for i in range(300):
        sigma = (1, 2, 3, 4, 26)[i % 5]
        out.append(bytes(rng.randrange(97, 97 + sigma) for _ in range(rng.randint(1, 40))))
    return out + T.fixed_texts()


def test_small_texts_against_the_reference_sweep(emu, oracle):
    for text in _texts():
        sa, lcp = _plain(oracle, text)
        a = T.tree_u32(emu, text, sa, lcp)
        assert T.canonical_from_arrays(text, sa, a) == T.canonical(text, T.reference_tree(text, sa, lcp)), text[:40]
        T.check_invariants(text, sa, a)
    every = T.fixed_texts()[-2]
    a = T.tree_u32(emu, every, *_plain(oracle, every))
    assert a["node_lb"].size == 1 and bytes(a["child_byte"]) == bytes(range(256))          # root fan-out 256, 0x00 .. 0xFF


def _large_texts():
    d = _gen.dna(3000, seed=9).tobytes()
    planted = _gen.dna(20_000, seed=5).tobytes() + d + b"T" + _gen.dna(7000, seed=6).tobytes() + d[100:2900] + b"C" + d[:1500] * 3
    return [("dna", _gen.dna(40_001, seed=3).tobytes()), ("english", _gen.english_like(60_000).tobytes()),
            ("planted", planted), ("chain", b"a" * 30_000)]


@pytest.mark.parametrize("which", range(4))
def test_large_texts_against_the_serial_sweep(emu, oracle, checker, tmp_path, which):
    """20 000 - 60 000 bytes: more than one 2 048-boundary tile, more than one scan block, segments of every length class."""
    name, text = _large_texts()[which]
    sa, lcp = _plain(oracle, text)
    exp = T.check_arrays(checker, tmp_path, text, sa, lcp)
    got = T.tree_u32(emu, text, sa, lcp)
    T.assert_equal_arrays(got, exp, name)
    T.check_invariants(text, sa, got)
    if name == "chain":                                       # 30 000 deep, every node but the root with a terminal
        assert got["node_lb"].size == len(text) and int((got["node_terminal"] != NONE).sum()) == len(text) - 1


def test_lcp0_is_not_looked_at(emu, oracle):
    text = _gen.english_like(5000).tobytes()
    sa, lcp = _plain(oracle, text)
    exp = T.tree_u32(emu, text, sa, lcp)
    for poison in (0xFFFFFFFF, len(text), 1):
        bad = lcp.copy()
        bad[0] = poison
        T.assert_equal_arrays(T.tree_u32(emu, text, sa, bad), exp, hex(poison))


def test_sizing_and_short_capacities(emu, oracle):
    text = _gen.dna(3001, seed=8).tobytes()
    sa, lcp = _plain(oracle, text)
    n = len(text)
    exp = T.tree_u32(emu, text, sa, lcp)
    m, c = exp["node_lb"].size, exp["child_lb"].size
    # the sizing call: zero capacities, NULL arrays, counts only -- through both entry points
    rc, m1, c1 = T.call_u32(emu, None, sa, lcp, 0, 0, {})
    assert (rc, m1, c1) == (T.OK, m, c)
    ws = np.zeros(int(emu.lib.sfx_suffix_tree_workspace_bytes(n)) + 16, dtype=np.uint8)
    mm, cc = ctypes.c_uint64(0), ctypes.c_uint64(0)
    wp = ctypes.c_void_p((ws.ctypes.data + 15) & ~15)
    rc = emu.lib.sfx_suffix_tree_dev(None, T._ptr(sa), T._ptr(lcp), n, 0, 0, *([None] * 10), ctypes.byref(mm), ctypes.byref(cc), wp,
                                     ws.size - 16, None)
    assert (rc, mm.value, cc.value) == (T.OK, m, c)
    # one short of m, or of C: counts come back, the guard-filled arrays stay as they were
    for ncap, ccap in ((m - 1, c), (m, c - 1), (m - 1, c - 1)):
        rc, m2, c2, ins, outs = T.dev_case(emu, "cpu", text, sa, lcp, ncap, ccap)
        assert (rc, m2, c2) == (T.OK, m, c) and T.untouched(outs), (ncap, ccap)
        for b in {**ins, **outs}.values():
            b.check_guards()
        out = T.alloc(n, ncap, ccap)
        rc, m2, c2 = T.call_u32(emu, text, sa, lcp, ncap, ccap, out)
        assert (rc, m2, c2) == (T.OK, m, c)
        assert all(bool((v.view(np.uint8) == 0xFF).all()) for v in out.values())
    # room to spare is fine: n nodes and 2n children always suffice
    rc, m2, c2, ins, outs = T.dev_case(emu, "cpu", text, sa, lcp, n, 2 * n, offsets=True, ws_fill="count")
    assert (rc, m2, c2) == (T.OK, m, c)
    T.assert_equal_arrays(T.dev_arrays(outs, m, c, n), exp)
    for b in {**ins, **outs}.values():
        b.check_guards()
    # without text and bytes, without leaf_parent
    rc, m2, c2, ins, outs = T.dev_case(emu, "cpu", text, sa, lcp, m, c, with_text=False, leaf_parent=False)
    got = T.dev_arrays(outs, m, c, n)
    assert rc == T.OK and T.untouched(outs, ("child_byte", "leaf_parent"))
    for k in T.ALL_ARRAYS[:8]:
        assert np.array_equal(got[k], exp[k]), k


def test_empty_and_single_byte(emu):
    m, c = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert emu.lib.sfx_suffix_tree_u32(None, None, None, 0, 0, 0, *([None] * 10), ctypes.byref(m), ctypes.byref(c)) == T.OK
    assert (m.value, c.value) == (0, 0)
    m, c = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert emu.lib.sfx_suffix_tree_dev(None, None, None, 0, 0, 0, *([None] * 10), ctypes.byref(m), ctypes.byref(c), None, 0, None) == T.OK
    assert (m.value, c.value) == (0, 0)
    assert emu.lib.sfx_suffix_tree_workspace_bytes(0) == 0
    a = T.tree_u32(emu, b"x", np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32))
    assert {k: v.tolist() for k, v in a.items()} == {
        "node_lb": [0], "node_rb": [0], "node_depth": [0], "node_parent": [NONE], "node_terminal": [NONE], "child_off": [0, 1],
        "child_lb": [0], "child_node": [NONE], "child_byte": [ord("x")], "leaf_parent": [0]}
    st = SuffixTree.new("", engine=emu)
    assert st.root().children() == [] and list(st.root().suffix_indices()) == [] and list(st.root().leaves()) == []
    assert [x.id for x in st.root().preorder()] == [0] and st.root().suffixes() == [0] and "ROOT" in repr(st)


def test_error_statuses(emu, oracle):
    text = b"mississippi"
    sa, lcp = _plain(oracle, text)
    n = len(text)
    exp = T.tree_u32(emu, text, sa, lcp)
    m, c = exp["node_lb"].size, exp["child_lb"].size
    # a table entry >= n, found on the device
    bad = sa.copy()
    bad[4] = n
    assert T.call_u32(emu, text, bad, lcp, m, c, T.alloc(n, m, c))[0] == T.ERR_ARG
    assert T.dev_case(emu, "cpu", text, bad, lcp, m, c)[0] == T.ERR_ARG
    # exactly one of text / child_byte
    out = T.alloc(n, m, c)
    assert T.call_u32(emu, None, sa, lcp, m, c, out)[0] == T.ERR_ARG
    assert T.call_u32(emu, text, sa, lcp, m, c, T.alloc(n, m, c, child_byte=False))[0] == T.ERR_ARG
    assert T.dev_case(emu, "cpu", text, sa, lcp, m, c, drop=("text",))[0] == T.ERR_ARG
    assert T.dev_case(emu, "cpu", text, sa, lcp, m, c, drop=("child_byte",))[0] == T.ERR_ARG
    # a NULL among the required arrays when the capacities suffice -- and not when they do not
    for k in T.ALL_ARRAYS[:8]:
        rc, _, _, _, outs = T.dev_case(emu, "cpu", text, sa, lcp, m, c, drop=(k,))
        assert rc == T.ERR_ARG and T.untouched(outs), k
        assert T.dev_case(emu, "cpu", text, sa, lcp, m - 1, c, drop=(k,))[:3] == (T.OK, m, c), k
        o = T.alloc(n, m, c)
        o[k] = None
        assert T.call_u32(emu, text, sa, lcp, m, c, o)[0] == T.ERR_ARG, k
    # misaligned arrays
    mm, cc = ctypes.c_uint64(0), ctypes.c_uint64(0)
    ws = np.zeros(int(emu.lib.sfx_suffix_tree_workspace_bytes(n)) + 64, dtype=np.uint8)
    base = (ws.ctypes.data + 15) & ~15
    o = T.alloc(n, m, c)
    args = [T._ptr(o[k]) for k in T.ALL_ARRAYS]
    t = np.frombuffer(text, dtype=np.uint8)
    call = lambda a, w, wb: emu.lib.sfx_suffix_tree_dev(T._ptr(t), T._ptr(sa), T._ptr(lcp), n, m, c, *a, ctypes.byref(mm), ctypes.byref(cc),
                                                        ctypes.c_void_p(w), wb, None)
    assert call(args, base, ws.size - 64) == T.OK
    odd = list(args)
    odd[5] = ctypes.c_void_p(o["child_off"].ctypes.data + 4)
    assert call(odd, base, ws.size - 64) == T.ERR_ARG
    odd = list(args)
    odd[0] = ctypes.c_void_p(o["node_lb"].ctypes.data + 2)
    assert call(odd, base, ws.size - 64) == T.ERR_ARG
    assert call(args, base + 4, ws.size - 64) == T.ERR_ARG
    # a workspace one byte short, or none
    assert call(args, base, int(emu.lib.sfx_suffix_tree_workspace_bytes(n)) - 1) == T.ERR_WORKSPACE
    assert call(args, 0, 0) == T.ERR_WORKSPACE
    rc, _, _, ins, outs = T.dev_case(emu, "cpu", text, sa, lcp, m, c, ws_short=1)
    assert rc == T.ERR_WORKSPACE and T.untouched(outs)
    # n > u32::MAX; no place for the counts
    assert emu.lib.sfx_suffix_tree_dev(None, T._ptr(sa), T._ptr(lcp), 1 << 32, 0, 0, *([None] * 10), ctypes.byref(mm), ctypes.byref(cc),
                                       None, 0, None) == T.ERR_TOO_LARGE
    assert emu.lib.sfx_suffix_tree_u32(None, T._ptr(sa), T._ptr(lcp), 1 << 32, 0, 0, *([None] * 10), ctypes.byref(mm),
                                       ctypes.byref(cc)) == T.ERR_TOO_LARGE
    assert emu.lib.sfx_suffix_tree_u32(None, T._ptr(sa), T._ptr(lcp), n, 0, 0, *([None] * 10), None, ctypes.byref(cc)) == T.ERR_ARG


def test_garbage_lcp_stays_inside_its_arrays(emu):
    """Any lcp contents with a valid permutation as table: SFX_OK or SFX_ERR_ARG, every guard band intact."""
    rng = np.random.default_rng(11)
    for n, kind in ((1, "u32"), (2, "u32"), (700, "u32"), (5000, "u32"), (5000, "small"), (4099, "zero"), (4099, "ramp"), (3000, "saw")):
        text = rng.integers(0, 4, n, dtype=np.uint8).tobytes()
        sa = rng.permutation(n).astype(np.uint32)
        lcp = {"u32": lambda: rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
               "small": lambda: rng.integers(0, 4, n).astype(np.uint32), "zero": lambda: np.zeros(n, dtype=np.uint32),
               "ramp": lambda: np.arange(n, dtype=np.uint32)[::-1].copy(),
               "saw": lambda: (np.arange(n, dtype=np.uint32) % 3) * 0x7FFFFFFF}[kind]()
        rc, m, c, ins, outs = T.dev_case(emu, "cpu", text, sa, lcp, n, 2 * n, offsets=True, ws_fill="count")
        assert rc in (T.OK, T.ERR_ARG), (n, kind, rc)
        if rc == T.OK:
            assert 1 <= m <= n and c <= 2 * n, (n, kind, m, c)
        for name, b in {**ins, **outs}.items():
            b.check_guards(f"{kind} {n}: {name}")


def test_mirror_properties_of_the_reference(emu):
    """qc_n_leaves, qc_internals_have_at_least_two_children, qc_tree_enumerates_suffixes (lib.rs:528-566)."""
    rng = random.Random(5)
    for i in range(120):
        sigma = (1, 2, 3, 4, 26)[i % 5]
        text = bytes(rng.randrange(97, 97 + sigma) for _ in range(rng.randint(0, 30)))
        table = SuffixTable(text, engine=emu)
        st = SuffixTree.from_suffix_table(table)
        root = st.root()
        assert sum(1 for _ in root.leaves()) == len(text)
        for node in root.preorder():
            assert node.has_terminals() or len(node.children()) >= 2, (text, node)
            if node.has_terminals() and not node.is_root():      # the path from the root spells the terminal suffix
                assert b"".join(st.label(x) for x in reversed(list(node.ancestors()))) == text[node.suffixes()[0]:]
        got = list(root.suffix_indices())
        assert got == table.table().tolist()
        for k, s in enumerate(got):
            assert text[s:] == table.suffix_bytes(k)
        if text:
            sa, lcp = table.table(), table.lcp_lens()
            assert repr(st) == _debug_form(text, T.reference_tree(text, sa, lcp))
    with pytest.raises(TypeError):
        SuffixTree(b"banana")


def test_every_tree_kernel_maps_to_its_launch_name():
    sys.path.insert(0, os.path.join(os.path.dirname(EMU_DIR), os.pardir, "scripts"))
    import pmc_summary
    for k, name in (("k_tree_heads", "tree_heads"), ("k_tree_count", "tree_count"), ("k_tree_totals", "tree_totals"),
                    ("k_tree_fill", "tree_fill"), ("k_tree_order", "tree_order"), ("k_tree_parents", "tree_parents")):
        assert pmc_summary.profile_name(f"sfx::{k}(...)") == name
