"""GPU tests of the suffix-tree node table (sfx_suffix_tree_*), the torch entry point and the `SuffixTree` mirror, at the
smallest shapes at which the device code can still go wrong: many workgroups, every scan level, the open-list path of the
interval kernel, child segments of every length class.  References: the restatement of the reference's sweep and the serial
stack sweep of tests/tree_check.c (tests/_tree.py)."""
import numpy as np
import pytest
import torch

import _gen
import _tree as T
from suffix_amd import SuffixTree
from suffix_amd import device as sdev

pytestmark = pytest.mark.gpu
DEV = "cuda"
NONE = T.NONE


@pytest.fixture(scope="module")
def eng():
    import suffix_amd
    e = suffix_amd.default_engine()
    e.require_device()                      # fail loudly: no CPU fallback
    assert e.path.endswith("libsuffix_hip.so")
    return e


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return T.build_checker(tmp_path_factory.mktemp("tree_check"))


def _plain(oracle, text):
    sa = oracle.sais(text)
    return sa, oracle.lcp_kasai(text, sa)


def test_small_text_forms(eng, oracle):
    text = b"banana"
    sa, lcp = _plain(oracle, text)
    a = T.tree_u32(eng, text, sa, lcp)
    assert a["node_lb"].tolist() == [0, 0, 1, 4] and a["node_rb"].tolist() == [5, 2, 2, 5]
    assert a["node_depth"].tolist() == [0, 1, 3, 2] and a["node_parent"].tolist() == [NONE, 0, 1, 0]
    assert a["node_terminal"].tolist() == [NONE, 5, 3, 4] and a["child_off"].tolist() == [0, 3, 4, 5, 6]
    assert a["child_lb"].tolist() == [0, 3, 4, 1, 2, 5] and a["child_node"].tolist() == [1, NONE, 3, 2, NONE, NONE]
    assert bytes(a["child_byte"]) == b"abnnnn" and a["leaf_parent"].tolist() == [1, 2, 2, 0, 3, 3]
    for text in T.fixed_texts():
        sa, lcp = _plain(oracle, text)
        a = T.tree_u32(eng, text, sa, lcp)
        assert T.canonical_from_arrays(text, sa, a) == T.canonical(text, T.reference_tree(text, sa, lcp)), text[:40]
        T.check_invariants(text, sa, a)


LARGE = {
    "dna": lambda: _gen.dna_fast(1 << 22, seed=21),
    "english": lambda: _gen.english_like(1 << 22),
    "near_duplicates": lambda: _gen.near_duplicates(1 << 22),
    "bytes256": lambda: _gen.uniform_bytes(1 << 22, 256, seed=23),        # the root and every depth-1 node: 256 children
    "chain": lambda: np.full(1 << 20, ord("a"), dtype=np.uint8),          # 2^20 deep, every node with a terminal
}


@pytest.mark.parametrize("name", list(LARGE))
def test_large_texts_against_the_serial_sweep(eng, oracle, checker, tmp_path, name):
    text = np.ascontiguousarray(LARGE[name]()).tobytes()
    sa, lcp = _plain(oracle, text)
    exp = T.check_arrays(checker, tmp_path, text, sa, lcp)
    got = T.tree_u32(eng, text, sa, lcp)
    T.assert_equal_arrays(got, exp, name)
    T.check_invariants(text, sa, got)
    fan = np.diff(got["child_off"].astype(np.int64))
    if name == "bytes256":
        assert fan[0] == 256 and int((fan == 256).sum()) == 257
    if name == "chain":
        assert got["node_lb"].size == len(text) and int(fan.max()) == 1


def test_buffer_discipline_on_a_side_stream(eng, oracle, checker, tmp_path):
    """Offset addresses (child_byte at an odd one), a workspace of exactly sfx_suffix_tree_workspace_bytes(n) bytes of 0xFF,
    guard bands around every array, the call queued on a side stream -- all at once."""
    text = _gen.dna_fast(1 << 20, seed=22).tobytes()
    sa, lcp = _plain(oracle, text)
    exp = T.check_arrays(checker, tmp_path, text, sa, lcp)
    m, c, n = exp["node_lb"].size, exp["child_lb"].size, len(text)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        rc, m2, c2, ins, outs = T.dev_case(eng, DEV, text, sa, lcp, m, c, offsets=True, ws_fill=0xFF)
        assert (rc, m2, c2) == (T.OK, m, c)
        assert outs["child_byte"].ptr.value % 2 == 1 and outs["workspace"].nbytes == eng.lib.sfx_suffix_tree_workspace_bytes(n)
        s.synchronize()
        T.assert_equal_arrays(T.dev_arrays(outs, m, c, n), exp)
        for name, b in {**ins, **outs}.items():
            b.check_guards(name)


def test_torch_entry_and_mirror(eng, oracle):
    text = _gen.english_like(1 << 20, seed=7).tobytes()
    sa, lcp = _plain(oracle, text)
    t = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(DEV)
    dsa, dlcp = sdev.build_sa_lcp(t, engine=eng)
    out = sdev.suffix_tree(dsa, dlcp, text=t, engine=eng)
    torch.cuda.synchronize()
    exp = T.tree_u32(eng, text, sa, lcp)
    assert set(out) == set(T.ALL_ARRAYS)
    for k in T.ALL_ARRAYS:
        got = out[k].cpu().numpy()
        assert np.array_equal(got.view(T.DTYPES[k]), exp[k]), k
    T.check_invariants(text, sa, exp)
    bare = sdev.suffix_tree(dsa, dlcp, want_leaf_parent=False, engine=eng)
    assert "child_byte" not in bare and "leaf_parent" not in bare
    assert np.array_equal(bare["child_lb"].cpu().numpy().view(np.uint32), exp["child_lb"])
    st = SuffixTree.new(text, engine=eng)
    assert np.array_equal(st.arrays["child_node"], exp["child_node"])
    assert np.array_equal(np.fromiter(st.root().suffix_indices(), dtype=np.uint32, count=len(text)), sa)
