"""The suffix-tree navigation calls on the MI355X (sfx_lce_substr*, sfx_lce_lca*, sfx_lce_range_argmin*,
sfx_suffix_links_*): the emulator's cases (tests/_nav.py) through the product library, then 2^20 + 5 indexed bytes -- the
five levels of test_gpu_lce.py, the top one with two words -- of three kinds of text and a collection of about 400
documents: 2^16 substring queries and 2^16 LCA pairs each, every answer through the serial checker tests/nav_check.c
(which reads sa and lcp only), 2^16 argmins against numpy, the suffix links of the engine's node table once
tests/tree_check.c has accepted it, the unary text in closed form, and the resident index's pattern search of the same
substrings.  The tables are the oracle's; the collection's is the engine's generalized build once tests/gsa_check.c has
accepted it against the text."""
import random

import numpy as np
import pytest
import torch

import _gen
import _gsa
import _lce as L
import _nav as N
import _tree
from suffix_amd import SuffixTable
from suffix_amd import device as sdev

pytestmark = pytest.mark.gpu
SIZE, NQ = (1 << 20) + 5, 1 << 16
NONE = N.NONE
DEV = "cuda"


@pytest.fixture(scope="module")
def eng():
    import suffix_amd
    e = suffix_amd.default_engine()
    e.require_device()                      # fail loudly: no CPU fallback
    assert e.path.endswith("libsuffix_hip.so")
    return e


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    return N.build_checker(tmp_path_factory.mktemp("nav_check"))


def test_known_answers(eng, oracle):
    N.known_answers(eng, DEV, oracle)


def test_the_tables_handle_serves_the_new_calls(eng, oracle):
    N.handle_is_made_once(eng, oracle)


def test_small_random_texts_vs_brute(eng, oracle):
    assert N.small_random(eng, DEV, oracle) >= 150


def test_small_random_collections_vs_brute(eng, oracle):
    assert N.small_collections(eng, DEV, oracle) >= 60


def test_sizes_at_the_level_edges(eng):
    N.level_edges(eng, DEV)


def test_unary_and_edge_texts(eng, oracle):
    N.unary(eng, DEV, oracle)
    N.edge_texts(eng, DEV, oracle)


def test_refusals_and_workspace_bound(eng, oracle):
    N.refusals(eng, DEV, oracle)
    N.workspace_bound(eng)


def test_corrupted_arrays_stay_in_bounds(eng, oracle):
    N.corrupted(eng, DEV, oracle)


def test_dirty_workspaces_of_the_stated_size(eng, oracle):
    N.dirty_workspaces(eng, DEV, oracle)


def test_streams_and_threads(eng, oracle):
    N.streams_and_threads(eng, DEV, oracle)


def test_launch_names(eng, oracle):
    N.launch_names(eng, DEV, oracle)


# ---- scale -----------------------------------------------------------------------------------------------------------
TEXTS = {"english": lambda: _gen.english_like(SIZE), "dna": lambda: _gen.dna(SIZE), "near_duplicates": lambda: _gen.near_duplicates(SIZE)}
_cache = {}


def _tables(oracle, kind):
    """(text bytes, sa, lcp) of one kind of text, the oracle's, computed once and left unchanged."""
    if kind not in _cache:
        text = np.ascontiguousarray(TEXTS[kind](), dtype=np.uint8).tobytes()
        assert len(text) == SIZE
        sa = oracle.sais(text)
        _cache[kind] = (text, L._u32a(sa), L._u32a(oracle.lcp_kasai(text, sa)))
    return _cache[kind]


def _dev(x):
    return N._dev(x, DEV)


def _host(t):
    return N._host(t, DEV)


def _input_conditions(text, sa, lcp, pos, ln):
    """Conditions on the INPUT, from the oracle's arrays alone: a quarter of the queries have two occurrences or more (a
    neighbour in rank order shares len bytes), and some interval is wider than 32 * 32 ranks (a one-byte substring whose
    byte occurs that often in its ... text), so some search climbs two levels."""
    n = len(text)
    r = L.expected_isa(sa).astype(np.int64)[pos]
    wide = (lcp[r] >= ln) & (r > 0) | (lcp[np.minimum(r + 1, n - 1)] >= ln) & (r + 1 < n)
    assert int(wide.sum()) * 4 >= pos.size, (int(wide.sum()), pos.size)
    counts = np.bincount(np.frombuffer(text, dtype=np.uint8), minlength=256)
    assert (counts[np.frombuffer(text, dtype=np.uint8)[pos[ln == 1]]] > 32 * 32).any()


def _queries_through_the_checker(chk, ix, text, sa, lcp, starts, seed):
    n = len(text)
    ends = None
    if starts is not None:
        e = np.concatenate((starts[1:], [n])).astype(np.int64)
        ends = e[np.searchsorted(starts, np.arange(n), side="right") - 1]
    pos, ln = N.scale_queries(n, sa, lcp, NQ, seed, ends)
    _input_conditions(text, sa, lcp, pos, ln)
    c = N.Checker(chk, sa, lcp, starts)
    try:
        lo, hi, depth = (_host(x) for x in ix.substr(_dev(pos), _dev(ln)))
        N.accept(c.substr(pos, ln, lo, hi, depth), "substr", pos, ln, lo, hi, depth)
        assert (lo != NONE).all()
        rng = np.random.default_rng(seed + 1)
        a, b = L.scale_pairs(n, sa, NQ, seed + 2)
        a[:64], b[:64] = rng.integers(n, n + 3, 64), rng.integers(0, n + 3, 64)
        lo2, hi2, d2 = (_host(x) for x in ix.lca(_dev(a), _dev(b)))
        N.accept(c.lca(a, b, lo2, hi2, d2), "lca", a, b, lo2, hi2, d2)
    finally:
        c.close()
    width = (hi - lo).astype(np.int64)
    print(f"substr: {int((width >= 2).sum())} of {NQ} with two occurrences or more, widest {int(width.max())}; "
          f"lca: deepest {int(d2[d2 != NONE].max())}, widest {int((hi2 - lo2)[lo2 != NONE].max())}")
    return pos, ln, lo, hi


@pytest.mark.parametrize("kind", ["english", "dna", "near_duplicates"])
def test_scale_queries_and_links_through_the_checker(eng, oracle, chk, tmp_path, kind):
    text, sa, lcp = _tables(oracle, kind)
    dsa, dlcp = _dev(sa), _dev(lcp)
    ix = sdev.LceDeviceIndex(dsa, dlcp, engine=eng)
    pos, ln, lo, hi = _queries_through_the_checker(chk, ix, text, sa, lcp, None, seed=len(kind))
    # the route the call replaces: the resident index's search of the same bytes as patterns
    st = SuffixTable.from_parts(text, sa, engine=eng)
    pick = np.random.default_rng(3).choice(NQ, 256, replace=False)
    s, e = st.positions_batch([text[int(pos[q]):int(pos[q]) + int(ln[q])] for q in pick])
    for k, q in enumerate(pick):
        assert set(sa[int(s[k]):int(e[k])].tolist()) == set(sa[int(lo[q]):int(hi[q])].tolist()), (int(pos[q]), int(ln[q]))
    # suffix links of the engine's node table, which the serial sweep accepts first
    exp = _tree.check_arrays(_tree.build_checker(tmp_path), tmp_path, text, sa, lcp)
    nodes = _tree.tree_u32(eng, text, sa, lcp)
    _tree.assert_equal_arrays(nodes, exp, kind)
    sl = _host(sdev.suffix_links(ix, dsa, *[_dev(nodes[k]) for k in ("node_lb", "node_rb", "node_depth")]))
    c = N.Checker(chk, sa, lcp)
    N.accept(c.slink(nodes["node_lb"], nodes["node_rb"], nodes["node_depth"], sl), "slink", nodes["node_lb"], nodes["node_rb"], nodes["node_depth"], sl)
    c.close()
    print(f"{kind}: {sl.size} nodes, deepest {int(nodes['node_depth'].max())}")
    ix.close()


def test_scale_collection(eng, oracle, chk, tmp_path):
    """About 400 documents of 1000 to 4200 bytes cut from the near-duplicates text, an empty one now and then: the
    intervals are those of the generalized table, no substring passes its document's end."""
    text, _, _ = _tables(oracle, "near_duplicates")
    rng = random.Random(8)
    starts, p = [0], 0
    while True:
        p += rng.randint(1000, 4200)
        if p >= SIZE:
            break
        starts.append(p)
        if rng.random() < 0.02:
            starts.append(p)
    starts = np.array(starts, dtype=np.int64)
    assert 350 <= starts.size <= 480
    dt, ds = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(DEV), torch.from_numpy(starts).to(DEV)
    gsa, gda, glcp = sdev.build_gsa(dt, ds, engine=eng)
    verdict = _gsa.run_checker(_gsa.build_checker(tmp_path), tmp_path, text, starts, *[_host(x) for x in (gsa, gda, glcp)])
    assert verdict.startswith("ok"), verdict
    ix = sdev.LceDeviceIndex(gsa, glcp, doc_starts=ds, engine=eng)
    _queries_through_the_checker(chk, ix, text, _host(gsa).copy(), _host(glcp).copy(), starts.astype(np.uint64), seed=12)
    ix.close()


def test_scale_argmins_against_numpy(eng, oracle):
    text, sa, lcp = _tables(oracle, "english")
    rng = np.random.default_rng(11)
    lo = rng.integers(0, SIZE, NQ)
    ln = rng.integers(1, 4096, NQ)
    ln[:256] = rng.integers(SIZE // 2 + 1, SIZE + 1, 256)                # 256 longer than n / 2
    lo[:256] = rng.integers(0, SIZE // 2 - 4, 256)
    hi = np.minimum(lo + ln, SIZE + 1)                                   # (hi = n + 1 now and then: the empty mark)
    lo[-8:], hi[-8:] = [0, 0, SIZE, SIZE - 1, 5, 32, 31, 33], [SIZE, SIZE + 1, SIZE, SIZE, 5, 64, 65, 1 << 20]
    ix = sdev.LceDeviceIndex(_dev(sa), _dev(lcp), engine=eng)
    got = _host(ix.range_argmin(_dev(lo), _dev(hi)))
    exp = L._u32a([l + int(np.argmin(lcp[l:h])) if l < h <= SIZE else NONE for l, h in zip(lo.tolist(), hi.tolist())])
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:4]
    ix.close()


def test_scale_unary_text_in_closed_form(eng):
    """a^n: sa[r] = n - 1 - r, lcp[r] = r; (pos, len) -> [len - 1, n) at depth len; m = n nodes, the node of depth d
    (id d, interval [d - 1, n)) links to the node of depth d - 1."""
    n = SIZE
    sa, lcp = np.arange(n - 1, -1, -1, dtype=np.uint32), np.arange(n, dtype=np.uint32)
    dsa = _dev(sa)
    ix = sdev.LceDeviceIndex(dsa, _dev(lcp), engine=eng)
    rng = np.random.default_rng(13)
    pos = rng.integers(0, n, NQ)
    ln = np.minimum(rng.integers(1, n + 1, NQ), n - pos)
    ln[:4096] = np.minimum(rng.integers(1, 70, 4096), n - pos[:4096])
    lo, hi, depth = (_host(x) for x in ix.substr(_dev(pos), _dev(ln)))
    assert np.array_equal(lo, ln - 1) and (hi == n).all() and np.array_equal(depth, ln)
    d = np.arange(n, dtype=np.uint32)
    sl = _host(sdev.suffix_links(ix, dsa, _dev(np.maximum(d, 1) - 1), _dev(np.full(n, n - 1)), _dev(d)))
    assert sl[0] == NONE and np.array_equal(sl[1:], d[:-1])
    ix.close()
