"""CPU run of the high-position cases (tests/_highpos.py) on the emulator build at pad_len = 40 000: the same check_*
functions test_gpu_highpos.py runs at n = 2^31 + 35 539 and n = 2^32 - 1.  Here the expectation builder itself is held
against oracle.sais and lcp_kasai of the WHOLE small text, and the two LZ properties against the definition, so what
the GPU tests expect of the tail is proven where a full oracle is affordable."""
import numpy as np
import pytest

import _highpos as HP
import _lce
import _lz
from suffix_amd import Engine

PAD = 40000


@pytest.fixture(scope="module")
def emu():
    return Engine(_lce.build_emulator())


@pytest.fixture(scope="module")
def fx(emu, oracle):
    f = HP.HighText(emu, "cpu", oracle, PAD)
    yield f
    f.close()


@pytest.fixture(scope="module")
def whole(fx, oracle):
    """The oracle's tables of the whole text."""
    text = fx.text.numpy().tobytes()
    sa = oracle.sais(text)
    return text, np.asarray(sa, dtype=np.uint32), np.asarray(oracle.lcp_kasai(text, sa), dtype=np.uint32)


def test_the_tail_is_what_the_issue_describes(oracle):
    t = HP.tail(oracle)
    S = t["S"]
    assert S.size == HP.TAIL_LEN == 65539 and set(np.unique(S).tolist()) == {0x01, 0x02, 0xFE, 0xFF}
    assert np.array_equal(S, HP.make_tail())                                  # a fixed seed
    block = S[20000:23000]
    assert np.array_equal(S[33000:36000], block) and np.array_equal(S[46600:49600], block)
    assert (S[36000:36600] == 0xFF).all() and (S[49600:50200] == 0x01).all()
    assert int(t["lcp"].max()) >= 3000 > 1024 and t["a"] + t["b"] == S.size and min(t["a"], t["b"]) > 30000


def test_expected_blocks_equal_the_whole_text_oracle(fx, whole, oracle):
    text, sa, lcp = whole
    n, a, b = fx.n, fx.a, fx.b
    sa_lo, sa_hi, lcp_lo, lcp_hi = HP.expected_blocks(oracle, PAD)
    assert np.array_equal(sa[:a], sa_lo) and np.array_equal(sa[n - b:], sa_hi)
    lcp = lcp.copy()
    lcp[0] = 0
    assert np.array_equal(lcp[:a + 1], lcp_lo) and np.array_equal(lcp[n - b:], lcp_hi)
    assert lcp[a] == 0 and lcp[n - b] == 0
    mid = sa[a:n - b].astype(np.int64)
    assert mid.min() == 0 and mid.max() == PAD - 1                            # the padding's block holds the padding alone
    isa = _lce.expected_isa(sa)[PAD:].astype(np.int64)
    assert np.array_equal(isa, fx.rank_T(fx.t["isa"]))


def test_lpf_and_lz_properties_against_the_definition(oracle):
    """lpf_from_tables is the definition's array; at tail positions the LPF of T is the LPF of S, and no greedy phrase
    crosses pad_len: on a padding of 3000 bytes and a tail of 400 with a planted repeat and two runs."""
    rng = np.random.default_rng(2)
    uni = lambda k: HP.ALPHABET[rng.integers(0, 4, k)]
    block = uni(60)
    S = np.concatenate((uni(80), block, uni(50), block, np.full(40, 0xFF, dtype=np.uint8), uni(30), np.full(40, 0x01, dtype=np.uint8), uni(40)))
    pad = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 3000)]
    T = np.concatenate((pad, S)).tobytes()
    assert S.size == 400
    tables = lambda x: (oracle.sais(x), oracle.lcp_kasai(x, oracle.sais(x)))
    lpf_t, lpf_s = _lz.lpf(T), _lz.lpf(S.tobytes())
    assert np.array_equal(HP.lpf_from_tables(*tables(T)), lpf_t) and np.array_equal(HP.lpf_from_tables(*tables(S.tobytes())), lpf_s)
    assert np.array_equal(lpf_t[3000:], lpf_s) and int(lpf_s.max()) >= 60
    begin, ln, _ = _lz.reference(lpf_t, 1)
    assert 3000 in begin
    assert not ((np.array(begin) < 3000) & (np.array(begin) + np.array(ln) > 3000)).any()
    piece = HP.tail(oracle)["bytes"][19000:25000]                            # uniform bytes, then the first planted block
    assert np.array_equal(HP.lpf_from_tables(*tables(piece)), _lz.lpf(piece))


def test_search_cases_against_the_whole_table(fx, whole):
    """The brute-force intervals of the cases are those of the whole text's oracle table."""
    text, sa, _ = whole
    t = np.frombuffer(text, dtype=np.uint8)
    isa = _lce.expected_isa(sa).astype(np.int64)
    for pat, lo, hi, pos, there in HP.search_cases(fx):
        occ = HP._occ(t, pat)
        assert sorted(occ.tolist()) == sorted(pos.tolist()), pat[:16]
        if lo is not None and there:
            assert np.array_equal(np.sort(isa[occ]), np.arange(lo, hi)), pat[:16]
            assert np.array_equal(sa[lo:hi].astype(np.int64), pos), pat[:16]


def test_interval_sweep_on_a_hand_worked_array():
    # banana: lcp 0 1 3 0 0 2 -> boundary 1 (depth 1) spans ranks 0..2, boundary 2 (depth 3) ranks 1..2, boundary 5 ranks 4..5
    lb, rb = HP.tail_intervals(np.array([0, 1, 3, 0, 0, 2]))
    assert (lb[1], rb[1], lb[2], rb[2], lb[5], rb[5]) == (0, 2, 1, 2, 4, 5)


@pytest.mark.parametrize("group", list(HP.CHECKS))
def test_group(emu, fx, group):
    HP.CHECKS[group](emu, "cpu", fx)
