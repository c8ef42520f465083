"""Maximal repetitions and Lyndon arrays on the MI355X (sfx_runs_*, sfx_lyndon_array_*): the emulator's cases
(tests/_runs.py) through the product library; then five kinds of text at 2^20 + 5 bytes through the serial checker
tests/runs_check.c (every triple verified, every run of period <= 256 enumerated from the definition) and at 2^16 + 5 bytes
through its complete sweep, tandem repeats planted in random bytes with periods far above the sweep's, the Fibonacci string
of 832 040 bytes through the complete sweep and its closed form, one repeated byte and pair against theirs, both Lyndon arrays against a serial stack, and the host route against the
device route.  The tables are the oracle's; the checker reads the text and the triples only."""
import numpy as np
import pytest
import torch

import _gen
import _runs as R
from suffix_amd import device as sdev

pytestmark = pytest.mark.gpu
N, N_SMALL = (1 << 20) + 5, (1 << 16) + 5
KINDS = ("english", "dna", "bytes", "binary", "near_duplicates")


@pytest.fixture(scope="module")
def eng():
    import suffix_amd
    e = suffix_amd.default_engine()
    e.require_device()                      # fail loudly: no CPU fallback
    assert e.path.endswith("libsuffix_hip.so")
    return e


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    return R.build_checker(tmp_path_factory.mktemp("runs_check"))


def test_known_answers(eng, oracle):
    R.known_answers(eng, "cuda", oracle)


def test_small_random_texts_vs_brute(eng, oracle):
    assert R.small_random(eng, "cuda", oracle) >= 300


def test_edge_texts(eng, oracle):
    R.edge_texts(eng, "cuda", oracle)


def test_filters_and_capacity(eng, oracle):
    R.filters(eng, "cuda", oracle)
    R.capacities(eng, "cuda", oracle)


def test_buffers_streams_and_no_allocation(eng, oracle):
    R.buffers_and_streams(eng, "cuda", oracle)
    R.no_allocations(eng, "cuda", oracle, lambda: eng.resource_stats()["device_allocs_total"])


def test_refusals_and_size_bound(eng, oracle):
    R.refusals(eng, "cuda", oracle)
    R.size_bound(eng)


def test_corrupted_lcp_stays_in_bounds(eng, oracle):
    R.corrupted_lcp(eng, "cuda", oracle)


def test_launch_names(eng, oracle):
    R.launch_names(eng, "cuda", oracle)


# ---- scale -----------------------------------------------------------------------------------------------------------
def _near_duplicates(n, copies=8, every=400):
    """One English-like document written `copies` times, every later copy with a substituted byte about every `every` bytes
    (_gen.near_duplicates repeats only after 16 MiB)."""
    doc = _gen.english_like(n // copies + 1)
    t = np.resize(doc, n).copy()
    rng = np.random.default_rng(13)
    at = rng.integers(doc.size, n, n // every)
    t[at] = rng.integers(97, 123, at.size).astype(np.uint8)
    return t


def _text(kind, n):
    gen = {"english": lambda: _gen.english_like(n), "dna": lambda: _gen.dna(n), "bytes": lambda: _gen.uniform_bytes(n, 256, 7),
           "binary": lambda: _gen.uniform_bytes(n, 2, 9, base=97), "near_duplicates": lambda: _near_duplicates(n)}[kind]
    text = np.ascontiguousarray(gen(), dtype=np.uint8).tobytes()
    assert len(text) == n
    return text


_cache = {}


def _tables(oracle, key, make):
    """(text, sa, lcp) of one text, the oracle's, computed once and left unchanged."""
    if key not in _cache:
        text = make()
        sa = oracle.sais(text)
        _cache[key] = (text, R._u32a(sa), R._u32a(oracle.lcp_kasai(text, sa)))
    return _cache[key]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32).copy()).to("cuda")


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def _runs(eng, text, sa, lcp, **kw):
    b, e, p, z = sdev.runs(torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to("cuda"), _dev(sa), _dev(lcp), engine=eng, **kw)
    assert z == b.numel() == e.numel() == p.numel()
    return _host(b), _host(e), _host(p)


@pytest.mark.parametrize("kind", KINDS)
def test_scale_verify_and_sweep_256(eng, oracle, chk, kind):
    text, sa, lcp = _tables(oracle, (kind, N), lambda: _text(kind, N))
    got = _runs(eng, text, sa, lcp)
    found = R.accept(chk, text, got, 256, threads=R.check_threads())
    assert found == int((got[2] <= 256).sum())
    print(f"{kind}: {got[0].size} runs in {N} bytes, {found} of period <= 256, longest period {int(got[2].max()) if got[2].size else 0}")
    if kind == "binary":
        assert 0.40 * N <= got[0].size <= 0.44 * N                     # the count stress: about 0.42 n runs


@pytest.mark.parametrize("kind", KINDS)
def test_scale_complete_sweep(eng, oracle, chk, kind):
    text, sa, lcp = _tables(oracle, (kind, N_SMALL), lambda: _text(kind, N_SMALL))
    got = _runs(eng, text, sa, lcp)
    assert R.accept(chk, text, got, N_SMALL // 2, threads=R.check_threads()) == got[0].size


def test_planted_tandem_repeats(eng, oracle, chk):
    """Units of 1000, 5000 and 100 000 random bytes written 2, 3.5 and 2.0 times into 2^20 random bytes: one begins at 0, one
    ends at n, one straddles a multiple of 2048.  Their exact triples come from byte comparison and must be reported."""
    text, want = R.planted()
    _, sa, lcp = _tables(oracle, "planted", lambda: text)
    got = _runs(eng, text, sa, lcp)
    have = set(zip(*(g.tolist() for g in got)))
    for r in want:
        assert r in have, (r, sorted(x for x in have if x[2] >= 1000))
    assert sorted(x for x in have if x[2] >= 1000) == sorted(want)
    R.accept(chk, text, got, 256, threads=R.check_threads())
    big = _runs(eng, text, sa, lcp, min_period=1000)
    assert sorted(zip(*(g.tolist() for g in big))) == sorted(want)


def test_fibonacci_closed_form(eng, oracle, chk):
    """832 040 bytes: the runs are deeply nested and their lengths sum to n log n.  verify and the complete sweep (every period
    up to n / 2 from the definition, the periods spread over the checker's threads); the count equals the sweep's, and
    2 |f(k-2)| - 3 as the cross-check."""
    text, sa, lcp = _tables(oracle, "fib", lambda: R.fibonacci(832040))
    got = _runs(eng, text, sa, lcp)
    found = R.accept(chk, text, got, len(text) // 2, threads=R.check_threads())
    assert found == got[0].size
    assert got[0].size == 2 * 317811 - 3 == 635619
    total = int((got[1].astype(np.int64) - got[0]).sum())
    assert total > 8 * len(text), total                                # (the n log n of nested runs)


def test_one_byte_and_one_pair_repeated(eng, oracle):
    for unit, p in ((b"a", 1), (b"ab", 2)):
        text = (unit * (N // p + 1))[:N]
        _, sa, lcp = _tables(oracle, ("rep", p), lambda: text)
        got = _runs(eng, text, sa, lcp)
        assert [g.tolist() for g in got] == [[0], [N], [p]]


@pytest.mark.parametrize("kind", KINDS)
def test_scale_lyndon_arrays_of_both_orders(eng, oracle, chk, kind):
    text, sa, _ = _tables(oracle, (kind, N), lambda: _text(kind, N))
    for order in (0, 1):
        isa = R.inverse(sa if order == 0 else oracle.sais(R.complement(text)))
        lyn = _host(sdev.lyndon_array(_dev(isa), engine=eng))
        R.accept_lyndon(chk, isa, lyn)
        starts, i = [], 0
        while i < N and len(starts) < 10 ** 6:
            starts.append(i)
            i += int(lyn[i])
        assert i == N
        if order == 0 and kind == "dna":
            from suffix_amd import SuffixTable
            assert SuffixTable.from_parts(text, sa, engine=eng).lyndon_factorization().tolist() == starts


@pytest.mark.parametrize("kind", ("dna", "binary"))
def test_host_route_equals_device_route(eng, oracle, kind):
    text, sa, lcp = _tables(oracle, (kind, N_SMALL), lambda: _text(kind, N_SMALL))
    dev = _runs(eng, text, sa, lcp)
    rc, z, got = R.host_runs(eng, text)                                # sa and lcp NULL: built
    assert rc == R.OK and z == dev[0].size
    for k in range(3):
        assert np.array_equal(np.array([r[k] for r in got], dtype=np.uint32), dev[k]), k
    for order in (0, 1):
        rc, lyn = R.host_lyndon(eng, text, order)
        assert rc == R.OK
        isa = R.inverse(sa if order == 0 else oracle.sais(R.complement(text)))
        assert np.array_equal(lyn, _host(sdev.lyndon_array(_dev(isa), engine=eng)))
