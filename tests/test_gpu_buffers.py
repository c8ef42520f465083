"""How callers hand buffers and streams to the `*_dev` ABI, on the MI355X (run with -m gpu): the cases of tests/_buffers.py
on the hardware geometry (offset texts and arrays, dirty workspaces of exactly the stated size, guard bands around everything
an entry point writes), every suffix_amd.device entry point on a side stream behind unsynchronised producers, builds from
concurrent threads, and the two-phase query path with its scratch shared across streams and threads.  Every input is one
the contract of include/suffix_hip.h accepts, or one the host refuses before a launch."""
import random
import threading
import time

import numpy as np
import pytest
import torch

import _buffers
import _cases
import _gen
import _gsa
import _repeats
from suffix_amd import GeneralizedSuffixTable, SuffixTable
from suffix_amd import device as sdev

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def eng():
    import suffix_amd
    e = suffix_amd.default_engine()
    e.require_device()                      # fail loudly: no CPU fallback
    assert e.path.endswith("libsuffix_hip.so")
    return e


# ---- the cases of _buffers.py at the sizes where the product's branches differ --------------------------------------------
def test_one_workgroup_build_offsets_and_dirt(eng, oracle):
    """n <= 16 KiB: the 16-byte LDS fill of sfx_tiny.hip and its `i + 16 <= n` edge, aligned and unaligned texts."""
    for n in (1, 2, 15, 16, 17, 31, 4097, 16384):
        for text in (_gen.dna(n, seed=40 + n).tobytes(), _gen.english_like(n).tobytes()):
            _buffers.build_sa_case(eng, oracle, text, DEV, which=_buffers.combos(always=[(0, 0, 0xFF)]))


@pytest.mark.parametrize("n", [16385, 70_001, 300_007, 1_000_003])
def test_general_build_offsets_and_dirt(eng, oracle, n):
    """Every packing (1, 2, 2, 4, 7, 8 bits per symbol); 70 001 and up with more than 16 symbols bring in the count histogram
    (head / vectors / tail) and, memory permitting, the bigram counts of the context codes' pilot.  An unaligned text takes
    the LDS-staged pack kernel and the byte paths and still gives the oracle's table."""
    for _name, text in _buffers.alphabets(n):
        _buffers.build_sa_case(eng, oracle, text, DEV)


def test_general_build_of_small_texts(eng, oracle):
    with _cases.general_build(eng):
        for n in (2, 17, 4097):
            for _name, text in _buffers.alphabets(n):
                _buffers.build_sa_case(eng, oracle, text, DEV, which=_buffers.combos()[:4])


@pytest.mark.parametrize("n", [70_000, 70_001, 70_007, 1_048_583])    # n mod 8 = 0, 1, 7; from 2^20 on the direct LCP route
def test_lcp_offsets_and_dirt(eng, oracle, n):
    _buffers.lcp_case(eng, oracle, _gen.dna(n, seed=n).tobytes(), DEV)
    if n < 100_000:
        _buffers.lcp_case(eng, oracle, _gen.english_like(n).tobytes(), DEV)
        small = _gen.dna(n // 16, seed=n).tobytes()                     # (the fused LCP over the one-workgroup build, and the general one)
        _buffers.lcp_case(eng, oracle, small, DEV)
        with _cases.general_build(eng):
            _buffers.lcp_case(eng, oracle, small, DEV)


def test_lcp_pending_pairs_at_every_offset(eng, oracle):
    """Repeat-rich texts: pairs the initial sort leaves pending -- finished by k_lcp_pending for a d_lcp on a 16-byte boundary,
    by the separate LCP routine at the other offsets."""
    for text in _buffers.repeat_rich(3000):
        _buffers.lcp_case(eng, oracle, text, DEV)


def test_queries_index_and_slices(eng, oracle):
    rng = np.random.default_rng(5)
    for text in _cases.directory_texts(1):
        _buffers.query_case(eng, oracle, text, _cases.directory_query_list(text, rng, random_count=200), DEV)


def test_suffix_tree_doc_lookup_widen(eng, oracle):
    for text in (b"banana", _gen.dna(70_001, seed=3).tobytes(), b"ab" * 3000 + b"a", _gen.english_like(300_007).tobytes()):
        _buffers.intervals_case(eng, oracle, text, DEV)
    _buffers.doc_lookup_case(eng, DEV)
    _buffers.doc_lookup_case(eng, DEV, n=3_000_000, ndocs=5000, seed=8)
    _buffers.widen_case(eng, DEV, counts=(1, 7, 255, 256, 257, 10001, 1_000_003))


def test_generalized_build_and_index(eng):
    _buffers.gsa_cases(eng, DEV, iters=12, max_docs=64, max_len=40)
    with _cases.general_build(eng):
        _buffers.gsa_cases(eng, DEV, iters=6, seed=13)


def test_repeat_lens_and_spans(eng, oracle):
    _buffers.repeats_cases(eng, oracle, DEV, iters=8)


def test_range_build_unaligned_text(eng, oracle):
    _buffers.range_case(eng, oracle, _gen.dna(300_007, seed=8).tobytes(), DEV)
    _buffers.range_case(eng, oracle, _gen.english_like(70_001).tobytes(), DEV, nranges=2)
    _buffers.range_case(eng, oracle, _gen.utf8_mixed(70_001).tobytes(), DEV, nranges=5)


def test_refusals_leave_everything_untouched(eng, oracle):
    _buffers.refusals(eng, oracle, DEV)


# ---- non-default streams ------------------------------------------------------------------------------------------------------
_CYCLES_PER_MS = []


def _spin(ms=3.0):
    """A few ms of filler on the current stream (the spin kernel's clock is calibrated once, with events)."""
    if not _CYCLES_PER_MS:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000)
        a.record()
        torch.cuda._sleep(1_000_000)
        b.record()
        b.synchronize()
        _CYCLES_PER_MS.append(1.0e6 / max(a.elapsed_time(b), 1.0e-3))
    torch.cuda._sleep(int(ms * _CYCLES_PER_MS[0]))


class _Late:
    """Arrays that reach HBM late: the buffer first holds other bytes (0x5A) and is overwritten by an asynchronous copy queued
    behind filler work on the CURRENT stream.  A step of the engine that ran on another stream would read the other bytes."""

    def __init__(self):
        self.keep = []

    def __call__(self, arr, dtype=torch.uint8):
        a = np.ascontiguousarray(arr)
        host = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).pin_memory()
        d = torch.empty(host.numel(), dtype=torch.uint8, device=DEV).fill_(0x5A)
        _spin()
        d.copy_(host, non_blocking=True)
        self.keep.append(host)
        return d.view(dtype)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def test_every_entry_point_on_a_side_stream(eng, oracle):
    """Inputs produced on the side stream immediately before each call, no host synchronisation in between; results looked
    at after s.synchronize().  (Detection of a stray NULL-stream step is probabilistic; a correct engine passes always.)"""
    text = _gen.english_like(300_007, seed=3).tobytes()
    small = _gen.dna(5000, seed=3).tobytes()
    exp, exp_s = oracle.sais(text), oracle.sais(small)
    lcp, lcp_s = oracle.lcp_kasai(text, exp), oracle.lcp_kasai(small, exp_s)
    rng = np.random.default_rng(3)
    qs = _cases.directory_query_list(text, rng, random_count=300)
    qb, qoff = _buffers.query_arrays(qs)
    ps, pe = oracle.positions_batch(text, exp, qb, qoff)
    docs = [small[a:a + ln] for a, ln in ((0, 700), (700, 0), (700, 900), (100, 650), (1600, 1200))]
    gtext, gstarts = b"".join(docs), _gsa.doc_starts(docs)
    naive = GeneralizedSuffixTable.new_naive(docs, engine=eng)
    gqs = [gtext[a:a + 1 + a % 7] for a in range(0, len(gtext), 41)] + [b"", b"zz"] + _gsa.boundary_queries(docs, random.Random(2), k=20)
    gqb, gqoff = _buffers.query_arrays(gqs)
    rep_any = np.maximum(lcp, np.append(lcp[1:], 0))                      # rep[sa[r]] = max(lcp[r], lcp[r + 1]) (suffix_hip.h)
    rep_any[0] = lcp[1] if len(lcp) > 1 else 0
    exp_rep = np.zeros(len(text), dtype=np.uint32)
    exp_rep[exp] = rep_any
    lo, hi = len(text) // 3, len(text) // 2
    tree = oracle.suffix_tree_sweep(lcp)
    pos = rng.integers(0, len(gtext), 4000).astype(np.uint32)

    s = torch.cuda.Stream()
    late = _Late()
    out = {}
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        out["sa"] = sdev.build_sa(late(text), engine=eng)
        out["sa_small"] = sdev.build_sa(late(small), engine=eng)        # (the one-workgroup build)
        out["fused"] = sdev.build_sa_lcp(late(text), engine=eng)
        out["fused_small"] = sdev.build_sa_lcp(late(small), engine=eng)
        out["lcp"] = sdev.build_lcp(late(text), late(exp, torch.int32), engine=eng)
        t, sa = late(text), late(exp, torch.int32)
        out["query"] = sdev.query_batch(t, sa, late(qb), late(qoff, torch.int64), engine=eng)
        t2, sa2 = late(text), late(exp, torch.int32)
        ix = sdev.DeviceIndex(t2, sa2, engine=eng)
        out["index"] = ix.query(late(qb), late(qoff, torch.int64))
        out["tree"] = sdev.lcp_intervals(late(lcp, torch.int32), engine=eng)
        out["doc"] = sdev.doc_lookup(late(pos, torch.int32), late(gstarts, torch.int64), engine=eng)
        out["gsa"] = sdev.build_gsa(late(gtext), late(gstarts, torch.int64), engine=eng)
        keep = (late(gtext), late(gstarts, torch.int64), late(naive.table(), torch.int32), late(naive.doc_array(), torch.int32))
        gx = sdev.GeneralizedDeviceIndex(*keep, engine=eng)
        out["gquery"] = gx.query(late(gqb), late(gqoff, torch.int64))
        out["rep"] = sdev.repeat_lens(late(exp, torch.int32), late(lcp, torch.int32), "any", want_src=True, engine=eng)
        out["lpf"] = sdev.repeat_lens(late(exp_s, torch.int32), late(lcp_s, torch.int32), "earlier", engine=eng)
        out["spans"] = sdev.repeat_spans(late(exp_rep, torch.int32), 12, engine=eng)
        out["wide"] = sdev.widen_u64(late(exp, torch.int32), engine=eng)
        out["lcp_part"] = sdev.build_lcp_range(late(text), late(exp[lo:hi], torch.int32), prev_suffix=int(exp[lo - 1]), engine=eng)
        out["query_part"] = sdev.query_batch_range(late(text), late(exp[lo:hi], torch.int32), late(qb), late(qoff, torch.int64), engine=eng)
    s.synchronize()
    assert np.array_equal(_u32(out["sa"]), exp) and np.array_equal(_u32(out["sa_small"]), exp_s)
    assert np.array_equal(_u32(out["fused"][0]), exp) and np.array_equal(_u32(out["fused"][1]), lcp)
    assert np.array_equal(_u32(out["fused_small"][0]), exp_s) and np.array_equal(_u32(out["fused_small"][1]), lcp_s)
    assert np.array_equal(_u32(out["lcp"]), lcp)
    for name in ("query", "index"):
        s_, e_, f_, a_ = out[name]
        assert np.array_equal(_u32(s_), ps) and np.array_equal(_u32(e_), pe), name
        assert np.array_equal(f_.cpu().numpy() != 0, pe > ps), name
        a_ = _u32(a_)
        for k in np.flatnonzero(pe > ps)[::7].tolist():
            assert text[int(a_[k]):int(a_[k]) + len(qs[k])] == qs[k]
        assert (a_[pe == ps] == _buffers.NONE).all()
    for k, v in out["tree"].items():
        assert np.array_equal(_u32(v), tree[k]), k
    want_d = np.searchsorted(gstarts, pos.astype(np.int64), side="right") - 1
    assert np.array_equal(_u32(out["doc"][0]), want_d) and np.array_equal(_u32(out["doc"][1]), pos - gstarts[want_d])
    for got, want in zip(out["gsa"], (naive.table(), naive.doc_array(), naive.lcp_lens())):
        assert np.array_equal(_u32(got), want)
    gs, ge, gf, ga, gn = [x.cpu().numpy() for x in out["gquery"]]
    for k, q in enumerate(gqs):
        m = _gsa.naive_matches(docs, q)
        got = sorted((int(naive.doc_array()[r]), int(naive.table()[r]) - int(gstarts[naive.doc_array()[r]])) for r in range(int(gs[k]), int(ge[k])))
        assert got == m and int(gn[k]) == len({d for d, _ in m}) and bool(gf[k]) == bool(m), q
    rep, src = _u32(out["rep"][0]), _u32(out["rep"][1])
    assert np.array_equal(rep, exp_rep)
    for p in np.flatnonzero(rep)[::997].tolist():
        q = int(src[p])
        assert q != p and text[p:p + int(rep[p])] == text[q:q + int(rep[p])]
    assert (src[rep == 0] == _buffers.NONE).all()
    lpf = _u32(out["lpf"])
    for p in range(0, len(small), 97):                                   # LPF by the definition, sampled
        best = 0
        for q in range(p):
            k = 0
            while p + k < len(small) and small[q + k] == small[p + k]:
                k += 1
            best = max(best, k)
        assert int(lpf[p]) == best, p
    assert [tuple(r) for r in out["spans"].cpu().numpy().tolist()] == _repeats.span_reference(exp_rep, 12)
    assert np.array_equal(out["wide"].cpu().numpy(), exp.astype(np.int64))
    assert np.array_equal(_u32(out["lcp_part"]), lcp[lo:hi])
    s_, e_, f_, a_ = out["query_part"]
    ws = np.clip(ps.astype(np.int64), lo, hi) - lo
    we = np.clip(pe.astype(np.int64), lo, hi) - lo
    empty = we <= ws
    ws[empty] = 0; we[empty] = 0
    assert np.array_equal(_u32(s_), ws) and np.array_equal(_u32(e_), we) and np.array_equal(f_.cpu().numpy() != 0, ~empty)
    ix.close(); gx.close()


# ---- concurrent threads ------------------------------------------------------------------------------------------------------
def test_concurrent_threads_host_and_device_entries(eng, oracle):
    """4 threads released together, 3 rounds, each with its own texts (5 KB: one workgroup; 60 KB and 400 KB: the general
    build; English-like ones have spaces), alternating between the host-pointer entry (per-thread stream, pooled buffers,
    the polled read-back page) and the device entry on a stream of its own.  Thread-local build statistics, the pool
    emptied from the main thread meanwhile."""
    nthreads, rounds = 4, 3
    texts = {}
    for i in range(nthreads):
        texts[i] = [_gen.english_like(5000 + 17 * i, seed=100 + i).tobytes(), _gen.dna(60_000 + 101 * i, seed=200 + i).tobytes(),
                    _gen.english_like(400_000 + 1001 * i, seed=300 + i).tobytes()]
    want = {(i, j): oracle.sais(t) for i in range(nthreads) for j, t in enumerate(texts[i])}
    want_lcp = {(i, j): oracle.lcp_kasai(texts[i][j], want[(i, j)]) for i in range(nthreads) for j in range(3)}
    errors = []

    def work(i, barrier):
        try:
            stream = torch.cuda.Stream()
            for r in range(rounds):
                if barrier is not None:
                    barrier.wait(timeout=60)
                for j, t in enumerate(texts[i]):
                    if (i + j + r) % 2:
                        st = SuffixTable(t, engine=eng)
                        n_seen = eng.build_stats()["n"]
                        sa, lcp = st.table(), st.lcp_lens()
                    else:
                        with torch.cuda.stream(stream):
                            d = torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).to(DEV, non_blocking=True)
                            dsa, dlcp = sdev.build_sa_lcp(d, engine=eng)
                            n_seen = eng.build_stats()["n"]
                            stream.synchronize()
                            sa, lcp = _u32(dsa), _u32(dlcp)
                    if n_seen != len(t):
                        errors.append(("build stats of another thread", i, j, r, n_seen, len(t)))
                    if not np.array_equal(sa, want[(i, j)]):
                        errors.append(("SA differs", i, j, r))
                    if not np.array_equal(lcp, want_lcp[(i, j)]):
                        errors.append(("LCP differs", i, j, r))
        except Exception as exc:                                         # noqa: BLE001
            errors.append((repr(exc), i))

    t0 = time.perf_counter()
    for i in range(nthreads):
        work(i, None)
    serial = time.perf_counter() - t0
    assert not errors, errors
    barrier = threading.Barrier(nthreads)
    threads = [threading.Thread(target=work, args=(i, barrier), daemon=True) for i in range(nthreads)]
    for th in threads:
        th.start()
    deadline = time.perf_counter() + max(30.0, 20.0 * serial)
    while any(th.is_alive() for th in threads) and time.perf_counter() < deadline:
        eng.release_cached_buffers()                                     # (the pool holds idle buffers only)
        next((th for th in threads if th.is_alive()), threads[0]).join(0.002)
    for th in threads:
        th.join(max(0.0, deadline - time.perf_counter()))
    assert not any(th.is_alive() for th in threads), "a worker thread is still running"
    assert not errors, errors


# ---- two-phase query batches --------------------------------------------------------------------------------------------------
def _batch(text, rng, count):
    qs = _cases.directory_query_list(text, rng, random_count=count)[:count]
    qb, qoff = _buffers.query_arrays(qs)
    return qs, qb, qoff, torch.from_numpy(qb.copy()).to(DEV), torch.from_numpy(qoff.astype(np.int64)).to(DEV)


def _check_batch(oracle, text, exp, batch, got, other=None):
    qs, qb, qoff, _d1, _d2 = batch
    ps, pe = oracle.positions_batch(text, exp, qb, qoff)
    s, e, f, a = [x.cpu().numpy() for x in got]
    bad = np.flatnonzero((s.view(np.uint32) != ps) | (e.view(np.uint32) != pe))
    assert bad.size == 0, (qs[int(bad[0])], int(s[bad[0]]), int(e[bad[0]]), int(ps[bad[0]]), int(pe[bad[0]]))
    assert np.array_equal(f != 0, pe > ps)
    a = a.view(np.uint32)
    assert (a[pe == ps] == _buffers.NONE).all()
    for k in np.flatnonzero(pe > ps)[::53].tolist():
        assert text[int(a[k]):int(a[k]) + len(qs[k])] == qs[k]
    if other is not None:
        for x, y in zip(got[:3], other[:3]):
            assert torch.equal(x, y)


def test_two_phase_batches_adversarial_queries(eng, oracle):
    """Batches of >= 4096 queries take k_query_tree_long with the per-thread scratch: the adversarial list of every text
    (padding runs, queries over the end of the text, the 16 / 17 / 24 / 25-byte boundaries) extended to 5000 queries, then
    12 000 on the same index so that the scratch grows; against the oracle and the undirected search."""
    rng = np.random.default_rng(11)
    for text in _cases.directory_texts(1):
        exp = oracle.sais(text)
        t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(DEV)
        sa = torch.from_numpy(exp.view(np.int32).copy()).to(DEV)
        ix = sdev.DeviceIndex(t, sa, engine=eng)
        for count in (5000, 12_000):
            b = _batch(text, rng, count)
            got = ix.query(b[3], b[4])
            plain = sdev.query_batch(t, sa, b[3], b[4], engine=eng)
            torch.cuda.synchronize()
            _check_batch(oracle, text, exp, b, got, other=plain)
        ix.close()


def test_two_phase_scratch_across_streams(eng, oracle):
    """Batch A (200 000 queries) on stream s1, batch B (5000) on s2, A again on s1, queued from one thread without a host
    synchronisation: the three share the thread's scratch list, handed from stream to stream by an event."""
    text = _cases.directory_texts(1)[-1]
    assert len(text) == 270_000
    exp = oracle.sais(text)
    rng = np.random.default_rng(12)
    t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(DEV)
    sa = torch.from_numpy(exp.view(np.int32).copy()).to(DEV)
    ix = sdev.DeviceIndex(t, sa, engine=eng)
    A, B = _batch(text, rng, 200_000), _batch(text, rng, 5000)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        r1 = ix.query(A[3], A[4])
    with torch.cuda.stream(s2):
        r2 = ix.query(B[3], B[4])
    with torch.cuda.stream(s1):
        r3 = ix.query(A[3], A[4])
    torch.cuda.synchronize()
    _check_batch(oracle, text, exp, A, r1)
    _check_batch(oracle, text, exp, B, r2)
    _check_batch(oracle, text, exp, A, r3, other=r1)
    ix.close()


def test_generalized_index_scratch_across_streams_and_threads(eng):
    """sfx_gindex_query_dev keeps one scratch per index behind a mutex and an event: batches alternating between two streams
    of one thread, then between two threads, all on one index."""
    rng = random.Random(9)
    base = _gen.english_like(4000, seed=9).tobytes()
    docs, p = [], 0
    while p < len(base):
        ln = rng.randint(0, 300)
        docs.append(base[p:p + ln])
        p += ln
    docs += [docs[3], docs[5][:40], b""]
    text, starts = b"".join(docs), _gsa.doc_starts(docs)
    naive = GeneralizedSuffixTable.new_naive(docs, engine=eng)
    sa_h, da_h = naive.table(), naive.doc_array()

    def batch(count):
        qs = []
        for _ in range(count):
            a = rng.randrange(len(text))
            q = text[a:a + rng.randint(1, 9)]
            qs.append(q if rng.random() < 0.7 else q[:-1] + bytes([q[-1] ^ 0x55]))
        qb, qoff = _buffers.query_arrays(qs)
        memo = {}
        ref = []
        for q in qs:
            if q not in memo:
                m = _gsa.naive_matches(docs, q)
                memo[q] = (len(m), len({d for d, _ in m}), sorted(m))
            ref.append(memo[q])
        return qs, ref, torch.from_numpy(qb.copy()).to(DEV), torch.from_numpy(qoff.astype(np.int64)).to(DEV)

    def check(b, got):
        s, e, f, a, nd = [x.cpu().numpy() for x in got]
        for k, (cnt, ndocs, m) in enumerate(b[1]):
            assert int(e[k]) - int(s[k]) == cnt and int(nd[k]) == ndocs and bool(f[k]) == bool(cnt), b[0][k]
            if k % 37 == 0:
                assert sorted((int(da_h[r]), int(sa_h[r]) - int(starts[da_h[r]])) for r in range(int(s[k]), int(e[k]))) == m

    keep = [torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(DEV), torch.from_numpy(starts).to(DEV),
            torch.from_numpy(sa_h.view(np.int32).copy()).to(DEV), torch.from_numpy(da_h.view(np.int32).copy()).to(DEV)]
    gx = sdev.GeneralizedDeviceIndex(*keep, engine=eng)
    A, B = batch(6000), batch(300)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        r1 = gx.query(A[2], A[3])
    with torch.cuda.stream(s2):
        r2 = gx.query(B[2], B[3])
    with torch.cuda.stream(s1):
        r3 = gx.query(A[2], A[3])
    torch.cuda.synchronize()
    check(A, r1); check(B, r2); check(A, r3)
    # two threads, one index
    results, errors = {}, []
    barrier = threading.Barrier(2)

    def work(i):
        try:
            st = torch.cuda.Stream()
            barrier.wait(timeout=60)
            out = []
            with torch.cuda.stream(st):
                for r in range(4):
                    b = (A, B)[(i + r) % 2]
                    out.append((b, gx.query(b[2], b[3])))
            st.synchronize()
            results[i] = out
        except Exception as exc:                                         # noqa: BLE001
            errors.append((repr(exc), i))

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(60)
    assert not any(th.is_alive() for th in threads), "a query thread is still running"
    assert not errors, errors
    for i in range(2):
        for b, got in results[i]:
            check(b, got)
    gx.close()
