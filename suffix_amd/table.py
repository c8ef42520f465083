"""`SuffixTable` -- host-side mirror of the reference's public type
(/root/reference/src/table.rs:54-294) on top of the MI355X engine.

Same method names, argument meaning and error behaviour as the Rust API:

    reference (Rust)                         here
    SuffixTable::new(text)            :78    SuffixTable.new(text) / SuffixTable(text)
    SuffixTable::new_naive(text)      :93    SuffixTable.new_naive(text)   (doc-hidden upstream: the definition, on the host)
    SuffixTable::from_parts(t, sa)    :111   SuffixTable.from_parts(text, table)
    .into_parts()                     :125   .into_parts()
    .lcp_lens()                       :130   .lcp_lens()
    .table() / .text()                :142   .table() / .text()
    .len() / .is_empty()              :156   .len() / .is_empty()
    .suffix(i) / .suffix_bytes(i)     :168   .suffix(i) / .suffix_bytes(i)
    .contains(q)                      :197   .contains(q)
    .positions(q)                     :223   .positions(q)
    .any_position(q)                  :279   .any_position(q)
    (none)                                   .positions_batch(qs) / .contains_batch(qs)
    (none)                                   .repeat_lens(scope) / .repeated_spans(min_len, scope)
    (none)                                   .match_stats(query, max_len) / .shared_spans(query, min_len)
    (none)                                   .mems(query, min_len, unique): the maximal exact matches of a new text
    (none)                                   .approx_positions(query, mismatches) / .approx_positions_batch: k-mismatch occurrences
    (none)                                   .bwt(sample_step) / suffix_amd.unbwt(bwt, samples, sample_step)
    (none)                                   .fm_index(sample_step) / suffix_amd.FmIndex: the same queries from the transform alone
    (none)                                   .inverse_table() / .lce(i, j, mismatches) / .lce_batch / .lcp_range_min[_batch]
    (none)                                   .runs(min_period, max_period, min_len) / .lyndon_array(order) / .lyndon_factorization()

Text is indexed by BYTES (every UTF-8 byte offset has a suffix, :29-31 of the
crate docs and :379); `str` input is encoded as UTF-8.  Construction, LCP and
all queries run on the GPU through the C ABI; there is no CPU path.
"""
import ctypes

import numpy as np

from ._lib import REP_SCOPES, FmInfo, RunsFilter, SuffixHipError, default_engine

_NONE = 0xFFFFFFFF


def _as_bytes(x):
    if isinstance(x, str):
        return x.encode("utf-8")
    if isinstance(x, (bytes, bytearray, memoryview)):
        return bytes(x)
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x, dtype=np.uint8).tobytes()
    raise TypeError("text/query must be str, bytes or a uint8 array")


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data if a.size else 0)


def _repeat_lens(eng, table, lcp, da, scope, with_source):
    """sfx_repeat_lens_u32 on host arrays -> rep, or (rep, src)."""
    if scope not in REP_SCOPES or (scope == "other_doc" and da is None):
        raise ValueError(f"unknown scope {scope!r}")
    n = int(table.size)
    rep = np.zeros(n, dtype=np.uint32)
    src = np.full(n, _NONE, dtype=np.uint32) if with_source else None
    if n:
        eng.require_device()
        eng.check(eng.lib.sfx_repeat_lens_u32(_ptr(table), _ptr(lcp), _ptr(da) if scope == "other_doc" else None, n,
                                              REP_SCOPES[scope], _ptr(rep), _ptr(src) if with_source else None),
                  "sfx_repeat_lens_u32")
    return (rep, src) if with_source else rep


def _repeat_spans(eng, rep, min_len, starts):
    """sfx_repeat_spans_u32 on host arrays -> (begin, end) uint32 arrays."""
    min_len = int(min_len)
    if min_len < 1 or min_len > 0xFFFFFFFF:
        raise ValueError("min_len must be in 1 .. 2^32 - 1")
    n = int(rep.size)
    cap = n // min_len + 1
    begin = np.zeros(cap, dtype=np.uint32)
    end = np.zeros(cap, dtype=np.uint32)
    count = ctypes.c_uint64(0)
    if n:
        eng.require_device()
        eng.check(eng.lib.sfx_repeat_spans_u32(_ptr(rep), n, min_len, _ptr(starts) if starts is not None else None,
                                               starts.size if starts is not None else 0, _ptr(begin), _ptr(end), cap,
                                               ctypes.byref(count)), "sfx_repeat_spans_u32")
    k = int(count.value)
    return begin[:k], end[:k]


def _match_stats(eng, fn, name, index, n, query, max_len, with_source, with_intervals):
    """sfx_index_match_stats / sfx_gindex_match_stats on host arrays -> len, or (len[, src][, start, end]).
    `index` is called for the handle only when there is something to search."""
    q = np.frombuffer(_as_bytes(query), dtype=np.uint8)
    max_len = int(max_len or 0)
    if max_len < 0 or max_len > 0xFFFFFFFF:
        raise ValueError("max_len must be in 0 .. 2^32 - 1 (None or 0 = no cap)")
    m = int(q.size)
    ln = np.zeros(m, dtype=np.uint32)
    src = np.full(m, _NONE, dtype=np.uint32) if with_source else None
    start = np.zeros(m, dtype=np.uint32) if with_intervals else None
    end = np.zeros(m, dtype=np.uint32) if with_intervals else None
    if m and n:
        eng.require_device()
        eng.check(fn(index(), _ptr(q), m, max_len, _ptr(ln), _ptr(src) if with_source else None,
                     _ptr(start) if with_intervals else None, _ptr(end) if with_intervals else None), name)
    if not with_source and not with_intervals:
        return ln
    return (ln,) + ((src,) if with_source else ()) + ((start, end) if with_intervals else ())


def _shared_spans(eng, match_stats, query, min_len):
    """The spans of `query` that occur in the indexed text with at least min_len bytes: the search capped at min_len
    (the covered bytes are the same for every cap >= min_len), then the span report of the repeats."""
    min_len = int(min_len)
    if min_len < 1 or min_len > 0xFFFFFFFF:
        raise ValueError("min_len must be in 1 .. 2^32 - 1")
    b, e = _repeat_spans(eng, match_stats(query, max_len=min_len), min_len, None)
    return list(zip(b.tolist(), e.tolist()))


def _u32_arg(x, name):
    a = np.asarray(x)
    if a.ndim != 1:
        raise ValueError(f"{name} must be one-dimensional")
    if a.size and (a.dtype.kind not in "iu" or int(a.min()) < 0 or int(a.max()) > _NONE):
        raise ValueError(f"{name} must hold integers in 0 .. 2^32 - 1")
    return np.ascontiguousarray(a, dtype=np.uint32)


class _LceHandle:
    """The lazily made sfx_lce handle of a table (SuffixTable, GeneralizedSuffixTable): sfx_lce_create over host arrays,
    which copies them; freed with its owner."""

    def __init__(self, eng):
        self._eng, self._h = eng, None

    def get(self, table, lcp, starts=None):
        """lcp: the array, or a callable that makes it -- called only when the handle does not exist yet."""
        if self._h is None:
            self._eng.require_device()
            if callable(lcp):
                lcp = lcp()
            h = ctypes.c_void_p()
            self._eng.check(self._eng.lib.sfx_lce_create(_ptr(table), _ptr(lcp), int(table.size), _ptr(starts) if starts is not None else None,
                                                         int(starts.size) if starts is not None else 0, ctypes.byref(h)), "sfx_lce_create")
            self._h = h
        return self._h

    def close(self):
        h, self._h = self._h, None
        if h:
            try:
                self._eng.lib.sfx_lce_destroy(h)
            except Exception:
                pass

    def lce(self, h, a, b, mismatches):
        a, b = _u32_arg(a, "a"), _u32_arg(b, "b")
        if a.size != b.size:
            raise ValueError("a and b must hold one position per pair")
        k = int(mismatches)
        if k < 0 or k > _NONE:
            raise ValueError("mismatches must be in 0 .. 2^32 - 1")
        out = np.zeros(a.size, dtype=np.uint32)
        if a.size:
            self._eng.check(self._eng.lib.sfx_lce_query(h(), _ptr(a), _ptr(b), int(a.size), k, _ptr(out)), "sfx_lce_query")
        return out

    def range_min(self, h, lo, hi):
        lo, hi = _u32_arg(lo, "lo"), _u32_arg(hi, "hi")
        if lo.size != hi.size:
            raise ValueError("lo and hi must hold one bound per range")
        out = np.zeros(lo.size, dtype=np.uint32)
        if lo.size:
            self._eng.check(self._eng.lib.sfx_lce_range_min(h(), _ptr(lo), _ptr(hi), int(lo.size), _ptr(out)), "sfx_lce_range_min")
        return out

    def range_argmin(self, h, lo, hi):
        lo, hi = _u32_arg(lo, "lo"), _u32_arg(hi, "hi")
        if lo.size != hi.size:
            raise ValueError("lo and hi must hold one bound per range")
        out = np.zeros(lo.size, dtype=np.uint32)
        if lo.size:
            self._eng.check(self._eng.lib.sfx_lce_range_argmin(h(), _ptr(lo), _ptr(hi), int(lo.size), _ptr(out)), "sfx_lce_range_argmin")
        return out

    def _intervals(self, h, name, a, b, what):
        a, b = _u32_arg(a, what[0]), _u32_arg(b, what[1])
        if a.size != b.size:
            raise ValueError(f"{what[0]} and {what[1]} must hold one entry per query")
        lo, hi, depth = (np.zeros(a.size, dtype=np.uint32) for _ in range(3))
        if a.size:
            self._eng.check(getattr(self._eng.lib, name)(h(), _ptr(a), _ptr(b), int(a.size), _ptr(lo), _ptr(hi), _ptr(depth)), name)
        return lo, hi, depth

    def substr(self, h, pos, length):
        return self._intervals(h, "sfx_lce_substr", pos, length, ("pos", "length"))

    def lca(self, h, a, b):
        return self._intervals(h, "sfx_lce_lca", a, b, ("a", "b"))


class Mems:
    """The maximal exact matches of a query text (SuffixTable.mems, GeneralizedSuffixTable.mems): uint32 arrays qpos /
    tpos / len, one entry per match, ascending by qpos and for equal qpos by the table rank of tpos; `pairs` = the
    number of candidate pairs the call looked at.  A collection's result also carries doc / offset of every tpos."""

    def __init__(self, qpos, tpos, len, pairs, doc=None, offset=None):
        self.qpos, self.tpos, self.len, self.pairs = qpos, tpos, len, int(pairs)
        if doc is not None:
            self.doc, self.offset = doc, offset

    def __len__(self):
        return int(self.len.size)

    def triples(self):
        return list(zip(self.qpos.tolist(), self.tpos.tolist(), self.len.tolist()))

    def __repr__(self):
        return f"Mems(z={len(self)}, pairs={self.pairs})"


MEM_UNIQUE = 1


def _mems(eng, fn, name, index, n, query, min_len, unique, max_pairs):
    """sfx_index_mems / sfx_gindex_mems on host arrays -> (qpos, tpos, len, pairs).  The first call guesses the room
    (one match per query byte); a second one follows when there were more."""
    q = np.frombuffer(_as_bytes(query), dtype=np.uint8)
    min_len, max_pairs = int(min_len), int(max_pairs)
    if min_len < 1 or min_len > 0xFFFFFFFF:
        raise ValueError("min_len must be in 1 .. 2^32 - 1")
    if max_pairs < 1:
        raise ValueError("max_pairs must be at least 1")
    m = int(q.size)
    empty = np.zeros(0, dtype=np.uint32)
    if not m or not n:
        return empty, empty.copy(), empty.copy(), 0
    max_pairs = min(max_pairs, m * n)                            # (there are no more pairs)
    eng.require_device()
    flags = MEM_UNIQUE if unique else 0
    pairs, count = ctypes.c_uint64(0), ctypes.c_uint64(0)
    cap = min(max(m, 1024), max_pairs)
    for _ in range(2):
        out = [np.zeros(cap, dtype=np.uint32) for _ in range(3)]
        eng.check(fn(index(), _ptr(q), m, min_len, flags, max_pairs, *[_ptr(a) for a in out], cap, ctypes.byref(pairs),
                     ctypes.byref(count)), name)
        if pairs.value > max_pairs:
            raise SuffixHipError(f"{name}: {pairs.value} candidate pairs exceed max_pairs = {max_pairs}; raise min_len or max_pairs")
        if count.value <= cap:
            break
        cap = int(count.value)
    z = int(count.value)
    return out[0][:z].copy(), out[1][:z].copy(), out[2][:z].copy(), int(pairs.value)


def _approx_positions(eng, fn, name, index, n, queries, mismatches, max_candidates, sort):
    """sfx_index_hamming / sfx_gindex_hamming on host arrays -> (first uint64, tpos uint32, mism uint8).  The first call
    guesses the room; a second one follows when there were more.  sort: every pattern's slice by position, on the host."""
    qs = [_as_bytes(q) for q in queries]
    k, max_candidates = int(mismatches), int(max_candidates)
    if not 0 <= k <= 255:
        raise ValueError("mismatches must be in 0 .. 255")
    if max_candidates < 1:
        raise ValueError("max_candidates must be at least 1")
    nq = len(qs)
    first = np.zeros(nq + 1, dtype=np.uint64)
    if not nq or not n:
        return first, np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8)
    off = np.zeros(nq + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(q) for q in qs], dtype=np.uint64)
    blob = np.frombuffer(b"".join(qs) or b"\0", dtype=np.uint8)
    max_candidates = min(max_candidates, nq * (k + 1) * n)          # (there are no more candidates)
    eng.require_device()
    cands, count = ctypes.c_uint64(0), ctypes.c_uint64(0)
    cap = min(max(4 * nq, 1024), max_candidates)
    for _ in range(2):
        pat, tpos, mism = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint8)
        eng.check(fn(index(), _ptr(blob), _ptr(off), nq, k, max_candidates, _ptr(pat), _ptr(tpos), _ptr(mism), cap, _ptr(first),
                     ctypes.byref(cands), ctypes.byref(count)), name)
        if cands.value > max_candidates:
            raise SuffixHipError(f"{name}: {cands.value} candidates exceed max_candidates = {max_candidates}; use longer patterns, "
                                 "fewer mismatches or raise max_candidates")
        if count.value <= cap:
            break
        cap = int(count.value)
    z = int(count.value)
    tpos, mism = tpos[:z].copy(), mism[:z].copy()
    if sort and z:
        order = np.lexsort((tpos, pat[:z]))                         # (the patterns ascend already: slices stay in place)
        tpos, mism = tpos[order], mism[order]
    return first, tpos, mism


def _edit_positions(eng, fn, name, index, n, queries, errors, max_candidates, max_hits):
    """sfx_index_edit / sfx_gindex_edit on host arrays -> (first uint64, tbegin uint32, tend uint32, dist uint8).  The
    first call guesses the room; a second one follows when there were more."""
    qs = [_as_bytes(q) for q in queries]
    k, max_candidates, max_hits = int(errors), int(max_candidates), int(max_hits)
    if not 0 <= k <= 31:
        raise ValueError("errors must be in 0 .. 31")
    if max_candidates < 1 or not 1 <= max_hits < 1 << 32:
        raise ValueError("max_candidates must be at least 1 and max_hits in 1 .. 2^32 - 1")
    if any(len(q) <= k for q in qs):
        raise ValueError(f"every pattern needs at least errors + 1 = {k + 1} bytes")
    nq = len(qs)
    first = np.zeros(nq + 1, dtype=np.uint64)
    if not nq or not n:
        return first, np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8)
    off = np.zeros(nq + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(q) for q in qs], dtype=np.uint64)
    blob = np.frombuffer(b"".join(qs), dtype=np.uint8)
    max_candidates = min(max_candidates, nq * (k + 1) * n)          # (there are no more candidates)
    max_hits = min(max_hits, max_candidates * (2 * k + 1))
    eng.require_device()
    cands, hits, count = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    cap = min(max(4 * nq, 1024), max_hits)
    for _ in range(2):
        pat, tbegin, tend = (np.zeros(cap, dtype=np.uint32) for _ in range(3))
        dist = np.zeros(cap, dtype=np.uint8)
        eng.check(fn(index(), _ptr(blob), _ptr(off), nq, k, max_candidates, max_hits, _ptr(pat), _ptr(tbegin), _ptr(tend), _ptr(dist), cap,
                     _ptr(first), ctypes.byref(cands), ctypes.byref(hits), ctypes.byref(count)), name)
        if cands.value > max_candidates:
            raise SuffixHipError(f"{name}: {cands.value} candidates exceed max_candidates = {max_candidates}; use longer patterns, "
                                 "fewer errors or raise max_candidates")
        if hits.value > max_hits:
            raise SuffixHipError(f"{name}: {hits.value} hits exceed max_hits = {max_hits}; use longer patterns, fewer errors or raise "
                                 "max_hits")
        if count.value <= cap:
            break
        cap = int(count.value)
    z = int(count.value)
    return first, tbegin[:z].copy(), tend[:z].copy(), dist[:z].copy()


def _bwt_step(sample_step):
    step = int(sample_step or 0)
    if step < 0 or step > 0x80000000 or step & (step - 1):
        raise ValueError("sample_step must be 0 or a power of two of at most 2^31")
    return step


def unbwt(bwt, samples, sample_step, engine=None):
    """The text (bytes) whose Burrows-Wheeler transform is (bwt, samples) as SuffixTable.bwt(sample_step) returns it.
    A pair that is the transform of no text raises SuffixHipError: the walks check themselves (sfx_unbwt)."""
    eng = engine or default_engine()
    b = np.frombuffer(_as_bytes(bwt), dtype=np.uint8)
    sm = np.ascontiguousarray(samples, dtype=np.uint32)
    step = _bwt_step(sample_step)
    out = np.zeros(b.size, dtype=np.uint8)
    if b.size:
        eng.require_device()
    eng.check(eng.lib.sfx_unbwt(_ptr(b), int(b.size), _ptr(sm), int(sm.size), step, _ptr(out)), "sfx_unbwt")
    return out.tobytes()


def unlz(len, src, lit, engine=None):
    """The text (bytes) of the LZ77 phrases (len, src, lit) as LzFactorization holds them: a literal (src 0xFFFFFFFF,
    len 1) is its byte, a copy repeats len bytes from position src < its own begin and may overlap itself.  A list
    that is no factorization raises SuffixHipError (sfx_unlz)."""
    eng = engine or default_engine()
    ln = np.ascontiguousarray(len, dtype=np.uint32)
    sr = np.ascontiguousarray(src, dtype=np.uint32)
    lt = np.frombuffer(_as_bytes(lit), dtype=np.uint8)
    if sr.size != ln.size or lt.size != ln.size:
        raise ValueError("len, src and lit must have one entry per phrase")
    n = int(ln.sum(dtype=np.uint64))
    out = np.zeros(min(n, _NONE), dtype=np.uint8)
    if n:
        eng.require_device()
    eng.check(eng.lib.sfx_unlz(_ptr(ln), _ptr(sr), _ptr(lt), int(ln.size), n, _ptr(out)), "sfx_unlz")
    return out.tobytes()


class LzFactorization:
    """The greedy LZ77 parse of a text (SuffixTable.lz77): numpy arrays begin / len / src (uint32) and lit (uint8), one
    entry per phrase, and the text length n.  len(f) = z; iteration yields (begin, len, src) with src None for a literal."""

    def __init__(self, begin, len, src, lit, n, engine=None):
        self.begin, self.len, self.src, self.lit, self.n = begin, len, src, lit, int(n)
        self._eng = engine

    def __len__(self):
        return int(self.len.size)

    def __iter__(self):
        for b, l, s in zip(self.begin.tolist(), self.len.tolist(), self.src.tolist()):
            yield b, l, (None if s == _NONE else s)

    def decode(self):
        return unlz(self.len, self.src, self.lit, engine=self._eng)

    def __repr__(self):
        return f"LzFactorization(n={self.n}, z={len(self)})"


class Runs:
    """The maximal repetitions of a text (SuffixTable.runs): uint32 arrays begin / end / period, one entry per run,
    ascending by (begin, period).  text[begin:end] has smallest period `period`, is at least two periods long and cannot be
    extended to either side; exponent = (end - begin) / period says how often the unit is written."""

    def __init__(self, begin, end, period, n):
        self.begin, self.end, self.period, self.n = begin, end, period, int(n)

    def __len__(self):
        return int(self.begin.size)

    def triples(self):
        return list(zip(self.begin.tolist(), self.end.tolist(), self.period.tolist()))

    @property
    def exponent(self):
        return (self.end.astype(np.float64) - self.begin) / self.period

    def __repr__(self):
        return f"Runs(n={self.n}, runs={len(self)})"


class SuffixTable:
    def __init__(self, text, _table=None, engine=None):
        self._eng = engine or default_engine()
        self._was_str = isinstance(text, str)
        self._text = _as_bytes(text)
        self._tarr = np.frombuffer(self._text, dtype=np.uint8)
        self._index = None
        self._lce = _LceHandle(self._eng)
        if _table is None:
            # sais_table (:378-386): assert len <= u32::MAX, allocate, fill
            n = self._tarr.size
            table = np.zeros(n, dtype=np.uint32)
            if n:
                self._eng.require_device()
            self._eng.check(self._eng.lib.sfx_build_sa_u32(_ptr(self._tarr), n, _ptr(table)),
                            "SuffixTable::new")
            self._table = table
        else:
            self._table = _table

    # -- constructors -----------------------------------------------------------------
    @classmethod
    def new(cls, text, engine=None):
        return cls(text, engine=engine)

    @classmethod
    def new_naive(cls, text, engine=None):
        """SuffixTable::new_naive (:93-100, #[doc(hidden)]) -> naive_table (:367-376): the definition -- every byte suffix
        sorted by comparison on the host, O(n^2 log n).  Upstream keeps it as the known answer of its own tests
        (tests/tests.rs:18-20) and so does this mirror: it is what a caller compares new() against, never a fallback of
        new() (which has none: it raises without the HIP library or a device)."""
        t = _as_bytes(text)
        if len(t) > 0xFFFFFFFF:
            raise OverflowError("SuffixTable::new_naive: text longer than u32::MAX")      # the table is Vec<u32> (:57)
        table = np.array(sorted(range(len(t)), key=lambda i: t[i:]), dtype=np.uint32)
        return cls(text, _table=table, engine=engine)

    @classmethod
    def new_with_lcp(cls, text, engine=None):
        """SuffixTable::new + lcp_lens in one engine call (sfx_build_sa_lcp_u32): -> (table, lcp array).
        The pair of calls suffix_tree/src/lib.rs:71 + :413 makes; same arrays as new() then lcp_lens()."""
        eng = engine or default_engine()
        tarr = np.frombuffer(_as_bytes(text), dtype=np.uint8)
        n = tarr.size
        table = np.zeros(n, dtype=np.uint32)
        lcp = np.zeros(n, dtype=np.uint32)
        if n:
            eng.require_device()
        eng.check(eng.lib.sfx_build_sa_lcp_u32(_ptr(tarr), n, _ptr(table), _ptr(lcp)), "SuffixTable::new + lcp_lens")
        return cls(text, _table=table, engine=engine), lcp

    @classmethod
    def from_parts(cls, text, table, engine=None):
        """Unchecked, like the reference (:105-119): only the lengths must agree."""
        t = np.ascontiguousarray(table, dtype=np.uint32)
        if len(_as_bytes(text)) != t.size:
            raise AssertionError("text.len() != table.len()")        # assert_eq! :117
        return cls(text, _table=t, engine=engine)

    def into_parts(self):
        text = self._text.decode("utf-8") if self._was_str else self._text
        return text, self._table

    def __del__(self):
        ix, self._index = getattr(self, "_index", None), None
        if ix:
            try:
                self._eng.lib.sfx_index_destroy(ix)
            except Exception:
                pass
        lx = getattr(self, "_lce", None)
        if lx:
            lx.close()

    # -- accessors ----------------------------------------------------------------------
    def table(self):
        return self._table

    def text(self):
        return self._text.decode("utf-8") if self._was_str else self._text

    def len(self):
        return int(self._table.size)

    __len__ = len

    def is_empty(self):
        return self.len() == 0

    def suffix_bytes(self, i):
        return self._text[int(self._table[i]):]

    def suffix(self, i):
        # the reference slices a &str and panics off a char boundary (:168-170)
        return self.suffix_bytes(i).decode("utf-8")

    def __eq__(self, other):                      # derive(PartialEq) on (text, table), :54
        return (isinstance(other, SuffixTable) and self._text == other._text
                and np.array_equal(self._table, other._table))

    # -- LCP ------------------------------------------------------------------------------
    def lcp_lens(self):
        n = self.len()
        lcp = np.zeros(n, dtype=np.uint32)
        if n:
            self._eng.require_device()
        self._eng.check(self._eng.lib.sfx_build_lcp_u32(_ptr(self._tarr), n, _ptr(self._table),
                                                         _ptr(lcp)), "lcp_lens")
        return lcp

    # -- queries ----------------------------------------------------------------------------
    def _ensure_index(self):
        if self._index is None:
            self._eng.require_device()
            h = ctypes.c_void_p()
            self._eng.check(self._eng.lib.sfx_index_create(_ptr(self._tarr), self.len(),
                                                           _ptr(self._table), ctypes.byref(h)),
                            "sfx_index_create")
            self._index = h
        return self._index

    @staticmethod
    def _pack(queries):
        qs = [_as_bytes(q) for q in queries]
        off = np.zeros(len(qs) + 1, dtype=np.uint64)
        if qs:
            off[1:] = np.cumsum([len(q) for q in qs], dtype=np.uint64)
        blob = np.frombuffer(b"".join(qs), dtype=np.uint8)
        return blob, off

    def positions_batch(self, queries):
        """-> (start, end) uint32 arrays; positions(q_k) == table()[start[k]:end[k]]."""
        blob, off = self._pack(queries)
        nq = off.size - 1
        start = np.zeros(nq, dtype=np.uint32)
        end = np.zeros(nq, dtype=np.uint32)
        if nq:
            self._eng.check(self._eng.lib.sfx_positions_batch(self._ensure_index(), _ptr(blob),
                                                               _ptr(off), nq, _ptr(start), _ptr(end)),
                            "positions_batch")
        return start, end

    def contains_batch(self, queries):
        """-> (found bool array, any_position uint32 array with 0xFFFFFFFF = None)."""
        blob, off = self._pack(queries)
        nq = off.size - 1
        found = np.zeros(nq, dtype=np.uint8)
        anyp = np.full(nq, _NONE, dtype=np.uint32)
        if nq:
            self._eng.check(self._eng.lib.sfx_contains_batch(self._ensure_index(), _ptr(blob),
                                                              _ptr(off), nq, _ptr(found), _ptr(anyp)),
                            "contains_batch")
        return found.astype(bool), anyp

    def positions(self, query):
        """Unordered (SA-order) occurrences of `query`, a slice of table() (:223-259)."""
        if self.len() == 0 or len(_as_bytes(query)) == 0:
            return self._table[0:0]
        s, e = self.positions_batch([query])
        return self._table[int(s[0]):int(e[0])]

    def any_position(self, query):
        if self.len() == 0 or len(_as_bytes(query)) == 0:
            return None                                              # :281-283
        _, anyp = self.contains_batch([query])
        return None if int(anyp[0]) == _NONE else int(anyp[0])

    def contains(self, query):
        return self.any_position(query) is not None                  # :197-199

    # -- repeats --------------------------------------------------------------------------------
    def repeat_lens(self, scope="any", with_source=False):
        """rep[p] = the longest common prefix of the suffix at byte p with any other suffix (scope "any") or with any
        suffix that starts earlier ("earlier": the longest-previous-factor array) -- uint32, indexed by text position.
        with_source: -> (rep, src), src[p] = a position that attains rep[p] (which one is arbitrary), 0xFFFFFFFF where
        rep[p] == 0."""
        if scope not in ("any", "earlier"):
            raise ValueError('scope must be "any" or "earlier"')
        return _repeat_lens(self._eng, self._table, self.lcp_lens(), None, scope, with_source)

    def repeated_spans(self, min_len, scope="any"):
        """[(begin, end)] in ascending order: the maximal runs of bytes that lie inside a repeat of at least min_len
        bytes (scope as for repeat_lens; "earlier" keeps the first copy of everything out of the report)."""
        b, e = _repeat_spans(self._eng, self.repeat_lens(scope), min_len, None)
        return list(zip(b.tolist(), e.tolist()))

    # -- longest common extensions -----------------------------------------------------------------
    def inverse_table(self):
        """isa (uint32): isa[table()[r]] = r, the rank of the suffix at every text position (sfx_inverse_table_u32).
        Raises SuffixHipError for a table (from_parts) that is no permutation of the positions."""
        n = self.len()
        isa = np.zeros(n, dtype=np.uint32)
        if n:
            self._eng.require_device()
        self._eng.check(self._eng.lib.sfx_inverse_table_u32(_ptr(self._table), n, _ptr(isa)), "sfx_inverse_table_u32")
        return isa

    def _lce_index(self):
        return self._lce.get(self._table, self.lcp_lens)             # (the LCP array is built for the first call only)

    def lce_batch(self, a, b, mismatches=0):
        """len (uint32): how far the suffixes at byte positions a[q] and b[q] agree when up to `mismatches` bytes may
        differ (one budget for the batch) -- the largest l with at most that many differing places among the first l
        bytes, never past the end of the text.  A position equal to len() gives 0, one above 0xFFFFFFFF; a[q] == b[q]
        gives the rest of the text.  The handle (inverse table + min-tree over lcp_lens()) is made on the first call."""
        return self._lce.lce(self._lce_index, a, b, mismatches)

    def lce(self, i, j, mismatches=0):
        return int(self.lce_batch([int(i)], [int(j)], mismatches)[0])

    def lcp_range_min_batch(self, lo, hi):
        """min lcp_lens()[lo[q]:hi[q]] (uint32); 0xFFFFFFFF for an empty range or hi > len()."""
        return self._lce.range_min(self._lce_index, lo, hi)

    def lcp_range_min(self, lo, hi):
        return int(self.lcp_range_min_batch([int(lo)], [int(hi)])[0])

    def lcp_range_argmin_batch(self, lo, hi):
        """The smallest index that attains min lcp_lens()[lo[q]:hi[q]] (uint32); 0xFFFFFFFF for an empty range or
        hi > len()."""
        return self._lce.range_argmin(self._lce_index, lo, hi)

    def lcp_range_argmin(self, lo, hi):
        return int(self.lcp_range_argmin_batch([int(lo)], [int(hi)])[0])

    # -- suffix-tree navigation --------------------------------------------------------------------
    def substring_intervals_batch(self, pos, length):
        """(lo, hi, depth), uint32 each: table()[lo[q]:hi[q]] are the occurrences of text[pos[q] : pos[q] + length[q]],
        found from the position alone -- no byte of the substring is read (sfx_lce_substr).  depth is the string depth
        of the lowest suffix-tree node at or below the substring's locus.  length 0 gives (0, len(), 0); a substring
        that leaves the text gives 0xFFFFFFFF three times."""
        return self._lce.substr(self._lce_index, pos, length)

    def substring_interval(self, pos, length):
        """(lo, hi) of one substring; raises IndexError for one that is not inside the text."""
        lo, hi, _ = self.substring_intervals_batch([int(pos)], [int(length)])
        if int(lo[0]) == _NONE:
            raise IndexError(f"text[{int(pos)}:{int(pos) + int(length)}] is not inside the text")
        return int(lo[0]), int(hi[0])

    def substring_count(self, pos, length):
        """How often text[pos : pos + length] occurs."""
        lo, hi = self.substring_interval(pos, length)
        return hi - lo

    def lca_batch(self, a, b):
        """(lo, hi, depth), uint32 each: the lowest common ancestor of the suffixes at positions a[q] and b[q] as a rank
        interval with its string depth -- their longest common prefix (sfx_lce_lca).  a[q] == b[q] gives the suffix's own
        rank; a position >= len() gives 0xFFFFFFFF three times."""
        return self._lce.lca(self._lce_index, a, b)

    def lca(self, i, j):
        """(lo, hi, depth) for one pair of positions; raises IndexError for a position >= len()."""
        lo, hi, d = self.lca_batch([int(i)], [int(j)])
        if int(lo[0]) == _NONE:
            raise IndexError(f"({int(i)}, {int(j)}): no positions of the text")
        return int(lo[0]), int(hi[0]), int(d[0])

    # -- Burrows-Wheeler transform ----------------------------------------------------------------
    def bwt(self, sample_step=256):
        """-> (bwt bytes, samples uint32): the last column of the sorted rotations of text$ without its $ entry, and the
        row of the suffix at every sample_step-th text position (samples[0] = the primary row; 0: the primary only).
        `suffix_amd.unbwt(bwt, samples, sample_step)` restores the text."""
        step = _bwt_step(sample_step)
        n = self.len()
        out = np.zeros(n, dtype=np.uint8)
        samples = np.zeros(int(self._eng.lib.sfx_bwt_sample_count(n, step)), dtype=np.uint32)
        if n:
            self._eng.require_device()
            self._eng.check(self._eng.lib.sfx_bwt_u32(_ptr(self._tarr), n, _ptr(self._table), step, _ptr(out), _ptr(samples)),
                            "sfx_bwt_u32")
        return out.tobytes(), samples

    # -- LZ77 factorization ---------------------------------------------------------------------------
    def lz77(self, min_len=1):
        """The greedy LZ77 factorization (LzFactorization): every phrase is the longest prefix of what is left that also
        starts at an earlier position -- it may run into itself -- when that is at least min_len bytes, else one literal
        byte.  min_len = 1 is the classical parse; len(result) is the phrase count z."""
        min_len = int(min_len)
        if min_len < 1 or min_len > 0xFFFFFFFF:
            raise ValueError("min_len must be in 1 .. 2^32 - 1")
        n = self.len()
        arrs = [np.zeros(n, dtype=np.uint32) for _ in range(3)] + [np.zeros(n, dtype=np.uint8)]
        count = ctypes.c_uint64(0)
        if n:
            self._eng.require_device()
            self._eng.check(self._eng.lib.sfx_lz77_u32(_ptr(self._tarr), n, _ptr(self._table), None, min_len, *[_ptr(a) for a in arrs],
                                                       n, ctypes.byref(count)), "sfx_lz77_u32")
        z = int(count.value)
        return LzFactorization(*[a[:z].copy() for a in arrs], n, engine=self._eng)

    # -- maximal repetitions, Lyndon array ------------------------------------------------------------
    def lyndon_array(self, order=0):
        """lyn (uint32): lyn[i] = the length of the longest Lyndon word that starts at byte i, under byte order (order
        0) or reversed byte order (order 1); in both a proper prefix is smaller than its extension.  Order 1 builds the
        table of the complemented text (sfx_lyndon_array_u32)."""
        if order not in (0, 1):
            raise ValueError("order must be 0 (byte order) or 1 (reversed byte order)")
        n = self.len()
        lyn = np.zeros(n, dtype=np.uint32)
        if n:
            self._eng.require_device()
            self._eng.check(self._eng.lib.sfx_lyndon_array_u32(_ptr(self._tarr), n, _ptr(self._table) if order == 0 else None, order,
                                                               _ptr(lyn)), "sfx_lyndon_array_u32")
        return lyn

    def lyndon_factorization(self):
        """The starts (int64) of the Lyndon factors of the text: 0, then every start plus the Lyndon word at it."""
        lyn = self.lyndon_array(0)
        starts, i, n = [], 0, self.len()
        while i < n:
            starts.append(i)
            i += int(lyn[i])
        return np.asarray(starts, dtype=np.int64)

    def runs(self, min_period=1, max_period=None, min_len=0):
        """The maximal repetitions (Runs) -- the tandem repeats of the text: every (begin, end, period) such that period
        is the smallest period of text[begin:end], end - begin >= 2 * period and the repetition extends to neither side;
        kept when min_period <= period <= max_period (None: no limit) and end - begin >= min_len."""
        if max_period is not None and int(max_period) < 1:
            raise ValueError("max_period must be at least 1 (None: no limit)")
        for v in (min_period, min_len, max_period or 0):
            if not 0 <= int(v) <= _NONE:
                raise ValueError("filters must be in 0 .. 2^32 - 1")
        n = self.len()
        arrs = [np.zeros(n, dtype=np.uint32) for _ in range(3)]
        count = ctypes.c_uint64(0)
        flt = RunsFilter(int(min_period), 0 if max_period is None else int(max_period), int(min_len), 0)
        if n:
            self._eng.require_device()
            self._eng.check(self._eng.lib.sfx_runs_u32(_ptr(self._tarr), n, _ptr(self._table), None, ctypes.byref(flt),
                                                       *[_ptr(a) for a in arrs], n, ctypes.byref(count)), "sfx_runs_u32")
        z = int(count.value)
        return Runs(*[a[:z].copy() for a in arrs], n)

    def fm_index(self, sample_step=64, occ_step=0):
        """An FmIndex over this table's transform: the same positions() / contains() / count() from about 1.4 n bytes
        of HBM, without the text or the table."""
        b, sm = self.bwt(sample_step)
        return FmIndex.from_bwt(b, sm, sample_step, occ_step=occ_step, engine=self._eng)

    # -- matching statistics of a second text ---------------------------------------------------
    def match_stats(self, query, max_len=None, with_source=False, with_intervals=False):
        """len[i] = the longest prefix of query[i:] (at most max_len bytes; None = no cap) that occurs in the text --
        uint32, one entry per query byte.  -> len, or the tuple (len[, src][, start, end]): src[i] = a text position
        where those bytes stand (which one is arbitrary), 0xFFFFFFFF where len[i] == 0; table()[start[i]:end[i]] =
        every such position (0 / 0 where len[i] == 0).  The cost grows with the lengths found: cap a query that may
        repeat the text itself."""
        return _match_stats(self._eng, self._eng.lib.sfx_index_match_stats, "sfx_index_match_stats", self._ensure_index,
                            self.len(), query, max_len, with_source, with_intervals)

    def shared_spans(self, query, min_len):
        """[(begin, end)] in query coordinates, ascending: the maximal runs of query bytes that lie inside a stretch of
        at least min_len bytes which also occurs in the text."""
        return _shared_spans(self._eng, self.match_stats, query, min_len)

    def mems(self, query, min_len, unique=False, max_pairs=1 << 30):
        """The maximal exact matches (Mems) of at least min_len bytes between `query` and the text: triples
        (qpos, tpos, len) with query[qpos : qpos + len] == text[tpos : tpos + len] that can be extended neither to the
        left nor to the right, ascending by qpos and then by the table rank of tpos.  unique: only those whose bytes
        occur once in the text (MUMmer's -mumreference; the default is its -maxmatch).
        The work grows with the number of candidate pairs -- a shared stretch of M bytes is M - min_len + 1 of them,
        two copies of a^n about n^2 / 2 -- so a call that would look at more than max_pairs raises SuffixHipError
        naming the count; raise min_len or max_pairs then.  The pair kernel takes 46.5 G pairs/s against 10^9 bytes
        of DNA on an MI355X (more while the text fits the cache): the default of 2^30 pairs is
        about 25 ms of it, and a buffer of up to 12 bytes per pair for the matches."""
        return Mems(*_mems(self._eng, self._eng.lib.sfx_index_mems, "sfx_index_mems", self._ensure_index, self.len(), query,
                           min_len, unique, max_pairs))

    # -- k-mismatch pattern search ------------------------------------------------------------------
    def approx_positions_batch(self, queries, mismatches, max_candidates=1 << 30, sort=False):
        """Where do the queries occur if up to `mismatches` (0 .. 255) bytes may differ (Hamming distance: no insertions
        or deletions)?  -> (first, tpos, mism): the occurrences of queries[j] are tpos[first[j]:first[j + 1]] (uint32
        window starts) with mism[...] differing bytes each (uint8).  A slice is ordered by the owning piece of the
        pigeonhole cut, then by table rank -- at mismatches = 0 it is positions(q) exactly; sort=True orders every slice
        by position, on the host.  An empty query has no occurrence.
        The work grows with the exact hits of the k + 1 pieces of every query, the candidates: a call that would look
        at more than max_candidates raises SuffixHipError naming the count."""
        return _approx_positions(self._eng, self._eng.lib.sfx_index_hamming, "sfx_index_hamming", self._ensure_index, self.len(),
                                 queries, mismatches, max_candidates, sort)

    def approx_positions(self, query, mismatches):
        """(positions, mismatches) of `query` with up to `mismatches` differing bytes: uint32 window starts ascending
        and the uint8 number of differing bytes of each."""
        _, tpos, mism = self.approx_positions_batch([query], mismatches, sort=True)
        return tpos, mism

    # -- k-error pattern search ---------------------------------------------------------------------
    def edit_positions_batch(self, queries, errors, max_candidates=1 << 30, max_hits=1 << 22):
        """Where do the queries occur within `errors` (0 .. 31) substitutions, insertions and deletions (unit-cost edit
        distance)?  -> (first, tbegin, tend, dist): the occurrences of queries[j] are the entries first[j]:first[j + 1],
        ascending by tend.  An occurrence is an END position tend for which some text[s:tend] is within `errors` edits
        of the query; dist (uint8) is the least such distance and tbegin (uint32) the largest s that attains it.
        Neighbouring ends of one alignment are occurrences of their own.  Every query needs more than `errors` bytes
        (ValueError otherwise: it would occur everywhere).
        The work grows with the exact hits of the k + 1 pieces of every query, the candidates, and with the (candidate,
        end) pairs they find: more than max_candidates or max_hits raise SuffixHipError naming the count."""
        return _edit_positions(self._eng, self._eng.lib.sfx_index_edit, "sfx_index_edit", self._ensure_index, self.len(), queries, errors,
                               max_candidates, max_hits)

    def edit_positions(self, pattern, k):
        """[(begin, end, dist)] of `pattern` within k edits, ascending by end (see edit_positions_batch)."""
        _, tbegin, tend, dist = self.edit_positions_batch([pattern], k)
        return list(zip(tbegin.tolist(), tend.tolist(), dist.tolist()))

    def __repr__(self):                                              # Debug, :296-312
        lines = ["", "-----------------------------------------", "SUFFIX TABLE",
                 f"text: {self.text()}"]
        for rank, s in enumerate(self._table.tolist()):
            lines.append(f"suffix[{rank}] {s}, {self._text[s:].decode('utf-8', 'replace')}")
        lines.append("-----------------------------------------")
        return "\n".join(lines) + "\n"


class FmIndex:
    """Backward search over the Burrows-Wheeler pair of SuffixTable.bwt(): count(), contains() and positions() of a
    pattern from (bwt, samples) alone (sfx_fm_*; include/suffix_hip.h).  The handle lives in HBM (`nbytes`); neither the
    text nor the table is kept.  A pattern of m bytes costs m steps whatever the text's length; every position costs at
    most sample_step - 1 more."""

    def __init__(self, handle, engine):
        self._eng, self._h = engine, handle
        info = FmInfo()
        engine.check(engine.lib.sfx_fm_info(handle, ctypes.byref(info)), "sfx_fm_info")
        self.info = info.as_dict()

    @classmethod
    def from_bwt(cls, bwt, samples, sample_step, occ_step=0, engine=None):
        """(bwt, samples) as SuffixTable.bwt(sample_step) returns them.  Creation checks the samples, not that the
        pair is a transform (suffix_amd.unbwt does)."""
        eng = engine or default_engine()
        b = np.frombuffer(_as_bytes(bwt), dtype=np.uint8)
        sm = np.ascontiguousarray(samples, dtype=np.uint32)
        step = _bwt_step(sample_step)
        if b.size:
            eng.require_device()
        h = ctypes.c_void_p()
        eng.check(eng.lib.sfx_fm_create(_ptr(b), int(b.size), _ptr(sm), int(sm.size), step, int(occ_step), ctypes.byref(h)),
                  "sfx_fm_create")
        return cls(h, eng)

    @classmethod
    def from_text(cls, text, sample_step=64, occ_step=0, engine=None):
        return SuffixTable(text, engine=engine).fm_index(sample_step, occ_step)

    def len(self):
        return self.info["n"]

    __len__ = len

    @property
    def nbytes(self):
        return self.info["bytes"]

    def count_batch(self, queries):
        """-> (start, end) uint32 arrays of table ranks, as SuffixTable.positions_batch."""
        blob, off = SuffixTable._pack(queries)
        nq = off.size - 1
        start = np.zeros(nq, dtype=np.uint32)
        end = np.zeros(nq, dtype=np.uint32)
        if nq:
            self._eng.check(self._eng.lib.sfx_fm_count(self._h, _ptr(blob), _ptr(off), nq, _ptr(start), _ptr(end)), "sfx_fm_count")
        return start, end

    def count(self, query):
        s, e = self.count_batch([query])
        return int(e[0]) - int(s[0])

    def contains(self, query):
        return self.count(query) > 0

    def lookup(self, ranks=None, first=0, count=None):
        """Table entries of the given ranks (uint32 array), or of first .. first + count - 1; 0xFFFFFFFF for a rank >= n."""
        if ranks is not None:
            r = np.ascontiguousarray(ranks, dtype=np.uint32)
            count = int(r.size)
        else:
            r, count = None, max(0, int(self.len() - first if count is None else count))
        pos = np.zeros(count, dtype=np.uint32)
        self._eng.check(self._eng.lib.sfx_fm_lookup(self._h, _ptr(r) if r is not None else None, int(first), count, _ptr(pos)),
                        "sfx_fm_lookup")
        return pos

    def positions(self, query):
        """The occurrences of `query` in table order: element for element SuffixTable.positions(query)."""
        s, e = self.count_batch([query])
        return self.lookup(first=int(s[0]), count=int(e[0]) - int(s[0]))

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._eng.lib.sfx_fm_destroy(h)

    __del__ = close
