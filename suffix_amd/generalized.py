"""`GeneralizedSuffixTable` -- one suffix table over many documents, the capability the reference names as
missing (/root/reference/README.md:60-74) and approximates by joining the documents with a separator byte.

Here no separator is involved: documents may hold any byte, no suffix runs past the end of its document, and
no match spans two documents.

    table()          every (document, offset) as the text position doc_starts[i] + offset, ordered by the
                     TRUNCATED suffix D_i[offset..] (a proper prefix first; equal ones by document index)
    doc_array()      the document of every table entry
    lcp_lens()       common prefix of neighbouring truncated suffixes (0 first)
    positions(q)     [(doc, offset)] of every occurrence of q, in table order
    documents(q)     sorted distinct documents containing q; document_frequency(q) = their number
    document_listing(q, order, top_k)         (docs, tf): those documents with q's count in each, by id or ranked by count
    interval_documents(start, end, ...)       the same for any rank interval of the table
    document_counts()             distinct documents under every lcp-interval (per boundary of the table)
    interval_document_frequency(start, end)   the same for any pattern's rank interval, from two prefix sums
    common_substring_lengths()    the longest string common to at least d documents, for every d
    longest_common_substring(min_docs)        the bytes of one, and in how many documents they occur
    repeat_lens(scope)            longest repeat starting at every position: anywhere, earlier, or in another document
    repeated_spans(min_len, ...)  [(document, begin_offset, end_offset)] of the bytes inside such repeats
    match_stats(query, max_len)   longest match of every suffix of a NEW text inside one document of the collection
    shared_spans(query, min_len)  [(begin, end)] of the query bytes inside such matches of at least min_len bytes
    mems(query, min_len, unique)  the maximal exact matches of a NEW text, each inside one document
    approx_positions(query, k)    the occurrences with up to k differing bytes, each inside one document
    lce((doc, off), (doc, off), mismatches)   how far two suffixes of the collection agree, never past a document end
    extend(docs, match_limit)     a NEW table over these documents followed by `docs`: only the added ones are built, then merged in
    merge(other, match_limit)     the same for two existing tables, from the arrays both already hold

Construction and queries run on the GPU through the C ABI (sfx_build_gsa_u32, sfx_gindex_*); there is no CPU
path except `new_naive`, the definition itself.
"""
import ctypes

import numpy as np

from ._lib import default_engine
from .table import Mems, _LceHandle, _approx_positions, _as_bytes, _edit_positions, _match_stats, _mems, _ptr, _repeat_lens, _repeat_spans, _shared_spans

_NONE = 0xFFFFFFFF
_DOCLIST_ORDERS = {"doc": 0, "tf": 1}


class GeneralizedSuffixTable:
    def __init__(self, docs, engine=None, _arrays=None):
        self._eng = engine or default_engine()
        docs = list(docs)
        self._was_str = [isinstance(d, str) for d in docs]
        self._docs = [_as_bytes(d) for d in docs]
        self._text = b"".join(self._docs)
        self._tarr = np.frombuffer(self._text, dtype=np.uint8)
        starts = np.zeros(len(self._docs), dtype=np.uint64)
        if len(self._docs) > 1:
            starts[1:] = np.cumsum([len(d) for d in self._docs[:-1]], dtype=np.uint64)
        self._starts = starts
        self._index = None
        self._lce = _LceHandle(self._eng)
        self._doclist = None                             # the sfx_doclist handle: made on first use
        self._counts = self._common_arrays = None        # (df, dup_prefix) / (len, pos): made on first use
        n = self._tarr.size
        if n > 0xFFFFFFFF:
            raise OverflowError("GeneralizedSuffixTable: more than u32::MAX bytes in all")
        if _arrays is not None:
            self._table, self._da, self._lcp = _arrays
            return
        table = np.zeros(n, dtype=np.uint32)
        da = np.zeros(n, dtype=np.uint32)
        lcp = np.zeros(n, dtype=np.uint32)
        if n:
            self._eng.require_device()
            self._eng.check(self._eng.lib.sfx_build_gsa_u32(_ptr(self._tarr), n, _ptr(starts), starts.size, _ptr(table),
                                                             _ptr(da), _ptr(lcp)), "GeneralizedSuffixTable::new")
        self._table, self._da, self._lcp = table, da, lcp

    # -- constructors -----------------------------------------------------------------------
    @classmethod
    def new(cls, docs, engine=None):
        return cls(docs, engine=engine)

    @classmethod
    def new_naive(cls, docs, engine=None):
        """The definition on the host: every (document, offset) sorted by (truncated suffix, document) with Python's
        byte comparison, the LCP by direct comparison.  O(N^2 log N) in the worst case (N = total bytes): meant for
        collections of up to a few thousand bytes, as the known answer of tests -- never a fallback of new()."""
        bdocs = [_as_bytes(d) for d in docs]
        items = [(d, o) for d, doc in enumerate(bdocs) for o in range(len(doc))]
        items.sort(key=lambda it: (bdocs[it[0]][it[1]:], it[0]))
        starts = np.zeros(len(bdocs), dtype=np.int64)
        if len(bdocs) > 1:
            starts[1:] = np.cumsum([len(b) for b in bdocs[:-1]])
        table = np.array([starts[d] + o for d, o in items], dtype=np.uint32)
        da = np.array([d for d, _ in items], dtype=np.uint32)
        lcp = np.zeros(len(items), dtype=np.uint32)
        for r in range(1, len(items)):
            a = bdocs[items[r - 1][0]][items[r - 1][1]:]
            b = bdocs[items[r][0]][items[r][1]:]
            k, m = 0, min(len(a), len(b))
            while k < m and a[k] == b[k]:
                k += 1
            lcp[r] = k
        return cls(docs, engine=engine, _arrays=(table, da, lcp))

    # -- adding documents without a rebuild ----------------------------------------------------
    last_extend_route = None                             # "merge" | "rebuild": what made this table in extend() / merge()

    def _grown(self, docs, arrays, route):
        g = type(self)(docs, engine=self._eng, _arrays=arrays)
        g.last_extend_route = route
        return g

    def extend(self, docs, match_limit=1 << 16):
        """A NEW table over this table's documents followed by `docs`, equal in all three arrays to new() of all of them;
        this one stays as it is.  Only the added documents are built; their suffixes are then ranked among the old ones
        and the arrays merged in one pass (sfx_gsa_extend_u32).  An added suffix that shares more than match_limit bytes
        with an old one (a near-copy of a long document: the ranking would compare a number of bytes quadratic in its
        length) makes the call build the whole collection instead; match_limit 0 never does.  The new table's
        last_extend_route says which ran: "merge" or "rebuild"."""
        docs = list(docs)
        whole = [self.document(i) for i in range(self.num_docs())] + docs
        bdocs = self._docs + [_as_bytes(d) for d in docs]
        n = sum(len(d) for d in bdocs)
        if n > 0xFFFFFFFF:
            raise OverflowError("GeneralizedSuffixTable.extend: more than u32::MAX bytes in all")
        match_limit = int(match_limit)
        if not 0 <= match_limit <= _NONE:
            raise ValueError("match_limit must be in 0 .. 2^32 - 1")
        table, da, lcp = (np.zeros(n, dtype=np.uint32) for _ in range(3))
        route = ctypes.c_uint32(1)
        if n:
            self._eng.require_device()
            text = np.frombuffer(b"".join(bdocs), dtype=np.uint8)
            starts = np.zeros(len(bdocs), dtype=np.uint64)
            starts[1:] = np.cumsum([len(d) for d in bdocs[:-1]], dtype=np.uint64)
            longest = ctypes.c_uint64(0)
            self._eng.check(self._eng.lib.sfx_gsa_extend_u32(_ptr(text), n, _ptr(starts), starts.size, len(self._docs), _ptr(self._table),
                                                              _ptr(self._da), _ptr(self._lcp), match_limit, 1, _ptr(table), _ptr(da), _ptr(lcp),
                                                              ctypes.byref(longest), ctypes.byref(route)), "sfx_gsa_extend_u32")
        return self._grown(whole, (table, da, lcp), {1: "merge", 2: "rebuild"}[int(route.value)])

    def merge(self, other, match_limit=1 << 16):
        """As extend() for two existing tables: a NEW table over this table's documents followed by `other`'s, from the
        arrays both already hold (sfx_gsa_merge_u32); beyond match_limit, one build of the whole collection."""
        whole = [t.document(i) for t in (self, other) for i in range(t.num_docs())]
        bdocs = self._docs + other._docs
        n_a, n_b = self.len(), other.len()
        n = n_a + n_b
        if n > 0xFFFFFFFF:
            raise OverflowError("GeneralizedSuffixTable.merge: more than u32::MAX bytes in all")
        match_limit = int(match_limit)
        if not 0 <= match_limit <= _NONE:
            raise ValueError("match_limit must be in 0 .. 2^32 - 1")
        table, da, lcp = (np.zeros(n, dtype=np.uint32) for _ in range(3))
        if n:
            self._eng.require_device()
            text = np.frombuffer(b"".join(bdocs), dtype=np.uint8)
            starts = np.zeros(len(bdocs), dtype=np.uint64)
            starts[1:] = np.cumsum([len(d) for d in bdocs[:-1]], dtype=np.uint64)
            longest = ctypes.c_uint64(0)
            self._eng.check(self._eng.lib.sfx_gsa_merge_u32(_ptr(text), _ptr(starts), starts.size, len(self._docs), _ptr(self._table),
                                                             _ptr(self._da), _ptr(self._lcp), n_a, _ptr(other._table), _ptr(other._da),
                                                             _ptr(other._lcp), n_b, match_limit, _ptr(table), _ptr(da), _ptr(lcp),
                                                             ctypes.byref(longest)), "sfx_gsa_merge_u32")
            if match_limit and longest.value > match_limit:
                g = type(self)(whole, engine=self._eng)
                g.last_extend_route = "rebuild"
                return g
        return self._grown(whole, (table, da, lcp), "merge")

    def __del__(self):
        ix, self._index = getattr(self, "_index", None), None
        if ix:
            try:
                self._eng.lib.sfx_gindex_destroy(ix)
            except Exception:
                pass
        lx = getattr(self, "_lce", None)
        if lx:
            lx.close()
        dx, self._doclist = getattr(self, "_doclist", None), None
        if dx:
            try:
                self._eng.lib.sfx_doclist_destroy(dx)
            except Exception:
                pass

    # -- accessors --------------------------------------------------------------------------
    def table(self):
        return self._table

    def doc_array(self):
        return self._da

    def lcp_lens(self):
        return self._lcp

    def doc_starts(self):
        return self._starts

    def len(self):
        return int(self._table.size)

    __len__ = len

    def is_empty(self):
        return self.len() == 0

    def num_docs(self):
        return len(self._docs)

    def document(self, i):
        d = self._docs[i]
        return d.decode("utf-8") if self._was_str[i] else d

    def position(self, r):
        """-> (document, offset inside it) of table()[r]."""
        d = int(self._da[r])
        return d, int(self._table[r]) - int(self._starts[d])

    def suffix_bytes(self, r):
        d, o = self.position(r)
        return self._docs[d][o:]

    def suffix(self, r):
        return self.suffix_bytes(r).decode("utf-8")

    # -- queries ----------------------------------------------------------------------------
    def _ensure_index(self):
        if self._index is None:
            self._eng.require_device()
            h = ctypes.c_void_p()
            self._eng.check(self._eng.lib.sfx_gindex_create(_ptr(self._tarr), self.len(), _ptr(self._starts), self._starts.size,
                                                             _ptr(self._table), _ptr(self._da), ctypes.byref(h)),
                            "sfx_gindex_create")
            self._index = h
        return self._index

    def query_batch(self, queries):
        """-> dict of uint32 arrays start, end (table()[start:end] = the matches; 0/0 when none), found (bool),
        any (a position or 0xFFFFFFFF), ndocs (distinct documents containing the query)."""
        qs = [_as_bytes(q) for q in queries]
        nq = len(qs)
        off = np.zeros(nq + 1, dtype=np.uint64)
        if qs:
            off[1:] = np.cumsum([len(q) for q in qs], dtype=np.uint64)
        blob = np.frombuffer(b"".join(qs), dtype=np.uint8)
        out = {"start": np.zeros(nq, dtype=np.uint32), "end": np.zeros(nq, dtype=np.uint32),
               "found": np.zeros(nq, dtype=np.uint8), "any": np.full(nq, _NONE, dtype=np.uint32),
               "ndocs": np.zeros(nq, dtype=np.uint32)}
        if nq and self.len():
            self._eng.check(self._eng.lib.sfx_gindex_query(self._ensure_index(), _ptr(blob), _ptr(off), nq, _ptr(out["start"]),
                                                            _ptr(out["end"]), _ptr(out["found"]), _ptr(out["any"]),
                                                            _ptr(out["ndocs"])), "sfx_gindex_query")
        out["found"] = out["found"].astype(bool)
        return out

    def _pairs(self, s, e):
        d = self._da[s:e].astype(np.int64)
        o = self._table[s:e].astype(np.int64) - self._starts[d].astype(np.int64)
        return list(zip(d.tolist(), o.tolist()))

    def positions_batch(self, queries):
        res = self.query_batch(queries)
        return [self._pairs(int(s), int(e)) for s, e in zip(res["start"], res["end"])]

    def positions(self, query):
        """[(document, offset)] of every occurrence of `query` inside one document, in table order."""
        return self.positions_batch([query])[0]

    def contains_batch(self, queries):
        return self.query_batch(queries)["found"]

    def contains(self, query):
        return bool(self.contains_batch([query])[0])

    def any_position_batch(self, queries):
        res = self.query_batch(queries)
        out = []
        for p in res["any"].tolist():
            if p == _NONE:
                out.append(None)
            else:
                d = int(np.searchsorted(self._starts, p, side="right")) - 1
                out.append((d, p - int(self._starts[d])))
        return out

    def any_position(self, query):
        """(document, offset) of some occurrence, or None (the empty query included, as SuffixTable)."""
        return self.any_position_batch([query])[0]

    def _doclist_index(self):
        """The sfx_doclist handle, made by the first listing (sfx_doclist_create copies da and doc_starts) and kept."""
        if self._doclist is None:
            self._eng.require_device()
            h = ctypes.c_void_p()
            self._eng.check(self._eng.lib.sfx_doclist_create(_ptr(self._da), self.len(), _ptr(self._starts), self._starts.size, 0,
                                                             ctypes.byref(h)), "sfx_doclist_create")
            self._doclist = h
        return self._doclist

    def _list_intervals(self, start, end, order, top_k):
        """-> (doc, tf, first) of sfx_doclist_list for the rank intervals [start[j], end[j])."""
        if order not in _DOCLIST_ORDERS:
            raise ValueError(f"order must be one of {sorted(_DOCLIST_ORDERS)}")
        top_k = int(top_k)
        if not 0 <= top_k <= _NONE:
            raise ValueError("top_k must be in 0 .. 2^32 - 1")
        s, e = np.ascontiguousarray(start, dtype=np.uint32), np.ascontiguousarray(end, dtype=np.uint32)
        nq = int(s.size)
        first = np.zeros(nq + 1, dtype=np.uint64)
        cap = int(np.minimum(e.astype(np.int64) - s.astype(np.int64), max(self._starts.size, 1)).sum()) if nq else 0
        doc, tf = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
        if cap:
            listed, count = ctypes.c_uint64(0), ctypes.c_uint64(0)
            self._eng.check(self._eng.lib.sfx_doclist_list(self._doclist_index(), _ptr(s), _ptr(e), nq, _DOCLIST_ORDERS[order], top_k, cap,
                                                           _ptr(doc), _ptr(tf), cap, _ptr(first), ctypes.byref(listed), ctypes.byref(count)),
                            "sfx_doclist_list")
            doc, tf = doc[:int(count.value)], tf[:int(count.value)]
        return doc, tf, first

    def document_listing_batch(self, queries, order="doc", top_k=0):
        """Per query one (docs, tf) pair of uint32 arrays: the documents that contain it and how often it occurs in each,
        ascending by document id (order "doc") or by descending count with ties by id ("tf"); top_k > 0 keeps the first
        top_k entries of that order.  One search and one listing call for the batch."""
        res = self.query_batch(queries)
        doc, tf, first = self._list_intervals(res["start"], res["end"], order, top_k)
        return [(doc[int(a):int(b)], tf[int(a):int(b)]) for a, b in zip(first[:-1], first[1:])]

    def document_listing(self, query, order="doc", top_k=0):
        return self.document_listing_batch([query], order=order, top_k=top_k)[0]

    def interval_documents(self, start, end, order="doc", top_k=0):
        """(docs, tf) for any rank interval of the table -- table()[start:end], e.g. a tree node's lb .. rb + 1."""
        start, end = int(start), int(end)
        if not 0 <= start <= end <= self.len():
            raise IndexError("interval_documents: not a rank interval of the table")
        doc, tf, _ = self._list_intervals([start], [end], order, top_k)
        return doc, tf

    def documents_batch(self, queries):
        return [d.tolist() for d, _ in self.document_listing_batch(queries)]

    def documents(self, query):
        """Sorted distinct ids of the documents that contain `query`."""
        return self.documents_batch([query])[0]

    def document_frequency_batch(self, queries):
        return self.query_batch(queries)["ndocs"]

    def document_frequency(self, query):
        return int(self.document_frequency_batch([query])[0])

    # -- what the documents share ---------------------------------------------------------------
    def _doc_counts(self):
        """(df, dup_prefix), made by the first call that needs them (sfx_doc_counts_u32) and kept."""
        if self._counts is None:
            n = self.len()
            df, dup = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
            if n:
                self._eng.require_device()
                self._eng.check(self._eng.lib.sfx_doc_counts_u32(_ptr(self._da), _ptr(self._lcp), n, self._starts.size, _ptr(dup), _ptr(df)),
                                "sfx_doc_counts_u32")
            self._counts = (df, dup)
        return self._counts

    def _common(self):
        """(len, pos) of sfx_common_substrings_u32, likewise."""
        if self._common_arrays is None:
            nd = self._starts.size
            ln, pos = np.zeros(nd, dtype=np.uint32), np.full(nd, _NONE, dtype=np.uint32)
            if nd and self.len():
                df = self.document_counts()
                self._eng.check(self._eng.lib.sfx_common_substrings_u32(_ptr(self._table), _ptr(self._lcp), _ptr(df), self.len(), _ptr(self._starts),
                                                                        nd, _ptr(ln), _ptr(pos)), "sfx_common_substrings_u32")
            self._common_arrays = (ln, pos)
        return self._common_arrays

    def document_counts(self):
        """df[p] (uint32, per boundary p between ranks p - 1 and p) = the number of distinct documents among the ranks of
        the lcp-interval that boundary belongs to; boundary 0 and every boundary of depth 0 give the number of non-empty
        documents."""
        return self._doc_counts()[0]

    def interval_document_frequency(self, start, end):
        """Distinct documents among table()[start:end] for a rank interval as query_batch returns it (all occurrences of
        one string): two reads of the prefix sums kept with the table.  Scalars or arrays; an empty interval gives 0."""
        dup = self._doc_counts()[1].astype(np.int64)
        s, e = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
        if ((s < 0) | (e > self.len()) | (s > e)).any():
            raise IndexError("interval_document_frequency: not a rank interval of the table")
        ok = e > s
        last, first = np.where(ok, e - 1, 0), np.where(ok, s, 0)
        out = np.where(ok, (e - s) - (dup[last] - dup[first]) if dup.size else 0, 0)
        return int(out) if out.ndim == 0 else out.astype(np.uint32)

    def common_substring_lengths(self):
        """len[d - 1] (uint32, d = 1 .. num_docs()) = the length of the longest string that occurs in at least d distinct
        documents; 0 where there is none."""
        return self._common()[0]

    def longest_common_substring(self, min_docs=None):
        """(bytes, document count) of the longest string that occurs in at least min_docs distinct documents -- None:
        in every non-empty one.  The count is that of the string itself (>= min_docs).  More documents than there are
        non-empty ones, or nothing in common: (b"", 0)."""
        nonempty = sum(1 for d in self._docs if d)
        k = nonempty if min_docs is None else int(min_docs)
        if k < 1:
            raise ValueError("min_docs must be at least 1")
        ln, pos = self._common()
        if k > nonempty or not ln[k - 1]:
            return b"", 0
        s = self._text[int(pos[k - 1]):int(pos[k - 1]) + int(ln[k - 1])]
        res = self.query_batch([s])
        return s, self.interval_document_frequency(int(res["start"][0]), int(res["end"][0]))

    # -- repeats --------------------------------------------------------------------------------
    def repeat_lens(self, scope="any", with_source=False):
        """rep[p] (indexed by text position doc_starts[i] + offset) = the longest common prefix of the truncated suffix
        at p with any other one (scope "any"), any at an earlier position ("earlier") or any of ANOTHER document
        ("other_doc").  with_source: -> (rep, src), src[p] = a position attaining rep[p], 0xFFFFFFFF where rep[p] == 0."""
        return _repeat_lens(self._eng, self._table, self._lcp, self._da, scope, with_source)

    def repeated_spans(self, min_len, scope="any"):
        """[(document, begin_offset, end_offset)] in ascending order: the maximal runs of bytes inside a repeat of at
        least min_len bytes; no run spans two documents."""
        b, e = _repeat_spans(self._eng, self.repeat_lens(scope), min_len, self._starts)
        d = np.searchsorted(self._starts, b, side="right").astype(np.int64) - 1
        s = self._starts[d].astype(np.int64) if b.size else np.zeros(0, dtype=np.int64)
        return list(zip(d.tolist(), (b.astype(np.int64) - s).tolist(), (e.astype(np.int64) - s).tolist()))

    # -- matching statistics of a second text ---------------------------------------------------
    def match_stats(self, query, max_len=None, with_source=False, with_intervals=False):
        """As SuffixTable.match_stats, against the collection: a match lies inside ONE document; src is a text position
        doc_starts[i] + offset, and table()[start:end] are GSA ranks."""
        return _match_stats(self._eng, self._eng.lib.sfx_gindex_match_stats, "sfx_gindex_match_stats", self._ensure_index,
                            self.len(), query, max_len, with_source, with_intervals)

    def shared_spans(self, query, min_len):
        """[(begin, end)] in query coordinates, ascending: the query bytes inside a stretch of at least min_len bytes
        that occurs within one document."""
        return _shared_spans(self._eng, self.match_stats, query, min_len)

    def mems(self, query, min_len, unique=False, max_pairs=1 << 30):
        """As SuffixTable.mems, against the collection: a match lies inside ONE document and ends at its ends; tpos is
        a text position doc_starts[doc] + offset, and the result also has the arrays doc and offset.  unique: the
        bytes occur once among all documents."""
        qpos, tpos, ln, pairs = _mems(self._eng, self._eng.lib.sfx_gindex_mems, "sfx_gindex_mems", self._ensure_index, self.len(),
                                      query, min_len, unique, max_pairs)
        # the document of a match: the last one that starts at or before tpos and is not empty (a match has bytes)
        d = np.searchsorted(self._starts, tpos.astype(np.uint64), side="right").astype(np.int64) - 1
        off = (tpos.astype(np.int64) - self._starts[d].astype(np.int64)).astype(np.uint32) if tpos.size else tpos.copy()
        return Mems(qpos, tpos, ln, pairs, doc=d.astype(np.uint32), offset=off)

    # -- k-mismatch pattern search ------------------------------------------------------------------
    def approx_positions_batch(self, queries, mismatches, max_candidates=1 << 30, sort=False):
        """As SuffixTable.approx_positions_batch, against the collection: a window lies inside ONE document; tpos is a
        text position doc_starts[doc] + offset."""
        return _approx_positions(self._eng, self._eng.lib.sfx_gindex_hamming, "sfx_gindex_hamming", self._ensure_index, self.len(),
                                 queries, mismatches, max_candidates, sort)

    def approx_positions(self, query, mismatches):
        """(positions, mismatches): text positions ascending and the differing bytes of each window."""
        _, tpos, mism = self.approx_positions_batch([query], mismatches, sort=True)
        return tpos, mism

    # -- k-error pattern search ---------------------------------------------------------------------
    def edit_positions_batch(self, queries, errors, max_candidates=1 << 30, max_hits=1 << 22):
        """As SuffixTable.edit_positions_batch, against the collection: an occurrence lies inside ONE document; tbegin and
        tend are text positions doc_starts[doc] + offset.  -> (first, tbegin, tend, dist, doc)."""
        first, tbegin, tend, dist = _edit_positions(self._eng, self._eng.lib.sfx_gindex_edit, "sfx_gindex_edit", self._ensure_index,
                                                    self.len(), queries, errors, max_candidates, max_hits)
        # the document of an occurrence: the last one that starts before tend (an occurrence has text bytes: tend > tbegin)
        d = np.searchsorted(self._starts, tend.astype(np.uint64), side="left").astype(np.int64) - 1
        return first, tbegin, tend, dist, d.astype(np.uint32)

    def edit_positions(self, pattern, k):
        """[(doc, begin, end, dist)] of `pattern` within k edits, begin and end as offsets in the document, ascending by
        document and end."""
        _, tbegin, tend, dist, doc = self.edit_positions_batch([pattern], k)
        base = self._starts[doc].astype(np.int64) if doc.size else np.zeros(0, dtype=np.int64)
        return list(zip(doc.tolist(), (tbegin - base).tolist(), (tend - base).tolist(), dist.tolist()))

    # -- longest common extensions ----------------------------------------------------------------
    def _lce_index(self):
        return self._lce.get(self._table, self._lcp, self._starts)

    def lce_batch(self, a, b, mismatches=0):
        """len (uint32) for pairs of TEXT positions (doc_starts[doc] + offset): how far the two truncated suffixes agree
        with at most `mismatches` differing bytes; no extension passes the end of either position's document.  A
        position equal to len() gives 0, one above 0xFFFFFFFF."""
        return self._lce.lce(self._lce_index, a, b, mismatches)

    def lce(self, a, b, mismatches=0):
        """As lce_batch for one pair of (document, offset) positions inside their documents."""
        pos = []
        for d, o in (a, b):
            d, o = int(d), int(o)
            if not 0 <= d < len(self._docs) or not 0 <= o < len(self._docs[d]):
                raise IndexError(f"({d}, {o}) is no position of the collection")
            pos.append(int(self._starts[d]) + o)
        return int(self.lce_batch([pos[0]], [pos[1]], mismatches)[0])

    # -- suffix-tree navigation --------------------------------------------------------------------
    def _text_pos(self, p):
        d, o = int(p[0]), int(p[1])
        if not 0 <= d < len(self._docs) or not 0 <= o < len(self._docs[d]):
            raise IndexError(f"({d}, {o}) is no position of the collection")
        return int(self._starts[d]) + o

    def substring_intervals_batch(self, pos, length):
        """(lo, hi, depth), uint32 each, for TEXT positions (doc_starts[doc] + offset): table()[lo[q]:hi[q]] are the
        occurrences of the length[q] bytes at pos[q] in all documents; a substring that leaves its document gives
        0xFFFFFFFF three times (sfx_lce_substr)."""
        return self._lce.substr(self._lce_index, pos, length)

    def substring_interval(self, pos, length):
        """(lo, hi) for the `length` bytes at the (document, offset) position `pos`."""
        lo, hi, _ = self.substring_intervals_batch([self._text_pos(pos)], [int(length)])
        if int(lo[0]) == 0xFFFFFFFF:
            raise IndexError(f"{int(length)} bytes from {tuple(pos)} leave the document")
        return int(lo[0]), int(hi[0])

    def substring_count(self, pos, length):
        lo, hi = self.substring_interval(pos, length)
        return hi - lo

    def lca_batch(self, a, b):
        """(lo, hi, depth), uint32 each, for pairs of TEXT positions: the lowest common ancestor of the two truncated
        suffixes as a rank interval of the generalized table, with its string depth (sfx_lce_lca)."""
        return self._lce.lca(self._lce_index, a, b)

    def lca(self, a, b):
        """(lo, hi, depth) for one pair of (document, offset) positions."""
        lo, hi, d = self.lca_batch([self._text_pos(a)], [self._text_pos(b)])
        return int(lo[0]), int(hi[0]), int(d[0])

    def lcp_range_argmin_batch(self, lo, hi):
        """The smallest index that attains min lcp_lens()[lo[q]:hi[q]] (uint32); 0xFFFFFFFF for an empty range or
        hi > len()."""
        return self._lce.range_argmin(self._lce_index, lo, hi)

    def lcp_range_argmin(self, lo, hi):
        return int(self.lcp_range_argmin_batch([int(lo)], [int(hi)])[0])
