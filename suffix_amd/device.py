"""Device-resident entry points: torch tensors are used only as HBM buffers and
for the current HIP stream; all compute is the C ABI's `*_dev` functions.

Inputs stay in HBM, outputs are left in HBM, scratch comes from a caller-owned
(or freshly allocated) workspace tensor -- the engine itself never allocates
device memory on this path, so a build is a pure kernel sequence on the
caller's stream.
"""
import contextlib
import ctypes

import torch

from ._lib import REP_SCOPES, FmInfo, RunsFilter, SuffixHipError, default_engine


def _on(t):
    """Make the tensor's device the current one for the duration of an engine call: the C side launches
    on, allocates pinned staging for and pools scratch by the CURRENT device, and the stream handed over
    belongs to the tensor's device."""
    if t is not None and t.is_cuda:
        return torch.cuda.device(t.device)
    return contextlib.nullcontext()


def _stream_ptr(t):
    if t.is_cuda:
        return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    return ctypes.c_void_p(0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def _check_u8(text):
    if text.dtype != torch.uint8 or text.dim() != 1 or not text.is_contiguous():
        raise TypeError("text must be a contiguous 1-D uint8 tensor")


def sa_workspace(n, device, engine=None):
    eng = engine or default_engine()
    return torch.empty(int(eng.lib.sfx_sa_workspace_bytes(int(n))), dtype=torch.uint8, device=device)


def build_sa(text, out=None, workspace=None, engine=None):
    """Suffix array (uint32, viewed through torch.int32 storage) of a uint8 tensor."""
    eng = engine or default_engine()
    _check_u8(text)
    n = text.numel()
    if text.is_cuda:
        eng.require_device()
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=text.device)
    if workspace is None:
        workspace = sa_workspace(n, text.device, eng)
    with _on(text):
        eng.check(eng.lib.sfx_build_sa_u32_dev(_p(text), n, _p(out), _p(workspace), workspace.numel(),
                                               _stream_ptr(text)), "sfx_build_sa_u32_dev")
    return out


def sa_lcp_workspace(n, device, engine=None):
    eng = engine or default_engine()
    return torch.empty(int(eng.lib.sfx_sa_lcp_workspace_bytes(int(n))), dtype=torch.uint8, device=device)


def build_sa_lcp(text, out_sa=None, out_lcp=None, workspace=None, engine=None):
    """SuffixTable::new + lcp_lens in one call: -> (sa, lcp), both uint32 in int32 storage."""
    eng = engine or default_engine()
    _check_u8(text)
    n = text.numel()
    if text.is_cuda:
        eng.require_device()
    if out_sa is None:
        out_sa = torch.empty(n, dtype=torch.int32, device=text.device)
    if out_lcp is None:
        out_lcp = torch.empty(n, dtype=torch.int32, device=text.device)
    if workspace is None:
        workspace = sa_lcp_workspace(n, text.device, eng)
    with _on(text):
        eng.check(eng.lib.sfx_build_sa_lcp_u32_dev(_p(text), n, _p(out_sa), _p(out_lcp), _p(workspace), workspace.numel(),
                                                   _stream_ptr(text)), "sfx_build_sa_lcp_u32_dev")
    return out_sa, out_lcp


def lcp_workspace(n, device, engine=None):
    eng = engine or default_engine()
    return torch.empty(int(eng.lib.sfx_lcp_workspace_bytes(int(n))), dtype=torch.uint8, device=device)


def build_lcp(text, sa, out=None, workspace=None, engine=None):
    eng = engine or default_engine()
    _check_u8(text)
    n = text.numel()
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=text.device)
    if workspace is None:
        workspace = lcp_workspace(n, text.device, eng)
    with _on(text):
        eng.check(eng.lib.sfx_build_lcp_u32_dev(_p(text), n, _p(sa), _p(out), _p(workspace),
                                                workspace.numel(), _stream_ptr(text)),
                  "sfx_build_lcp_u32_dev")
    return out


def query_batch(text, sa, qbytes, qoff, engine=None):
    """qbytes: uint8 tensor, qoff: int64 tensor of nq+1 offsets (same device as text).
    -> (start, end, found, any) tensors; positions(q_k) = sa[start[k]:end[k]]."""
    eng = engine or default_engine()
    nq = qoff.numel() - 1
    dev = text.device
    start = torch.empty(nq, dtype=torch.int32, device=dev)
    end = torch.empty(nq, dtype=torch.int32, device=dev)
    found = torch.empty(nq, dtype=torch.uint8, device=dev)
    anyp = torch.empty(nq, dtype=torch.int32, device=dev)
    with _on(text):
        eng.check(eng.lib.sfx_query_batch_dev(_p(text), text.numel(), _p(sa), _p(qbytes), _p(qoff), nq,
                                              _p(start), _p(end), _p(found), _p(anyp), _stream_ptr(text)),
                  "sfx_query_batch_dev")
    return start, end, found, anyp


def _ms_outputs(query, dev, max_len, want_src, want_interval):
    """Checks of a matching-statistics call and its freshly allocated outputs: (m, max_len, len, src, start, end)."""
    if query.dtype != torch.uint8 or query.dim() != 1 or not query.is_contiguous():
        raise TypeError("query must be a contiguous 1-D uint8 tensor")
    if query.device != dev:
        raise ValueError(f"query must be on the text's device ({dev})")
    max_len = int(max_len or 0)
    if max_len < 0 or max_len > 0xFFFFFFFF:
        raise ValueError("max_len must be in 0 .. 2^32 - 1 (0 = no cap)")
    m = query.numel()
    ln = torch.empty(m, dtype=torch.int32, device=dev)
    src = torch.empty(m, dtype=torch.int32, device=dev) if want_src else None
    start = torch.empty(m, dtype=torch.int32, device=dev) if want_interval else None
    end = torch.empty(m, dtype=torch.int32, device=dev) if want_interval else None
    return m, max_len, ln, src, start, end


def _ms_result(ln, src, start, end, want_src, want_interval):
    if not want_src and not want_interval:
        return ln
    return (ln,) + ((src,) if want_src else ()) + ((start, end) if want_interval else ())


def match_stats(text, sa, query, max_len=0, want_src=False, want_interval=False, engine=None):
    """Matching statistics of the uint8 tensor `query` against (text, sa) on the same device: len[i] = the longest
    prefix of query[i:] (at most max_len bytes; 0 = no cap) that occurs in text -- uint32 in int32 storage.
    -> len, or the tuple (len[, src][, start, end]): src[i] = a text position of that match (0xFFFFFFFF where len is
    0), [start[i], end[i]) = the ranks of the suffixes that begin with it.  Runs on the current stream without a
    synchronisation (sfx_match_stats_dev); the table is not checked."""
    eng = engine or default_engine()
    _check_u8(text)
    _check_u32(sa, "sa", text.numel())
    if sa.device != text.device:
        raise ValueError(f"sa must be on the text's device ({text.device})")
    m, max_len, ln, src, start, end = _ms_outputs(query, text.device, max_len, want_src, want_interval)
    if text.is_cuda:
        eng.require_device()
    with _on(text):
        eng.check(eng.lib.sfx_match_stats_dev(_p(text), text.numel(), _p(sa), _p(query), m, max_len, _p(ln), _p(src), _p(start),
                                              _p(end), _stream_ptr(text)), "sfx_match_stats_dev")
    return _ms_result(ln, src, start, end, want_src, want_interval)


def _bwt_step(sample_step):
    step = int(sample_step or 0)
    if step < 0 or step > 0x80000000 or step & (step - 1):
        raise ValueError("sample_step must be 0 or a power of two of at most 2^31")
    return step


def bwt(text, sa, sample_step=256, out_bwt=None, out_samples=None, engine=None):
    """Burrows-Wheeler transform of the uint8 tensor `text` with its suffix array `sa` (same device) -> (bwt, samples):
    bwt = the last column of the sorted rotations of text$ without its $ entry (uint8, n bytes); samples[k] = the row
    of the suffix that starts at k * sample_step (uint32 in int32 storage; samples[0] = the primary row; sample_step 0:
    the primary only).  Runs on the current stream without a synchronisation (sfx_bwt_dev); the table is not checked."""
    eng = engine or default_engine()
    _check_u8(text)
    n = text.numel()
    _check_u32(sa, "sa", n)
    if sa.device != text.device:
        raise ValueError(f"sa must be on the text's device ({text.device})")
    step = _bwt_step(sample_step)
    cnt = int(eng.lib.sfx_bwt_sample_count(n, step))
    if out_bwt is None:
        out_bwt = torch.empty(n, dtype=torch.uint8, device=text.device)
    if out_samples is None:
        out_samples = torch.empty(cnt, dtype=torch.int32, device=text.device)
    _check_u8(out_bwt)
    _check_u32(out_samples, "out_samples", cnt)
    if out_bwt.numel() != n:
        raise ValueError(f"out_bwt must hold {n} bytes")
    if text.is_cuda:
        eng.require_device()
    with _on(text):
        eng.check(eng.lib.sfx_bwt_dev(_p(text), n, _p(sa), step, _p(out_bwt), _p(out_samples), _stream_ptr(text)), "sfx_bwt_dev")
    return out_bwt, out_samples


def unbwt_workspace(n, device, engine=None):
    eng = engine or default_engine()
    return torch.empty(int(eng.lib.sfx_unbwt_workspace_bytes(int(n))), dtype=torch.uint8, device=device)


def unbwt(bwt, samples, sample_step, out=None, workspace=None, engine=None):
    """The text whose transform (bwt, samples) is, as `bwt()` returns it, with the same sample_step.  One lane walks one
    segment of sample_step bytes (at most 2^20; sample_step 0: the whole text as one chain).  Synchronises the current
    stream once; a pair that is no transform of any text raises SuffixHipError (sfx_unbwt_dev)."""
    eng = engine or default_engine()
    _check_u8(bwt)
    n = bwt.numel()
    _check_u32(samples, "samples")
    if samples.device != bwt.device:
        raise ValueError(f"samples must be on the transform's device ({bwt.device})")
    step = _bwt_step(sample_step)
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=bwt.device)
    _check_u8(out)
    if out.numel() != n:
        raise ValueError(f"out must hold {n} bytes")
    if workspace is None:
        workspace = unbwt_workspace(n, bwt.device, eng)
    if bwt.is_cuda:
        eng.require_device()
    with _on(bwt):
        eng.check(eng.lib.sfx_unbwt_dev(_p(bwt), n, _p(samples), samples.numel(), step, _p(out), _p(workspace), workspace.numel(),
                                        _stream_ptr(bwt)), "sfx_unbwt_dev")
    return out


class FmDeviceIndex:
    """FM-index over the device tensors (bwt, samples) of `bwt()`: backward-search count and locate from the pair alone
    (sfx_fm_create_dev).  The handle owns its HBM and the binding keeps no reference to the pair -- it may be freed afterwards.  Creation synchronises the current
    stream; `count`, `lookup` and `sa_range` queue on it without a synchronisation."""

    def __init__(self, bwt, samples, sample_step, occ_step=0, engine=None):
        self._eng = engine or default_engine()
        _check_u8(bwt)
        _check_u32(samples, "samples")
        if samples.device != bwt.device:
            raise ValueError(f"samples must be on the transform's device ({bwt.device})")
        step = _bwt_step(sample_step)
        if bwt.is_cuda:
            self._eng.require_device()
        self._dev = bwt.device
        # (a tensor of the device, for _on / _stream_ptr; its own storage: a slice of bwt would keep the transform in HBM)
        self._on = torch.empty(0, dtype=torch.uint8, device=bwt.device)
        h = ctypes.c_void_p()
        with _on(bwt):
            self._eng.check(self._eng.lib.sfx_fm_create_dev(_p(bwt), bwt.numel(), _p(samples), samples.numel(), step, int(occ_step),
                                                            _stream_ptr(bwt), ctypes.byref(h)), "sfx_fm_create_dev")
        self._h = h
        info = FmInfo()
        self._eng.check(self._eng.lib.sfx_fm_info(h, ctypes.byref(info)), "sfx_fm_info")
        self.info = info.as_dict()

    def _check_queries(self, qbytes, qoff):
        if qbytes.dtype != torch.uint8 or qbytes.dim() != 1 or not qbytes.is_contiguous():
            raise TypeError("qbytes must be a contiguous 1-D uint8 tensor")
        if qoff.dtype != torch.int64 or qoff.dim() != 1 or not qoff.is_contiguous() or qoff.numel() < 1:
            raise TypeError("qoff must be a contiguous 1-D int64 tensor of nq + 1 offsets")
        if qbytes.device != self._dev or qoff.device != self._dev:
            raise ValueError(f"qbytes and qoff must be on the index's device ({self._dev})")

    def count(self, qbytes, qoff):
        """-> (start, end): the table ranks of the suffixes that begin with pattern k = qbytes[qoff[k]:qoff[k + 1]],
        (0, 0) where there is none -- the interval DeviceIndex.query reports."""
        self._check_queries(qbytes, qoff)
        nq = qoff.numel() - 1
        start = torch.empty(nq, dtype=torch.int32, device=self._dev)
        end = torch.empty(nq, dtype=torch.int32, device=self._dev)
        with _on(self._on):
            self._eng.check(self._eng.lib.sfx_fm_count_dev(self._h, _p(qbytes), _p(qoff), nq, _p(start), _p(end), _stream_ptr(self._on)),
                            "sfx_fm_count_dev")
        return start, end

    def lookup(self, ranks):
        """The table entries of `ranks` (uint32 in int32 storage); 0xFFFFFFFF for a rank >= n."""
        _check_u32(ranks, "ranks")
        if ranks.device != self._dev:
            raise ValueError(f"ranks must be on the index's device ({self._dev})")
        pos = torch.empty(ranks.numel(), dtype=torch.int32, device=self._dev)
        with _on(self._on):
            self._eng.check(self._eng.lib.sfx_fm_lookup_dev(self._h, _p(ranks), 0, ranks.numel(), _p(pos), _stream_ptr(self._on)),
                            "sfx_fm_lookup_dev")
        return pos

    def sa_range(self, first, count):
        """table[first : first + count] regenerated from the index (sa_range(0, n): the whole suffix array)."""
        pos = torch.empty(int(count), dtype=torch.int32, device=self._dev)
        with _on(self._on):
            self._eng.check(self._eng.lib.sfx_fm_lookup_dev(self._h, None, int(first), int(count), _p(pos), _stream_ptr(self._on)),
                            "sfx_fm_lookup_dev")
        return pos

    def locate(self, qbytes, qoff):
        """-> (offsets int64[nq + 1], positions): positions[offsets[k]:offsets[k + 1]] = the occurrences of pattern k in
        table order.  The rank list between count and lookup is torch plumbing; reading its total synchronises."""
        start, end = self.count(qbytes, qoff)
        s = start.to(torch.int64) & 0xFFFFFFFF
        cnt = (end.to(torch.int64) & 0xFFFFFFFF) - s
        offsets = torch.zeros(cnt.numel() + 1, dtype=torch.int64, device=self._dev)
        offsets[1:] = torch.cumsum(cnt, 0)
        total = int(offsets[-1])
        which = torch.repeat_interleave(torch.arange(cnt.numel(), device=self._dev), cnt)
        ranks = s[which] + (torch.arange(total, device=self._dev) - offsets[:-1][which])
        return offsets, self.lookup(ranks.to(torch.int32))

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._eng.lib.sfx_fm_destroy(h)

    __del__ = close


class DeviceIndex:
    """Resident index over device tensors (text, suffix array): the engine adds its bucket directory
    (sfx_index_create_dev); `query` = batched positions() / contains() / any_position(); `match_stats` = the
    matching statistics of a query text."""

    def __init__(self, text, sa, engine=None):
        self._eng = engine or default_engine()
        _check_u8(text)
        self._text, self._sa = text, sa                     # (borrowed by the index: keep them alive)
        h = ctypes.c_void_p()
        with _on(text):
            self._eng.check(self._eng.lib.sfx_index_create_dev(_p(text), text.numel(), _p(sa), _stream_ptr(text),
                                                               ctypes.byref(h)), "sfx_index_create_dev")
        self._h = h

    def query(self, qbytes, qoff):
        nq = qoff.numel() - 1
        dev = self._text.device
        start = torch.empty(nq, dtype=torch.int32, device=dev)
        end = torch.empty(nq, dtype=torch.int32, device=dev)
        found = torch.empty(nq, dtype=torch.uint8, device=dev)
        anyp = torch.empty(nq, dtype=torch.int32, device=dev)
        with _on(self._text):
            self._eng.check(self._eng.lib.sfx_index_query_dev(self._h, _p(qbytes), _p(qoff), nq, _p(start), _p(end),
                                                              _p(found), _p(anyp), _stream_ptr(self._text)),
                            "sfx_index_query_dev")
        return start, end, found, anyp

    def match_stats(self, query, max_len=0, want_src=False, want_interval=False):
        """As the module's match_stats, against the index's text and (checked) table: sfx_index_match_stats_dev."""
        m, max_len, ln, src, start, end = _ms_outputs(query, self._text.device, max_len, want_src, want_interval)
        with _on(self._text):
            self._eng.check(self._eng.lib.sfx_index_match_stats_dev(self._h, _p(query), m, max_len, _p(ln), _p(src), _p(start),
                                                                    _p(end), _stream_ptr(self._text)), "sfx_index_match_stats_dev")
        return _ms_result(ln, src, start, end, want_src, want_interval)

    def mems(self, query, min_len, unique=False, max_pairs=1 << 30, capacity=None, workspace=None):
        """As the module's mems, against the index's text and (checked) table, searching through its directory
        (sfx_index_mems_dev).  Keeps no state in the index: threads may call at once."""
        call = lambda *tail: self._eng.lib.sfx_index_mems_dev(self._h, *tail)
        return _mems(self._eng, call, "sfx_index_mems_dev", self._text.numel(), query, self._text, min_len, unique, max_pairs,
                     capacity, workspace)

    def hamming(self, qbytes, qoff, mismatches, max_candidates=1 << 30, capacity=None, workspace=None):
        """As the module's hamming, against the index's text and (checked) table; the pieces are searched through the
        directory and the key tree (sfx_index_hamming_dev).  Keeps no state in the index: threads may call at once."""
        call = lambda *tail: self._eng.lib.sfx_index_hamming_dev(self._h, *tail)
        return _hamming(self._eng, call, "sfx_index_hamming_dev", self._text.numel(), qbytes, qoff, self._text, mismatches,
                        max_candidates, capacity, workspace)

    def edit_search(self, qbytes, qoff, errors, max_candidates=1 << 30, max_hits=1 << 22, capacity=None, workspace=None):
        """As the module's edit_search, against the index's text and (checked) table; the pieces are searched through the
        directory and the key tree (sfx_index_edit_dev).  Keeps no state in the index: threads may call at once."""
        call = lambda *tail: self._eng.lib.sfx_index_edit_dev(self._h, *tail)
        return _edit_search(self._eng, call, "sfx_index_edit_dev", self._text.numel(), qbytes, qoff, self._text, errors, max_candidates,
                            max_hits, capacity, workspace)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._eng.lib.sfx_index_destroy(h)

    __del__ = close


def lcp_intervals(lcp, engine=None):
    """Suffix-tree topology as flat arrays from the LCP array (uint32 in int32 storage, on any device the
    engine runs on): -> dict(lb, rb, node, parent, leaf_parent), see include/suffix_hip.h."""
    eng = engine or default_engine()
    n = lcp.numel()
    dev = lcp.device
    out = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in ("lb", "rb", "node", "parent", "leaf_parent")}
    ws = torch.empty(int(eng.lib.sfx_lcp_intervals_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    with _on(lcp):
        eng.check(eng.lib.sfx_lcp_intervals_dev(_p(lcp), n, _p(out["lb"]), _p(out["rb"]), _p(out["node"]), _p(out["parent"]),
                                                _p(out["leaf_parent"]), _p(ws), ws.numel(), _stream_ptr(lcp)),
                  "sfx_lcp_intervals_dev")
    return out


def suffix_tree_workspace(n, device, engine=None):
    eng = engine or default_engine()
    return torch.empty(int(eng.lib.sfx_suffix_tree_workspace_bytes(int(n))), dtype=torch.uint8, device=device)


def suffix_tree(sa, lcp, text=None, want_leaf_parent=True, workspace=None, engine=None):
    """Suffix-tree node table with ordered children from a suffix array and its LCP array (uint32 in int32 storage, on one
    device): -> dict(node_lb, node_rb, node_depth, node_parent, node_terminal, child_off (int64, m + 1), child_lb,
    child_node, child_byte (uint8; only with text), leaf_parent (only if wanted)), cut to the m nodes and C children of
    the tree.  One sizing call, then one filling call; each synchronises the stream once.  See include/suffix_hip.h."""
    eng = engine or default_engine()
    n = sa.numel()
    _check_u32(sa, "sa")
    _check_u32(lcp, "lcp", n)
    if text is not None:
        _check_u8(text)
        if text.numel() != n:
            raise ValueError(f"text must hold {n} bytes")
    for t in (lcp, text):
        if t is not None and t.device != sa.device:
            raise ValueError(f"all arrays must be on one device ({sa.device})")
    if sa.is_cuda:
        eng.require_device()
    dev = sa.device
    if workspace is None:
        workspace = suffix_tree_workspace(n, dev, eng)
    m, c = ctypes.c_uint64(0), ctypes.c_uint64(0)
    with _on(sa):
        eng.check(eng.lib.sfx_suffix_tree_dev(None, _p(sa), _p(lcp), n, 0, 0, None, None, None, None, None, None, None, None, None,
                                              None, ctypes.byref(m), ctypes.byref(c), _p(workspace), workspace.numel(),
                                              _stream_ptr(sa)), "sfx_suffix_tree_dev")
    nm, nc = int(m.value), int(c.value)
    out = {k: torch.empty(nm, dtype=torch.int32, device=dev) for k in ("node_lb", "node_rb", "node_depth", "node_parent", "node_terminal")}
    out["child_off"] = torch.zeros(nm + 1, dtype=torch.int64, device=dev)
    out["child_lb"] = torch.empty(nc, dtype=torch.int32, device=dev)
    out["child_node"] = torch.empty(nc, dtype=torch.int32, device=dev)
    # (a byte array of no entries still has to be a pointer when there is a text: both or neither)
    cbyte = torch.empty(max(nc, 1), dtype=torch.uint8, device=dev) if text is not None else None
    leaf = torch.empty(n, dtype=torch.int32, device=dev) if want_leaf_parent else None
    if n:
        with _on(sa):
            eng.check(eng.lib.sfx_suffix_tree_dev(_p(text), _p(sa), _p(lcp), n, nm, nc, _p(out["node_lb"]), _p(out["node_rb"]),
                                                  _p(out["node_depth"]), _p(out["node_parent"]), _p(out["node_terminal"]),
                                                  _p(out["child_off"]), _p(out["child_lb"]), _p(out["child_node"]), _p(cbyte),
                                                  _p(leaf), ctypes.byref(m), ctypes.byref(c), _p(workspace), workspace.numel(),
                                                  _stream_ptr(sa)), "sfx_suffix_tree_dev")
    if cbyte is not None:
        out["child_byte"] = cbyte[:nc]
    if leaf is not None:
        out["leaf_parent"] = leaf
    return out


def doc_lookup(positions, doc_starts, engine=None):
    """Generalized suffix array: text positions (uint32 in int32 storage) -> (document index, offset inside it);
    doc_starts = sorted int64 start offsets of the documents inside the concatenated text."""
    eng = engine or default_engine()
    cnt = positions.numel()
    doc = torch.empty(cnt, dtype=torch.int32, device=positions.device)
    off = torch.empty(cnt, dtype=torch.int32, device=positions.device)
    with _on(positions):
        eng.check(eng.lib.sfx_doc_lookup_dev(_p(positions), cnt, _p(doc_starts), doc_starts.numel(), _p(doc), _p(off),
                                             _stream_ptr(positions)), "sfx_doc_lookup_dev")
    return doc, off


def gsa_workspace(n, ndocs, device, engine=None):
    eng = engine or default_engine()
    return torch.empty(int(eng.lib.sfx_gsa_workspace_bytes(int(n), int(ndocs))), dtype=torch.uint8, device=device)


def build_gsa(text, doc_starts, out_sa=None, out_da=None, out_lcp=None, workspace=None, want_da=True, want_lcp=True,
              engine=None):
    """Generalized suffix array of the documents text[doc_starts[i]:doc_starts[i + 1]] (no separators; doc_starts an
    int64 tensor on the text's device, doc_starts[0] == 0): -> (sa, da, lcp), uint32 in int32 storage; da / lcp are
    None unless wanted.  See include/suffix_hip.h for the order and the LCP."""
    eng = engine or default_engine()
    _check_u8(text)
    if doc_starts.dtype != torch.int64 or doc_starts.dim() != 1 or not doc_starts.is_contiguous():
        raise TypeError("doc_starts must be a contiguous 1-D int64 tensor")
    n, nd = text.numel(), doc_starts.numel()
    if text.is_cuda:
        eng.require_device()
    if out_sa is None:
        out_sa = torch.empty(n, dtype=torch.int32, device=text.device)
    if want_da and out_da is None:
        out_da = torch.empty(n, dtype=torch.int32, device=text.device)
    if want_lcp and out_lcp is None:
        out_lcp = torch.empty(n, dtype=torch.int32, device=text.device)
    if workspace is None:
        workspace = gsa_workspace(n, nd, text.device, eng)
    with _on(text):
        eng.check(eng.lib.sfx_build_gsa_u32_dev(_p(text), n, _p(doc_starts), nd, _p(out_sa), _p(out_da), _p(out_lcp),
                                                _p(workspace), workspace.numel(), _stream_ptr(text)), "sfx_build_gsa_u32_dev")
    return out_sa, out_da, out_lcp


def _check_u32(t, name, n=None):
    if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
        raise TypeError(f"{name} must be a contiguous 1-D int32 tensor (uint32 values in int32 storage)")
    if n is not None and t.numel() != n:
        raise ValueError(f"{name} must hold {n} entries")


def gsa_merge_workspace(n_a, n_b, device, engine=None):
    eng = engine or default_engine()
    return torch.empty(int(eng.lib.sfx_gsa_merge_workspace_bytes(int(n_a), int(n_b))), dtype=torch.uint8, device=device)


def gsa_merge(text, doc_starts, ndocs_a, sa_a, lcp_a, sa_b, lcp_b, da_a=None, da_b=None, match_limit=0, out_sa=None, out_da=None,
              out_lcp=None, want_da=True, want_lcp=True, workspace=None, engine=None):
    """The arrays of a whole collection from those of its first ndocs_a documents (sa_a, lcp_a[, da_a]) and of the documents
    behind them (sa_b, lcp_b[, da_b], as build_gsa returns them for those documents alone): a stable merge, no sort.  text
    and doc_starts describe the whole collection.  -> (sa, da, lcp, longest); da / lcp are None unless wanted.  longest =
    the longest common prefix of a new suffix with an old one; with match_limit > 0 a longer one refuses the merge --
    (None, None, None, longest) with longest == match_limit + 1 and the outputs untouched -- because its cost grows with
    the square of such a match; build_gsa of the whole collection is the answer then.  Synchronises the current stream
    twice.  See include/suffix_hip.h."""
    eng = engine or default_engine()
    _check_u8(text)
    if doc_starts.dtype != torch.int64 or doc_starts.dim() != 1 or not doc_starts.is_contiguous():
        raise TypeError("doc_starts must be a contiguous 1-D int64 tensor")
    dev = text.device
    _check_u32(sa_a, "sa_a")
    _check_u32(sa_b, "sa_b")
    n_a, n_b = sa_a.numel(), sa_b.numel()
    n = text.numel()
    if n_a + n_b != n:
        raise ValueError(f"sa_a and sa_b hold {n_a} + {n_b} entries, the text {n} bytes")
    for t, name, cnt in ((lcp_a, "lcp_a", n_a), (lcp_b, "lcp_b", n_b), (da_a, "da_a", n_a), (da_b, "da_b", n_b),
                         (out_sa, "out_sa", n), (out_da, "out_da", n), (out_lcp, "out_lcp", n)):
        if t is not None:
            _check_u32(t, name, cnt)
    if any(t is not None and t.device != dev for t in (doc_starts, sa_a, lcp_a, sa_b, lcp_b, da_a, da_b, out_sa, out_da, out_lcp)):
        raise ValueError(f"all arrays must be on the text's device ({dev})")
    match_limit = int(match_limit)
    if not 0 <= match_limit <= 0xFFFFFFFF:
        raise ValueError("match_limit must be in 0 .. 2^32 - 1")
    if text.is_cuda:
        eng.require_device()
    if out_sa is None:
        out_sa = torch.empty(n, dtype=torch.int32, device=dev)
    if want_da and out_da is None:
        out_da = torch.empty(n, dtype=torch.int32, device=dev)
    if want_lcp and out_lcp is None:
        out_lcp = torch.empty(n, dtype=torch.int32, device=dev)
    if workspace is None:
        workspace = gsa_merge_workspace(n_a, n_b, dev, eng)
    longest = ctypes.c_uint64(0)
    with _on(text):
        eng.check(eng.lib.sfx_gsa_merge_dev(_p(text), _p(doc_starts), doc_starts.numel(), int(ndocs_a), _p(sa_a), _p(da_a), _p(lcp_a), n_a,
                                            _p(sa_b), _p(da_b), _p(lcp_b), n_b, match_limit, _p(out_sa), _p(out_da), _p(out_lcp),
                                            ctypes.byref(longest), _p(workspace), workspace.numel(), _stream_ptr(text)), "sfx_gsa_merge_dev")
    if match_limit and longest.value > match_limit:
        return None, None, None, int(longest.value)
    return out_sa, out_da, out_lcp, int(longest.value)


def repeat_lens_workspace(n, scope, device, engine=None):
    eng = engine or default_engine()
    return torch.empty(int(eng.lib.sfx_repeat_lens_workspace_bytes(int(n), REP_SCOPES[scope])), dtype=torch.uint8, device=device)


def repeat_lens(sa, lcp, scope="any", da=None, want_src=False, workspace=None, engine=None):
    """Repeat lengths from a suffix array and its LCP array (uint32 in int32 storage, on one device): rep[p] = the
    longest common prefix of the suffix at text position p with any other suffix (scope "any"), any suffix at an
    earlier position ("earlier": the LPF array) or any suffix of another document ("other_doc": needs da, and the
    arrays of build_gsa).  -> rep, or (rep, src) with want_src: src[p] = a position attaining rep[p], 0xFFFFFFFF
    where rep[p] == 0.  See include/suffix_hip.h."""
    eng = engine or default_engine()
    if scope not in REP_SCOPES:
        raise ValueError(f"scope must be one of {sorted(REP_SCOPES)}")
    n = sa.numel()
    _check_u32(sa, "sa")
    _check_u32(lcp, "lcp", n)
    if scope == "other_doc":
        if da is None:
            raise ValueError('scope "other_doc" needs the document array da')
        _check_u32(da, "da", n)
    else:
        da = None
    for t in (lcp, da):
        if t is not None and t.device != sa.device:
            raise ValueError(f"all arrays must be on one device ({sa.device})")
    if sa.is_cuda:
        eng.require_device()
    rep = torch.empty(n, dtype=torch.int32, device=sa.device)
    src = torch.empty(n, dtype=torch.int32, device=sa.device) if want_src else None
    if workspace is None:
        workspace = repeat_lens_workspace(n, scope, sa.device, eng)
    with _on(sa):
        eng.check(eng.lib.sfx_repeat_lens_dev(_p(sa), _p(lcp), _p(da), n, REP_SCOPES[scope], _p(rep), _p(src), _p(workspace),
                                              workspace.numel(), _stream_ptr(sa)), "sfx_repeat_lens_dev")
    return (rep, src) if want_src else rep


def repeat_spans(rep, min_len, doc_starts=None, engine=None):
    """The maximal runs of bytes covered by a repeat of at least min_len bytes (rep from repeat_lens), split at every
    document start when doc_starts (int64, on rep's device) is given: -> an (k, 2) int32 tensor of [begin, end) rows in
    ascending order."""
    eng = engine or default_engine()
    _check_u32(rep, "rep")
    min_len = int(min_len)
    if min_len < 1 or min_len > 0xFFFFFFFF:
        raise ValueError("min_len must be in 1 .. 2^32 - 1")
    nd = 0
    if doc_starts is not None:
        if doc_starts.dtype != torch.int64 or doc_starts.dim() != 1 or not doc_starts.is_contiguous():
            raise TypeError("doc_starts must be a contiguous 1-D int64 tensor")
        if doc_starts.device != rep.device:
            raise ValueError(f"doc_starts must be on rep's device ({rep.device})")
        nd = doc_starts.numel()
    n = rep.numel()
    if rep.is_cuda:
        eng.require_device()
    cap = n // min_len + 1                                   # every run is at least min_len long
    begin = torch.empty(cap, dtype=torch.int32, device=rep.device)
    end = torch.empty(cap, dtype=torch.int32, device=rep.device)
    ws = torch.empty(int(eng.lib.sfx_repeat_spans_workspace_bytes(n)), dtype=torch.uint8, device=rep.device)
    count = ctypes.c_uint64(0)
    with _on(rep):
        eng.check(eng.lib.sfx_repeat_spans_dev(_p(rep), n, min_len, _p(doc_starts), nd, _p(begin), _p(end), cap, ctypes.byref(count),
                                               _p(ws), ws.numel(), _stream_ptr(rep)), "sfx_repeat_spans_dev")
    k = int(count.value)
    return torch.stack((begin[:k], end[:k]), dim=1)


def lz_parse_workspace(n, device, engine=None):
    eng = engine or default_engine()
    return torch.empty(int(eng.lib.sfx_lz_parse_workspace_bytes(int(n))), dtype=torch.uint8, device=device)


def lz_parse(rep, src, text=None, min_len=1, want_begin=True, workspace=None, engine=None):
    """The greedy LZ77 factorization from the longest-previous-factor array: rep, src = repeat_lens(sa, lcp, "earlier",
    want_src=True).  A phrase at position b copies rep[b] bytes from src[b] when rep[b] >= min_len and is the single
    byte text[b] otherwise.  -> (begin, len, src, lit) cut to the z phrases: begin is None without want_begin, a
    literal has src 0xFFFFFFFF (-1 in int32 storage), lit (uint8, None without text) is 0 for a copy.  Synchronises
    the current stream once; arrays that are no repeat lengths raise SuffixHipError (sfx_lz_parse_dev)."""
    eng = engine or default_engine()
    _check_u32(rep, "rep")
    n = rep.numel()
    _check_u32(src, "src", n)
    min_len = int(min_len)
    if min_len < 1 or min_len > 0xFFFFFFFF:
        raise ValueError("min_len must be in 1 .. 2^32 - 1")
    if text is not None:
        _check_u8(text)
        if text.numel() != n:
            raise ValueError(f"text must hold {n} bytes")
    for t in (src, text):
        if t is not None and t.device != rep.device:
            raise ValueError(f"all arrays must be on one device ({rep.device})")
    if rep.is_cuda:
        eng.require_device()
    dev = rep.device
    begin = torch.empty(n, dtype=torch.int32, device=dev) if want_begin else None
    ln = torch.empty(n, dtype=torch.int32, device=dev)
    psrc = torch.empty(n, dtype=torch.int32, device=dev)
    lit = torch.empty(n, dtype=torch.uint8, device=dev) if text is not None else None
    if workspace is None:
        workspace = lz_parse_workspace(n, dev, eng)
    count = ctypes.c_uint64(0)
    with _on(rep):
        eng.check(eng.lib.sfx_lz_parse_dev(_p(rep), _p(src), _p(text), n, min_len, _p(begin), _p(ln), _p(psrc), _p(lit), n,
                                           ctypes.byref(count), _p(workspace), workspace.numel(), _stream_ptr(rep)),
                  "sfx_lz_parse_dev")
    z = int(count.value)
    cut = lambda t: None if t is None else t[:z].clone()          # (the phrases, not n entries of storage behind them)
    return cut(begin), cut(ln), cut(psrc), cut(lit)


def lz_decode_workspace(n, z, device, engine=None):
    eng = engine or default_engine()
    return torch.empty(int(eng.lib.sfx_lz_decode_workspace_bytes(int(n), int(z))), dtype=torch.uint8, device=device)


def lz_decode(len, src, lit, n=None, out=None, workspace=None, engine=None):
    """The text of the phrases (len, src, lit) as lz_parse returns them; n = the sum of len when not given (one
    read-back).  A list that is no factorization -- a zero length, a literal of another length than 1, a copy that
    does not point backwards, a wrong sum -- raises SuffixHipError with `out` untouched (sfx_lz_decode_dev)."""
    eng = engine or default_engine()
    _check_u32(len, "len")
    z = len.numel()
    _check_u32(src, "src", z)
    _check_u8(lit)
    if lit.numel() != z:
        raise ValueError(f"lit must hold {z} bytes")
    for t in (src, lit):
        if t.device != len.device:
            raise ValueError(f"all arrays must be on one device ({len.device})")
    if n is None:
        n = int((len.to(torch.int64) & 0xFFFFFFFF).sum().item()) if z else 0
    n = int(n)
    if out is None:
        out = torch.empty(min(n, 0xFFFFFFFF), dtype=torch.uint8, device=len.device)
    _check_u8(out)
    if out.numel() != min(n, 0xFFFFFFFF) or out.device != len.device:
        raise ValueError(f"out must hold {n} bytes on {len.device}")
    if workspace is None:
        workspace = lz_decode_workspace(n, z, len.device, eng)
    if len.is_cuda:
        eng.require_device()
    with _on(len):
        eng.check(eng.lib.sfx_lz_decode_dev(_p(len), _p(src), _p(lit), z, n, _p(out), _p(workspace), workspace.numel(),
                                            _stream_ptr(len)), "sfx_lz_decode_dev")
    return out


def mems_workspace(m, max_pairs, device, engine=None):
    eng = engine or default_engine()
    return torch.empty(int(eng.lib.sfx_mems_workspace_bytes(int(m), int(max_pairs))), dtype=torch.uint8, device=device)


def _mems(eng, call, name, n, query, anchor, min_len, unique, max_pairs, capacity, workspace):
    """The checks, buffers and the repeated call every mems entry shares; call(tail...) -> status."""
    if query.dtype != torch.uint8 or query.dim() != 1 or not query.is_contiguous():
        raise TypeError("query must be a contiguous 1-D uint8 tensor")
    dev = anchor.device
    if query.device != dev:
        raise ValueError(f"query must be on the text's device ({dev})")
    min_len, max_pairs = int(min_len), int(max_pairs)
    if min_len < 1 or min_len > 0xFFFFFFFF:
        raise ValueError("min_len must be in 1 .. 2^32 - 1")
    if max_pairs < 1:
        raise ValueError("max_pairs must be at least 1")
    m = query.numel()
    max_pairs = min(max_pairs, max(m * n, 1))                # (there are no more pairs: keeps the workspace small)
    if anchor.is_cuda:
        eng.require_device()
    if workspace is None:
        workspace = mems_workspace(m, max_pairs, dev, eng)
    cap = min(max(m, 1024), max_pairs) if capacity is None else int(capacity)
    pairs, count = ctypes.c_uint64(0), ctypes.c_uint64(0)
    for _ in range(2):
        out = [torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3)]
        with _on(anchor):
            eng.check(call(_p(query), m, min_len, 1 if unique else 0, max_pairs, _p(out[0]), _p(out[1]), _p(out[2]), cap,
                           ctypes.byref(pairs), ctypes.byref(count), _p(workspace), workspace.numel(), _stream_ptr(anchor)), name)
        if pairs.value > max_pairs:
            raise SuffixHipError(f"{name}: {pairs.value} candidate pairs exceed max_pairs = {max_pairs}; raise min_len or max_pairs")
        if count.value <= cap or capacity is not None:
            break
        cap = int(count.value)
    z = min(int(count.value), cap)
    return out[0][:z].clone(), out[1][:z].clone(), out[2][:z].clone(), int(pairs.value)


def mems(text, sa, query, min_len, unique=False, max_pairs=1 << 30, capacity=None, workspace=None, engine=None):
    """The maximal exact matches of at least min_len bytes between the uint8 tensor `query` and (text, sa), all on one
    device: -> (qpos, tpos, len, pairs), three uint32 tensors in int32 storage cut to the matches -- ascending by qpos,
    then by the table rank of tpos -- and the number of candidate pairs looked at.  unique: only matches whose bytes
    occur once in the text.  More than max_pairs candidate pairs raise SuffixHipError naming the count.  The room is
    guessed (one match per query byte) and the call repeated once when there were more; with `capacity` it runs once
    and returns the first `capacity` matches.  Runs on the current stream and synchronises it once per call; the table
    is not checked (sfx_mems_dev)."""
    eng = engine or default_engine()
    _check_u8(text)
    _check_u32(sa, "sa", text.numel())
    if sa.device != text.device:
        raise ValueError(f"sa must be on the text's device ({text.device})")
    n = text.numel()
    call = lambda *tail: eng.lib.sfx_mems_dev(_p(text), n, _p(sa), *tail)
    return _mems(eng, call, "sfx_mems_dev", n, query, text, min_len, unique, max_pairs, capacity, workspace)


def hamming_workspace(nq, mismatches, max_candidates, device, engine=None):
    eng = engine or default_engine()
    return torch.empty(int(eng.lib.sfx_hamming_workspace_bytes(int(nq), int(mismatches), int(max_candidates))), dtype=torch.uint8,
                       device=device)


def _hamming(eng, call, name, n, qbytes, qoff, anchor, mismatches, max_candidates, capacity, workspace):
    """The checks, buffers and the repeated call every hamming entry shares; call(tail...) -> status."""
    if qbytes.dtype != torch.uint8 or qbytes.dim() != 1 or not qbytes.is_contiguous():
        raise TypeError("qbytes must be a contiguous 1-D uint8 tensor")
    if qoff.dtype != torch.int64 or qoff.dim() != 1 or not qoff.is_contiguous() or qoff.numel() < 1:
        raise TypeError("qoff must be a contiguous 1-D int64 tensor of nq + 1 offsets")
    dev = anchor.device
    if qbytes.device != dev or qoff.device != dev:
        raise ValueError(f"qbytes and qoff must be on the text's device ({dev})")
    k, max_candidates = int(mismatches), int(max_candidates)
    if not 0 <= k <= 255:
        raise ValueError("mismatches must be in 0 .. 255")
    if max_candidates < 1:
        raise ValueError("max_candidates must be at least 1")
    nq = qoff.numel() - 1
    max_candidates = min(max_candidates, max(nq * (k + 1) * n, 1))   # (there are no more: keeps the workspace small)
    if anchor.is_cuda:
        eng.require_device()
    if workspace is None:
        workspace = hamming_workspace(nq, k, max_candidates, dev, eng)
    first = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    cap = min(max(4 * nq, 1024), max_candidates) if capacity is None else int(capacity)
    cands, count = ctypes.c_uint64(0), ctypes.c_uint64(0)
    for _ in range(2):
        pat, tpos = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(2))
        mism = torch.empty(cap, dtype=torch.uint8, device=dev)
        with _on(anchor):
            eng.check(call(_p(qbytes), _p(qoff), nq, k, max_candidates, _p(pat), _p(tpos), _p(mism), cap, _p(first),
                           ctypes.byref(cands), ctypes.byref(count), _p(workspace), workspace.numel(), _stream_ptr(anchor)), name)
        if cands.value > max_candidates:
            raise SuffixHipError(f"{name}: {cands.value} candidates exceed max_candidates = {max_candidates}; use longer patterns, "
                                 "fewer mismatches or raise max_candidates")
        if count.value <= cap or capacity is not None:
            break
        cap = int(count.value)
    z = min(int(count.value), cap)
    return first, pat[:z].clone(), tpos[:z].clone(), mism[:z].clone(), int(cands.value)


def hamming(text, sa, qbytes, qoff, mismatches, max_candidates=1 << 30, capacity=None, workspace=None, engine=None):
    """Where do the patterns (qbytes uint8, qoff int64 of nq + 1 offsets, as for DeviceIndex.query) occur in (text, sa)
    if up to `mismatches` (0 .. 255) bytes may differ -- Hamming distance, no insertions or deletions; all tensors on
    one device.  -> (first, pattern, tpos, mism, candidates): the occurrences of pattern j are the entries
    first[j] .. first[j + 1] of pattern (uint32 in int32 storage, = j), tpos (likewise: the window's start) and mism
    (uint8: the differing bytes of the window), ordered by the owning piece of the pigeonhole cut and then by table
    rank; candidates = the exact piece hits looked at.  More than max_candidates raise SuffixHipError naming the count.
    The room is guessed and the call repeated once when there were more; with `capacity` it runs once and returns the
    first `capacity` occurrences (first stays complete).  Runs on the current stream and synchronises it once per call;
    the table is not checked (sfx_hamming_dev)."""
    eng = engine or default_engine()
    _check_u8(text)
    _check_u32(sa, "sa", text.numel())
    if sa.device != text.device:
        raise ValueError(f"sa must be on the text's device ({text.device})")
    n = text.numel()
    call = lambda *tail: eng.lib.sfx_hamming_dev(_p(text), n, _p(sa), *tail)
    return _hamming(eng, call, "sfx_hamming_dev", n, qbytes, qoff, text, mismatches, max_candidates, capacity, workspace)


EDIT_MAX_ERRORS = 31


def edit_workspace(nq, errors, max_candidates, max_hits, device, engine=None):
    eng = engine or default_engine()
    return torch.empty(int(eng.lib.sfx_edit_workspace_bytes(int(nq), int(errors), int(max_candidates), int(max_hits))), dtype=torch.uint8,
                       device=device)


def _edit_search(eng, call, name, n, qbytes, qoff, anchor, errors, max_candidates, max_hits, capacity, workspace):
    """The checks, buffers and the repeated call every edit_search entry shares; call(tail...) -> status."""
    if qbytes.dtype != torch.uint8 or qbytes.dim() != 1 or not qbytes.is_contiguous():
        raise TypeError("qbytes must be a contiguous 1-D uint8 tensor")
    if qoff.dtype != torch.int64 or qoff.dim() != 1 or not qoff.is_contiguous() or qoff.numel() < 1:
        raise TypeError("qoff must be a contiguous 1-D int64 tensor of nq + 1 offsets")
    dev = anchor.device
    if qbytes.device != dev or qoff.device != dev:
        raise ValueError(f"qbytes and qoff must be on the text's device ({dev})")
    k, max_candidates, max_hits = int(errors), int(max_candidates), int(max_hits)
    if not 0 <= k <= EDIT_MAX_ERRORS:
        raise ValueError(f"errors must be in 0 .. {EDIT_MAX_ERRORS}")
    if max_candidates < 1 or not 1 <= max_hits < 1 << 32:
        raise ValueError("max_candidates must be at least 1 and max_hits in 1 .. 2^32 - 1")
    nq = qoff.numel() - 1
    if nq and int((qoff[1:] - qoff[:-1]).min()) <= k:                # (the library finds it too: SFX_ERR_ARG)
        raise ValueError(f"every pattern needs at least errors + 1 = {k + 1} bytes")
    max_candidates = min(max_candidates, max(nq * (k + 1) * n, 1))   # (there are no more: keeps the workspace small)
    max_hits = min(max_hits, max_candidates * (2 * k + 1))
    if anchor.is_cuda:
        eng.require_device()
    if workspace is None:
        workspace = edit_workspace(nq, k, max_candidates, max_hits, dev, eng)
    first = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    cap = min(max(4 * nq, 1024), max_hits) if capacity is None else int(capacity)
    cands, hits, count = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    for _ in range(2):
        pat, tbegin, tend = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3))
        dist = torch.empty(cap, dtype=torch.uint8, device=dev)
        with _on(anchor):
            eng.check(call(_p(qbytes), _p(qoff), nq, k, max_candidates, max_hits, _p(pat), _p(tbegin), _p(tend), _p(dist), cap, _p(first),
                           ctypes.byref(cands), ctypes.byref(hits), ctypes.byref(count), _p(workspace), workspace.numel(),
                           _stream_ptr(anchor)), name)
        if cands.value > max_candidates:
            raise SuffixHipError(f"{name}: {cands.value} candidates exceed max_candidates = {max_candidates}; use longer patterns, "
                                 "fewer errors or raise max_candidates")
        if hits.value > max_hits:
            raise SuffixHipError(f"{name}: {hits.value} hits exceed max_hits = {max_hits}; use longer patterns, fewer errors or raise "
                                 "max_hits")
        if count.value <= cap or capacity is not None:
            break
        cap = int(count.value)
    z = min(int(count.value), cap)
    return first, pat[:z].clone(), tbegin[:z].clone(), tend[:z].clone(), dist[:z].clone(), int(cands.value), int(hits.value)


def edit_search(text, sa, qbytes, qoff, errors, max_candidates=1 << 30, max_hits=1 << 22, capacity=None, workspace=None, engine=None):
    """Where do the patterns (qbytes uint8, qoff int64 of nq + 1 offsets, as for hamming) occur in (text, sa) within
    `errors` (0 .. 31) substitutions, insertions and deletions -- unit-cost edit distance; all tensors on one device.
    Every pattern needs more than `errors` bytes: a shorter one raises ValueError (the offsets are read back for it).
    -> (first, pattern, tbegin, tend, dist, candidates, hits): the occurrences of pattern j are the entries
    first[j] .. first[j + 1], ascending by tend; an occurrence is an end tend with its least distance dist (uint8) and
    the largest begin that attains it.  candidates = the exact piece hits looked at, hits = the (candidate, end) pairs
    they found before the merge.  More than max_candidates / max_hits raise SuffixHipError naming the count.  The room
    is guessed and the call repeated once when there were more; with `capacity` it runs once and returns the first
    `capacity` occurrences (first stays complete).  Runs on the current stream and synchronises it at most twice per
    call; the table is not checked (sfx_edit_dev)."""
    eng = engine or default_engine()
    _check_u8(text)
    _check_u32(sa, "sa", text.numel())
    if sa.device != text.device:
        raise ValueError(f"sa must be on the text's device ({text.device})")
    n = text.numel()
    call = lambda *tail: eng.lib.sfx_edit_dev(_p(text), n, _p(sa), *tail)
    return _edit_search(eng, call, "sfx_edit_dev", n, qbytes, qoff, text, errors, max_candidates, max_hits, capacity, workspace)


def inverse_table_workspace(n, device, engine=None):
    eng = engine or default_engine()
    return torch.empty(int(eng.lib.sfx_inverse_table_workspace_bytes(int(n))), dtype=torch.uint8, device=device)


def inverse_table(sa, out=None, workspace=None, engine=None):
    """isa[sa[r]] = r (uint32 in int32 storage): sfx_inverse_table_dev.  Raises for a table that is no permutation of
    [0, n); reading that verdict synchronises the current stream."""
    eng = engine or default_engine()
    _check_u32(sa, "sa")
    n = sa.numel()
    if sa.is_cuda:
        eng.require_device()
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=sa.device)
    _check_u32(out, "out", n)
    if workspace is None:
        workspace = inverse_table_workspace(n, sa.device, eng)
    with _on(sa):
        eng.check(eng.lib.sfx_inverse_table_dev(_p(sa), n, _p(out), _p(workspace), workspace.numel(), _stream_ptr(sa)),
                  "sfx_inverse_table_dev")
    return out


def lyndon_array_workspace(n, device, engine=None):
    eng = engine or default_engine()
    return torch.empty(int(eng.lib.sfx_lyndon_array_workspace_bytes(int(n))), dtype=torch.uint8, device=device)


def lyndon_array(isa, out=None, workspace=None, engine=None):
    """The Lyndon array of the order whose inverse table isa is (inverse_table of the text's table: byte order; of the
    complemented text's table: reversed byte order): lyn[i] = the distance to the next j > i with isa[j] < isa[i], or to
    n.  uint32 in int32 storage; queued on the current stream, nothing is read back (sfx_lyndon_array_dev)."""
    eng = engine or default_engine()
    _check_u32(isa, "isa")
    n = isa.numel()
    if isa.is_cuda:
        eng.require_device()
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=isa.device)
    _check_u32(out, "out", n)
    if workspace is None:
        workspace = lyndon_array_workspace(n, isa.device, eng)
    with _on(isa):
        eng.check(eng.lib.sfx_lyndon_array_dev(_p(isa), n, _p(out), _p(workspace), workspace.numel(), _stream_ptr(isa)),
                  "sfx_lyndon_array_dev")
    return out


def runs_workspace(n, device, engine=None):
    eng = engine or default_engine()
    return torch.empty(int(eng.lib.sfx_runs_workspace_bytes(int(n))), dtype=torch.uint8, device=device)


def runs(text, sa, lcp, min_period=1, max_period=None, min_len=0, capacity=None, workspace=None, engine=None):
    """The maximal repetitions (runs) of a plain text from its table and LCP array (uint32 in int32 storage, on the
    text's device): every (begin, end, period) with period the smallest period of text[begin:end], end - begin >= 2 *
    period, and no extension to either side; min_period <= period <= max_period (None: n) and end - begin >= min_len.
    -> (begin, end, period, count): three int32 tensors cut to min(count, capacity) triples ascending by (begin,
    period), and the full count.  capacity None: n, which always suffices.  Synchronises the current stream once for
    the count; the three arrays are complete in stream order (sfx_runs_dev)."""
    eng = engine or default_engine()
    _check_u8(text)
    n = text.numel()
    _check_u32(sa, "sa", n)
    _check_u32(lcp, "lcp", n)
    for t in (sa, lcp):
        if t.device != text.device:
            raise ValueError(f"all arrays must be on one device ({text.device})")
    if max_period is not None and int(max_period) < 1:
        raise ValueError("max_period must be at least 1 (None: no limit)")
    for v in (min_period, min_len, max_period or 0):
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError("filters must be in 0 .. 2^32 - 1")
    flt = RunsFilter(int(min_period), 0 if max_period is None else int(max_period), int(min_len), 0)
    if text.is_cuda:
        eng.require_device()
    cap = n if capacity is None else int(capacity)
    dev = text.device
    begin, end, period = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3))
    if workspace is None:
        workspace = runs_workspace(n, dev, eng)
    count = ctypes.c_uint64(0)
    with _on(text):
        eng.check(eng.lib.sfx_runs_dev(_p(text), n, _p(sa), _p(lcp), ctypes.byref(flt), _p(begin), _p(end), _p(period), cap,
                                       ctypes.byref(count), _p(workspace), workspace.numel(), _stream_ptr(text)), "sfx_runs_dev")
    z = int(count.value)
    k = min(z, cap)
    return begin[:k].clone(), end[:k].clone(), period[:k].clone(), z


def doc_counts_workspace(n, device, engine=None):
    eng = engine or default_engine()
    return torch.empty(int(eng.lib.sfx_doc_counts_workspace_bytes(int(n))), dtype=torch.uint8, device=device)


def doc_counts(da, lcp, ndocs, want_df=True, want_prefix=False, workspace=None, engine=None):
    """Distinct documents under every lcp-interval of a collection, from the da and lcp of build_gsa (uint32 in int32
    storage, on one device): df[p] = the document count of the interval boundary p belongs to; dup_prefix, from which
    the count of any interval [lb, rb] is (rb - lb + 1) - (dup_prefix[rb] - dup_prefix[lb]).  -> df, dup_prefix, or
    (df, dup_prefix) when both are wanted.  Raises for a da entry >= ndocs; reading that verdict synchronises the
    current stream.  See include/suffix_hip.h."""
    eng = engine or default_engine()
    if not (want_df or want_prefix):
        raise ValueError("doc_counts: nothing wanted")
    _check_u32(da, "da")
    n = da.numel()
    _check_u32(lcp, "lcp", n)
    if lcp.device != da.device:
        raise ValueError(f"all arrays must be on one device ({da.device})")
    if da.is_cuda:
        eng.require_device()
    df = torch.empty(n, dtype=torch.int32, device=da.device) if want_df else None
    dup = torch.empty(n, dtype=torch.int32, device=da.device) if want_prefix else None
    if workspace is None:
        workspace = doc_counts_workspace(n, da.device, eng)
    with _on(da):
        eng.check(eng.lib.sfx_doc_counts_dev(_p(da), _p(lcp), n, int(ndocs), _p(dup), _p(df), _p(workspace), workspace.numel(),
                                             _stream_ptr(da)), "sfx_doc_counts_dev")
    return (df, dup) if want_df and want_prefix else df if want_df else dup


def common_substrings(sa, lcp, df, doc_starts, engine=None):
    """The longest strings common to at least d documents, d = 1 .. ndocs, from the sa and lcp of build_gsa, the df of
    doc_counts and doc_starts (int64): -> (len, pos), ndocs entries each (uint32 in int32 storage); pos is a text
    position, 0xFFFFFFFF where len is 0.  Synchronises the current stream once.  See include/suffix_hip.h."""
    eng = engine or default_engine()
    _check_u32(sa, "sa")
    n = sa.numel()
    _check_u32(lcp, "lcp", n)
    _check_u32(df, "df", n)
    if doc_starts.dtype != torch.int64 or doc_starts.dim() != 1 or not doc_starts.is_contiguous():
        raise TypeError("doc_starts must be a contiguous 1-D int64 tensor")
    for t in (lcp, df, doc_starts):
        if t.device != sa.device:
            raise ValueError(f"all arrays must be on one device ({sa.device})")
    nd = doc_starts.numel()
    if sa.is_cuda:
        eng.require_device()
    ln = torch.empty(nd, dtype=torch.int32, device=sa.device)
    pos = torch.empty(nd, dtype=torch.int32, device=sa.device)
    ws = torch.empty(int(eng.lib.sfx_common_substrings_workspace_bytes(nd)), dtype=torch.uint8, device=sa.device)
    with _on(sa):
        eng.check(eng.lib.sfx_common_substrings_dev(_p(sa), _p(lcp), _p(df), n, _p(doc_starts), nd, _p(ln), _p(pos), _p(ws), ws.numel(),
                                                    _stream_ptr(sa)), "sfx_common_substrings_dev")
    return ln, pos


class LceDeviceIndex:
    """Longest common extensions between positions of the indexed text, from the device tensors (sa, lcp) of `build_sa_lcp`
    -- or of `build_gsa` with its `doc_starts` (int64), where no extension passes a document end (sfx_lce_create_dev).
    The handle holds the inverse table and a 32-ary min-tree over lcp; lcp and doc_starts are borrowed (kept alive here),
    sa is free again after creation, which synchronises the current stream once.  `lce`, `range_min` and `rank_of` queue
    on the current stream without a synchronisation."""

    def __init__(self, sa, lcp, doc_starts=None, engine=None):
        self._eng = engine or default_engine()
        _check_u32(sa, "sa")
        _check_u32(lcp, "lcp", sa.numel())
        if lcp.device != sa.device:
            raise ValueError(f"lcp must be on the table's device ({sa.device})")
        if doc_starts is not None:
            if doc_starts.dtype != torch.int64 or doc_starts.dim() != 1 or not doc_starts.is_contiguous() or not doc_starts.numel():
                raise TypeError("doc_starts must be a contiguous 1-D int64 tensor with one entry per document")
            if doc_starts.device != sa.device:
                raise ValueError(f"doc_starts must be on the table's device ({sa.device})")
        if sa.is_cuda:
            self._eng.require_device()
        self._dev, self.n = sa.device, sa.numel()
        self._lcp, self._starts = lcp, doc_starts                       # (borrowed by the index: keep them alive)
        self._on = torch.empty(0, dtype=torch.uint8, device=sa.device)
        h = ctypes.c_void_p()
        with _on(sa):
            self._eng.check(self._eng.lib.sfx_lce_create_dev(_p(sa), _p(lcp), self.n, _p(doc_starts),
                                                             0 if doc_starts is None else doc_starts.numel(), _stream_ptr(sa),
                                                             ctypes.byref(h)), "sfx_lce_create_dev")
        self._h = h
        self.nbytes = int(self._eng.lib.sfx_lce_bytes(self.n))

    def _arg(self, t, name, n=None):
        _check_u32(t, name, n)
        if t.device != self._dev:
            raise ValueError(f"{name} must be on the index's device ({self._dev})")

    def lce(self, a, b, mismatches=0):
        """len[q] = how far the suffixes at a[q] and b[q] agree with at most `mismatches` differing bytes (the same budget
        for the whole batch); 0 for a position equal to n, 0xFFFFFFFF for one above."""
        self._arg(a, "a")
        self._arg(b, "b", a.numel())
        if not 0 <= int(mismatches) <= 0xFFFFFFFF:
            raise ValueError("mismatches must be in 0 .. 2^32 - 1")
        out = torch.empty(a.numel(), dtype=torch.int32, device=self._dev)
        with _on(self._on):
            self._eng.check(self._eng.lib.sfx_lce_query_dev(self._h, _p(a), _p(b), a.numel(), int(mismatches), _p(out),
                                                            _stream_ptr(self._on)), "sfx_lce_query_dev")
        return out

    def range_min(self, lo, hi):
        """min lcp[lo[q] : hi[q]]; 0xFFFFFFFF for an empty range or hi > n."""
        self._arg(lo, "lo")
        self._arg(hi, "hi", lo.numel())
        out = torch.empty(lo.numel(), dtype=torch.int32, device=self._dev)
        with _on(self._on):
            self._eng.check(self._eng.lib.sfx_lce_range_min_dev(self._h, _p(lo), _p(hi), lo.numel(), _p(out), _stream_ptr(self._on)),
                            "sfx_lce_range_min_dev")
        return out

    def rank_of(self, pos):
        """The table rank of every position; 0xFFFFFFFF for a position >= n."""
        self._arg(pos, "pos")
        out = torch.empty(pos.numel(), dtype=torch.int32, device=self._dev)
        with _on(self._on):
            self._eng.check(self._eng.lib.sfx_lce_ranks_dev(self._h, _p(pos), pos.numel(), _p(out), _stream_ptr(self._on)),
                            "sfx_lce_ranks_dev")
        return out

    def range_argmin(self, lo, hi):
        """The smallest index that attains min lcp[lo[q] : hi[q]]; 0xFFFFFFFF for an empty range or hi > n."""
        self._arg(lo, "lo")
        self._arg(hi, "hi", lo.numel())
        out = torch.empty(lo.numel(), dtype=torch.int32, device=self._dev)
        with _on(self._on):
            self._eng.check(self._eng.lib.sfx_lce_range_argmin_dev(self._h, _p(lo), _p(hi), lo.numel(), _p(out), _stream_ptr(self._on)),
                            "sfx_lce_range_argmin_dev")
        return out

    def _intervals(self, name, a, b, what):
        self._arg(a, what[0])
        self._arg(b, what[1], a.numel())
        lo, hi, depth = (torch.empty(a.numel(), dtype=torch.int32, device=self._dev) for _ in range(3))
        with _on(self._on):
            self._eng.check(getattr(self._eng.lib, name)(self._h, _p(a), _p(b), a.numel(), _p(lo), _p(hi), _p(depth), _stream_ptr(self._on)),
                            name)
        return lo, hi, depth

    def substr(self, pos, len):
        """(lo, hi, depth): sa[lo[q] : hi[q]] are the occurrences of the len[q] bytes at pos[q], depth the string depth of
        the lowest suffix-tree node at or below that locus; len 0 gives (0, n, 0), a substring that leaves the text (its
        document) 0xFFFFFFFF three times.  No byte of the text is read."""
        return self._intervals("sfx_lce_substr_dev", pos, len, ("pos", "len"))

    def lca(self, a, b):
        """(lo, hi, depth): the lowest common ancestor of the suffixes at positions a[q] and b[q] as a rank interval with
        its string depth; a[q] == b[q] gives the suffix's own rank, a position >= n 0xFFFFFFFF three times."""
        return self._intervals("sfx_lce_lca_dev", a, b, ("a", "b"))

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._eng.lib.sfx_lce_destroy(h)

    __del__ = close


def suffix_links_workspace(n, device, engine=None):
    eng = engine or default_engine()
    return torch.empty(int(eng.lib.sfx_suffix_links_workspace_bytes(int(n))), dtype=torch.uint8, device=device)


def suffix_links(index, sa, node_lb, node_rb, node_depth, out=None, workspace=None):
    """slink (uint32 in int32 storage): for every internal node of `suffix_tree`'s table the dense id of the node that
    spells its string without the first byte; 0xFFFFFFFF for the root.  `index` is the LceDeviceIndex made from (sa, lcp)
    -- a plain table's; sa is that table.  Queues on the current stream without a synchronisation
    (sfx_suffix_links_dev)."""
    if not isinstance(index, LceDeviceIndex):
        raise TypeError("index must be an LceDeviceIndex")
    eng = index._eng
    index._arg(sa, "sa", index.n)
    nodes = node_lb.numel()
    for t, name in ((node_lb, "node_lb"), (node_rb, "node_rb"), (node_depth, "node_depth")):
        index._arg(t, name, nodes)
    if out is None:
        out = torch.empty(nodes, dtype=torch.int32, device=index._dev)
    else:
        index._arg(out, "out", nodes)
    if workspace is None:
        workspace = suffix_links_workspace(index.n, index._dev, eng)
    with _on(index._on):
        eng.check(eng.lib.sfx_suffix_links_dev(index._h, _p(sa), nodes, _p(node_lb), _p(node_rb), _p(node_depth), _p(out), _p(workspace),
                                               workspace.numel(), _stream_ptr(index._on)), "sfx_suffix_links_dev")
    return out


DOCLIST_ORDERS = {"doc": 0, "tf": 1}


class DocListDeviceIndex:
    """Which documents lie in a rank interval of a collection, and how often each: from the device tensors da (uint32 in
    int32 storage) and doc_starts (int64) of `build_gsa` (sfx_doclist_create_dev).  The handle holds PREV and the ranks
    ordered by (document, rank), 8n bytes; da and doc_starts are borrowed (kept alive here).  Creation verifies da against
    doc_starts and synchronises the current stream once.  occ_cut: intervals longer than it are listed by document, the
    others by occurrence (0 = automatic, 32 ndocs); both give the same arrays."""

    def __init__(self, da, doc_starts, occ_cut=0, engine=None):
        self._eng = engine or default_engine()
        _check_u32(da, "da")
        if doc_starts.dtype != torch.int64 or doc_starts.dim() != 1 or not doc_starts.is_contiguous():
            raise TypeError("doc_starts must be a contiguous 1-D int64 tensor with one entry per document")
        if doc_starts.device != da.device:
            raise ValueError(f"doc_starts must be on the device of da ({da.device})")
        if da.is_cuda:
            self._eng.require_device()
        self._dev, self.n, self.ndocs = da.device, da.numel(), doc_starts.numel()
        self._keep = (da, doc_starts)                                   # (borrowed by the index: keep them alive)
        self._on = torch.empty(0, dtype=torch.uint8, device=da.device)
        h = ctypes.c_void_p()
        with _on(da):
            self._eng.check(self._eng.lib.sfx_doclist_create_dev(_p(da), self.n, _p(doc_starts), self.ndocs, int(occ_cut), None, 0,
                                                                 _stream_ptr(da), ctypes.byref(h)), "sfx_doclist_create_dev")
        self._h = h
        self.nbytes = int(self._eng.lib.sfx_doclist_bytes(self.n))

    def workspace(self, nq, list_limit):
        return torch.empty(int(self._eng.lib.sfx_doclist_workspace_bytes(int(nq), int(list_limit))), dtype=torch.uint8, device=self._dev)

    def list(self, start, end, order="doc", top_k=0, list_limit=1 << 30, capacity=None, workspace=None):
        """-> (doc, tf, first, listed): list j -- the documents with a rank in [start[j], end[j]) and their counts there,
        ascending by document (order "doc") or by descending count, ties by document ("tf"), cut to the first top_k
        entries when top_k > 0 -- is doc / tf [first[j] : first[j + 1]] (uint32 in int32 storage; first int64, nq + 1
        entries); listed = the number of entries before the cut.  More than list_limit of those raise SuffixHipError.
        Without a workspace of the caller's, list_limit is lowered to what the interval lengths allow, which reads their
        sum back (one more synchronisation).  With `capacity` only the first `capacity` entries are returned (first stays
        complete).  Runs on the current stream and synchronises it once; doc and tf are complete in stream order: the ordering
        is queued behind that synchronisation and reads the workspace, so a `workspace` of the caller's must stay alive and
        unwritten until the stream has passed it (the one made here is torch's, which frees in stream order)."""
        if order not in DOCLIST_ORDERS:
            raise ValueError(f"order must be one of {sorted(DOCLIST_ORDERS)}")
        _check_u32(start, "start")
        nq = start.numel()
        _check_u32(end, "end", nq)
        if start.device != self._dev or end.device != self._dev:
            raise ValueError(f"start and end must be on the index's device ({self._dev})")
        top_k, list_limit = int(top_k), int(list_limit)
        if not 0 <= top_k <= 0xFFFFFFFF:
            raise ValueError("top_k must be in 0 .. 2^32 - 1")
        if list_limit < 1:
            raise ValueError("list_limit must be at least 1")
        if workspace is None:
            if nq:
                lens = (end.to(torch.int64) & 0xFFFFFFFF) - (start.to(torch.int64) & 0xFFFFFFFF)
                list_limit = min(list_limit, max(int(lens.clamp(0, max(self.ndocs, 1)).sum().item()), 1))
            workspace = self.workspace(nq, list_limit)
        first = torch.zeros(nq + 1, dtype=torch.int64, device=self._dev)
        cap = min(list_limit, 0xFFFFFFFF) if capacity is None else int(capacity)
        doc, tf = (torch.empty(cap, dtype=torch.int32, device=self._dev) for _ in range(2))
        listed, count = ctypes.c_uint64(0), ctypes.c_uint64(0)
        with _on(self._on):
            self._eng.check(self._eng.lib.sfx_doclist_list_dev(self._h, _p(start), _p(end), nq, DOCLIST_ORDERS[order], top_k, list_limit,
                                                               _p(doc), _p(tf), cap, _p(first), ctypes.byref(listed), ctypes.byref(count),
                                                               _p(workspace), workspace.numel(), _stream_ptr(self._on)), "sfx_doclist_list_dev")
        if listed.value > min(list_limit, 0xFFFFFFFF):
            raise SuffixHipError(f"sfx_doclist_list_dev: {listed.value} entries exceed list_limit = {list_limit}")
        z = min(int(count.value), cap)
        return doc[:z], tf[:z], first, int(listed.value)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._eng.lib.sfx_doclist_destroy(h)

    __del__ = close


class GeneralizedDeviceIndex:
    """Resident generalized index over device tensors (text, doc_starts, GSA, DA) -- borrowed, keep them alive;
    `query` = per query (start, end, found, any, ndocs): matches inside one document only, ndocs = the number of
    distinct documents that contain the query (sfx_gindex_query_dev)."""

    def __init__(self, text, doc_starts, sa, da, engine=None, occ_cut=0):
        self._eng = engine or default_engine()
        _check_u8(text)
        self._keep = (text, doc_starts, sa, da)
        self.occ_cut = int(occ_cut)                 # of the listing index `documents` makes: DocListDeviceIndex's (0 = automatic)
        self._text = text
        h = ctypes.c_void_p()
        with _on(text):
            self._eng.check(self._eng.lib.sfx_gindex_create_dev(_p(text), text.numel(), _p(doc_starts), doc_starts.numel(), _p(sa),
                                                                _p(da), _stream_ptr(text), ctypes.byref(h)), "sfx_gindex_create_dev")
        self._h = h

    def query(self, qbytes, qoff):
        """qbytes: uint8 tensor, qoff: int64 tensor of nq + 1 offsets, both contiguous and on the text's device."""
        dev = self._text.device
        if qbytes.dtype != torch.uint8 or qbytes.dim() != 1 or not qbytes.is_contiguous():
            raise TypeError("qbytes must be a contiguous 1-D uint8 tensor")
        if qoff.dtype != torch.int64 or qoff.dim() != 1 or not qoff.is_contiguous() or qoff.numel() < 1:
            raise TypeError("qoff must be a contiguous 1-D int64 tensor of nq + 1 offsets")
        if qbytes.device != dev or qoff.device != dev:
            raise ValueError(f"qbytes and qoff must be on the index's device ({dev})")
        nq = qoff.numel() - 1
        start = torch.empty(nq, dtype=torch.int32, device=dev)
        end = torch.empty(nq, dtype=torch.int32, device=dev)
        found = torch.empty(nq, dtype=torch.uint8, device=dev)
        anyp = torch.empty(nq, dtype=torch.int32, device=dev)
        ndocs = torch.empty(nq, dtype=torch.int32, device=dev)
        with _on(self._text):
            self._eng.check(self._eng.lib.sfx_gindex_query_dev(self._h, _p(qbytes), _p(qoff), nq, _p(start), _p(end), _p(found),
                                                               _p(anyp), _p(ndocs), _stream_ptr(self._text)), "sfx_gindex_query_dev")
        return start, end, found, anyp, ndocs

    def documents(self, qbytes, qoff, order="doc", top_k=0, list_limit=1 << 30, capacity=None):
        """The documents that hold each query and its count in each: the search (without its count of documents, which
        walks every occurrence) and then DocListDeviceIndex.list over the intervals -> (doc, tf, first, listed).  The
        listing index is made on the first call, with the occ_cut given to the constructor, and kept."""
        dev = self._text.device
        if qoff.dtype != torch.int64 or qoff.dim() != 1 or not qoff.is_contiguous() or qoff.numel() < 1:
            raise TypeError("qoff must be a contiguous 1-D int64 tensor of nq + 1 offsets")
        if qbytes.dtype != torch.uint8 or qbytes.dim() != 1 or not qbytes.is_contiguous() or qbytes.device != dev or qoff.device != dev:
            raise TypeError(f"qbytes must be a contiguous 1-D uint8 tensor on the index's device ({dev}), as qoff")
        if getattr(self, "_doclist", None) is None:
            self._doclist = DocListDeviceIndex(self._keep[3], self._keep[1], occ_cut=self.occ_cut, engine=self._eng)
        nq = qoff.numel() - 1
        start = torch.zeros(nq, dtype=torch.int32, device=dev)
        end = torch.zeros(nq, dtype=torch.int32, device=dev)
        with _on(self._text):
            self._eng.check(self._eng.lib.sfx_gindex_query_dev(self._h, _p(qbytes), _p(qoff), nq, _p(start), _p(end), None, None, None,
                                                               _stream_ptr(self._text)), "sfx_gindex_query_dev")
        return self._doclist.list(start, end, order=order, top_k=top_k, list_limit=list_limit, capacity=capacity)

    def match_stats(self, query, max_len=0, want_src=False, want_interval=False):
        """As the module's match_stats, against the collection: a match lies inside one document, ranks are GSA ranks
        (sfx_gindex_match_stats_dev)."""
        m, max_len, ln, src, start, end = _ms_outputs(query, self._text.device, max_len, want_src, want_interval)
        with _on(self._text):
            self._eng.check(self._eng.lib.sfx_gindex_match_stats_dev(self._h, _p(query), m, max_len, _p(ln), _p(src), _p(start),
                                                                     _p(end), _stream_ptr(self._text)), "sfx_gindex_match_stats_dev")
        return _ms_result(ln, src, start, end, want_src, want_interval)

    def mems(self, query, min_len, unique=False, max_pairs=1 << 30, capacity=None, workspace=None):
        """As the module's mems, against the collection: a match lies inside one document, tpos is a text position
        (sfx_gindex_mems_dev)."""
        call = lambda *tail: self._eng.lib.sfx_gindex_mems_dev(self._h, *tail)
        return _mems(self._eng, call, "sfx_gindex_mems_dev", self._text.numel(), query, self._text, min_len, unique, max_pairs,
                     capacity, workspace)

    def hamming(self, qbytes, qoff, mismatches, max_candidates=1 << 30, capacity=None, workspace=None):
        """As the module's hamming, against the collection: a window lies inside one document, tpos is a text position
        (sfx_gindex_hamming_dev)."""
        call = lambda *tail: self._eng.lib.sfx_gindex_hamming_dev(self._h, *tail)
        return _hamming(self._eng, call, "sfx_gindex_hamming_dev", self._text.numel(), qbytes, qoff, self._text, mismatches,
                        max_candidates, capacity, workspace)

    def edit_search(self, qbytes, qoff, errors, max_candidates=1 << 30, max_hits=1 << 22, capacity=None, workspace=None):
        """As the module's edit_search, against the collection: an occurrence lies inside one document, tbegin and tend
        are text positions (sfx_gindex_edit_dev)."""
        call = lambda *tail: self._eng.lib.sfx_gindex_edit_dev(self._h, *tail)
        return _edit_search(self._eng, call, "sfx_gindex_edit_dev", self._text.numel(), qbytes, qoff, self._text, errors, max_candidates,
                            max_hits, capacity, workspace)

    def close(self):
        dx, self._doclist = getattr(self, "_doclist", None), None
        if dx is not None:
            dx.close()
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._eng.lib.sfx_gindex_destroy(h)

    __del__ = close


def widen_u64(sa32, out=None, engine=None):
    """u32 index tensor (int32 storage) -> int64 tensor holding the same indices (config 4)."""
    eng = engine or default_engine()
    if out is None:
        out = torch.empty(sa32.numel(), dtype=torch.int64, device=sa32.device)
    with _on(sa32):
        eng.check(eng.lib.sfx_widen_u32_to_u64_dev(_p(sa32), sa32.numel(), _p(out), _stream_ptr(sa32)),
                  "sfx_widen_u32_to_u64_dev")
    return out


def build_lcp_range(text, sa_part, prev_suffix=None, engine=None):
    """LCP of one contiguous slice of the suffix array (direct comparison with the predecessor;
    prev_suffix = last suffix of the previous slice, None for the first slice)."""
    eng = engine or default_engine()
    _check_u8(text)
    out = torch.empty(sa_part.numel(), dtype=torch.int32, device=text.device)
    prev = 0xFFFFFFFF if prev_suffix is None else int(prev_suffix) & 0xFFFFFFFF
    with _on(text):
        eng.check(eng.lib.sfx_build_lcp_range_u32_dev(_p(text), text.numel(), _p(sa_part), sa_part.numel(), prev,
                                                      _p(out), _stream_ptr(text)), "sfx_build_lcp_range_u32_dev")
    return out


def query_batch_range(text, sa_part, qbytes, qoff, engine=None):
    """Like query_batch, against one contiguous slice of the suffix array: start/end index the slice."""
    eng = engine or default_engine()
    nq = qoff.numel() - 1
    dev = text.device
    start = torch.empty(nq, dtype=torch.int32, device=dev)
    end = torch.empty(nq, dtype=torch.int32, device=dev)
    found = torch.empty(nq, dtype=torch.uint8, device=dev)
    anyp = torch.empty(nq, dtype=torch.int32, device=dev)
    with _on(text):
        eng.check(eng.lib.sfx_query_batch_range_dev(_p(text), text.numel(), _p(sa_part), sa_part.numel(), _p(qbytes),
                                                    _p(qoff), nq, _p(start), _p(end), _p(found), _p(anyp),
                                                    _stream_ptr(text)), "sfx_query_batch_range_dev")
    return start, end, found, anyp
