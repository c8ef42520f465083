"""Text positions and ranks above 2^31 through every structure built on the suffix array, shared by test_highpos_emu.py
(the emulator build, a small padding) and test_gpu_highpos.py (libsuffix_hip.so, n = 2^31 + 35 539 and n = 2^32 - 1).

The text is T = padding + S.  The padding is uniform over b"ACGT" and never enters an expectation except for its last
256 bytes, which are read back.  S -- the tail, TAIL_LEN bytes over {0x01, 0x02, 0xFE, 0xFF} from a fixed seed -- ends the
text and shares no byte with the padding, so with a = the number of tail suffixes whose first byte is <= 0x02, b = s - a:

  * SA_T[0:a] = pad_len + SA_S[0:a] and SA_T[n-b:n] = pad_len + SA_S[a:s]: a block of low ranks and one of high ranks,
    both of high positions; LCP_T equals LCP_S inside both blocks and LCP_T[a] = LCP_T[n-b] = 0;
  * the longest previous factor of a tail position in T is the one in S (a source in the padding matches 0 bytes), and
    no greedy LZ phrase crosses pad_len.

So a small oracle -- oracle.sais and lcp_kasai of S, the serial checkers of the other suites, numpy brute force over the
last s + 256 bytes for whatever touches the padding -- gives exact answers at exactly the high positions and ranks.
Nothing expected comes from an engine run alone, and every u32 output is read as unsigned."""
import ctypes
import shutil
import tempfile

import numpy as np
import pytest
import torch

import _gsa
import _lce
import _lz
import _match
import _mem
import _repeats
from suffix_amd import SuffixTable
from suffix_amd import device as sdev

NONE = 0xFFFFFFFF
TAIL_LEN = 65539
TAIL_SEED = 0x71A11
WIN = 256                                   # the padding bytes that are read back
ALPHABET = np.array([0x01, 0x02, 0xFE, 0xFF], dtype=np.uint8)
BLOCK, RUN = 3000, 600                      # the planted block (agrees beyond the LCP route's 1024-byte hand-over), the runs
BWT_STEP = 256
PLACEMENTS = {"A": (1 << 31) - 30000, "B": (1 << 32) - 1 - TAIL_LEN}


# ---- the tail and what the small oracle says about it --------------------------------------------------------------------
def make_tail():
    rng = np.random.default_rng(TAIL_SEED)
    uni = lambda k: ALPHABET[rng.integers(0, 4, k)]
    block = uni(BLOCK)
    parts = [uni(20000), block, uni(10000), block, np.full(RUN, 0xFF, dtype=np.uint8), uni(10000), block,
             np.full(RUN, 0x01, dtype=np.uint8)]
    parts.append(uni(TAIL_LEN - sum(p.size for p in parts)))
    s = np.concatenate(parts)
    assert s.size == TAIL_LEN
    return s


_tail_cache = {}


def tail(orc):
    """What is known about S alone, computed once and left unchanged: bytes, oracle SA / LCP, inverse table, a, b, LPF."""
    if not _tail_cache:
        S = make_tail()
        sa = np.ascontiguousarray(orc.sais(S.tobytes()), dtype=np.uint32)
        lcp = np.ascontiguousarray(orc.lcp_kasai(S.tobytes(), sa), dtype=np.uint32)
        lcp[0] = 0
        isa = _lce.expected_isa(sa)
        a = int((S <= 0x02).sum())
        assert (S[sa[:a].astype(np.int64)] <= 0x02).all() and (S[sa[a:].astype(np.int64)] >= 0xFE).all() and lcp[a] == 0
        _tail_cache.update(S=S, bytes=S.tobytes(), sa=sa, lcp=lcp, isa=isa, a=a, b=TAIL_LEN - a)
    return _tail_cache


def lpf_from_tables(sa, lcp):
    """The longest-previous-factor array from a suffix array and its LCP array by the stack sweep of Crochemore and Ilie
    (2008): a rank leaves the stack when a smaller position arrives, with the larger of the two LCP values beside it.
    test_highpos_emu.py holds it against the definition (_lz.lpf)."""
    n = len(sa)
    SA, L = [int(x) for x in sa] + [-1], [int(x) for x in lcp] + [0]
    out = np.zeros(n, dtype=np.uint32)
    if n == 0:
        return out
    L[0] = 0
    st = [0]
    for i in range(1, n + 1):
        while st and (SA[i] < SA[st[-1]] or L[i] <= L[st[-1]]):
            top = st.pop()
            if SA[i] < SA[top]:
                out[SA[top]] = max(L[top], L[i])
                L[i] = min(L[top], L[i])
            else:
                out[SA[top]] = L[top]
        if i < n:
            st.append(i)
    return out


def tail_lpf(orc):
    t = tail(orc)
    if "lpf" not in t:
        t["lpf"] = lpf_from_tables(t["sa"], t["lcp"])
    return t["lpf"]


def expected_blocks(orc, pad_len):
    """-> (sa_low, sa_high, lcp_low, lcp_high): SA_T[0:a], SA_T[n-b:n], LCP_T[0:a+1], LCP_T[n-b:n] (uint32)."""
    t = tail(orc)
    a = t["a"]
    sa = (t["sa"].astype(np.int64) + pad_len).astype(np.uint32)
    lcp_low = np.concatenate((t["lcp"][:a], [0])).astype(np.uint32)
    return sa[:a], sa[a:], lcp_low, t["lcp"][a:].copy()


def U(x):
    """uint32 in int32 storage -> int64 values."""
    return x.to(torch.int64) & 0xFFFFFFFF


def H(x):
    """-> the host's uint32 view of an int32 tensor."""
    return x.cpu().numpy().view(np.uint32)


def I32(a, device):
    """uint32 values -> int32 storage on the device."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to(device)


def _sync(device):
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()


# ---- the fixture -----------------------------------------------------------------------------------------------------------
class HighText:
    """Text, SA and LCP of one placement on `device`, and the tail's expectations.  may_skip: a placement that may be
    skipped for want of memory (B); the reason names the need and what is free."""

    def __init__(self, eng, device, orc, pad_len, may_skip=False, seed=0x9AD):
        self.eng, self.device, self.orc, self.pad_len, self.may_skip = eng, device, orc, int(pad_len), may_skip
        self.cuda = str(device).startswith("cuda")
        self.t = tail(orc)
        self.s, self.a, self.b = TAIL_LEN, self.t["a"], self.t["b"]
        self.n = self.pad_len + self.s
        self.shift = self.n - self.s                              # rank shift of the high block (= pad_len)
        self.tmp, self._checkers = tempfile.mkdtemp(prefix="highpos_"), {}
        self.text = self._make_text(seed)
        self.require(int(eng.lib.sfx_sa_lcp_workspace_bytes(self.n)) + 8 * self.n, "build_sa_lcp")
        ws = sdev.sa_lcp_workspace(self.n, device, eng)
        self.sa, self.lcp = sdev.build_sa_lcp(self.text, workspace=ws, engine=eng)
        _sync(device)
        self.stats_n = eng.build_stats().get("n")
        del ws
        self.release()
        self.win = self.text[self.pad_len - WIN:].cpu().numpy()    # the last 256 padding bytes and the tail, read back
        assert np.array_equal(self.win[WIN:], self.t["S"])
        self.win_base = self.pad_len - WIN

    def _make_text(self, seed):
        n, pad = self.n, self.pad_len
        if not self.cuda:
            rng = np.random.default_rng(seed)
            return torch.from_numpy(np.concatenate((np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, pad)], self.t["S"])))
        self.require(n + (9 << 27), "the text")
        text = torch.empty(n, dtype=torch.uint8, device=self.device)
        g = torch.Generator(device=self.device)
        g.manual_seed(seed)
        lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=self.device)
        for lo in range(0, pad, 1 << 27):
            c = min(1 << 27, pad - lo)
            text[lo:lo + c] = lut[torch.randint(0, 4, (c,), generator=g, device=self.device)]
        text[pad:] = torch.from_numpy(self.t["S"]).to(self.device)
        return text

    def release(self):
        if self.cuda:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            self.eng.release_cached_buffers()

    def require(self, nbytes, what):
        if not self.cuda:
            return
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
        if free < nbytes:
            msg = f"n = {self.n}: {what} needs {nbytes} bytes of device memory, {free} are free"
            if self.may_skip:
                pytest.skip(msg)
            raise AssertionError(msg)

    def close(self):
        self.text = self.sa = self.lcp = self.isa = self.rep_any = self.rep_earlier = None
        self.release()
        shutil.rmtree(self.tmp, ignore_errors=True)

    # -- ranks and intervals of T from those of S
    def rank_T(self, r):
        r = np.asarray(r, dtype=np.int64)
        return np.where(r < self.a, r, r + self.shift)

    def checker(self, name, build):
        """A serial checker of another suite, compiled once per fixture into its scratch directory."""
        if name not in self._checkers:
            self._checkers[name] = build(self.tmp)
        return self._checkers[name]


# ---- patterns ------------------------------------------------------------------------------------------------------------
def _occ(S, pat):
    p = np.frombuffer(bytes(pat), dtype=np.uint8)
    if p.size > S.size:
        return np.zeros(0, dtype=np.int64)
    return np.flatnonzero((np.lib.stride_tricks.sliding_window_view(S, p.size) == p).all(axis=1))


def search_cases(fx):
    """-> [(pattern, start, end, positions in table order or None, found)] by brute force: 512 substrings of S (their
    interval is S's, shifted by n - s where the first byte is >= 0xFE), 64 patterns that straddle pad_len (one
    occurrence each, at pad_len - j; the rank is read from the checked inverse table by the caller) and absent strings."""
    S, isa, sa_s = fx.t["S"], fx.t["isa"].astype(np.int64), fx.t["sa"].astype(np.int64)
    rng = np.random.default_rng(5)
    cases = []
    for q in range(512):
        m = int(rng.integers(9, 41)) if q % 8 else (2 if q == 8 else int(rng.integers(5, 9)))   # (short ones: many occurrences)
        p = int(rng.integers(0, fx.s - m + 1)) if q % 16 else fx.s - m            # (every 16th: a suffix of the text)
        pat = S[p:p + m].tobytes()
        occ = _occ(S, pat)
        r = np.sort(isa[occ])
        assert r.size and r[-1] - r[0] + 1 == r.size
        lo, hi = int(fx.rank_T(r[0])), int(fx.rank_T(r[-1])) + 1
        cases.append((pat, lo, hi, sa_s[r] + fx.pad_len, True))
    for q in range(64):
        j, i = 1 + q % 32, 1 + (q * 7) % 19
        pat = fx.win[WIN - j:WIN + i].tobytes()
        cases.append((pat, None, None, np.array([fx.pad_len - j], dtype=np.int64), True))
    absent = [b"\xff" * (RUN + 64), b"\x01" * (RUN + 64), b"\x01A", b"A\xfe\x41"]
    assert all(_occ(S, pat).size == 0 for pat in absent)
    while len(absent) < 24:
        pat = ALPHABET[rng.integers(0, 4, 24)].tobytes()
        if _occ(S, pat).size == 0:
            absent.append(pat)
    cases += [(pat, 0, 0, np.zeros(0, dtype=np.int64), False) for pat in absent]
    return cases


def pack(patterns, device):
    off = np.zeros(len(patterns) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(p) for p in patterns])
    qb = np.frombuffer(b"".join(patterns), dtype=np.uint8).copy()
    return torch.from_numpy(qb).to(device), torch.from_numpy(off).to(device)


def _check_intervals(fx, cases, start, end, what, found=None, anyp=None):
    """start / end (int64 tensors) against the cases; the positions are read from the table between them."""
    st, en = start.cpu().numpy(), end.cpu().numpy()
    sa = fx.sa
    for k, (pat, lo, hi, pos, there) in enumerate(cases):
        s_, e_ = int(st[k]), int(en[k])
        if lo is not None:
            assert (s_, e_) == (lo, hi), (what, k, pat[:16], (s_, e_), (lo, hi))
        assert e_ - s_ == pos.size, (what, k, pat[:16], s_, e_, pos.size)
        if found is not None:
            assert bool(found[k]) == there, (what, "found", k)
            ap = int(anyp[k])
            assert (ap in pos.tolist()) if there else ap == NONE, (what, "any", k, ap)
    # the occurrences, in table order, in one gather
    tot = sum(c[3].size for c in cases)
    ranks = np.concatenate([np.arange(int(st[k]), int(en[k])) for k in range(len(cases))]) if tot else np.zeros(0, dtype=np.int64)
    got = U(sa[torch.from_numpy(ranks).to(sa.device)]).cpu().numpy()
    want = np.concatenate([c[3] for c in cases])
    assert np.array_equal(got, want), (what, "positions", np.flatnonzero(got != want)[:4])


# ---- the groups ------------------------------------------------------------------------------------------------------------
def _blocks_equal(fx, sa, lcp, what):
    sa_lo, sa_hi, lcp_lo, lcp_hi = expected_blocks(fx.orc, fx.pad_len)
    n, a, b = fx.n, fx.a, fx.b
    if sa is not None:
        assert np.array_equal(H(sa[:a]), sa_lo), (what, "sa, low block")
        assert np.array_equal(H(sa[n - b:]), sa_hi), (what, "sa, high block")
    if lcp is not None:
        got = H(lcp[:a + 1])
        got[0] = 0                                                   # (lcp[0] is 0 by definition, whatever it holds)
        assert np.array_equal(got, lcp_lo), (what, "lcp, low block", np.flatnonzero(got != lcp_lo)[:4])
        got = H(lcp[n - b:])
        assert np.array_equal(got, lcp_hi), (what, "lcp, high block", np.flatnonzero(got != lcp_hi)[:4])


def check_builds(eng, device, fx, verify=None):
    """build_sa_lcp (the fixture's), build_sa and build_lcp on both blocks exactly; 2^16 sampled middle ranks of LCP by
    direct byte comparison; st["n"] == n; verify(text, sa) -> (ok, how) = the whole-array gate, where given."""
    n = fx.n
    assert fx.stats_n == n, (fx.stats_n, n)
    _blocks_equal(fx, fx.sa, fx.lcp, "build_sa_lcp")
    if verify is not None:
        ok, how = verify(fx.text, fx.sa)
        assert ok, how
    # middle ranks: lcp[r] against the bytes of sa[r - 1] and sa[r], 128 bytes wide (random DNA agrees on ~ log4 n)
    g = torch.Generator()
    g.manual_seed(7)
    r = torch.randint(fx.a + 1, n - fx.b, (1 << 16,), generator=g).to(fx.sa.device)
    x, y, h = U(fx.sa[r - 1]), U(fx.sa[r]), U(fx.lcp[r])
    assert int(h.max()) < 128 and bool((x < fx.pad_len).all()) and bool((y < fx.pad_len).all())
    w = torch.arange(128, device=fx.sa.device)
    bx, by = fx.text[torch.clamp(x[:, None] + w, max=n - 1)], fx.text[torch.clamp(y[:, None] + w, max=n - 1)]
    same = (bx == by) & (x[:, None] + w < n) & (y[:, None] + w < n)
    first = torch.where(same.all(dim=1), torch.full_like(h, 128), (~same).to(torch.int8).argmax(dim=1))
    assert torch.equal(first, h), ("sampled lcp", int((first != h).sum()))
    del bx, by, same
    fx.require(int(eng.lib.sfx_sa_workspace_bytes(n)) + 4 * n, "build_sa")
    ws = sdev.sa_workspace(n, fx.text.device, eng)
    sa2 = sdev.build_sa(fx.text, workspace=ws, engine=eng)
    _sync(device)
    assert eng.build_stats().get("n") == n
    del ws
    fx.release()
    _blocks_equal(fx, sa2, None, "build_sa")
    assert torch.equal(sa2, fx.sa), "build_sa and build_sa_lcp disagree"
    fx.require(int(eng.lib.sfx_lcp_workspace_bytes(n)) + 4 * n, "build_lcp")
    lcp2 = sdev.build_lcp(fx.text, sa2, engine=eng)
    _sync(device)
    _blocks_equal(fx, None, lcp2, "build_lcp")
    assert torch.equal(lcp2[1:], fx.lcp[1:]), "build_lcp and build_sa_lcp disagree"
    del sa2, lcp2
    fx.release()


def inverse(fx):
    """The inverse table, made once per fixture (several groups lean on it; check_inverse is what checks it)."""
    if getattr(fx, "isa", None) is None:
        fx.require(int(fx.eng.lib.sfx_inverse_table_workspace_bytes(fx.n)) + 4 * fx.n, "inverse_table")
        fx.isa = sdev.inverse_table(fx.sa, engine=fx.eng)
        _sync(fx.device)
        fx.release()
    return fx.isa


def check_inverse(eng, device, fx):
    isa = inverse(fx)
    got = H(isa[fx.pad_len:]).astype(np.int64)
    want = fx.rank_T(fx.t["isa"])
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:4]
    for lo in range(0, fx.n, 1 << 28):                               # isa[sa[r]] == r over the whole array
        hi = min(fx.n, lo + (1 << 28))
        back = U(isa[U(fx.sa[lo:hi])])
        assert torch.equal(back, torch.arange(lo, hi, device=back.device)), lo
        del back


def _boundary_ranks(fx, cases):
    """The straddling patterns get their rank from the inverse table (checked by check_inverse)."""
    isa = inverse(fx)
    out = []
    for pat, lo, hi, pos, there in cases:
        if lo is None:
            lo = int(U(isa[int(pos[0]):int(pos[0]) + 1])[0])
            hi = lo + 1
        out.append((pat, lo, hi, pos, there))
    return out


def check_search(eng, device, fx):
    """query_batch and DeviceIndex.query."""
    cases = _boundary_ranks(fx, search_cases(fx))
    qb, qo = pack([c[0] for c in cases], fx.text.device)
    res = sdev.query_batch(fx.text, fx.sa, qb, qo, engine=eng)
    _sync(device)
    _check_intervals(fx, cases, U(res[0]), U(res[1]), "query_batch", res[2].cpu().numpy(), H(res[3]))
    ix = sdev.DeviceIndex(fx.text, fx.sa, engine=eng)
    try:
        res = ix.query(qb, qo)
        _sync(device)
        _check_intervals(fx, cases, U(res[0]), U(res[1]), "DeviceIndex.query", res[2].cpu().numpy(), H(res[3]))
    finally:
        _sync(device)
        ix.close()
    fx.release()
    # the host index over host copies of text and table: sfx_index_create / sfx_positions_batch / sfx_contains_batch
    t_host, sa_host = fx.text.cpu().numpy(), fx.sa.cpu().numpy().view(np.uint32)
    blob = np.frombuffer(b"".join(c[0] for c in cases), dtype=np.uint8)
    off = np.concatenate(([0], np.cumsum([len(c[0]) for c in cases]))).astype(np.uint64)
    nq = len(cases)
    start, end, anyp = (np.full(nq, 0xDEADBEEF, dtype=np.uint32) for _ in range(3))
    found = np.full(nq, 7, dtype=np.uint8)
    h = ctypes.c_void_p()
    eng.check(eng.lib.sfx_index_create(_gsa.ptr(t_host), fx.n, _gsa.ptr(sa_host), ctypes.byref(h)), "sfx_index_create")
    try:
        eng.check(eng.lib.sfx_positions_batch(h, _gsa.ptr(blob), _gsa.ptr(off), nq, _gsa.ptr(start), _gsa.ptr(end)), "sfx_positions_batch")
        eng.check(eng.lib.sfx_contains_batch(h, _gsa.ptr(blob), _gsa.ptr(off), nq, _gsa.ptr(found), _gsa.ptr(anyp)), "sfx_contains_batch")
    finally:
        eng.lib.sfx_index_destroy(h)
    del t_host, sa_host
    as64 = lambda x: torch.from_numpy(x.astype(np.int64))
    _check_intervals(fx, cases, as64(start), as64(end), "sfx_positions_batch", found, anyp)
    fx.release()


def splice_query(fx, m=8192, seed=11):
    """m bytes spliced from pieces of S of 20 to 400 bytes, one byte of each changed."""
    rng = np.random.default_rng(seed)
    S, out, have = fx.t["S"], [], 0
    while have < m:
        ln = int(rng.integers(20, 401))
        p = int(rng.integers(0, fx.s - ln + 1)) if len(out) % 5 else fx.s - ln    # (every fifth piece: the end of the text)
        piece = S[p:p + ln].copy()
        piece[int(rng.integers(0, ln))] = ALPHABET[rng.integers(0, 4)]
        out.append(piece)
        have += ln
    return np.concatenate(out)[:m].copy()


def _unshift(fx, ranks):
    r = np.asarray(ranks, dtype=np.int64)
    assert ((r <= fx.a) | (r >= fx.n - fx.b)).all(), "a rank in the padding's block"
    return np.where(r > fx.a, r - fx.shift, r)


def check_match_stats(eng, device, fx):
    """Matching statistics of the spliced query, raw and through the index: len, the interval and src -- moved back by
    pad_len and the block shift -- are accepted by the serial checker against S and S's oracle table."""
    fn = fx.checker("ms_check", _match.build_checker)
    q = splice_query(fx)
    dq = torch.from_numpy(q).to(fx.text.device)
    ix = sdev.DeviceIndex(fx.text, fx.sa, engine=eng)
    try:
        for what, run in (("match_stats", lambda: sdev.match_stats(fx.text, fx.sa, dq, want_src=True, want_interval=True, engine=eng)),
                          ("DeviceIndex.match_stats", lambda: ix.match_stats(dq, want_src=True, want_interval=True))):
            got = run()
            _sync(device)
            ln, src, st, en = (H(x) for x in got)
            assert (ln >= 1).all(), what                              # (every query byte is a tail byte)
            assert (src.astype(np.int64) >= fx.pad_len).all() and (src.astype(np.int64) + ln <= fx.n).all(), (what, "src")
            first_hi = q >= 0xFE
            st_s = np.where(first_hi, st.astype(np.int64) - fx.shift, st.astype(np.int64))
            en_s = np.where(first_hi, en.astype(np.int64) - fx.shift, en.astype(np.int64))
            assert (st_s >= 0).all() and (en_s <= fx.s).all() and (st_s < en_s).all(), (what, "interval outside its block")
            _match.accept(fn, fx.t["bytes"], fx.t["sa"], q.tobytes(), 0,
                          (ln, (src.astype(np.int64) - fx.pad_len).astype(np.uint32), st_s.astype(np.uint32), en_s.astype(np.uint32)))
    finally:
        _sync(device)
        ix.close()
    fx.release()


def check_mems(eng, device, fx, min_len=24):
    """MEMs of the spliced query, raw and through the index: with tpos - pad_len the list is S's -- accepted by the serial
    checker and complete by the identities of _mem.verify, whose pair counts come from matching statistics over S alone
    that tests/ms_check.c accepted."""
    chk = fx.checker("mem_check", _mem.build_checker)
    q = splice_query(fx)
    dq = torch.from_numpy(q).to(fx.text.device)
    ix = sdev.DeviceIndex(fx.text, fx.sa, engine=eng)
    try:
        lists = []
        for what, run in (("mems", lambda: sdev.mems(fx.text, fx.sa, dq, min_len, engine=eng)), ("DeviceIndex.mems", lambda: ix.mems(dq, min_len))):
            qpos, tpos, ln, pairs = run()
            _sync(device)
            tp = H(tpos).astype(np.int64)
            assert (tp >= fx.pad_len).all() and (tp + H(ln) <= fx.n).all(), (what, "tpos")
            lists.append((H(qpos), (tp - fx.pad_len).astype(np.uint32), H(ln), pairs))
    finally:
        _sync(device)
        ix.close()
    fx.release()
    assert lists[0][0].size >= 20
    assert all(np.array_equal(lists[0][k], lists[1][k]) for k in range(3)) and lists[0][3] == lists[1][3]
    sdevice = "cuda" if fx.cuda else "cpu"
    _mem.verify(eng, sdevice, chk, fx.t["bytes"], fx.t["sa"], q.tobytes(), min_len, lists[0])


def hamming_patterns(fx, count=256, seed=13):
    """16 to 64 bytes each: three quarters cut from the tail with up to 3 bytes changed, a quarter straddling pad_len with
    at least 8 tail bytes (so that no window inside the padding alone can come within 3 mismatches)."""
    rng = np.random.default_rng(seed)
    pats = []
    for j in range(count):
        m = int(rng.integers(16, 65))
        if j % 4 == 3:
            p = WIN - int(rng.integers(1, m - 7))
        else:
            p = WIN + (int(rng.integers(0, fx.s - m + 1)) if j % 8 else fx.s - m)
        pat = fx.win[p:p + m].copy()
        for _ in range(int(rng.integers(0, 4))):
            x = int(rng.integers(0, m))
            if pat[x] < 0x41 or pat[x] > 0x54:
                pat[x] = ALPHABET[rng.integers(0, 4)]
        pats.append(pat.tobytes())
    return pats


def hamming_brute(win, patterns, k):
    """{(pattern, window start in win, mismatches)} by comparing every window."""
    out = set()
    for j, pat in enumerate(patterns):
        p = np.frombuffer(pat, dtype=np.uint8)
        mism = (np.lib.stride_tricks.sliding_window_view(win, p.size) != p).sum(axis=1)
        out.update((j, int(w), int(mism[w])) for w in np.flatnonzero(mism <= k))
    return out


def check_hamming(eng, device, fx, ks=(0, 1, 3)):
    """k-mismatch search, raw and through the index, against the brute force over the last s + 256 bytes: windows that
    start in the padding and end in the tail count.  (A window further left lies in the padding alone and differs in
    every tail byte of the pattern: at least 8.)"""
    pats = hamming_patterns(fx)
    qb, qo = pack(pats, fx.text.device)
    ix = sdev.DeviceIndex(fx.text, fx.sa, engine=eng)
    try:
        for k in ks:
            want = {(j, w + fx.win_base, c) for j, w, c in hamming_brute(fx.win, pats, k)}
            assert len(want) >= len(pats) // 2
            for what, run in (("hamming", lambda: sdev.hamming(fx.text, fx.sa, qb, qo, k, engine=eng)), ("DeviceIndex.hamming", lambda: ix.hamming(qb, qo, k))):
                first, pat, tpos, mism, _ = run()
                _sync(device)
                got = list(zip(H(pat).tolist(), H(tpos).tolist(), mism.cpu().numpy().tolist()))
                assert len(set(got)) == len(got), (what, k, "a window twice")
                assert set(got) == want, (what, k, sorted(set(got) ^ want)[:4])
                cnt = np.bincount([g[0] for g in got], minlength=len(pats))
                assert np.array_equal(np.diff(first.cpu().numpy()), cnt), (what, k, "first")
    finally:
        _sync(device)
        ix.close()
    fx.release()


def check_bwt_fm(eng, device, fx):
    """bwt on both blocks against the definition, the samples against the inverse table, unbwt(bwt(T)) == T; the FM index:
    count and locate of the search patterns, sa_range over the high block, lookup of 4096 ranks at the top."""
    n, a, b, S = fx.n, fx.a, fx.b, fx.t["S"]
    isa = inverse(fx)
    fx.require(n + int(eng.lib.sfx_unbwt_workspace_bytes(n)) + n, "bwt + unbwt")
    L, samples = sdev.bwt(fx.text, fx.sa, BWT_STEP, engine=eng)
    _sync(device)
    sa_s = fx.t["sa"].astype(np.int64)
    before = fx.win[WIN - 1 + sa_s]                                   # T[pad_len + SA_S[r] - 1]: the last padding byte for SA_S[r] == 0
    # row 0 is the text's last byte; the suffix at position 0 lies in the padding's block, so rank r sits in row r + 1 below it and row r above
    assert int(L[0]) == int(S[-1])
    assert np.array_equal(L[1:a + 1].cpu().numpy(), before[:a]), "bwt, low block"
    assert np.array_equal(L[n - b:].cpu().numpy(), before[a:]), "bwt, high block"
    assert torch.equal(U(samples), U(isa[::BWT_STEP]) + 1), "samples"
    back = sdev.unbwt(L, samples, BWT_STEP, engine=eng)
    _sync(device)
    assert torch.equal(back, fx.text), "unbwt(bwt(T)) != T"
    del back
    fx.release()
    fm = sdev.FmDeviceIndex(L, samples, BWT_STEP, engine=eng)
    del L, samples
    try:
        cases = _boundary_ranks(fx, search_cases(fx))
        qb, qo = pack([c[0] for c in cases], fx.text.device)
        st, en = fm.count(qb, qo)
        _sync(device)
        _check_intervals(fx, cases, U(st), U(en), "FmDeviceIndex.count")
        off, pos = fm.locate(qb, qo)
        _sync(device)
        want = np.concatenate([c[3] for c in cases])
        assert np.array_equal(np.diff(off.cpu().numpy()), [c[3].size for c in cases]), "locate offsets"
        assert np.array_equal(H(pos).astype(np.int64), want), "locate positions"
        assert (H(pos).astype(np.int64) >= fx.pad_len - 32).all()
        got = fm.sa_range(n - b, b)
        _sync(device)
        assert np.array_equal(H(got), expected_blocks(fx.orc, fx.pad_len)[1]), "sa_range over the high block"
        lo = 1 << 31 if n > (1 << 31) + 4096 else n - b - 1000        # explicit ranks >= 2^31 where there are any
        g = torch.Generator()
        g.manual_seed(3)
        ranks = torch.cat((torch.randint(lo, n, (1024,), generator=g), torch.randint(n - b, n, (3068,), generator=g),
                           torch.tensor([lo, n - b - 1, n - b, n - 1]))).to(fx.sa.device)
        got = fm.lookup(ranks.to(torch.int32))
        _sync(device)
        assert torch.equal(U(got), U(fx.sa[ranks])), "lookup"
        inside = (ranks >= n - b).cpu().numpy()
        assert inside.sum() >= 2000
        assert np.array_equal(H(got)[inside], expected_blocks(fx.orc, fx.pad_len)[1][(ranks.cpu().numpy() - (n - b))[inside]])
    finally:
        _sync(device)
        fm.close()
    fx.release()


def check_lce(eng, device, fx, ks=(0, 1, 5)):
    """2^16 pairs inside the tail against S and 4096 pairs with one side in the last 256 padding bytes against the last
    s + 256 bytes, both through the serial checker tests/lce_check.c (plain byte comparison; both suffixes run to the end
    of the text, as in T); range minima inside each block and across [n - b - 5, n); ranks of tail positions."""
    chk = fx.checker("lce_check", _lce.build_checker)
    n, a, b, s = fx.n, fx.a, fx.b, fx.s
    rng = np.random.default_rng(17)
    sa_s, lcp_s = fx.t["sa"].astype(np.int64), fx.t["lcp"]
    q = 1 << 14
    r = rng.integers(0, s - 40, q)
    pa = np.concatenate((rng.integers(0, s, q), sa_s[r], rng.integers(0, s, q), rng.integers(0, s, q)))
    pb = np.concatenate((rng.integers(0, s, q), sa_s[r + rng.integers(1, 40, q)], np.minimum(pa[2 * q:3 * q] + rng.integers(0, 64, q), s - 1),
                         rng.integers(s - 300, s, q)))
    pb[:8], pa[:8] = [s - 1, s - 1, 0, s - 1, 0, 1, s - 2, 0], [s - 1, 0, s - 1, s - 2, 0, 0, s - 1, 1]
    wa = np.concatenate((rng.integers(0, WIN, 4096 - 2), [0, WIN - 1]))
    wb = rng.integers(0, WIN + s, 4096)
    wb[:1024] = rng.integers(0, WIN, 1024)
    swap = rng.random(4096) < 0.5
    wa, wb = np.where(swap, wb, wa), np.where(swap, wa, wb)
    fx.require(int(eng.lib.sfx_lce_bytes(n)) + (4 << 20), "LceDeviceIndex")
    ix = sdev.LceDeviceIndex(fx.sa, fx.lcp, engine=eng)
    try:
        da, db = I32(pa + fx.pad_len, fx.sa.device), I32(pb + fx.pad_len, fx.sa.device)
        dwa, dwb = I32(wa + fx.win_base, fx.sa.device), I32(wb + fx.win_base, fx.sa.device)
        for k in ks:
            got = ix.lce(da, db, mismatches=k)
            gotw = ix.lce(dwa, dwb, mismatches=k)
            _sync(device)
            _lce.accept_pairs(chk, fx.t["bytes"], None, pa, pb, k, H(got))
            _lce.accept_pairs(chk, fx.win.tobytes(), None, wa, wb, k, H(gotw))
        edge = ix.lce(I32([n - 1, n, n, n - 1], fx.sa.device), I32([n - 1, n - 1, n, 0], fx.sa.device), mismatches=2)
        _sync(device)
        assert H(edge).tolist() == [1, 0, 0, 1], H(edge).tolist()     # (one byte of room, whatever the budget)
        # range minima: [lo, hi) inside the low block (boundaries 1 .. a - 1 are S's), inside the high one, and across its first boundary
        m = 2048
        lo1 = rng.integers(1, a - 1, m)
        hi1 = np.minimum(lo1 + 1 + (rng.integers(0, a, m) >> rng.integers(0, 15, m)), a)
        lo2 = rng.integers(a + 1, s - 1, m)
        hi2 = np.minimum(lo2 + 1 + (rng.integers(0, b, m) >> rng.integers(0, 15, m)), s)
        want = [int(lcp_s[l:h].min()) for l, h in zip(lo1, hi1)] + [int(lcp_s[l:h].min()) for l, h in zip(lo2, hi2)]
        lo = np.concatenate((lo1, lo2 + fx.shift, [n - b - 5, n - b, n - b + 1, 0, a, n - 1, n - 1]))
        hi = np.concatenate((hi1, hi2 + fx.shift, [n, n, n, a + 1, a + 1, n, n - 1]))
        want += [0, 0, int(lcp_s[a + 1:].min()), 0, 0, int(lcp_s[-1]), NONE]
        got = ix.range_min(I32(lo, fx.sa.device), I32(hi, fx.sa.device))
        _sync(device)
        bad = np.flatnonzero(H(got) != np.array(want, dtype=np.uint32))
        assert bad.size == 0, [(int(lo[x]), int(hi[x]), int(H(got)[x]), want[x]) for x in bad[:4]]
        pos = rng.integers(0, s, 4096)
        got = ix.rank_of(I32(np.concatenate((pos + fx.pad_len, [n - 1, n])), fx.sa.device))
        _sync(device)
        wantr = np.concatenate((fx.rank_T(fx.t["isa"][pos]), fx.rank_T(fx.t["isa"][-1:]), [NONE]))
        assert np.array_equal(H(got).astype(np.int64), wantr), "rank_of"
    finally:
        _sync(device)
        ix.close()
    fx.release()


def _check_sources(fx, rep, src, earlier):
    """At tail positions: every src is a tail position other than (earlier: in front of) its own and shares rep bytes."""
    S = fx.t["S"]
    src = src.astype(np.int64)
    zero = rep == 0
    assert (src[zero] == NONE).all() and (src[~zero] >= fx.pad_len).all() and (src[~zero] < fx.n).all(), "src"
    p = np.flatnonzero(~zero)
    q = src[p] - fx.pad_len
    assert (q < p).all() if earlier else (q != p).all(), "src: not allowed by the scope"
    assert (q + rep[p] <= fx.s).all(), "src: past the end"
    long_ = rep[p] > 64
    for pi, qi, k in zip(p[long_].tolist(), q[long_].tolist(), rep[p][long_].tolist()):
        assert S[pi:pi + k].tobytes() == S[qi:qi + k].tobytes(), ("witness", pi, qi, k)
    ps, qs, ks = p[~long_], q[~long_], rep[p][~long_].astype(np.int64)
    w = np.arange(64)
    same = S[np.minimum(ps[:, None] + w, fx.s - 1)] == S[np.minimum(qs[:, None] + w, fx.s - 1)]
    assert (same | (w >= ks[:, None])).all(), "witness"


def repeat_arrays(fx, scope):
    key = "rep_" + scope
    if getattr(fx, key, None) is None:
        fx.require(int(fx.eng.lib.sfx_repeat_lens_workspace_bytes(fx.n, sdev.REP_SCOPES[scope])) + 8 * fx.n, f"repeat_lens {scope}")
        got = sdev.repeat_lens(fx.sa, fx.lcp, scope, want_src=True, engine=fx.eng)
        _sync(fx.device)
        fx.release()
        setattr(fx, key, got)
    return getattr(fx, key)


def check_repeats(eng, device, fx):
    """repeat_lens "any" and "earlier" with src: at tail positions S's -- max(lcp[r], lcp[r + 1]) of the oracle's arrays and
    the LPF array of the oracle's arrays (lpf_from_tables) --, every src valid and >= pad_len."""
    lcp_s, isa_s = fx.t["lcp"].astype(np.int64), fx.t["isa"].astype(np.int64)
    nxt = np.concatenate((lcp_s[1:], [0]))
    want = {"any": np.maximum(lcp_s, nxt)[isa_s], "earlier": tail_lpf(fx.orc).astype(np.int64)}
    for scope in ("any", "earlier"):
        rep, src = repeat_arrays(fx, scope)
        r, q = H(rep[fx.pad_len:]).astype(np.int64), H(src[fx.pad_len:])
        bad = np.flatnonzero(r != want[scope])
        assert bad.size == 0, (scope, [(int(x), int(r[x]), int(want[scope][x])) for x in bad[:4]])
        _check_sources(fx, r, q, scope == "earlier")
        if scope == "any":
            fx.rep_any = None                                        # (only "earlier" is used again: by check_lz)
            fx.release()


def check_lz(eng, device, fx):
    """lz_parse from the "earlier" arrays: a phrase begins exactly at pad_len; from there (len, lit) are S's parse by the
    definition, each copy's src a valid earlier source >= pad_len; lz_decode of the whole parse is T."""
    n, S = fx.n, fx.t["S"]
    rep, src = repeat_arrays(fx, "earlier")
    fx.require(int(eng.lib.sfx_lz_parse_workspace_bytes(n)) + 13 * n + (n >> 1), "lz_parse")
    begin, ln, psrc, lit = sdev.lz_parse(rep, src, text=fx.text, engine=eng)
    _sync(device)
    fx.rep_earlier = None
    del rep, src
    fx.release()
    z = ln.numel()
    wb, wl, wc = _lz.reference(tail_lpf(fx.orc), 1)
    zt = len(wb)
    assert z > zt and int(U(begin[z - zt:z - zt + 1])[0]) == fx.pad_len, "no phrase begins at pad_len"
    if z > zt + 1:
        assert int(U(begin[z - zt - 1:z - zt])[0]) < fx.pad_len
    assert np.array_equal(H(begin[z - zt:]).astype(np.int64), np.array(wb) + fx.pad_len), "phrase starts"
    assert np.array_equal(H(ln[z - zt:]), np.array(wl, dtype=np.uint32)), "phrase lengths"
    got_src, got_lit = H(psrc[z - zt:]).astype(np.int64), lit[z - zt:].cpu().numpy()
    copy = np.array(wc)
    wlit = np.where(copy, 0, S[np.array(wb)])
    assert np.array_equal(got_lit, wlit), "literals"
    assert (got_src[~copy] == NONE).all()
    for bb, l, q in zip(np.array(wb)[copy].tolist(), np.array(wl)[copy].tolist(), (got_src[copy] - fx.pad_len).tolist()):
        assert 0 <= q < bb and S[q:q + l].tobytes() == S[bb:bb + l].tobytes(), ("copy", bb, l, q)
    # the phrases tile the text: begin[k + 1] == begin[k] + len[k]
    assert int(U(begin[:1])[0]) == 0 and torch.equal(U(begin[1:]), U(begin[:-1]) + U(ln[:-1])), "the phrases do not tile the text"
    del begin
    fx.require(int(eng.lib.sfx_lz_decode_workspace_bytes(n, z)) + n, "lz_decode")
    out = sdev.lz_decode(ln, psrc, lit, n=n, engine=eng)
    _sync(device)
    assert torch.equal(out, fx.text), "lz_decode(lz_parse(T)) != T"
    del out, ln, psrc, lit
    fx.release()


def tail_intervals(lcp):
    """lb / rb of every boundary of S by two stack sweeps: the nearest boundary with a smaller value on either side
    (boundary 0 and boundary s count as 0)."""
    n = len(lcp)
    v = [int(x) for x in lcp]
    v[0] = 0
    lb, rb = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    st = []
    for p in range(n):
        while st and v[st[-1]] >= v[p]:
            st.pop()
        lb[p] = st[-1] if st else 0
        st.append(p)
    st = []
    for p in range(n - 1, -1, -1):
        while st and v[st[-1]] >= v[p]:
            st.pop()
        rb[p] = (st[-1] if st else n) - 1
        st.append(p)
    return lb, rb


def check_intervals(eng, device, fx):
    """lb / rb of every boundary inside a block with lcp >= 1 are S's, shifted."""
    n, a, b = fx.n, fx.a, fx.b
    fx.require(int(eng.lib.sfx_lcp_intervals_workspace_bytes(n)) + 20 * n, "lcp_intervals")
    out = sdev.lcp_intervals(fx.lcp, engine=eng)
    _sync(device)
    lb, rb = tail_intervals(fx.t["lcp"])
    deep = fx.t["lcp"] >= 1
    for name, want in (("lb", lb), ("rb", rb)):
        got = np.concatenate((H(out[name][:a]), H(out[name][n - b:]))).astype(np.int64)
        bad = np.flatnonzero((got != fx.rank_T(want)) & deep)
        assert bad.size == 0, (name, [(int(x), int(got[x]), int(fx.rank_T(want[x]))) for x in bad[:4]])
    assert deep.sum() > fx.s // 2
    del out
    fx.release()


TAIL_CUTS = (0, 4099, 13000, 20500, 34000, 36300, 50000)   # 7 documents of unequal length: inside a planted block and both runs


def check_collection(eng, device, fx):
    """The padding as document 0, then the tail as 7 documents, so every tail doc_start lies around pad_len.  The tail's
    blocks of build_gsa -- positions less pad_len, document ids less 1 -- are a generalized table of the 7 documents
    alone, accepted by the serial checker tests/gsa_check.c against S; on that table rest doc_lookup, the generalized
    index's query / match_stats / mems / hamming, the LCE index with doc_starts and repeat_lens "other_doc", each against
    brute force or its own serial checker over S."""
    n, a, b, s, pad, dev = fx.n, fx.a, fx.b, fx.s, fx.pad_len, fx.text.device
    S, Sb = fx.t["S"], fx.t["bytes"]
    cuts = np.array(TAIL_CUTS, dtype=np.int64)
    starts_T = np.concatenate(([0], cuts + pad)).astype(np.int64)
    ds = torch.from_numpy(starts_T).to(dev)
    fx.require(int(eng.lib.sfx_gsa_workspace_bytes(n, starts_T.size)) + 12 * n, "build_gsa")
    ws = sdev.gsa_workspace(n, starts_T.size, dev, eng)
    gsa, gda, glcp = sdev.build_gsa(fx.text, ds, workspace=ws, engine=eng)
    _sync(device)
    del ws
    fx.release()
    blk = lambda t: np.concatenate((H(t[:a]), H(t[n - b:])))
    sa_s, da_s, lcp_s = blk(gsa).astype(np.int64) - pad, blk(gda).astype(np.int64) - 1, blk(glcp)
    lcp_s[0] = 0
    assert (sa_s >= 0).all() and (sa_s < s).all() and (da_s >= 0).all() and int(U(glcp[a:a + 1])[0]) == 0
    assert bool((gda[a:n - b] == 0).all()), "the padding's block holds another document"
    sa_s, da_s = sa_s.astype(np.uint32), da_s.astype(np.uint32)
    verdict = _gsa.run_checker(fx.checker("gsa_check", _gsa.build_checker), fx.tmp, Sb, cuts, sa_s, da_s, lcp_s)
    assert verdict.startswith("ok"), verdict
    doc_of = lambda p: np.searchsorted(cuts, p, side="right") - 1
    rng = np.random.default_rng(19)
    # doc_lookup
    pos = np.concatenate((rng.integers(0, s, 4096) + pad, cuts + pad, cuts[1:] + pad - 1, [pad - 1, 0, n - 1]))
    d, o = sdev.doc_lookup(I32(pos, dev), ds, engine=eng)
    _sync(device)
    wd = np.searchsorted(starts_T, pos, side="right") - 1
    assert np.array_equal(H(d).astype(np.int64), wd) and np.array_equal(H(o).astype(np.int64), pos - starts_T[wd]), "doc_lookup"
    gx = sdev.GeneralizedDeviceIndex(fx.text, ds, gsa, gda, engine=eng)
    try:
        # query: occurrences inside one document, by brute force
        pats, want = [], []
        for j in range(256):
            m = int(rng.integers(6, 33))
            p = int(cuts[1 + j % 6]) - int(rng.integers(0, m + 1)) if j % 4 == 0 else int(rng.integers(0, s - m + 1))   # (a quarter at a cut)
            pat = Sb[p:p + m] if j % 16 != 1 else ALPHABET[rng.integers(0, 4, 24)].tobytes()
            occ = _occ(S, pat)
            pats.append(pat)
            want.append(occ[doc_of(occ) == doc_of(occ + len(pat) - 1)])
        qb, qo = pack(pats, dev)
        st, en, found, anyp, ndocs = gx.query(qb, qo)
        _sync(device)
        st, en = U(st).cpu().numpy(), U(en).cpu().numpy()
        for j, w in enumerate(want):
            got = U(gsa[int(st[j]):int(en[j])]).cpu().numpy() - pad
            assert sorted(got.tolist()) == w.tolist(), ("gindex query", j, pats[j])
            assert bool(found[j]) == bool(w.size) and int(H(ndocs)[j]) == np.unique(doc_of(w)).size, ("gindex query", j)
            ap = int(H(anyp)[j])
            assert (ap - pad in w.tolist()) if w.size else ap == NONE, ("gindex any", j)
            if w.size:
                d, o = sdev.doc_lookup(gsa[int(st[j]):int(en[j])], ds, engine=eng)
                assert np.array_equal(H(d).astype(np.int64), doc_of(got) + 1) and np.array_equal(H(o).astype(np.int64), got - cuts[doc_of(got)])
        assert sum(w.size > 0 for w in want) >= 128
        # matching statistics and MEMs: S's, by the serial checkers over the accepted table
        q = splice_query(fx)
        dq = torch.from_numpy(q).to(dev)
        ln, src, st, en = (H(x) for x in gx.match_stats(dq, want_src=True, want_interval=True))
        hi_first = q >= 0xFE
        assert (ln >= 1).all() and (src.astype(np.int64) >= pad).all()
        st_s, en_s = (np.where(hi_first, x.astype(np.int64) - fx.shift, x.astype(np.int64)) for x in (st, en))
        assert (st_s >= 0).all() and (en_s <= s).all()
        _match.accept(fx.checker("ms_check", _match.build_checker), Sb, sa_s, q.tobytes(), 0,
                      (ln, (src.astype(np.int64) - pad).astype(np.uint32), st_s.astype(np.uint32), en_s.astype(np.uint32)), starts=cuts)
        qpos, tpos, mlen, pairs = gx.mems(dq, 24)
        _sync(device)
        tp = H(tpos).astype(np.int64)
        assert (tp >= pad).all() and qpos.numel() >= 20
        _mem.verify(eng, "cuda" if fx.cuda else "cpu", fx.checker("mem_check", _mem.build_checker), Sb, sa_s, q.tobytes(), 24,
                    (H(qpos), (tp - pad).astype(np.uint32), H(mlen), pairs), starts=cuts, da=da_s)
        # k-mismatch windows inside one document (none crosses pad_len: that is a document end)
        hp = hamming_patterns(fx)
        qb, qo = pack(hp, dev)
        wstarts = np.concatenate(([0], cuts + WIN))
        wdoc = lambda p: np.searchsorted(wstarts, p, side="right") - 1
        for k in (0, 1, 3):
            want = {(j, w + fx.win_base, c) for j, w, c in hamming_brute(fx.win, hp, k) if wdoc(w) == wdoc(w + len(hp[j]) - 1)}
            first, pat, tpos, mism, _ = gx.hamming(qb, qo, k)
            _sync(device)
            got = list(zip(H(pat).tolist(), H(tpos).tolist(), mism.cpu().numpy().tolist()))
            assert len(set(got)) == len(got) and set(got) == want, ("gindex hamming", k, sorted(set(got) ^ want)[:4])
    finally:
        _sync(device)
        gx.close()
    # the LCE index with doc_starts never passes a document end
    q4 = 1 << 12
    psa = fx.t["sa"].astype(np.int64)
    r = rng.integers(0, s - 1, q4)
    pa = np.concatenate((rng.integers(0, s, q4), psa[r], cuts[rng.integers(1, 7, q4)] - rng.integers(1, 40, q4), rng.integers(0, s, q4)))
    pb = np.concatenate((rng.integers(0, s, q4), psa[r + 1], rng.integers(0, s, q4), pa[3 * q4:]))
    chk = fx.checker("lce_check", _lce.build_checker)
    fx.require(int(eng.lib.sfx_lce_bytes(n)) + (4 << 20), "LceDeviceIndex")
    ix = sdev.LceDeviceIndex(gsa, glcp, doc_starts=ds, engine=eng)
    try:
        for k in (0, 1, 5):
            got = ix.lce(I32(pa + pad, dev), I32(pb + pad, dev), mismatches=k)
            _sync(device)
            _lce.accept_pairs(chk, Sb, cuts.astype(np.uint64), pa, pb, k, H(got))
    finally:
        _sync(device)
        ix.close()
    fx.release()
    # repeat_lens "other_doc": the padding shares no byte with the tail, so a tail position's answer is S's collection's
    fx.require(int(eng.lib.sfx_repeat_lens_workspace_bytes(n, sdev.REP_SCOPES["other_doc"])) + 8 * n, "repeat_lens other_doc")
    rep, src = sdev.repeat_lens(gsa, glcp, "other_doc", da=gda, want_src=True, engine=eng)
    _sync(device)
    rep_s, src_s = H(rep[pad:]), H(src[pad:]).astype(np.int64)
    assert (src_s[rep_s > 0] >= pad).all() and (src_s[rep_s == 0] == NONE).all() and int(rep_s.max()) >= 1024
    src_s = np.where(src_s == NONE, NONE, src_s - pad).astype(np.uint32)
    verdict = _repeats.run_checker(fx.checker("rep_check", _repeats.build_checker), fx.tmp, Sb, cuts, sa_s, lcp_s, da_s, "other_doc", rep_s, src_s)
    assert verdict.startswith("ok"), verdict
    del rep, src, gsa, gda, glcp
    fx.release()


def check_host(eng, device, fx):
    """SuffixTable and FmIndex on host bytes: what reaches Python at tail positions is non-negative and correct."""
    n, a, b, s, pad = fx.n, fx.a, fx.b, fx.s, fx.pad_len
    S, Sb = fx.t["S"], fx.t["bytes"]
    sa_lo, sa_hi, lcp_lo, lcp_hi = expected_blocks(fx.orc, pad)
    st = SuffixTable(fx.text.cpu().numpy().tobytes(), engine=eng)
    tab = st.table()
    assert tab.dtype == np.uint32 and np.array_equal(tab[:a], sa_lo) and np.array_equal(tab[n - b:], sa_hi), "table()"
    lcp = st.lcp_lens()
    assert lcp.dtype == np.uint32 and np.array_equal(lcp[1:a + 1], lcp_lo[1:]) and np.array_equal(lcp[n - b:], lcp_hi), "lcp_lens()"
    del lcp
    isa = st.inverse_table()
    assert isa.dtype == np.uint32 and np.array_equal(isa[pad:].astype(np.int64), fx.rank_T(fx.t["isa"])), "inverse_table()"
    cases = search_cases(fx)
    cases = [(pat, lo if lo is not None else int(isa[int(pos[0])]), hi if hi is not None else int(isa[int(pos[0])]) + 1, pos, there)
             for pat, lo, hi, pos, there in cases]
    del isa
    start, end = st.positions_batch([c[0] for c in cases])
    found, anyp = st.contains_batch([c[0] for c in cases])
    assert start.dtype == end.dtype == anyp.dtype == np.uint32
    for k, (pat, lo, hi, pos, there) in enumerate(cases):
        assert (int(start[k]), int(end[k])) == (lo, hi), ("positions_batch", k)
        assert bool(found[k]) == there and ((int(anyp[k]) in pos.tolist()) if there else int(anyp[k]) == NONE), ("contains_batch", k)
    for pat, lo, hi, pos, there in cases[::37] + cases[512:520] + cases[-3:]:
        got = st.positions(pat)
        assert np.array_equal(np.asarray(got).astype(np.int64), pos) and all(int(x) >= 0 for x in got), ("positions", pat[:16])
        ap = st.any_position(pat)
        assert (ap is None) if not there else (ap >= 0 and ap in pos.tolist()), ("any_position", pat[:16], ap)
        assert st.contains(pat) == there
    rng = np.random.default_rng(23)
    for _ in range(12):
        i, j, k = int(rng.integers(0, s)), int(rng.integers(0, s)), int(rng.integers(0, 3))
        got = st.lce(pad + i, pad + j, k)
        assert got == _lce.brute(Sb, i, j, k) and got >= 0, ("lce", i, j, k, got)
    assert st.lce(n - 1, n - 1) == 1 and st.lce(n, n - 1) == 0
    r = rng.integers(0, s - 1, 2048)
    pa, pb = fx.t["sa"].astype(np.int64)[r], fx.t["sa"].astype(np.int64)[r + 1]
    _lce.accept_pairs(fx.checker("lce_check", _lce.build_checker), Sb, None, pa, pb, 1, st.lce_batch(pa + pad, pb + pad, 1))
    assert st.lcp_range_min(n - b + 1, n) == int(fx.t["lcp"][a + 1:].min()) and st.lcp_range_min(n - b - 5, n) == 0
    fm = st.fm_index(64)
    try:
        assert fm.len() == n
        cs, ce = fm.count_batch([c[0] for c in cases])
        assert np.array_equal(cs, start) and np.array_equal(ce, end), "FmIndex.count_batch"
        for pat, lo, hi, pos, there in cases[::41] + cases[512:516]:
            got = fm.positions(pat)
            assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), pos), ("FmIndex.positions", pat[:16])
        ranks = np.concatenate((rng.integers(n - b, n, 1000), [n - b, n - 1, 0, a - 1]))
        assert np.array_equal(fm.lookup(ranks), tab[ranks]), "FmIndex.lookup"
        assert np.array_equal(fm.lookup(first=n - b, count=b), sa_hi)
    finally:
        fm.close()
    del st, tab
    fx.release()


CHECKS = {"builds": check_builds, "inverse": check_inverse, "search": check_search, "match_stats": check_match_stats, "mems": check_mems,
          "hamming": check_hamming, "bwt_fm": check_bwt_fm, "lce": check_lce, "repeats": check_repeats, "lz": check_lz,
          "intervals": check_intervals, "collection": check_collection, "host": check_host}
