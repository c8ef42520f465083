"""Shared pieces of the repeat-length / repeated-span tests (test_repeats_emu.py on the emulator, test_gpu_repeats.py on
the GPU): rep by the definition, a span reference that uses another method than the engine, witness validation, and the
serial checker tests/rep_check.c for large inputs."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SCOPES = {"any": 0, "earlier": 1, "other_doc": 2}
NONE = 0xFFFFFFFF


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data if a is not None and a.size else 0)


def _lcp(a, b):
    k, m = 0, min(len(a), len(b))
    while k < m and a[k] == b[k]:
        k += 1
    return k


def doc_of(starts, n):
    """Document of every text position (the last start <= p; empty documents own nothing)."""
    return np.searchsorted(np.asarray(starts, dtype=np.int64), np.arange(n), side="right") - 1


def truncated_suffixes(text, starts=None):
    """S_p for every p: to the end of the text, or of p's document."""
    n = len(text)
    if starts is None:
        return [text[p:] for p in range(n)]
    ends = np.append(np.asarray(starts, dtype=np.int64)[1:], n)
    d = doc_of(starts, n)
    return [text[p:int(ends[d[p]])] for p in range(n)]


def brute_rep(text, scope, starts=None):
    """rep by the definition: every pair compared (inputs of at most 80 bytes)."""
    n = len(text)
    assert n <= 80
    suf = truncated_suffixes(text, starts)
    d = doc_of(starts if starts is not None else [0], n)
    rep = np.zeros(n, dtype=np.uint32)
    for p in range(n):
        for q in range(n):
            ok = q != p if scope == "any" else q < p if scope == "earlier" else d[q] != d[p]
            if ok:
                rep[p] = max(rep[p], _lcp(suf[p], suf[q]))
    return rep


def span_reference(rep, min_len, starts=None):
    """Maximal runs of covered bytes by a difference array (+1 at p, -1 at p + rep[p] for qualifying p) and its
    cumulative sum -- not the engine's prefix maximum -- split at document starts.  -> [(begin, end)]."""
    rep = np.asarray(rep, dtype=np.int64)
    n = rep.size
    if n == 0:
        return []
    q = np.nonzero(rep >= min_len)[0]
    diff = np.bincount(q, minlength=n + 1) - np.bincount(np.minimum(q + rep[q], n), minlength=n + 1)
    cov = np.cumsum(diff[:n]) > 0
    cut = np.zeros(n, dtype=bool)
    if starts is not None:
        s = np.asarray(starts, dtype=np.int64)
        cut[s[s < n]] = True
    prev = np.concatenate(([False], cov[:-1]))
    nxt = np.concatenate((cov[1:], [False]))
    begin = np.nonzero(cov & (~prev | cut))[0]
    end = np.nonzero(cov & (~nxt | np.concatenate((cut[1:], [True]))))[0] + 1
    assert begin.size == end.size
    return list(zip(begin.tolist(), end.tolist()))


def check_witnesses(text, scope, rep, src, starts=None):
    """Every src[p] is allowed by the scope and shares rep[p] bytes with p (inside both documents); NONE iff rep[p] == 0."""
    n = len(text)
    suf = truncated_suffixes(text, starts)
    d = doc_of(starts if starts is not None else [0], n)
    for p in range(n):
        q, k = int(src[p]), int(rep[p])
        if k == 0:
            assert q == NONE, (p, q)
            continue
        assert q < n, (p, q)
        assert q != p if scope == "any" else q < p if scope == "earlier" else d[q] != d[p], (scope, p, q)
        assert len(suf[q]) >= k and suf[p][:k] == suf[q][:k], (scope, p, q, k)


class _Mem:
    """Arrays where the engine computes: the host's own memory for the emulator, HBM (through torch) for the product."""

    def __init__(self, eng):
        self.gpu = os.path.basename(eng.path) == "libsuffix_hip.so"
        if self.gpu:
            import torch
            self.torch = torch

    def put(self, a):
        """-> (handle, pointer) of a copy the engine may read and write; None stays NULL."""
        if a is None:
            return None, ctypes.c_void_p(0)
        a = np.ascontiguousarray(a)
        if not self.gpu:
            a = a.copy()
            return a, ptr(a)
        t = self.torch.from_numpy(a.view(np.uint8).copy()).cuda()
        return t, ctypes.c_void_p(t.data_ptr() if t.numel() else 0)

    def get(self, h, dtype):
        if not self.gpu:
            return h
        self.torch.cuda.synchronize()
        return h.cpu().numpy().view(dtype)


def repeat_lens(eng, sa, lcp, scope, da=None, want_src=True, expect=0):
    """sfx_repeat_lens_dev -> (rep, src) on the host."""
    mem = _Mem(eng)
    n = int(sa.size)
    (_a, p_sa), (_b, p_lcp), (_c, p_da) = mem.put(sa), mem.put(lcp), mem.put(da if scope == "other_doc" else None)
    h_rep, p_rep = mem.put(np.full(n, 0xDEADBEEF, dtype=np.uint32))
    h_src, p_src = mem.put(np.full(n, 0xDEADBEEF, dtype=np.uint32) if want_src else None)
    h_ws, p_ws = mem.put(np.zeros(int(eng.lib.sfx_repeat_lens_workspace_bytes(n, SCOPES[scope])) + 8, dtype=np.uint8))
    rc = eng.lib.sfx_repeat_lens_dev(p_sa, p_lcp, p_da, n, SCOPES[scope], p_rep, p_src, p_ws,
                                     int(eng.lib.sfx_repeat_lens_workspace_bytes(n, SCOPES[scope])), None)
    assert rc == expect, (rc, scope)
    return mem.get(h_rep, np.uint32), mem.get(h_src, np.uint32) if want_src else None


def repeat_spans(eng, rep, min_len, starts=None, capacity=None):
    """sfx_repeat_spans_dev -> ([(begin, end)] of the entries written, total count); everything behind the entries
    written, a canary behind the capacity included, must survive."""
    mem = _Mem(eng)
    n = int(rep.size)
    cap = n // min_len + 1 if capacity is None else capacity
    h_b, p_b = mem.put(np.full(cap + 1, 0xCAFEF00D, dtype=np.uint32))
    h_e, p_e = mem.put(np.full(cap + 1, 0xCAFEF00D, dtype=np.uint32))
    wsb = int(eng.lib.sfx_repeat_spans_workspace_bytes(n))
    h_ws, p_ws = mem.put(np.zeros(wsb + 8, dtype=np.uint8))
    s = None if starts is None else np.ascontiguousarray(starts, dtype=np.uint64)
    (_r, p_rep), (_s, p_s) = mem.put(rep), mem.put(s)
    count = ctypes.c_uint64(12345)
    rc = eng.lib.sfx_repeat_spans_dev(p_rep, n, min_len, p_s, 0 if s is None else s.size, p_b, p_e, cap, ctypes.byref(count),
                                      p_ws, wsb, None)
    assert rc == 0, rc
    begin, end = mem.get(h_b, np.uint32), mem.get(h_e, np.uint32)
    k = min(int(count.value), cap)
    assert (begin[k:] == 0xCAFEF00D).all() and (end[k:] == 0xCAFEF00D).all()
    return list(zip(begin[:k].tolist(), end[:k].tolist())), int(count.value)


MIN_LENS = (1, 2, 3, 1000)


def check_small(eng, text, sa, lcp, scopes, starts=None, da=None):
    """Inputs of at most 80 bytes: all of `scopes` against brute force, witnesses against the text, spans at MIN_LENS
    (with and without the document starts) against the reference."""
    for scope in scopes:
        rep, src = repeat_lens(eng, sa, lcp, scope, da=da)
        exp = brute_rep(text, scope, starts)
        assert np.array_equal(rep, exp), (scope, text, starts, rep.tolist(), exp.tolist())
        check_witnesses(text, scope, rep, src, starts)
        rep2, none = repeat_lens(eng, sa, lcp, scope, da=da, want_src=False)
        assert none is None and np.array_equal(rep2, rep)
        for m in MIN_LENS:
            for st in ((None,) if starts is None else (None, starts)):
                got, count = repeat_spans(eng, rep, m, st)
                assert got == span_reference(rep, m, st) and count == len(got), (scope, m, text, st)


def random_text(rng, max_len=60):
    alpha = bytes(rng.sample(range(256), rng.randint(2, 4)))
    return bytes(rng.choice(alpha) for _ in range(rng.randint(0, max_len)))


def build_checker(out_dir):
    """tests/rep_check.c -> an executable (the serial, engine-independent checker of large inputs)."""
    exe = os.path.join(str(out_dir), "rep_check")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-o", exe, os.path.join(HERE, "rep_check.c")])
    return exe


def write_inputs(out_dir, text, starts, sa, lcp, da):
    """The arrays an input shares between its scopes, as raw files -> their paths."""
    paths = []
    for name, arr in (("text", np.frombuffer(text, dtype=np.uint8) if isinstance(text, bytes) else text),
                      ("starts", np.asarray(starts, dtype=np.uint64)), ("sa", sa), ("lcp", lcp),
                      ("da", da if da is not None else np.zeros(0, dtype=np.uint32))):
        p = os.path.join(str(out_dir), name + ".bin")
        np.ascontiguousarray(arr).tofile(p)
        paths.append(p)
    return paths


def check_with(exe, inputs, out_dir, scope, rep, src):
    """Runs the checker on written inputs + (rep, src); returns its output line ("ok ..." or the fault)."""
    outs = []
    for name, arr in (("rep", rep), ("src", src)):
        p = os.path.join(str(out_dir), name + ".bin")
        np.ascontiguousarray(arr).tofile(p)
        outs.append(p)
    r = subprocess.run([exe, str(SCOPES[scope]), *inputs, *outs], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip()


def run_checker(exe, out_dir, text, starts, sa, lcp, da, scope, rep, src):
    return check_with(exe, write_inputs(out_dir, text, starts, sa, lcp, da), out_dir, scope, rep, src)
