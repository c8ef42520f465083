#!/usr/bin/env python3
"""Suffix-tree topology (sfx_lcp_intervals_dev) and node table (sfx_suffix_tree_dev) timed on the LCP array of a full-size
config (development).  usage: gpu_tree_time.py [n] [names ...]   names among english dna chain (default: all; the chain is
"a" x 2^24 whatever n is).  Per input: one untimed call, then warm calls with device events around the `_dev` call alone --
workspaces and outputs are allocated beforehand -- and one more call under the engine's profiler for the per-kernel split."""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import _gen, suffix_amd
import _devlib
from suffix_amd import device as sdev
eng = _devlib.engine(); eng.require_device()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000_000
names = sys.argv[2:] or ["english", "dna", "chain"]
REPS = 3
inputs = {"english": lambda: _gen.english_like(n), "dna": lambda: _gen.dna_fast(n, seed=0x5AF1C5 + 2),
          "chain": lambda: np.full(1 << 24, ord("a"), dtype=np.uint8)}


def timed(fn):
    """fn() once untimed, then REPS times between device events -> (best ms, all ms); then once under the profiler."""
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(round(a.elapsed_time(b), 2))
    eng.profile(True); eng.profile_reset()
    fn(); torch.cuda.synchronize()
    k = {r["name"]: round(r["total_ms"], 2) for r in eng.profile_report()}; eng.profile(False)
    return min(ms), ms, k


for name in names:
    host = inputs[name]()
    nn = int(host.size)
    text = torch.from_numpy(host).cuda()
    sa, lcp = sdev.build_sa_lcp(text)
    torch.cuda.synchronize()
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device="cuda")
    p, st = sdev._p, sdev._stream_ptr(text)
    # the topology alone, as the library stood before the node table
    topo = [i32(nn) for _ in range(5)]
    ws = torch.empty(int(eng.lib.sfx_lcp_intervals_workspace_bytes(nn)), dtype=torch.uint8, device="cuda")
    iv = lambda: eng.check(eng.lib.sfx_lcp_intervals_dev(p(lcp), nn, *[p(t) for t in topo], p(ws), ws.numel(), st), "intervals")
    iv_ms, iv_all, iv_k = timed(iv)
    nodes = int((topo[2] == torch.arange(nn, device="cuda", dtype=torch.int32)).sum())
    del topo, ws
    # the node table: a sizing call, then filling calls into arrays of exactly m and C entries
    tws = sdev.suffix_tree_workspace(nn, "cuda", eng)
    m, c = ctypes.c_uint64(0), ctypes.c_uint64(0)
    size = lambda: eng.check(eng.lib.sfx_suffix_tree_dev(None, p(sa), p(lcp), nn, 0, 0, *([None] * 10), ctypes.byref(m), ctypes.byref(c),
                                                         p(tws), tws.numel(), st), "sizing")
    size_ms, size_all, size_k = timed(size)
    nm, nc = int(m.value), int(c.value)
    out = [i32(nm) for _ in range(5)] + [torch.empty(nm + 1, dtype=torch.int64, device="cuda"), i32(nc), i32(nc),
                                         torch.empty(max(nc, 1), dtype=torch.uint8, device="cuda"), i32(nn)]
    fill = lambda: eng.check(eng.lib.sfx_suffix_tree_dev(p(text), p(sa), p(lcp), nn, nm, nc, *[p(t) for t in out], ctypes.byref(m),
                                                         ctypes.byref(c), p(tws), tws.numel(), st), "filling")
    fill_ms, fill_all, fill_k = timed(fill)
    terminals = int((out[4] != -1).sum())
    fan = out[5][1:] - out[5][:-1]
    print(json.dumps({"text": name, "n": nn, "commit": open(os.path.join(ROOT, "suffix_amd", "_build_commit.txt")).read().strip(),
                      "intervals_ms": iv_ms, "intervals_all": iv_all, "intervals_kernel_ms": iv_k, "internal_nodes": nodes,
                      "tree_sizing_ms": size_ms, "tree_sizing_all": size_all, "tree_sizing_kernel_ms": size_k,
                      "tree_fill_ms": fill_ms, "tree_fill_all": fill_all, "tree_fill_kernel_ms": fill_k,
                      "m": nm, "C": nc, "T": terminals, "max_fanout": int(fan.max()), "fanout_over_8": int((fan > 8).sum()),
                      "workspace_bytes": int(tws.numel()), "output_bytes": int(sum(t.numel() * t.element_size() for t in out)),
                      "peak_allocated_bytes": int(torch.cuda.max_memory_allocated()), "max_depth": int(lcp.max())}), flush=True)
    del text, sa, lcp, out, tws
    torch.cuda.empty_cache()
