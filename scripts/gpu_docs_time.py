#!/usr/bin/env python3
"""Document counts (sfx_doc_counts_dev) and k-common substrings (sfx_common_substrings_dev) timed on two collections
(development).  usage: gpu_docs_time.py [n] [names ...]   names among english dna (default: both) --
  english   n bytes of English-like text in documents of about 10 KB (DESIGN.md section 12's collection)
  dna       n bytes of DNA in documents of 256 bytes (the hot-address case: nearly every p(r) is a shallow boundary)
Per input, in one process: sfx_build_gsa_u32_dev on the collection, sfx_lcp_intervals_dev on its lcp, then the two new
calls -- one untimed call each, then warm calls between device events around the `_dev` call alone (workspaces and
outputs allocated beforehand), and one more call under the engine's profiler for the per-launch split.  Both new calls
end with a read-back, so their event time includes it.  Writes profiles/docs_times.json."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import _gen, suffix_amd
import _devlib
from suffix_amd import device as sdev
eng = _devlib.engine(); eng.require_device()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
names = sys.argv[2:] or ["english", "dna"]
REPS = 3


def english_starts(nn):
    rng = np.random.default_rng(12)
    s = np.concatenate(([0], np.cumsum(rng.integers(5000, 15001, nn // 5000 + 2))))
    return s[s < nn].astype(np.int64)


inputs = {"english": (lambda: _gen.english_like(n), english_starts),
          "dna": (lambda: _gen.dna_fast(n, seed=0x5AF1C5 + 2), lambda nn: np.arange(0, nn, 256, dtype=np.int64))}


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
    k = {r["name"]: round(r["total_ms"], 3) for r in eng.profile_report()}; eng.profile(False)
    return min(ms), ms, k


results = []
for name in names:
    make, cut = inputs[name]
    host = make()
    nn = int(host.size)
    starts = cut(nn)
    nd = int(starts.size)
    text, ds = torch.from_numpy(host).cuda(), torch.from_numpy(starts).cuda()
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device="cuda")
    p, st = sdev._p, sdev._stream_ptr(text)
    sa, da, lcp = i32(nn), i32(nn), i32(nn)
    gws = sdev.gsa_workspace(nn, nd, "cuda", eng)
    gsa_ms, gsa_all, _ = timed(lambda: eng.check(eng.lib.sfx_build_gsa_u32_dev(p(text), nn, p(ds), nd, p(sa), p(da), p(lcp), p(gws), gws.numel(), st), "gsa"))
    del gws
    topo = [i32(nn) for _ in range(5)]
    ws = torch.empty(int(eng.lib.sfx_lcp_intervals_workspace_bytes(nn)), dtype=torch.uint8, device="cuda")
    iv_ms, iv_all, _ = timed(lambda: eng.check(eng.lib.sfx_lcp_intervals_dev(p(lcp), nn, *[p(t) for t in topo], p(ws), ws.numel(), st), "intervals"))
    del topo, ws
    df, dup = i32(nn), i32(nn)
    ws = sdev.doc_counts_workspace(nn, "cuda", eng)
    dc_ms, dc_all, dc_k = timed(lambda: eng.check(eng.lib.sfx_doc_counts_dev(p(da), p(lcp), nn, nd, p(dup), p(df), p(ws), ws.numel(), st), "doc_counts"))
    pf_ms, pf_all, _ = timed(lambda: eng.check(eng.lib.sfx_doc_counts_dev(p(da), p(lcp), nn, nd, p(dup), None, p(ws), ws.numel(), st), "dup_prefix"))
    ws_bytes = int(ws.numel())
    del ws
    ln, pos = i32(nd), i32(nd)
    cws = torch.empty(int(eng.lib.sfx_common_substrings_workspace_bytes(nd)), dtype=torch.uint8, device="cuda")
    cs_ms, cs_all, cs_k = timed(lambda: eng.check(eng.lib.sfx_common_substrings_dev(p(sa), p(lcp), p(df), nn, p(ds), nd, p(ln), p(pos), p(cws), cws.numel(), st),
                                                  "common"))
    lens = ln.cpu().numpy().view(np.uint32)
    walkers = int((dc_k.get("docs_argmin", 0) > 0))
    rec = {"collection": name, "n": nn, "ndocs": nd, "commit": open(os.path.join(ROOT, "suffix_amd", "_build_commit.txt")).read().strip(),
           "build_gsa_ms": gsa_ms, "build_gsa_all": gsa_all, "lcp_intervals_ms": iv_ms, "lcp_intervals_all": iv_all,
           "doc_counts_ms": dc_ms, "doc_counts_all": dc_all, "doc_counts_launch_ms": dc_k, "dup_prefix_only_ms": pf_ms, "dup_prefix_only_all": pf_all,
           "argmin_G_ranks_per_s": round(nn / dc_k["docs_argmin"] / 1e6, 2) if walkers else None,
           "common_substrings_ms": cs_ms, "common_substrings_all": cs_all, "common_substrings_launch_ms": cs_k,
           "workspace_bytes": ws_bytes, "len_1": int(lens[0]), "len_2": int(lens[1]) if nd > 1 else None, "len_all": int(lens[-1]),
           "docs_sharing_32_bytes": int((lens >= 32).sum()), "peak_allocated_bytes": int(torch.cuda.max_memory_allocated())}
    print(json.dumps(rec), flush=True)
    results.append(rec)
    del text, ds, sa, da, lcp, df, dup, ln, pos, cws
    torch.cuda.empty_cache()
with open(os.path.join(ROOT, "profiles", "docs_times.json"), "w") as fh:
    json.dump(results, fh, indent=1)
    fh.write("\n")
