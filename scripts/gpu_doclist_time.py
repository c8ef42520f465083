#!/usr/bin/env python3
"""Document listing (sfx_doclist_list_dev) timed on two collections, with the occ_cut sweep that sets the automatic route
threshold (development).  usage: gpu_doclist_time.py [n] [names ...]   names among english dna (default: both) --
  english   n bytes of English-like text in documents of about 10 KB
  dna       n bytes of DNA in documents of 256 bytes
the collections of gpu_docs_time.py.  Per input, in one process: sfx_build_gsa_u32_dev, the resident index, then
  patterns   2^16 patterns of 1 - 12 bytes sampled from the text, searched once (sfx_gindex_query_dev without ndocs);
  wide       256 intervals with e - s >= n / 4
and for each batch sfx_doclist_list_dev (BY_TF, top_k = 10; the workspace allocated beforehand) under occ_cut = 2^k for
k = 4 .. 34 and under the automatic value (32 ndocs): one untimed call, then warm calls between device events around the
`_dev` call alone (which includes its read-back), and one more call under the engine's profiler for the per-launch split.
For comparison the same pattern batch through sfx_gindex_query_dev WITH ndocs (the O(occurrences) count).  Writes
profiles/doclist_times.json.  A batch whose lists hold more than 2^32 - 1 entries is refused by the call after its
count phase: its record says so and its time is that of the count phase."""
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
        ms.append(round(a.elapsed_time(b), 3))
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
    sa, da, lcp = sdev.build_gsa(text, ds, engine=eng)
    del lcp
    gx = sdev.GeneralizedDeviceIndex(text, ds, sa, da, engine=eng)
    rng = np.random.default_rng(24)
    pos, ln = rng.integers(0, nn - 12, 1 << 16), rng.integers(1, 13, 1 << 16)
    qoff = np.zeros((1 << 16) + 1, dtype=np.int64)
    qoff[1:] = np.cumsum(ln)
    qb = torch.from_numpy(np.concatenate([host[p:p + k] for p, k in zip(pos, ln)])).cuda()
    dq = torch.from_numpy(qoff).cuda()
    query_ms, query_all, _ = timed(lambda: gx.query(qb, dq))             # with ndocs: the linear pass over PREV
    ps, pe, _, _, pnd = gx.query(qb, dq)
    wide_s = torch.from_numpy(rng.integers(0, nn // 2, 256).astype(np.int32)).cuda()
    wide_e = wide_s + torch.from_numpy(rng.integers(nn // 4, nn // 2, 256).astype(np.int32)).cuda()
    batches = {"patterns": (ps, pe), "wide": (wide_s, wide_e)}
    rec = {"collection": name, "n": nn, "ndocs": nd, "commit": open(os.path.join(ROOT, "suffix_amd", "_build_commit.txt")).read().strip(),
           "gindex_query_with_ndocs_ms": query_ms, "gindex_query_with_ndocs_all": query_all, "automatic_occ_cut": 32 * nd, "automatic_rule": "32 * ndocs", "sweep": []}
    for cutv in [1 << k for k in range(4, 35)] + [0]:
        dx = sdev.DocListDeviceIndex(da, ds, occ_cut=cutv, engine=eng)
        for bname, (s, e) in batches.items():
            limit = int(((e.to(torch.int64) & 0xFFFFFFFF) - (s.to(torch.int64) & 0xFFFFFFFF)).clamp(0, nd).sum().item())
            ws = dx.workspace(s.numel(), max(limit, 1))
            out = {}

            def call():
                try:
                    out["listed"] = dx.list(s, e, order="tf", top_k=10, list_limit=max(limit, 1), workspace=ws)[3]
                except suffix_amd.SuffixHipError:                        # more than 2^32 - 1 entries: refused after the count phase
                    out["listed"] = None
            ms, all_ms, k = timed(call)
            rec["sweep"].append({"occ_cut": cutv, "batch": bname, "ms": ms, "all": all_ms, "listed": out["listed"], "refused": out["listed"] is None,
                                 "launch_ms": {x: v for x, v in k.items() if x.startswith(("doclist_", "radix_", "gsa_scan"))}})
            del ws
        dx.close()
        torch.cuda.empty_cache()
        print(f"{name}: occ_cut {cutv} done", file=sys.stderr, flush=True)
    print(json.dumps(rec), flush=True)
    results.append(rec)
    gx.close()
    del text, ds, sa, da
    torch.cuda.empty_cache()
with open(os.path.join(ROOT, "profiles", "doclist_times.json"), "w") as fh:
    json.dump(results, fh, indent=1)
    fh.write("\n")
