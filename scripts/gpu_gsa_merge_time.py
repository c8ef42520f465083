#!/usr/bin/env python3
"""The GSA merge (sfx_gsa_merge_dev) timed against the one-shot build on two collections (development).
usage: gpu_gsa_merge_time.py [n] [names ...]   names among english dna (default: both) --
  english   n bytes of English-like text in documents of about 10 KB (DESIGN.md section 12's collection)
  dna       n bytes of DNA in documents of 256 bytes
Per input and for B = the last 1 %, 6 % and 50 % of the documents, in one process: the one-shot sfx_build_gsa_u32_dev of
the whole collection, the build of A and of B alone, then -- after the merged arrays were found equal to the one-shot
ones -- one untimed call and the best of 3 between device events (workspaces and outputs allocated beforehand) of
  merge            sfx_gsa_merge_dev alone (its two read-backs included), match_limit 0
  build_b_merge    sfx_build_gsa_u32_dev of B + the merge: what adding the documents costs
  one_shot         sfx_build_gsa_u32_dev of the whole collection: what it cost before
and one merge under the engine's profiler for the per-launch split.  Writes profiles/gsa_merge_times.json."""
import ctypes, json, os, sys
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
SHARES = (0.01, 0.06, 0.50)


def english_starts(nn):
    rng = np.random.default_rng(12)
    s = np.concatenate(([0], np.cumsum(rng.integers(5000, 15001, nn // 5000 + 2))))
    return s[s < nn].astype(np.int64)


inputs = {"english": (lambda: _gen.english_like(n), english_starts),
          "dna": (lambda: _gen.dna_fast(n, seed=0x5AF1C5 + 2), lambda nn: np.arange(0, nn, 256, dtype=np.int64))}


def timed(fn, profile=False):
    """fn() once untimed, then REPS times between device events -> (best ms, all ms[, per-launch ms of one more call])."""
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(round(a.elapsed_time(b), 2))
    if not profile:
        return min(ms), ms
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
    whole = [i32(nn) for _ in range(3)]
    gws = sdev.gsa_workspace(nn, nd, "cuda", eng)
    one_ms, one_all = timed(lambda: eng.check(eng.lib.sfx_build_gsa_u32_dev(p(text), nn, p(ds), nd, *[p(x) for x in whole], p(gws), gws.numel(), st), "gsa"))
    for share in SHARES:
        k = nd - max(1, int(round(nd * share)))
        na = int(starts[k])
        nb = nn - na
        ta, tb, dsa, dsb = text[:na], text[na:], ds[:k].contiguous(), (ds[k:] - na).contiguous()
        A, B, out = [i32(na) for _ in range(3)], [i32(nb) for _ in range(3)], [i32(nn) for _ in range(3)]
        eng.check(eng.lib.sfx_build_gsa_u32_dev(p(ta), na, p(dsa), k, *[p(x) for x in A], p(gws), gws.numel(), st), "gsa A")
        build_b = lambda: eng.check(eng.lib.sfx_build_gsa_u32_dev(p(tb), nb, p(dsb), nd - k, *[p(x) for x in B], p(gws), gws.numel(), st), "gsa B")
        build_b()
        mws = sdev.gsa_merge_workspace(na, nb, "cuda", eng)
        longest = ctypes.c_uint64(0)
        merge = lambda: eng.check(eng.lib.sfx_gsa_merge_dev(p(text), p(ds), nd, k, p(A[0]), p(A[1]), p(A[2]), na, p(B[0]), p(B[1]), p(B[2]), nb, 0,
                                                            *[p(x) for x in out], ctypes.byref(longest), p(mws), mws.numel(), st), "merge")
        merge(); torch.cuda.synchronize()
        for what, got, exp in zip(("sa", "da", "lcp"), out, whole):
            assert torch.equal(got, exp), (name, share, what)
        m_ms, m_all, m_k = timed(merge, profile=True)
        bm_ms, bm_all = timed(lambda: (build_b(), merge()))
        rec = {"collection": name, "n": nn, "ndocs": nd, "commit": open(os.path.join(ROOT, "suffix_amd", "_build_commit.txt")).read().strip(),
               "share_b": share, "ndocs_b": nd - k, "n_b": nb, "longest": int(longest.value), "merge_ms": m_ms, "merge_all": m_all,
               "merge_launch_ms": m_k, "build_b_merge_ms": bm_ms, "build_b_merge_all": bm_all, "one_shot_ms": one_ms, "one_shot_all": one_all,
               "one_shot_over_build_b_merge": round(one_ms / bm_ms, 2), "merge_workspace_bytes": int(mws.numel()),
               "one_shot_workspace_bytes": int(gws.numel())}
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del A, B, out, mws
    del text, ds, whole, gws
    torch.cuda.empty_cache()
with open(os.path.join(ROOT, "profiles", "gsa_merge_times.json"), "w") as fh:
    json.dump(results, fh, indent=1)
    fh.write("\n")
