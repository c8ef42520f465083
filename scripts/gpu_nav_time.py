#!/usr/bin/env python3
"""The suffix-tree navigation calls (sfx_lce_substr*, sfx_lce_lca*, sfx_lce_range_argmin*, sfx_suffix_links_*; DESIGN.md
section 28) timed.  Not a gate: a record for whoever has the card.

    gpu_nav_time.py [--out FILE.json] [--scale S] [--only CASE[,...]]   every case, each in a child process under its own
                                                                         `timeout`; the first case that fails ends the run
    gpu_nav_time.py --case NAME [--scale S]                             one case in this process: one JSON line

Cases: 10^8 and 10^9 bytes of English-like text and of DNA.  The table and its LCP array are the engine's own one-call
build.  2^26 uniform (pos, len) at len 8 / 32 / 256 (clipped to the end of the text); per kernel the medians of REPS runs
after a warm-up, next to three figures taken in the same process:
    lce_query          2^26 uniform pairs on the same handle;
    gather4            the random-4-byte-reads figure of the memory probe (SFX_MB_GATHER4), as lines/s;
    pattern search     the resident index's batch search of the same substrings as byte patterns -- the route the call
                       replaces.  Its intervals must equal [lo, hi) before anything is timed (2^16 of them are compared).
Also sfx_suffix_links_dev next to sfx_suffix_tree_dev on the same arrays.  Whatever the figures show is written down as
it comes, including a len at which the pattern search wins.  The committed profile is
    gpu_nav_time.py --out profiles/nav_times.json"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 5
NQ = 1 << 26
LENS = (8, 32, 256)
CASES = {                                                    # name: (kind, n, seconds allowed)
    "english_1e8": ("english", 100_000_000, 600),
    "dna_1e8": ("dna", 100_000_000, 600),
    "english_1e9": ("english", 1_000_000_000, 1100),
    "dna_1e9": ("dna", 1_000_000_000, 1100),
}


def timed(torch, fn, reps=REPS):
    """Device-event milliseconds of fn(): all `reps` runs (the caller warms up)."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(round(a.elapsed_time(b), 4))
    return out


def median(ms):
    return sorted(ms)[len(ms) // 2]


def run_case(name, scale):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import _gen
    import suffix_amd
    from suffix_amd import device as sdev
    kind, n, _ = CASES[name]
    n = int(n * scale)
    nq = max(1 << 16, int(NQ * min(1.0, scale * 64)))
    eng = suffix_amd.default_engine()
    eng.require_device()
    gen = {"english": _gen.english_like, "dna": _gen.dna_fast if n > 1 << 26 else _gen.dna}[kind]
    dt = torch.from_numpy(gen(n)).cuda()
    dsa, dlcp = sdev.build_sa_lcp(dt, engine=eng)
    ix = sdev.LceDeviceIndex(dsa, dlcp, engine=eng)
    rix = sdev.DeviceIndex(dt, dsa, engine=eng)
    out = {"case": name, "kind": kind, "n": n, "queries": nq, "library": os.path.basename(eng.path)}
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    rnd = lambda hi: torch.randint(0, hi, (nq,), generator=g, device="cuda", dtype=torch.int64)
    pos = rnd(n)
    out["gather4_lines_per_s"] = round(eng.microbench(eng.MB_GATHER4, min(4 * n, 1 << 30)) * 1e9 / 4)
    a32, b32 = rnd(n).to(torch.int32), rnd(n).to(torch.int32)
    ix.lce(a32, b32)
    torch.cuda.synchronize()
    ms = timed(torch, lambda: ix.lce(a32, b32))
    out["lce_query"] = {"runs_ms": ms, "per_s": round(nq / (median(ms) * 1e-3))}
    ix.lca(a32, b32)
    torch.cuda.synchronize()
    ms = timed(torch, lambda: ix.lca(a32, b32))
    out["nav_lca"] = {"runs_ms": ms, "per_s": round(nq / (median(ms) * 1e-3))}
    lo64 = torch.minimum(a32.to(torch.int64) & 0xFFFFFFFF, b32.to(torch.int64) & 0xFFFFFFFF)
    hi64 = torch.maximum(a32.to(torch.int64) & 0xFFFFFFFF, b32.to(torch.int64) & 0xFFFFFFFF) + 1
    lo32, hi32 = lo64.to(torch.int32), hi64.to(torch.int32)
    ix.range_argmin(lo32, hi32)
    torch.cuda.synchronize()
    for key, fn in (("lce_range_min", lambda: ix.range_min(lo32, hi32)), ("nav_argmin", lambda: ix.range_argmin(lo32, hi32))):
        ms = timed(torch, fn)
        out[key] = {"runs_ms": ms, "per_s": round(nq / (median(ms) * 1e-3))}
    del a32, b32, lo64, hi64, lo32, hi32
    out["substr"] = {}
    for ln in LENS:
        lens = torch.minimum(torch.full_like(pos, ln), n - pos)
        p32, l32 = pos.to(torch.int32), lens.to(torch.int32)
        lo, hi, _ = ix.substr(p32, l32)
        # the route the call replaces: the same bytes as patterns (a slice of the queries: the blob is nq * len bytes)
        m = min(nq, (1 << 30) // ln)
        qoff = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
        qoff[1:] = torch.cumsum(lens[:m], 0)
        idx = torch.repeat_interleave(pos[:m] - qoff[:m], lens[:m]) + torch.arange(int(qoff[m]), device="cuda")
        blob = dt[idx]
        del idx
        s, e, _, _ = rix.query(blob, qoff)
        torch.cuda.synchronize()
        k = min(m, 1 << 16)
        assert torch.equal(s[:k].to(torch.int64) & 0xFFFFFFFF, lo[:k].to(torch.int64) & 0xFFFFFFFF), (name, ln, "lo")
        assert torch.equal(e[:k].to(torch.int64) & 0xFFFFFFFF, hi[:k].to(torch.int64) & 0xFFFFFFFF), (name, ln, "hi")
        ms_nav = timed(torch, lambda: ix.substr(p32, l32))
        ms_pat = timed(torch, lambda: rix.query(blob, qoff))
        out["substr"][f"len{ln}"] = {"nav_runs_ms": ms_nav, "nav_per_s": round(nq / (median(ms_nav) * 1e-3)), "pattern_queries": m,
                                     "pattern_runs_ms": ms_pat, "pattern_per_s": round(m / (median(ms_pat) * 1e-3)),
                                     "checked": f"{k} intervals equal"}
        del blob, qoff, s, e, lo, hi
    rix.close()
    del pos
    # suffix links next to the node table they are computed for
    tree = sdev.suffix_tree(dsa, dlcp, text=dt, engine=eng)
    torch.cuda.synchronize()
    ms_tree = timed(torch, lambda: sdev.suffix_tree(dsa, dlcp, text=dt, engine=eng), reps=3)
    ws = sdev.suffix_links_workspace(n, "cuda", eng)
    link = lambda: sdev.suffix_links(ix, dsa, tree["node_lb"], tree["node_rb"], tree["node_depth"], workspace=ws)
    link()
    torch.cuda.synchronize()
    eng.profile(True)
    eng.profile_reset()
    link()
    torch.cuda.synchronize()
    steps = {r["name"]: round(r["total_ms"], 4) for r in eng.profile_report()}
    eng.profile(False)
    out["suffix_links"] = {"nodes": int(tree["node_lb"].numel()), "runs_ms": timed(torch, link), "steps_ms": steps, "suffix_tree_runs_ms": ms_tree}
    ix.close()
    print(json.dumps(out), flush=True)


def main(argv):
    scale, case, out_path, only = 1.0, None, None, None
    i = 0
    while i < len(argv):
        if argv[i] == "--scale":
            scale = float(argv[i + 1]); i += 2
        elif argv[i] == "--case":
            case = argv[i + 1]; i += 2
        elif argv[i] == "--out":
            out_path = argv[i + 1]; i += 2
        elif argv[i] == "--only" and i + 1 < len(argv):
            only = argv[i + 1].split(","); i += 2
            if not all(o in CASES for o in only):
                raise SystemExit(__doc__)
        else:
            raise SystemExit(__doc__)
    if case:
        run_case(case, scale)
        return 0
    names = [k for k in CASES if only is None or k in only]
    results = []
    for name in names:
        r = subprocess.run(["timeout", "-k", "10", str(CASES[name][2]), sys.executable, os.path.abspath(__file__), "--case", name,
                            "--scale", str(scale)], capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:                                  # a fault, an abort or a time limit: start nothing more
            print(f"{name}: exit status {r.returncode}; stopping", flush=True)
            break
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        results.append(json.loads(line))
        if out_path:                                           # (kept after every case: a later one may run out of time)
            with open(out_path, "w") as fh:
                json.dump({"source": f"scripts/gpu_nav_time.py: device events, {REPS} runs after a warm-up", "scale": scale, "cases": results},
                          fh, indent=1)
                fh.write("\n")
    return 0 if len(results) == len(names) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
