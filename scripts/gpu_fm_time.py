#!/usr/bin/env python3
"""The FM-index over the Burrows-Wheeler pair (sfx_fm_*) timed next to the resident index and the
engine's own random-read probe.

    gpu_fm_time.py [--out FILE.json] [--scale S]    every case, each in a child process under its own `timeout`;
                                                     the first case that fails ends the run
    gpu_fm_time.py --case NAME [--scale S]          one case in this process: one JSON line

Cases: 10^8 and 10^9 bytes of DNA and of English-like text.  Per case: the build (fm_build device events and the wall
time of creation, which includes its two read-backs), info.bytes / n, fm_count over 2^20 patterns of 8, 20 and 64 bytes
(half of them substrings of the text, half with one byte changed; patterns/s and backward steps/s, where a step is one
pattern byte actually consumed -- a search that runs empty stops; the steps are counted with the index itself, one
batch per suffix length, outside the timed runs), and fm_lookup over 2^22 random ranks at sample steps
32, 64 and 256 (ranks/s).  Before anything is timed the intervals are compared with the resident index's and the looked-up
ranks with the table.  Times are the engine's per-kernel device events (sfx_profile_report) over REPS repeats after a
warm-up: minimum, median, maximum.  The yardsticks, measured in the same run: the resident index's `query` on the same
pattern sets (all its kernels summed), and sfx_microbench(SFX_MB_GATHER4) over 4n bytes as the random-line rate."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 5
NPAT = 1 << 20
NRANKS = 1 << 22
CASES = {}                                                   # name: (kind, n, seconds allowed)
for _k in ("dna", "english"):
    CASES[f"{_k}_1e8"] = (_k, 100_000_000, 300)
    CASES[f"{_k}_1e9"] = (_k, 1_000_000_000, 900)
LENGTHS = (8, 20, 64)
STEPS = (32, 64, 256)


def spread(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def timed(eng, torch, fn, names=None):
    """Device-event milliseconds of fn() over REPS repeats: the kernels in `names` (None: all of them) summed."""
    fn()
    torch.cuda.synchronize()
    out = []
    eng.profile(True)
    for _ in range(REPS):
        eng.profile_reset()
        fn()
        torch.cuda.synchronize()
        out.append(sum(r["total_ms"] for r in eng.profile_report() if names is None or r["name"] in names))
    eng.profile(False)
    return out


def run_case(name, scale):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import _gen
    import suffix_amd
    from suffix_amd import device as sdev
    kind, n, _ = CASES[name]
    n = int(n * scale)
    eng = suffix_amd.default_engine()
    eng.require_device()
    host = {"dna": _gen.dna_fast, "english": _gen.english_like}[kind](n)
    text = torch.from_numpy(host).cuda()
    sa = sdev.build_sa(text)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    out = {"case": name, "kind": kind, "n": n, "reps": REPS, "patterns": NPAT, "ranks": NRANKS}
    g4 = eng.microbench(eng.MB_GATHER4, max(4 * n, 1 << 20), reps=5)
    out["gather4_gbps"] = round(g4, 3)
    out["gather4_lines_per_s"] = round(g4 * 1e9 / 4)
    # pattern sets: substrings at random positions, every second one with one byte changed
    gen = torch.Generator(device="cuda").manual_seed(18)
    sets = {}
    for m in LENGTHS:
        at = torch.randint(0, n - m, (NPAT,), device="cuda", generator=gen)
        q = text[(at[:, None] + torch.arange(m, device="cuda")[None, :]).reshape(-1)].reshape(NPAT, m).clone()
        col = torch.randint(0, m, (NPAT // 2,), device="cuda", generator=gen)
        q[torch.arange(0, NPAT, 2, device="cuda"), col] = text[torch.randint(0, n, (NPAT // 2,), device="cuda", generator=gen)]
        sets[m] = (q.reshape(-1).contiguous(), torch.arange(0, (NPAT + 1) * m, m, dtype=torch.int64, device="cuda"))
    ranks = torch.randint(0, n, (NRANKS,), device="cuda", generator=gen).to(torch.int32)
    want_pos = sa[ranks.to(torch.int64)]
    # the resident index: the expected intervals and the yardstick
    res = sdev.DeviceIndex(text, sa)
    want = {}
    out["resident_query"] = {}
    for m, (qb, qoff) in sets.items():
        s_, e_, _, _ = res.query(qb, qoff)
        want[m] = (s_.clone(), e_.clone())
        ms = spread(timed(eng, torch, lambda: res.query(qb, qoff)))
        out["resident_query"][str(m)] = {"ms": ms, "patterns_per_s": round(NPAT / (ms["median"] * 1e-3))}
    res.close()
    del res
    torch.cuda.empty_cache()
    out["steps"] = {}
    for s in STEPS:
        b, sm = sdev.bwt(text, sa, s)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ix = sdev.FmDeviceIndex(b, sm, s)
        wall = (time.perf_counter() - t0) * 1e3
        ix.close()
        build = []
        eng.profile(True)
        for _ in range(REPS):
            eng.profile_reset()
            ix = sdev.FmDeviceIndex(b, sm, s)
            torch.cuda.synchronize()
            build.append(sum(r["total_ms"] for r in eng.profile_report() if r["name"] in ("fm_build", "byte_hist")))
            if _ + 1 < REPS:
                ix.close()
        eng.profile(False)
        del b, sm
        rec = {"build_ms": spread(build), "create_wall_ms_first": round(wall, 3), "bytes": ix.info["bytes"],
               "bytes_per_n": round(ix.info["bytes"] / n, 4), "occ_step": ix.info["occ_step"], "sigma": ix.info["sigma"]}
        got = ix.lookup(ranks)
        if not torch.equal(got, want_pos):
            raise SystemExit(f"{name}: step {s}: lookup differs from the table")
        ms = spread(timed(eng, torch, lambda: ix.lookup(ranks), ("fm_lookup",)))
        rec["lookup"] = {"ms": ms, "ranks_per_s": round(NRANKS / (ms["median"] * 1e-3))}
        if s == STEPS[0]:                                   # count does not depend on the sample step
            rec["count"] = {}
            for m, (qb, qoff) in sets.items():
                gs, ge = ix.count(qb, qoff)
                if not (torch.equal(gs, want[m][0]) and torch.equal(ge, want[m][1])):
                    raise SystemExit(f"{name}: m = {m}: count differs from the resident index")
                # steps actually taken: step j + 1 runs iff the last j bytes of the pattern occur (j = 0: always), so a
                # pattern takes 1 + #{j in 1 .. m - 1 : its suffix of j bytes occurs} of them -- counted with the index
                # itself, one batch per suffix length, outside the timed runs
                mat = qb.reshape(NPAT, m)
                steps = NPAT
                for j in range(1, m):
                    suf = mat[:, m - j:].contiguous().reshape(-1)
                    a, b_ = ix.count(suf, torch.arange(0, (NPAT + 1) * j, j, dtype=torch.int64, device="cuda"))
                    steps += int((a != b_).sum())
                ms = spread(timed(eng, torch, lambda: ix.count(qb, qoff), ("fm_count",)))
                rec["count"][str(m)] = {"ms": ms, "patterns_per_s": round(NPAT / (ms["median"] * 1e-3)),
                                        "backward_steps": steps, "backward_steps_per_s": round(steps / (ms["median"] * 1e-3)),
                                        "present": int((ge != gs).sum())}
        out["steps"][str(s)] = rec
        ix.close()
    print(json.dumps(out), flush=True)


def main(argv):
    scale, case, out_path = 1.0, None, None
    i = 0
    while i < len(argv):
        if argv[i] == "--scale":
            scale = float(argv[i + 1]); i += 2
        elif argv[i] == "--case":
            case = argv[i + 1]; i += 2
        elif argv[i] == "--out":
            out_path = argv[i + 1]; i += 2
        else:
            raise SystemExit(__doc__)
    if case:
        run_case(case, scale)
        return 0
    results = []
    for name, (_, _, seconds) in CASES.items():
        r = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--case", name,
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
                json.dump({"source": f"scripts/gpu_fm_time.py: per-kernel device events, {REPS} repeats after a warm-up", "scale": scale,
                           "cases": results}, fh, indent=1)
                fh.write("\n")
    return 0 if len(results) == len(CASES) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
