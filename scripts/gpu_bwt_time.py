#!/usr/bin/env python3
"""The Burrows-Wheeler transform with sampled ranks and its inverse (sfx_bwt_dev, sfx_unbwt_dev)
timed next to the engine's own random-read probes.

    gpu_bwt_time.py [--out FILE.json] [--scale S]    every case, each in a child process under its own `timeout`;
                                                      the first case that fails ends the run
    gpu_bwt_time.py --case NAME [--scale S]          one case in this process: one JSON line

Cases: 10^8 and 10^9 bytes of DNA, English-like text and near-duplicate documents at the default step (256); at 10^9
bytes also the steps 64, 1024 and 4096; and one chain of 2^20 steps (sample_step 0 on 2^20 bytes), the longest the
contract admits (SFX_UNBWT_MAX_CHAIN).  Per case the round trip is compared with the text first.  Times are the
engine's per-kernel device events (sfx_profile_report) over REPS repeats after a warm-up: minimum, median, maximum.
The yardsticks are the project's measured random-read rates at the same byte count: bwt_gather next to
sfx_microbench(SFX_MB_GATHER1) over n bytes, bwt_rank and unbwt_walk next to SFX_MB_GATHER4 over 4n bytes; every
kernel is reported as a ratio to the time its probe needs for n elements, never against the code under test."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 7
KINDS = ("dna", "english", "near_duplicates")
CASES = {}                                                   # name: (kind, n, steps, seconds allowed)
for _k in KINDS:
    CASES[f"{_k}_1e8"] = (_k, 100_000_000, (256,), 300)
    CASES[f"{_k}_1e9"] = (_k, 1_000_000_000, (64, 256, 1024, 4096), 900)
CASES["one_chain_2p20"] = ("english", 1 << 20, (0,), 120)
KERNELS = ("bwt_primary", "bwt_gather", "bwt_rank", "unbwt_walk")


def spread(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def run_case(name, scale):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import _gen
    import suffix_amd
    from suffix_amd import device as sdev
    kind, n, steps, _ = CASES[name]
    if n > (1 << 20):
        n = int(n * scale)
    eng = suffix_amd.default_engine()
    eng.require_device()
    host = {"dna": _gen.dna, "english": _gen.english_like, "near_duplicates": _gen.near_duplicates}[kind](n)
    text = torch.from_numpy(host).cuda()
    sa = sdev.build_sa(text)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    out = {"case": name, "kind": kind, "n": n, "reps": REPS}
    g1 = eng.microbench(eng.MB_GATHER1, max(n, 1 << 20), reps=5)
    g4 = eng.microbench(eng.MB_GATHER4, max(4 * n, 1 << 20), reps=5)
    out["gather1_gbps"], out["gather4_gbps"] = round(g1, 3), round(g4, 3)
    probe1_ms, probe4_ms = n / (g1 * 1e9) * 1e3, 4.0 * n / (g4 * 1e9) * 1e3           # n elements at the probe's rate
    out["gather1_ms_for_n"], out["gather4_ms_for_n"] = round(probe1_ms, 4), round(probe4_ms, 4)
    ws = sdev.unbwt_workspace(n, text.device)
    back = torch.empty_like(text)
    out["steps"] = {}
    for s in steps:
        b, sm = sdev.bwt(text, sa, s)
        sdev.unbwt(b, sm, s, out=back, workspace=ws)
        if not torch.equal(back, text):
            raise SystemExit(f"{name}: step {s}: the round trip does not restore the text")
        times = {k: [] for k in KERNELS}
        eng.profile(True)
        for _ in range(REPS):
            eng.profile_reset()
            sdev.bwt(text, sa, s, out_bwt=b, out_samples=sm)
            sdev.unbwt(b, sm, s, out=back, workspace=ws)
            torch.cuda.synchronize()
            rep = {r["name"]: r["total_ms"] for r in eng.profile_report()}
            for k in KERNELS:
                times[k].append(rep[k])
        eng.profile(False)
        rec = {k + "_ms": spread(v) for k, v in times.items()}
        rec["samples"] = int(sm.numel())
        rec["bwt_gather_over_gather1"] = round(rec["bwt_gather_ms"]["median"] / probe1_ms, 3)
        rec["bwt_rank_over_gather4"] = round(rec["bwt_rank_ms"]["median"] / probe4_ms, 3)
        rec["unbwt_walk_over_gather4"] = round(rec["unbwt_walk_ms"]["median"] / probe4_ms, 3)
        out["steps"][str(s)] = rec
        del b, sm
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
    for name, (_, _, _, seconds) in CASES.items():
        r = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--case", name,
                            "--scale", str(scale)], capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:                                  # a fault, an abort or a time limit: start nothing more
            print(f"{name}: exit status {r.returncode}; stopping", flush=True)
            break
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        results.append(json.loads(line))
    if out_path and results:
        with open(out_path, "w") as fh:
            json.dump({"source": f"scripts/gpu_bwt_time.py: per-kernel device events, {REPS} repeats after a warm-up", "scale": scale,
                       "cases": results}, fh, indent=1)
            fh.write("\n")
    return 0 if len(results) == len(CASES) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
