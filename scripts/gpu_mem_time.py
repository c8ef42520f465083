#!/usr/bin/env python3
"""The maximal exact matches of a query text (sfx_index_mems_dev) timed step by step.

    gpu_mem_time.py [--out FILE.json] [--scale S] [--only small|large|CASE[,...]]
                                                     every case, each in a child process under its own `timeout`;
                                                     the first case that fails ends the run
    gpu_mem_time.py --case NAME [--scale S]         one case in this process: one JSON line

Cases: the five rows of tests/test_gpu_mem.py (2^22 indexed bytes, 2^18 query bytes) and 10^9 bytes of English-like text
and of DNA with queries of 2^24 bytes by the same recipe.  Per case one call that counts (capacity 0) and one that writes
every match, REPS times each after a warm-up, between device events; the library's own profiler gives the share of the
capped matching-statistics search, of mem_cand, of the scans, of mem_count and of mem_emit in the writing call.  Pairs/s
= P over mem_count's time: the figure to put next to the 52-55 G random lines/s of lab/gather_probe
(profiles/r6_gather_probe_modes.txt), the ceiling of one text byte per pair.  Before anything is timed the counts are
held against the identity Z = P_L - P_(L+1).

With SFX_DEV_LIB=suffix_amd/libsuffix_hip_dev.so (scripts/_devlib.py: the hooks compiled in) the two ways of dealing
positions to pairs -- the LDS expansion the product ships and one bisection per pair (SFX_MEM_BISECT=1) -- run
interleaved in the same process, REPS times each: "expand_vs_bisect".  The committed profiles are one run per library:
    gpu_mem_time.py --only small,dna_1e9_L13 --out profiles/mem_times.json
    SFX_DEV_LIB=suffix_amd/libsuffix_hip_dev.so gpu_mem_time.py --only small,dna_1e9_L13 --out profiles/mem_times_dev.json"""
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 5
LIMIT = 1 << 33
CASES = {                                                    # name: (kind, n, query bytes, L, seconds allowed)
    "english_L12": ("english", 1 << 22, 1 << 18, 12, 300),
    "english_L20": ("english", 1 << 22, 1 << 18, 20, 300),
    "dna_L8": ("dna", 1 << 22, 1 << 18, 8, 300),
    "dna_L12": ("dna", 1 << 22, 1 << 18, 12, 300),
    "near_duplicates_L16": ("near_duplicates", 1 << 22, 1 << 18, 16, 300),
    "english_1e9_L20": ("english", 1_000_000_000, 1 << 24, 20, 1100),
    "dna_1e9_L13": ("dna", 1_000_000_000, 1 << 24, 13, 1100),     # a 13-mer stands about 15 times in 10^9 random bases
}
SMALL = [k for k, v in CASES.items() if v[1] <= 1 << 22]


def timed(torch, fn, reps=REPS):
    """Device-event milliseconds of fn(): the median of `reps` runs, and all of them (the caller warms up)."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(round(a.elapsed_time(b), 4))
    return {"median": sorted(out)[len(out) // 2], "runs": out}


def run_case(name, scale):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import numpy as np
    import torch
    import _devlib
    import _gen
    import _mem
    from suffix_amd import device as sdev
    kind, n, qm, L, _ = CASES[name]
    n, qm = int(n * scale), max(1 << 14, int(qm * scale))
    eng = _devlib.engine()
    eng.require_device()
    dev_lib = bool(os.environ.get("SFX_DEV_LIB"))
    big = n > 1 << 26
    gen = {"english": _gen.english_like, "dna": _gen.dna_fast if big else _gen.dna, "near_duplicates": _gen.near_duplicates}[kind]
    text = gen(n)
    other = gen(qm, seed=99)
    noise = _gen.uniform_bytes(qm, 256, 5)
    if kind == "dna":
        noise = np.frombuffer(b"ACGT", dtype=np.uint8)[_gen.uniform_bytes(qm, 4, 5) % 4]
    q = _mem.mixture(text.tobytes() if not big else memoryview(text), other, noise, random.Random(17), qm)
    dt, dq = torch.from_numpy(text).cuda(), torch.from_numpy(q).cuda()
    dsa = sdev.build_sa(dt, engine=eng)
    ix = sdev.DeviceIndex(dt, dsa, engine=eng)
    out = {"case": name, "kind": kind, "n": n, "m": qm, "min_len": L, "library": os.path.basename(eng.path)}

    counts = {}
    for k in (L, L + 1):
        counts[k] = ix.mems(dq, k, max_pairs=LIMIT, capacity=0)[3]
    full = ix.mems(dq, L, max_pairs=LIMIT)
    z = int(full[0].numel())
    assert full[3] == counts[L] and z == counts[L] - counts[L + 1], (name, full[3], counts, z)
    uniq = ix.mems(dq, L, unique=True, max_pairs=LIMIT)
    out.update(pairs=counts[L], mems=z, unique_mems=int(uniq[0].numel()))
    del full, uniq
    ws = sdev.mems_workspace(qm, min(LIMIT, qm * n), "cuda", eng)

    def call(capacity, unique=False):
        return ix.mems(dq, L, unique=unique, max_pairs=LIMIT, capacity=capacity, workspace=ws)

    def profiled(fn):
        """Per launch name: milliseconds of one call (the profiler synchronises around every launch)."""
        eng.profile(True)
        eng.profile_reset()
        try:
            for _ in range(REPS):
                fn()
        finally:
            rep = {r["name"]: round(r["total_ms"] / REPS, 4) for r in eng.profile_report()}
            eng.profile(False)
        return rep

    call(z)
    torch.cuda.synchronize()
    out["count_only_ms"] = timed(torch, lambda: call(0))
    out["write_all_ms"] = timed(torch, lambda: call(z))
    out["write_unique_ms"] = timed(torch, lambda: call(z, True))
    steps = profiled(lambda: call(z))
    out["steps_ms"] = steps
    search = sum(v for k, v in steps.items() if k.startswith("ms_"))
    out["search_ms"] = round(search, 4)
    out["pairs_per_s"] = round(counts[L] / (steps["mem_count"] * 1e-3)) if steps.get("mem_count") else None
    out["mems_per_s"] = round(z / (steps["mem_emit"] * 1e-3)) if steps.get("mem_emit") else None
    out["steps_unique_ms"] = profiled(lambda: call(z, True))
    if dev_lib:                                                 # both ways of dealing positions to pairs, interleaved
        runs = {"expand": [], "bisect": []}
        for rep in range(REPS + 1):
            for mode, flag in (("expand", "0"), ("bisect", "1")):
                os.environ["SFX_MEM_BISECT"] = flag
                p = profiled(lambda: call(z))
                if rep:                                         # (the first round warms up)
                    runs[mode].append({k: p.get(k) for k in ("mem_count", "mem_emit")})
        os.environ["SFX_MEM_BISECT"] = "0"
        med = lambda mode, k: sorted(r[k] for r in runs[mode])[REPS // 2]
        out["expand_vs_bisect"] = {mode: {"mem_count_ms": med(mode, "mem_count"), "mem_emit_ms": med(mode, "mem_emit"), "runs": runs[mode]}
                                   for mode in runs}
    torch.cuda.synchronize()
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
            if not all(o in ("small", "large") or o in CASES for o in only):
                raise SystemExit(__doc__)
        else:
            raise SystemExit(__doc__)
    if case:
        run_case(case, scale)
        return 0
    names = [k for k in CASES if only is None or k in only or ("small" if k in SMALL else "large") in only]
    results = []
    for name in names:
        r = subprocess.run(["timeout", "-k", "10", str(CASES[name][4]), sys.executable, os.path.abspath(__file__), "--case", name,
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
                json.dump({"source": f"scripts/gpu_mem_time.py: device events and the library's profiler, {REPS} runs after a warm-up",
                           "library": os.path.basename(os.environ.get("SFX_DEV_LIB") or "libsuffix_hip.so"), "scale": scale,
                           "cases": results}, fh, indent=1)
                fh.write("\n")
    return 0 if len(results) == len(names) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
