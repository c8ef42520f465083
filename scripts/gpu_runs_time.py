#!/usr/bin/env python3
"""Maximal repetitions (sfx_runs_dev) timed: the whole call and its parts.

    gpu_runs_time.py [--out FILE.json] [--scale S] [--only CASE[,...]]   every case, each in a child process under its own
                                                                          `timeout`; the first case that fails ends the run
    gpu_runs_time.py --case NAME [--scale S]                             one case in this process: one JSON line

Cases: 10^8 bytes of English-like text, of DNA and of random bits, the Fibonacci string of 102 334 155 bytes, 10^9 bytes of
DNA.  The table and its LCP array are the engine's own one-call build, whose time in the same process is the yardstick
(`build_sa_lcp_ms`, median of REPS after a warm-up).  Before anything is timed the answer goes through the serial checker
tests/runs_check.c: every triple verified against the text, every run of period <= 256 enumerated from the definition.

Timed: the whole call between device events (REPS runs after a warm-up: all of them and the median), and its parts from the
library's profiler (device events per launch name, the median of REPS profiled calls):
    complement_build   runs_complement + every launch of the table build of the complemented text (the names a stand-alone
                       build of it shows, with that build's share of the radix passes)
    inverse_tables     runs_check + runs_scatter + runs_verify
    trees              runs_levels (the LCP tree and both inverse-table trees)
    lyndon             runs_lyndon_tile + runs_lyndon_open
    candidates         runs_candidates + runs_offsets + runs_compact
    extension          runs_extend + runs_gather
    sort               the radix passes of the call that the stand-alone build does not account for + runs_write
`survivors`: of the 2n candidates, how many pass the first extension and how many are accepted, per order (the first words
of the workspace keep them).  `gather4_lines_per_s`: sfx_microbench(SFX_MB_GATHER4) over 4n bytes in the same run.
    gpu_runs_time.py --out profiles/runs_times.json"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 5
CASES = {                                                    # name: (kind, n, seconds allowed)
    "english_2p22": ("english", 1 << 22, 300),
    "english_1e8": ("english", 100_000_000, 500),
    "dna_1e8": ("dna", 100_000_000, 500),
    "binary_1e8": ("binary", 100_000_000, 500),
    "fibonacci_102334155": ("fibonacci", 102_334_155, 560),
    "dna_1e9": ("dna", 1_000_000_000, 1100),
}
PARTS = {"inverse_tables": ("runs_check", "runs_scatter", "runs_verify"), "trees": ("runs_levels",),
         "lyndon": ("runs_lyndon_tile", "runs_lyndon_open"), "candidates": ("runs_candidates", "runs_offsets", "runs_compact"),
         "extension": ("runs_extend", "runs_gather")}


def median(xs):
    return sorted(xs)[len(xs) // 2]


def timed(torch, fn, reps=REPS):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(round(a.elapsed_time(b), 4))
    return out


def profiled(torch, eng, fn, reps=REPS):
    """name -> the median over `reps` profiled calls of the milliseconds all launches of that name took"""
    from suffix_amd import _lib
    seen = {}
    for _ in range(reps):
        eng.profile(True)
        eng.profile_reset()
        fn()
        torch.cuda.synchronize()
        arr = (_lib.KernelStat * 256)()                     # (a build and the call together show more names than Engine.profile_report holds)
        for i in range(min(eng.lib.sfx_profile_report(arr, 256), 256)):
            seen.setdefault(arr[i].name.decode(), []).append(float(arr[i].total_ms))
        eng.profile(False)
    return {k: round(median(v + [0.0] * (reps - len(v))), 4) for k, v in seen.items()}


def run_case(name, scale):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import tempfile

    import numpy as np
    import torch
    import _devlib
    import _gen
    import _runs
    from suffix_amd import device as sdev
    kind, n, _ = CASES[name]
    n = int(n * scale)
    eng = _devlib.engine()
    eng.require_device()
    if kind == "fibonacci":
        a, b = b"b", b"a"
        while len(b) < n:
            a, b = b, b + a
        text = np.frombuffer(b, dtype=np.uint8)
        n = text.size
    else:
        gen = {"english": _gen.english_like, "dna": _gen.dna_fast if n > 1 << 26 else _gen.dna,
               "binary": lambda m: _gen.uniform_bytes(m, 2, 9, base=97)}[kind]
        text = np.ascontiguousarray(gen(n), dtype=np.uint8)
    dt = torch.from_numpy(text.copy()).cuda()
    out = {"case": name, "kind": kind, "n": n, "reps": REPS, "library": os.path.basename(eng.path)}

    # ---- the yardstick: the one-call build of the same text ----
    ws = sdev.sa_lcp_workspace(n, dt.device, eng)
    dsa, dlcp = sdev.build_sa_lcp(dt, workspace=ws, engine=eng)
    torch.cuda.synchronize()
    ms = timed(torch, lambda: sdev.build_sa_lcp(dt, out_sa=dsa, out_lcp=dlcp, workspace=ws, engine=eng))
    out["build_sa_lcp_ms"] = {"runs": ms, "median": median(ms)}
    del ws
    g4 = eng.microbench(eng.MB_GATHER4, max(4 * n, 1 << 20), reps=5)
    out["gather4_gbps"] = round(g4, 3)
    out["gather4_lines_per_s"] = round(g4 * 1e9 / 4)

    # ---- the call, checked before it is timed ----
    ws = sdev.runs_workspace(n, dt.device, eng)
    out["workspace_bytes"] = ws.numel()
    call = lambda: sdev.runs(dt, dsa, dlcp, workspace=ws, engine=eng)
    b, e, p, z = call()
    torch.cuda.synchronize()
    res = ws[:48].cpu().numpy().view(np.uint32)
    out["runs"] = z
    out["survivors"] = {"candidates": 2 * n, "after_first_extension": [int(res[8]), int(res[9])], "accepted": [int(res[10]), int(res[11])]}
    got = tuple(x.cpu().numpy().view(np.uint32) for x in (b, e, p))
    out["sum_of_lengths"] = int((got[1].astype(np.int64) - got[0]).sum())
    out["longest_period"] = int(got[2].max()) if z else 0
    chk = _runs.build_checker(tempfile.mkdtemp())
    found = _runs.accept(chk, text.tobytes(), got, 256, threads=_runs.check_threads())
    assert found == int((got[2] <= 256).sum())
    if kind == "fibonacci":
        f0, f1 = 1, 1
        while f1 < n:
            f0, f1 = f1, f0 + f1
        assert f1 == n and z == 2 * (f1 - f0) - 3, (z, f0, f1)          # 2 |f(k-2)| - 3, |f(k-2)| = |f(k)| - |f(k-1)|
    out["checked"] = f"every triple verified, {found} runs of period <= 256 enumerated from the definition (tests/runs_check.c)"
    del b, e, p, got

    # ---- the whole call, then its parts ----
    ms = timed(torch, call)
    out["call_ms"] = {"runs": ms, "median": median(ms)}
    out["call_over_build"] = round(median(ms) / out["build_sa_lcp_ms"]["median"], 3)
    comp = 255 - dt
    bws = sdev.sa_workspace(n, dt.device, eng)
    bsa = sdev.build_sa(comp, workspace=bws, engine=eng)
    torch.cuda.synchronize()
    alone = profiled(torch, eng, lambda: sdev.build_sa(comp, out=bsa, workspace=bws, engine=eng))
    del bws, bsa, comp
    names = profiled(torch, eng, call)
    parts = {k: round(sum(names.get(x, 0.0) for x in v), 4) for k, v in PARTS.items()}
    parts["complement_build"] = round(names.get("runs_complement", 0.0) + sum(alone.values()), 4)
    parts["sort"] = round(names.get("runs_write", 0.0) + sum(v for k, v in names.items() if k.startswith("radix_")) -
                          sum(v for k, v in alone.items() if k.startswith("radix_")), 4)
    out["parts_ms"] = parts
    out["launch_ms"] = {k: v for k, v in sorted(names.items()) if k.startswith("runs_")}
    out["dominant_part"] = max(parts, key=parts.get)
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
    names = [k for k in CASES if (k != "english_2p22" if only is None else k in only)]
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
                json.dump({"source": f"scripts/gpu_runs_time.py: device events and the library's profiler, {REPS} runs after a warm-up",
                           "library": "libsuffix_hip.so", "scale": scale, "cases": results}, fh, indent=1)
                fh.write("\n")
    return 0 if len(results) == len(names) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
