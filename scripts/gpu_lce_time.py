#!/usr/bin/env python3
"""The LCE index (sfx_lce_*) timed: creation step by step, then batches of queries.

    gpu_lce_time.py [--out FILE.json] [--scale S] [--only CASE[,...]]   every case, each in a child process under its own
                                                                         `timeout`; the first case that fails ends the run
    gpu_lce_time.py --case NAME [--scale S]                             one case in this process: one JSON line

Cases: 10^9 bytes of English-like text and of DNA (and 2^22 bytes of the former, for a quick look).  The table and its LCP
array are the engine's own one-call build; before anything is timed, 2^12 answers of every kind of pair are held against
plain byte comparison on the host (tests/_lce.py's `brute`).

Creation: REPS creates after a warm-up between device events, and the library's profiler for the share of lce_check,
lce_scatter (with the partitioned scatter's passes from 2^27 entries on), lce_verify and lce_levels -- to hold against the
26 / 44 ms per 10^9 pairs that DESIGN.md section 4 quotes for the two scatters and, for lce_levels, against reading 4n
bytes once at the copy rate (`levels_over_copy`: the factor; sfx_microbench's copy kernel measured in the same process).

Queries: 2^26 pairs with 0 and 5 mismatches -- uniform pairs, rank neighbours at distance 1 and at distance 1024 --,
REPS runs each after a warm-up: pairs/s, and for 0 mismatches the implied lines/s with the 128-byte lines a query touches
counted by a restatement of the walk on 2^12 of the pairs (two isa lines, then the spans level by level), to hold against
the 52-55 G random lines/s of lab/gather_probe.

With SFX_DEV_LIB=suffix_amd/libsuffix_hip_dev.so (scripts/_devlib.py: the hooks compiled in) the three query variants --
one lane per query, 32 lanes per query, and the 64-ary Pyramid / range_min of sfx_tree.hip as the baseline -- run
interleaved in one process on one handle (SFX_LCE_VARIANT), REPS times each: "variants", with the gate
`slowest run of the variant < fastest run of the baseline` on uniform pairs evaluated for both new variants.
The committed profiles are one run per library:
    gpu_lce_time.py --only english_1e9,dna_1e9 --out profiles/lce_times.json
    SFX_DEV_LIB=suffix_amd/libsuffix_hip_dev.so gpu_lce_time.py --only english_1e9,dna_1e9 --out profiles/lce_times_dev.json"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 5
NQ = 1 << 26
CASES = {                                                    # name: (kind, n, seconds allowed)
    "english_2p22": ("english", 1 << 22, 300),
    "english_1e9": ("english", 1_000_000_000, 900),
    "dna_1e9": ("dna", 1_000_000_000, 900),
}
VARIANTS = ("lane", "team", "pyramid")


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


def lines_touched(n, lo, hi, fan_log=5):
    """128-byte lines the walk over [lo, hi) reads (a restatement of lce_walk): every span lies inside one node and a node
    is one line -- above level 0 always, on level 0 for a 128-byte-aligned lcp, which run_case asserts."""
    mask = (1 << fan_log) - 1
    lines, k, l, r = 0, 0, lo, hi
    levels = 1
    cnt = n
    while cnt > 1 << fan_log:
        cnt = (cnt + mask) >> fan_log
        levels += 1
    while True:
        if (l ^ (r - 1)) >> fan_log == 0 or k == levels - 1:
            return lines + 1
        if l & mask:
            lines += 1
            l = (l | mask) + 1
        if r & mask:
            lines += 1
            r &= ~mask
        if l >= r:
            return lines
        l >>= fan_log
        r >>= fan_log
        k += 1


def run_case(name, scale):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import numpy as np
    import torch
    import _devlib
    import _gen
    import _lce
    from suffix_amd import device as sdev
    kind, n, _ = CASES[name]
    n = int(n * scale)
    nq = max(1 << 16, int(NQ * min(1.0, scale * 64)))
    eng = _devlib.engine()
    eng.require_device()
    dev_lib = bool(os.environ.get("SFX_DEV_LIB"))
    if dev_lib:
        os.environ["SFX_LCE_VARIANT"] = "pyramid"           # (read at creation: the handle carries the baseline's pyramid too)
    gen = {"english": _gen.english_like, "dna": _gen.dna_fast if n > 1 << 26 else _gen.dna}[kind]
    text = gen(n)
    dt = torch.from_numpy(text).cuda()
    dsa, dlcp = sdev.build_sa_lcp(dt, engine=eng)
    del dt
    out = {"case": name, "kind": kind, "n": n, "pairs": nq, "library": os.path.basename(eng.path)}

    # ---- creation ----
    def create():
        return sdev.LceDeviceIndex(dsa, dlcp, engine=eng)

    create().close()
    runs = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ix = create()
        b.record()
        torch.cuda.synchronize()
        runs.append(round(a.elapsed_time(b), 4))
        ix.close()
    out["create_ms"] = runs
    eng.profile(True)
    eng.profile_reset()
    ix = create()
    torch.cuda.synchronize()
    out["create_steps_ms"] = {r["name"]: round(r["total_ms"], 4) for r in eng.profile_report()}
    eng.profile(False)
    out["bytes"] = ix.nbytes
    copy_gbs = eng.microbench(eng.MB_COPY, min(4 * n, 1 << 30))
    out["copy_GBps"] = round(copy_gbs, 1)
    lv = out["create_steps_ms"].get("lce_levels")
    if lv:
        out["levels_over_copy"] = round(lv / (4 * n / (copy_gbs * 1e9) * 1e3), 3)            # (the copy rate counts the bytes read and written)

    # ---- the pairs ----
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    rnd = lambda hi: torch.randint(0, hi, (nq,), generator=g, device="cuda", dtype=torch.int64)
    sa64 = lambda idx: (dsa[idx].to(torch.int64) & 0xFFFFFFFF)
    r1, r2 = rnd(n - 1), rnd(n - 1024)
    sets = {"uniform": (rnd(n), rnd(n)), "neighbours_d1": (sa64(r1), sa64(r1 + 1)), "neighbours_d1024": (sa64(r2), sa64(r2 + 1024))}
    sets = {k: (a.to(torch.int32), b.to(torch.int32)) for k, (a, b) in sets.items()}
    tbytes = text.tobytes() if n <= 1 << 26 else None
    tarr = text

    def brute(i, j, k):
        if tbytes is not None:
            return _lce.brute(tbytes, i, j, k)
        room = min(n - i, n - j)
        if i == j:
            return room
        step, done, miss = 1 << 12, 0, 0                      # (compare in pieces: extensions are short against n)
        while done < room:
            w = min(step, room - done)
            d = np.flatnonzero(tarr[i + done:i + done + w] != tarr[j + done:j + done + w])
            if d.size + miss > k:
                return done + int(d[k - miss])
            miss += d.size
            done += w
        return room

    def host(t):
        torch.cuda.synchronize()
        return t.cpu().numpy().view(np.uint32)

    def check(variant):
        for sname, (a, b) in sets.items():
            for k in (0, 5):
                got = host(ix.lce(a[:1 << 12], b[:1 << 12], mismatches=k))
                ha, hb = host(a[:1 << 12]), host(b[:1 << 12])
                for q in range(1 << 12):
                    want = brute(int(ha[q]), int(hb[q]), k)
                    assert int(got[q]) == want, (variant, sname, k, int(ha[q]), int(hb[q]), int(got[q]), want)

    for variant in (VARIANTS if dev_lib else ("shipped",)):
        if dev_lib:
            os.environ["SFX_LCE_VARIANT"] = variant
        check(variant)
    out["checked"] = f"{(1 << 12) * 6} answers per variant against byte comparison"

    # lines per query (0 mismatches): two isa lines + the walk's
    assert dlcp.data_ptr() % 128 == 0, "lines_touched counts one line per level-0 node: lcp must be 128-byte aligned"
    lines = {}
    for sname, (a, b) in sets.items():
        ra, rb = host(ix.rank_of(a[:1 << 12])).astype(np.int64), host(ix.rank_of(b[:1 << 12])).astype(np.int64)
        tot = 0
        for x, y in zip(ra.tolist(), rb.tolist()):
            tot += 2 + (lines_touched(n, min(x, y) + 1, max(x, y) + 1) if x != y else 0)
        lines[sname] = round(tot / (1 << 12), 3)
    out["lines_per_query_k0"] = lines

    # ---- queries ----
    def measure():
        res = {}
        for sname, (a, b) in sets.items():
            for k in (0, 5):
                ix.lce(a, b, mismatches=k)
                torch.cuda.synchronize()
                ms = timed(torch, lambda: ix.lce(a, b, mismatches=k))
                med = sorted(ms)[REPS // 2]
                r = {"runs_ms": ms, "pairs_per_s": round(nq / (med * 1e-3))}
                if k == 0:
                    r["lines_per_s"] = round(nq * lines[sname] / (med * 1e-3))
                res[f"{sname}_k{k}"] = r
        return res

    if not dev_lib:
        out["queries"] = measure()
    else:
        # the variants interleaved, uniform pairs first in every round; the gate on uniform pairs with 0 mismatches
        a, b = sets["uniform"]
        runs = {v: [] for v in VARIANTS}
        for rep in range(REPS + 1):
            for v in VARIANTS:
                os.environ["SFX_LCE_VARIANT"] = v
                ms = timed(torch, lambda: ix.lce(a, b, mismatches=0), reps=1)[0]
                if rep:                                       # (the first round warms up)
                    runs[v].append(ms)
        out["variants"] = {"uniform_k0_runs_ms": runs,
                           "gate": {v: {"slowest_ms": max(runs[v]), "baseline_fastest_ms": min(runs["pyramid"]),
                                        "beats_baseline": max(runs[v]) < min(runs["pyramid"])} for v in ("lane", "team")},
                           "lane_vs_team": {"lane_slowest_ms": max(runs["lane"]), "lane_fastest_ms": min(runs["lane"]),
                                            "team_slowest_ms": max(runs["team"]), "team_fastest_ms": min(runs["team"])}}
        for v in VARIANTS:
            os.environ["SFX_LCE_VARIANT"] = v
            out["variants"][v] = measure()
        os.environ["SFX_LCE_VARIANT"] = "lane"
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
                json.dump({"source": f"scripts/gpu_lce_time.py: device events and the library's profiler, {REPS} runs after a warm-up",
                           "library": os.path.basename(os.environ.get("SFX_DEV_LIB") or "libsuffix_hip.so"), "scale": scale,
                           "cases": results}, fh, indent=1)
                fh.write("\n")
    return 0 if len(results) == len(names) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
