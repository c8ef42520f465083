#!/usr/bin/env python3
"""Matching statistics of a query text against the resident index (sfx_index_match_stats_dev,
sfx_gindex_match_stats_dev) timed against the route the engine offered before them: the generalized suffix array over
the indexed documents plus the query as one more (sfx_build_gsa_u32_dev), then the other-document repeat lengths
(sfx_repeat_lens_dev), whose tail is the same `len` array.

    gpu_match_time.py [--out FILE.json] [--scale S]    every case, each in a child process under its own `timeout`;
                                                       the first case that fails ends the run
    gpu_match_time.py --case NAME [--scale S]          one case in this process: one JSON line

Per case: the outputs of the two routes are compared first (uncapped len == the rebuild's tail); then device-event
times, best of 3 after a warm-up, of the resident call at max_len 0 and 64, with and without the rank intervals, and of
the rebuild (its workspaces allocated beforehand).  Reported: milliseconds, query positions per second, and the ratio
rebuild / resident.  The search is bound by the latency of dependent random reads: no share of a bandwidth is quoted."""
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"english_1e9_unrelated": 420, "english_1e9_slices": 420, "english_docs_1e8_slices": 300}     # name: seconds allowed
QUERY_BYTES = 1 << 24


def best_ms(fn, torch, reps=3):
    fn()                                                                   # warm-up: code objects
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None else min(best, ms)
    return best


def slices_of(host, m, np, seed=5, piece=1 << 16, changed=0.01):
    """m bytes cut from the text in pieces, 1 % of the bytes replaced by a byte from elsewhere in the text"""
    rng = random.Random(seed)
    parts = []
    for _ in range(m // piece):
        a = rng.randrange(host.size - piece)
        parts.append(host[a:a + piece])
    q = np.concatenate(parts).copy()
    g = np.random.default_rng(seed)
    at = np.flatnonzero(g.random(q.size) < changed)
    q[at] = host[g.integers(0, host.size, at.size)]
    return q


def make_case(name, scale):
    """-> (text, doc_starts or None, query), uint8 / int64 arrays"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import _gen
    m = max(int(QUERY_BYTES * scale) & ~0xFFFF, 1 << 16)
    if name == "english_docs_1e8_slices":
        n = int(100_000_000 * scale)
        rng, starts, p = random.Random(1), [0], 0
        while True:
            p += rng.randint(5000, 15000)
            if p >= n:
                break
            starts.append(p)
        host = _gen.english_like(n)
        return host, np.array(starts, dtype=np.int64), slices_of(host, m, np)
    host = _gen.english_like(int(1_000_000_000 * scale))
    if name == "english_1e9_unrelated":
        return host, None, _gen.english_like(m, seed=99)
    if name == "english_1e9_slices":
        return host, None, slices_of(host, m, np)
    raise SystemExit(f"unknown case {name}")


def run_case(name, scale):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import suffix_amd
    from suffix_amd import device as sdev
    eng = suffix_amd.default_engine()
    eng.require_device()
    host, starts, qhost = make_case(name, scale)
    n, m = int(host.size), int(qhost.size)
    text, query = torch.from_numpy(host).cuda(), torch.from_numpy(qhost).cuda()
    out = {"case": name, "n": n, "m": m, "documents": 0 if starts is None else int(starts.size)}
    if starts is None:
        sa = sdev.build_sa(text)
        index = sdev.DeviceIndex(text, sa)
    else:
        ds = torch.from_numpy(starts).cuda()
        sa, da, _ = sdev.build_gsa(text, ds, want_lcp=False)
        index = sdev.GeneralizedDeviceIndex(text, ds, sa, da)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()

    # the rebuild route on the same inputs: {documents of T, Q}
    both = torch.cat([text, query])
    bstarts = torch.from_numpy(np.concatenate([starts if starts is not None else np.zeros(1, dtype=np.int64), [n]])).cuda()
    bsa, bda, blcp = (torch.empty(n + m, dtype=torch.int32, device="cuda") for _ in range(3))
    ws = sdev.gsa_workspace(n + m, bstarts.numel(), text.device)
    wr = sdev.repeat_lens_workspace(n + m, "other_doc", text.device)
    rep = [None]

    def rebuild():
        sdev.build_gsa(both, bstarts, out_sa=bsa, out_da=bda, out_lcp=blcp, workspace=ws)
        rep[0] = sdev.repeat_lens(bsa, blcp, "other_doc", da=bda, workspace=wr)

    rebuild()
    ln = index.match_stats(query)
    torch.cuda.synchronize()
    if not torch.equal(ln, rep[0][n:]):
        raise SystemExit(f"{name}: the resident call and the rebuild route disagree")
    out["len_sum"] = int(ln.long().sum())
    out["len_max"] = int(ln.max())
    out["rebuild_ms"] = best_ms(rebuild, torch)
    del ws, wr, bsa, bda, blcp, both
    rep[0] = None
    torch.cuda.empty_cache()
    for cap in (0, 64):
        for iv in (False, True):
            key = f"resident_cap{cap}" + ("_intervals" if iv else "")
            out[key + "_ms"] = best_ms(lambda: index.match_stats(query, max_len=cap, want_interval=iv), torch)
            out[key + "_positions_per_s"] = m / (out[key + "_ms"] * 1e-3)
    out["rebuild_over_resident"] = out["rebuild_ms"] / out["resident_cap0_ms"]
    for k, v in list(out.items()):
        if isinstance(v, float):
            out[k] = round(v, 4) if v < 1e6 else round(v)
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
    for name, seconds in CASES.items():
        r = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--case", name,
                            "--scale", str(scale)], capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:                                  # a fault, an abort or a time limit: start nothing more
            print(f"{name}: exit status {r.returncode}; stopping", flush=True)
            return 1
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        results.append(json.loads(line))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump({"source": "scripts/gpu_match_time.py: device events, best of 3 after a warm-up", "scale": scale,
                       "cases": results}, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
