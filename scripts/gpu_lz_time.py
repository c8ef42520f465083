#!/usr/bin/env python3
"""The LZ77 factorization and its decoder (sfx_lz_parse_dev, sfx_lz_decode_dev) timed next to the
SA + LCP build and the EARLIER repeat-length pass of the same process, which are the yardsticks.

    gpu_lz_time.py [--out FILE.json] [--scale S]    every case, each in a child process under its own `timeout`;
                                                     the first case that fails ends the run
    gpu_lz_time.py --case NAME [--scale S]          one case in this process: one JSON line

Cases: 10^8 and 10^9 bytes of DNA and of English-like text.  Per case: build_sa_lcp, repeat_lens("earlier", want_src),
lz_parse at min_len 1 and 8 and lz_decode of both parses, between device events, the median of REPS runs after a warm-up
(workspaces and outputs allocated beforehand where the binding allows it; lz_parse's and lz_decode's read-backs are part of
what they cost).  Before anything is timed every parse goes through the serial checker tests/lz_check.c over the EARLIER
array and every decode is compared with the text."""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 5
CASES = {}                                                   # name: (kind, n, seconds allowed)
for _k in ("dna", "english"):
    CASES[f"{_k}_1e8"] = (_k, 100_000_000, 300)
    CASES[f"{_k}_1e9"] = (_k, 1_000_000_000, 900)
MIN_LENS = (1, 8)


def timed(torch, fn):
    """Device-event milliseconds of fn(): the median of REPS runs after one warm-up, and all of them."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
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
    import numpy as np
    import torch
    import _gen
    import _lz
    import suffix_amd
    from suffix_amd import device as sdev
    kind, n, _ = CASES[name]
    n = int(n * scale)
    eng = suffix_amd.default_engine()
    eng.require_device()
    host = {"dna": _gen.dna_fast, "english": _gen.english_like}[kind](n)
    text = torch.from_numpy(host).cuda()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    out = {"case": name, "kind": kind, "n": n, "parse": {}, "decode": {}}
    ws = sdev.sa_lcp_workspace(n, "cuda")
    sa = torch.empty(n, dtype=torch.int32, device="cuda")
    lcp = torch.empty(n, dtype=torch.int32, device="cuda")
    out["build_sa_lcp_ms"] = timed(torch, lambda: sdev.build_sa_lcp(text, out_sa=sa, out_lcp=lcp, workspace=ws))
    del ws
    ws = sdev.repeat_lens_workspace(n, "earlier", "cuda")
    out["earlier_ms"] = timed(torch, lambda: sdev.repeat_lens(sa, lcp, "earlier", want_src=True, workspace=ws))
    rep, src = sdev.repeat_lens(sa, lcp, "earlier", want_src=True, workspace=ws)
    del ws, sa, lcp
    build = out["build_sa_lcp_ms"]["median"]
    with tempfile.TemporaryDirectory() as tmp:
        checker = _lz.build_checker(tmp)
        rep_h = u32(rep)
        pws = sdev.lz_parse_workspace(n, "cuda")
        for m in MIN_LENS:
            b, l, s, c = sdev.lz_parse(rep, src, text, min_len=m, workspace=pws)
            res = _lz.run_checker(checker, tmp, host, rep_h, m, u32(l), u32(s), c.cpu().numpy())
            assert res.startswith("ok"), (name, m, res)
            z, literals, longest = (int(x) for x in re.match(r"ok z=(\d+) literals=(\d+) longest=(\d+)", res).groups())
            back = torch.empty(n, dtype=torch.uint8, device="cuda")
            dws = sdev.lz_decode_workspace(n, z, "cuda")
            assert torch.equal(sdev.lz_decode(l, s, c, n=n, out=back, workspace=dws), text), (name, m)
            p = timed(torch, lambda: sdev.lz_parse(rep, src, text, min_len=m, workspace=pws))
            d = timed(torch, lambda: sdev.lz_decode(l, s, c, n=n, out=back, workspace=dws))
            out["parse"][str(m)] = {"z": z, "literals": literals, "longest": longest, "ms": p, "of_build": round(p["median"] / build, 3)}
            out["decode"][str(m)] = {"ms": d, "of_build": round(d["median"] / build, 3)}
            del back, dws, b, l, s, c
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
                json.dump({"source": f"scripts/gpu_lz_time.py: device events, median of {REPS} after a warm-up", "scale": scale,
                           "cases": results}, fh, indent=1)
                fh.write("\n")
    return 0 if len(results) == len(CASES) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
