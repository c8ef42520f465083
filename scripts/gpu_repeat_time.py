#!/usr/bin/env python3
"""Repeat lengths and repeated spans (sfx_repeat_lens_dev, sfx_repeat_spans_dev) timed against the build whose arrays
they read, on the two collections of DESIGN.md section 12 and on plain 10^9 B English-like text (section 13).

    gpu_repeat_time.py [--out FILE.json] [--scale S]    every case, each in a child process under its own `timeout`;
                                                        the first case that fails ends the run
    gpu_repeat_time.py --case NAME [--scale S]          one case in this process: one JSON line

Per case: device-event times, best of 3 after a warm-up, of the build (sfx_build_gsa_u32_dev / sfx_build_sa_lcp_u32_dev),
of every scope of sfx_repeat_lens_dev (rep only, the workspace allocated beforehand) and of sfx_repeat_spans_dev at
min_len 50 on the EARLIER array; the streaming-copy rate of sfx_microbench(SFX_MB_COPY) in the same process, and what
fraction of it ANY (12 bytes per suffix: SA and LCP read, rep written) and the spans (40 bytes per byte: rep read twice,
the prefix maxima written once and read twice, the flags written, read twice and written once by their scan, read once
more) reach."""
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"english_docs_1e8": 300, "copies_64x512k": 420, "english_plain_1e9": 600}       # name: seconds allowed
ANY_BYTES, SPAN_BYTES = 12, 40


def best_ms(fn, torch, reps=3):
    fn()                                                                   # warm-up: code objects, pooled scratch
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


def make_case(name, scale):
    """-> (text as a uint8 array, doc_starts as an int64 array or None)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import _gen
    if name == "english_docs_1e8":
        n = int(100_000_000 * scale)
        rng, starts, p = random.Random(1), [0], 0
        while True:
            p += rng.randint(5000, 15000)
            if p >= n:
                break
            starts.append(p)
        return _gen.english_like(n), np.array(starts, dtype=np.int64)
    if name == "copies_64x512k":
        k = max(int((1 << 19) * scale), 4096)
        base = _gen.english_like(k, seed=77).tobytes()
        docs = [base] * 64 + [base[:1000], base[:-1] + b"!", base[12345 % k:]]
        starts = np.zeros(len(docs), dtype=np.int64)
        starts[1:] = np.cumsum([len(d) for d in docs[:-1]])
        return np.frombuffer(b"".join(docs), dtype=np.uint8).copy(), starts
    if name == "english_plain_1e9":
        return _gen.english_like(int(1_000_000_000 * scale)), None
    raise SystemExit(f"unknown case {name}")


def run_case(name, scale):
    sys.path.insert(0, ROOT)
    import torch
    import suffix_amd
    from suffix_amd import device as sdev
    eng = suffix_amd.default_engine()
    eng.require_device()
    host, starts = make_case(name, scale)
    n = int(host.size)
    text = torch.from_numpy(host).cuda()
    out = {"case": name, "n": n, "documents": 0 if starts is None else int(starts.size)}
    sa = torch.empty(n, dtype=torch.int32, device="cuda")
    lcp = torch.empty(n, dtype=torch.int32, device="cuda")
    if starts is None:
        ws = sdev.sa_lcp_workspace(n, text.device)
        out["build"] = "sfx_build_sa_lcp_u32_dev"
        out["build_ms"] = best_ms(lambda: sdev.build_sa_lcp(text, out_sa=sa, out_lcp=lcp, workspace=ws), torch)
        da = ds = None
        scopes = ("any", "earlier")
    else:
        ds = torch.from_numpy(starts).cuda()
        da = torch.empty(n, dtype=torch.int32, device="cuda")
        ws = sdev.gsa_workspace(n, starts.size, text.device)
        out["build"] = "sfx_build_gsa_u32_dev"
        out["build_ms"] = best_ms(lambda: sdev.build_gsa(text, ds, out_sa=sa, out_da=da, out_lcp=lcp, workspace=ws), torch)
        scopes = ("any", "earlier", "other_doc")
    del ws
    torch.cuda.empty_cache()
    out["copy_gbps"] = eng.microbench(eng.MB_COPY, 1 << 30)
    rep = None
    for scope in scopes:
        w = sdev.repeat_lens_workspace(n, scope, text.device)
        out[f"lens_{scope}_ms"] = best_ms(lambda: sdev.repeat_lens(sa, lcp, scope=scope, da=da, workspace=w), torch)
        if scope == "earlier":
            rep = sdev.repeat_lens(sa, lcp, scope=scope, da=da, workspace=w)
        del w
    spans = [None]

    def do_spans():
        spans[0] = sdev.repeat_spans(rep, 50, doc_starts=ds)
    out["spans_min_len"] = 50
    out["spans_ms"] = best_ms(do_spans, torch)             # (includes allocating its workspace and the (k, 2) result)
    out["spans"] = int(spans[0].shape[0])
    out["bytes_covered"] = int((spans[0][:, 1].long() - spans[0][:, 0].long()).sum())
    out["any_fraction_of_copy"] = ANY_BYTES * n / (out["lens_any_ms"] * 1e-3) / (out["copy_gbps"] * 1e9)
    out["spans_fraction_of_copy"] = SPAN_BYTES * n / (out["spans_ms"] * 1e-3) / (out["copy_gbps"] * 1e9)
    for k, v in list(out.items()):
        if isinstance(v, float):
            out[k] = round(v, 4)
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
            json.dump({"source": "scripts/gpu_repeat_time.py: device events, best of 3 after a warm-up", "scale": scale,
                       "cases": results}, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
