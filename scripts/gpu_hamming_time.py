#!/usr/bin/env python3
"""The k-mismatch pattern search (sfx_index_hamming_dev) timed step by step.

    gpu_hamming_time.py [--out FILE.json] [--scale S] [--only KIND[,...]]
                                                     every text kind, each in a child process under its own `timeout`;
                                                     the first one that fails ends the run
    gpu_hamming_time.py --kind KIND [--scale S]      one kind in this process: one JSON line per row

Rows: 10^9 bytes of DNA and of English-like text (one table build per kind), 2^20 patterns of 32 and of 100 bytes, k in
0, 1, 2, 4.  Half of the patterns are sampled from the text with 0 .. k + 2 substituted bytes, a quarter sampled with one
inserted byte, a quarter random over the text's alphabet.  Before anything is timed the triples of the first 2^12 patterns
are compared with the text byte by byte (every window, its count, the planted origins with at most k substitutions).
Per row: C and Z, one writing call REPS times after a warm-up between device events, and the library's profiler for the
piece search, hm_count and hm_emit.  Candidates/s = C over hm_count's time: the figure to put next to the random-line rate
of sfx_microbench's one-byte gather over the same number of bytes, measured in this process -- hm_count reads one random
window per candidate that is not abandoned at once (52-55 G lines/s).  A row whose C exceeds the
limit of 2^33 is reported as refused, with its C.  The k = 0 row stands next to sfx_index_query_dev over the whole
patterns plus a gather of the same intervals from the table.

The committed profile is one run:  gpu_hamming_time.py --out profiles/hamming_times.json"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 5
LIMIT = 1 << 33
N, NQ, CHECKED = 1_000_000_000, 1 << 20, 1 << 12
KINDS = {"dna": 1100, "english": 1100}                        # seconds allowed per kind
LENGTHS, KS = (32, 100), (0, 1, 2, 4)


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


def make_patterns(np, text, m, k, nq, seed):
    """-> (qbytes (nq, m) uint8, origin positions, planted substitutions: -1 where the pattern is not a substituted sample)."""
    g = np.random.default_rng(seed)
    n = text.size
    alphabet = np.unique(text[:1 << 16])
    at = g.integers(0, n - m - 1, nq)
    pats = text[at[:, None] + np.arange(m)[None, :]]
    kind = np.arange(nq) % 4                                   # 0, 1: substitutions; 2: one inserted byte; 3: random
    subs = np.where(kind < 2, g.integers(0, k + 3, nq), 0)
    for r in range(k + 2):
        rows = np.flatnonzero(subs > r)
        pats[rows, g.integers(0, m, rows.size)] = alphabet[g.integers(0, alphabet.size, rows.size)]
    ins = np.flatnonzero(kind == 2)
    where = g.integers(0, m, ins.size)
    for j, w in zip(ins.tolist(), where.tolist()):
        pats[j, w + 1:] = pats[j, w:m - 1].copy()
        pats[j, w] = alphabet[(j * 7) % alphabet.size]
    rnd = np.flatnonzero(kind == 3)
    pats[rnd] = alphabet[g.integers(0, alphabet.size, (rnd.size, m))]
    planted = np.where(kind < 2, (pats != text[at[:, None] + np.arange(m)[None, :]]).sum(axis=1), -1)
    return np.ascontiguousarray(pats), at, planted


def check_answers(np, text, pats, at, planted, k, first, tpos, mism):
    """The triples of the first CHECKED patterns against the text, byte by byte; planted origins with <= k substitutions."""
    m = pats.shape[1]
    for j in range(min(CHECKED, pats.shape[0])):
        a, z = int(first[j]), int(first[j + 1])
        w = tpos[a:z].astype(np.int64)
        d = (text[w[:, None] + np.arange(m)[None, :]] != pats[j][None, :]).sum(axis=1)
        assert (d == mism[a:z]).all() and (d <= k).all() and np.unique(w).size == w.size, (j, "a wrong triple")
        if 0 <= planted[j] <= k:
            hit = np.flatnonzero(w == at[j])
            assert hit.size == 1 and int(mism[a:z][hit[0]]) == int(planted[j]), (j, "a planted origin is missing")


def run_kind(kind, scale):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import numpy as np
    import torch
    import _devlib
    import _gen
    from suffix_amd import device as sdev
    n, nq = int(N * scale), max(CHECKED, int(NQ * scale))
    eng = _devlib.engine()
    eng.require_device()
    gen = {"english": _gen.english_like, "dna": _gen.dna_fast if n > 1 << 26 else _gen.dna}[kind]
    text = gen(n)
    dt = torch.from_numpy(text).cuda()
    dsa = sdev.build_sa(dt, engine=eng)
    ix = sdev.DeviceIndex(dt, dsa, engine=eng)
    torch.cuda.synchronize()
    gather = round(eng.microbench(eng.MB_GATHER1, n, 0, 0, REPS), 2)     # GB/s of one-byte random reads = G lines/s

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

    for m in LENGTHS:
        for k in KS:
            pats, at, planted = make_patterns(np, text, m, k, nq, seed=1000 * m + k)
            dq = torch.from_numpy(pats.reshape(-1)).cuda()
            doff = torch.arange(0, (nq + 1) * m, m, dtype=torch.int64, device="cuda")
            row = {"kind": kind, "n": n, "patterns": nq, "m": m, "k": k, "library": os.path.basename(eng.path),
                   "gather1_G_lines_per_s": gather}
            try:
                got = ix.hamming(dq, doff, k, max_candidates=LIMIT)
            except Exception as e:                                        # noqa: BLE001 (a refusal names its count)
                words = [w for w in str(e).replace(";", " ").split() if w.isdigit()]
                row.update(refused=True, C=int(words[0]) if words else None, limit=LIMIT)
                print(json.dumps(row), flush=True)
                continue
            torch.cuda.synchronize()
            first, tpos, mism = got[0].cpu().numpy(), got[2].cpu().numpy().view(np.uint32), got[3].cpu().numpy()
            check_answers(np, text, pats, at, planted, k, first, tpos, mism)
            C, Z = got[4], int(tpos.size)
            del got
            ws = sdev.hamming_workspace(nq, k, min(LIMIT, nq * (k + 1) * n), "cuda", eng)
            call = lambda: ix.hamming(dq, doff, k, max_candidates=LIMIT, capacity=max(Z, 1), workspace=ws)
            call()
            torch.cuda.synchronize()
            row.update(C=C, Z=Z, call_ms=timed(torch, call))
            steps = profiled(call)
            search = sum(v for name, v in steps.items() if name.startswith("query_"))     # (query_batch_tree, query_tree_long, ..)
            row.update(steps_ms=steps, piece_search_ms=round(search, 4), hm_count_ms=steps.get("hm_count"), hm_emit_ms=steps.get("hm_emit"),
                       candidates_per_s=round(C / (steps["hm_count"] * 1e-3)) if steps.get("hm_count") else None)
            if k == 0:                                                    # the exact search and a gather of its intervals
                def exact():
                    s, e, _, _ = ix.query(dq, doff)
                    s, cnt = s.to(torch.int64) & 0xFFFFFFFF, (e.to(torch.int64) & 0xFFFFFFFF) - (s.to(torch.int64) & 0xFFFFFFFF)
                    offs = torch.cumsum(cnt, 0) - cnt
                    which = torch.repeat_interleave(torch.arange(nq, device="cuda"), cnt)
                    return dsa[s[which] + (torch.arange(which.numel(), device="cuda") - offs[which])]
                assert exact().numel() == Z
                torch.cuda.synchronize()
                row["exact_query_plus_gather_ms"] = timed(torch, exact)
                row["exact_query_ms"] = timed(torch, lambda: ix.query(dq, doff))
            print(json.dumps(row), flush=True)
    torch.cuda.synchronize()
    ix.close()


def main(argv):
    scale, kind, out_path, only = 1.0, None, None, None
    i = 0
    while i < len(argv):
        if argv[i] == "--scale":
            scale = float(argv[i + 1]); i += 2
        elif argv[i] == "--kind":
            kind = argv[i + 1]; i += 2
        elif argv[i] == "--out":
            out_path = argv[i + 1]; i += 2
        elif argv[i] == "--only" and i + 1 < len(argv):
            only = argv[i + 1].split(","); i += 2
            if not all(o in KINDS for o in only):
                raise SystemExit(__doc__)
        else:
            raise SystemExit(__doc__)
    if kind:
        run_kind(kind, scale)
        return 0
    names = [k for k in KINDS if only is None or k in only]
    results, failed = [], False
    for name in names:
        r = subprocess.run(["timeout", "-k", "10", str(KINDS[name]), sys.executable, os.path.abspath(__file__), "--kind", name,
                            "--scale", str(scale)], capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
        for row in rows:
            print(json.dumps(row), flush=True)
        results += rows
        if out_path:                                           # (kept after every kind: a later one may run out of time)
            with open(out_path, "w") as fh:
                json.dump({"source": f"scripts/gpu_hamming_time.py: device events and the library's profiler, {REPS} runs after a warm-up",
                           "library": os.path.basename(os.environ.get("SFX_DEV_LIB") or "libsuffix_hip.so"), "scale": scale,
                           "rows": results}, fh, indent=1)
                fh.write("\n")
        if r.returncode != 0:                                  # a fault, an abort or a time limit: start nothing more
            print(f"{name}: exit status {r.returncode}; stopping", flush=True)
            failed = True
            break
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
