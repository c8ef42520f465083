#!/usr/bin/env python3
"""The k-error pattern search (sfx_index_edit_dev) timed step by step.

    gpu_edit_time.py [--out FILE.json] [--sizes N[,N...]] [--only KIND[,...]] [--patterns NQ]
                                                     every (text kind, size), each in a child process under its own
                                                     `timeout`; the first one that fails ends the run
    gpu_edit_time.py --kind KIND --n N [--patterns NQ]   one text in this process: one JSON line per row

Rows: 10^8 and 10^9 bytes of DNA and of English-like text (one table build per text), 2^20 patterns, (m, k) in (32, 1),
(32, 2), (100, 2), (100, 4).  Half of the patterns are sampled from the text with 0 .. k + 1 random edits (substitutions,
insertions and deletions, the length kept at m), the rest random over the text's alphabet.  Before anything is timed
every quadruple goes through `verify` of tests/ed_check.c (the least distance at its end, the largest begin, strictly
ascending ends).  Per row: C, H and Z, one writing call REPS times after a warm-up between device events, and the
library's profiler for the piece search, ed_count, ed_emit and the sort + reduce.  Next to them, in the same process:
sfx_index_hamming_dev at the same (T, m, k) with hm_count's candidates/s, and the one-byte random gather of
sfx_microbench over the same number of bytes.  A row refused by a limit is reported as refused, with its counts.  A size
that was not run appears in the output file as "not timed yet".

The committed profile:  gpu_edit_time.py --out profiles/edit_times.json [--sizes 100000000]"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 5
LIMIT, HLIMIT = 1 << 31, 1 << 27
SIZES, NQ = (100_000_000, 1_000_000_000), 1 << 20
KINDS = {"dna": 900, "english": 900}                          # seconds allowed per (kind, size)
ROWS = ((32, 1), (32, 2), (100, 2), (100, 4))


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
    """-> qbytes (nq, m) uint8: the even rows sampled with 0 .. k + 1 edits, the odd ones random."""
    g = np.random.default_rng(seed)
    n = text.size
    alphabet = np.unique(text[:1 << 16])
    at = g.integers(0, n - m - 2, nq)
    pats = text[at[:, None] + np.arange(m)[None, :]]
    odd = np.arange(1, nq, 2)
    pats[odd] = alphabet[g.integers(0, alphabet.size, (odd.size, m))]
    edits = g.integers(0, k + 2, nq)
    for r in range(k + 1):
        rows = np.flatnonzero((edits > r) & (np.arange(nq) % 2 == 0))
        what, where = g.integers(0, 3, rows.size), g.integers(0, m, rows.size)
        sub = rows[what == 0]
        pats[sub, where[what == 0]] = alphabet[g.integers(0, alphabet.size, sub.size)]
        for j, w in zip(rows[what == 1].tolist(), where[what == 1].tolist()):      # a byte of the text left out
            pats[j, w:m - 1] = pats[j, w + 1:].copy()
            pats[j, m - 1] = text[at[j] + m]
        for j, w in zip(rows[what == 2].tolist(), where[what == 2].tolist()):      # a byte put in
            pats[j, w + 1:] = pats[j, w:m - 1].copy()
            pats[j, w] = alphabet[(j * 7) % alphabet.size]
    return np.ascontiguousarray(pats)


def run_kind(kind, n, nq):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import tempfile

    import numpy as np
    import torch
    import _devlib
    import _edit as E
    import _gen
    from suffix_amd import device as sdev
    eng = _devlib.engine()
    eng.require_device()
    chk = E.build_checker(tempfile.mkdtemp())
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

    def verify(pats, m, k, res):
        """tests/ed_check.c over every quadruple (no sweep), on the packed patterns."""
        t = np.ascontiguousarray(text)
        qb = np.ascontiguousarray(pats.reshape(-1))
        qoff = np.arange(0, (pats.shape[0] + 1) * m, m, dtype=np.uint64)
        first, pat, tb, te, dist = (np.ascontiguousarray(x) for x in res)
        where = ctypes.c_int64(-2)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = chk.ed_check(p(t), t.size, None, 0, p(qb), p(qoff), pats.shape[0], k, p(pat), p(tb), p(te), p(dist), pat.size, p(first), None,
                          ctypes.byref(where))
        assert rc == 0, (chk.ed_check_name(rc), where.value)

    for m, k in ROWS:
        pats = make_patterns(np, text, m, k, nq, seed=1000 * m + k)
        dq = torch.from_numpy(pats.reshape(-1)).cuda()
        doff = torch.arange(0, (nq + 1) * m, m, dtype=torch.int64, device="cuda")
        row = {"kind": kind, "n": n, "patterns": nq, "m": m, "k": k, "library": os.path.basename(eng.path), "gather1_G_lines_per_s": gather,
               "cand_limit": LIMIT, "hit_limit": HLIMIT}
        # the k-mismatch search at the same (T, m, k)
        try:
            hm = ix.hamming(dq, doff, k, max_candidates=LIMIT)
            torch.cuda.synchronize()
            hz = int(hm[1].numel())
            hws = sdev.hamming_workspace(nq, k, min(LIMIT, nq * (k + 1) * n), "cuda", eng)
            hcall = lambda: ix.hamming(dq, doff, k, max_candidates=LIMIT, capacity=max(hz, 1), workspace=hws)
            hcall()
            torch.cuda.synchronize()
            hsteps = profiled(hcall)
            row["hamming"] = {"C": hm[4], "Z": hz, "call_ms": timed(torch, hcall), "hm_count_ms": hsteps.get("hm_count"),
                              "candidates_per_s": round(hm[4] / (hsteps["hm_count"] * 1e-3)) if hsteps.get("hm_count") else None}
            del hm, hws
        except Exception as e:                                            # noqa: BLE001 (a refusal names its count)
            row["hamming"] = {"refused": True, "message": str(e)[:200]}
        try:
            got = ix.edit_search(dq, doff, k, max_candidates=LIMIT, max_hits=HLIMIT)
        except Exception as e:                                            # noqa: BLE001 (a refusal names its count)
            words = [w for w in str(e).replace(";", " ").split() if w.isdigit()]
            row.update(refused=True, count=int(words[0]) if words else None, message=str(e)[:200])
            print(json.dumps(row), flush=True)
            continue
        torch.cuda.synchronize()
        res = [got[0].cpu().numpy().view(np.uint64)] + [got[c].cpu().numpy().view(np.uint32) for c in (1, 2, 3)] + [got[4].cpu().numpy()]
        verify(pats, m, k, res)
        C, H, Z = got[5], got[6], int(res[1].size)
        del got
        ws = sdev.edit_workspace(nq, k, min(LIMIT, nq * (k + 1) * n), min(HLIMIT, LIMIT * (2 * k + 1)), "cuda", eng)
        call = lambda: ix.edit_search(dq, doff, k, max_candidates=LIMIT, max_hits=HLIMIT, capacity=max(Z, 1), workspace=ws)
        call()
        torch.cuda.synchronize()
        row.update(C=C, H=H, Z=Z, verified=True, call_ms=timed(torch, call))
        steps = profiled(call)
        search = sum(v for name, v in steps.items() if name.startswith("query_"))
        merge = sum(v for name, v in steps.items() if name.startswith("radix_") or name in ("ed_heads", "ed_reduce", "ed_first"))
        row.update(steps_ms=steps, piece_search_ms=round(search, 4), ed_count_ms=steps.get("ed_count"), ed_emit_ms=steps.get("ed_emit"),
                   sort_reduce_ms=round(merge, 4),
                   candidates_per_s=round(C / (steps["ed_count"] * 1e-3)) if steps.get("ed_count") else None)
        del ws
        print(json.dumps(row), flush=True)
    torch.cuda.synchronize()
    ix.close()


def main(argv):
    sizes, kind, n, out_path, only, nq = list(SIZES), None, None, None, None, NQ
    i = 0
    while i < len(argv):
        if argv[i] == "--sizes" and i + 1 < len(argv):
            sizes = [int(x) for x in argv[i + 1].split(",")]; i += 2
        elif argv[i] == "--kind" and i + 1 < len(argv):
            kind = argv[i + 1]; i += 2
        elif argv[i] == "--n" and i + 1 < len(argv):
            n = int(argv[i + 1]); i += 2
        elif argv[i] == "--patterns" and i + 1 < len(argv):
            nq = int(argv[i + 1]); i += 2
        elif argv[i] == "--out" and i + 1 < len(argv):
            out_path = argv[i + 1]; i += 2
        elif argv[i] == "--only" and i + 1 < len(argv):
            only = argv[i + 1].split(","); i += 2
            if not all(o in KINDS for o in only):
                raise SystemExit(__doc__)
        else:
            raise SystemExit(__doc__)
    if kind:
        run_kind(kind, n or SIZES[0], nq)
        return 0
    names = [k for k in KINDS if only is None or k in only]
    results, failed = [], False
    not_timed = [{"kind": k, "n": s, "status": "not timed yet"} for s in SIZES for k in KINDS if s not in sizes or k not in names]

    def save():
        if out_path:                                           # (kept after every text: a later one may run out of time)
            with open(out_path, "w") as fh:
                json.dump({"source": f"scripts/gpu_edit_time.py: device events and the library's profiler, the median of {REPS} runs after a "
                                     "warm-up; every answer through tests/ed_check.c first",
                           "library": os.path.basename(os.environ.get("SFX_DEV_LIB") or "libsuffix_hip.so"), "patterns": nq,
                           "rows": results, "not_timed_yet": not_timed}, fh, indent=1)
                fh.write("\n")
    save()
    for size in sizes:
        for name in names:
            r = subprocess.run(["timeout", "-k", "10", str(KINDS[name]), sys.executable, os.path.abspath(__file__), "--kind", name,
                                "--n", str(size), "--patterns", str(nq)], capture_output=True, text=True)
            sys.stderr.write(r.stderr[-2000:])
            rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
            for row in rows:
                print(json.dumps(row), flush=True)
            results += rows
            if r.returncode != 0:                              # a fault, an abort or a time limit: start nothing more
                print(f"{name} {size}: exit status {r.returncode}; stopping", flush=True)
                not_timed.append({"kind": name, "n": size, "status": f"not timed yet (the run ended with status {r.returncode} after {len(rows)} rows)"})
                failed = True
            save()
            if failed:
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
