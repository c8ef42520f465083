"""`suffix-array FILE --query Q --mismatches K` (tools/suffix_array.cpp over include/suffix_table.hpp): the occurrences
of Q with up to K differing bytes, one `position<TAB>mismatches` line each, sorted by position, equal to the definition as
a double loop (tests/_hamming.py); at K = 0 the positions of the plain `--query Q`.  CPU: linked against the emulator build
of the ABI; GPU: against libsuffix_hip.so."""
import os
import random
import re
import subprocess

import pytest

import _hamming as H
from test_cli_repeats import _build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("Suffixes: ")
    return lines[1:]


def _approx(exe, path, queries, k):
    """-> per query [(position, mismatches)], parsed from the report."""
    args = [path]
    for q in queries:
        args += ["--query", q]
    lines = _run(exe, *args, "--mismatches", str(k))
    out, i = [], 0
    for q in queries:
        m = re.fullmatch(rf'approx_positions\("{re.escape(q)}", {k}\): (\d+)', lines[i])
        assert m, lines[i]
        z = int(m.group(1))
        rows = lines[i + 1:i + 1 + z]
        assert all(re.fullmatch(r"\d+\t\d+", r) for r in rows), rows[:3]
        out.append([tuple(int(x) for x in r.split("\t")) for r in rows])
        i += 1 + z
    assert i == len(lines)
    return out


def _exercise(exe, tmp_path):
    rng = random.Random(14)
    text = bytes(rng.choice(b"abc") for _ in range(160))
    text = text[:100] + text[20:50] + text[100:]
    path = os.path.join(str(tmp_path), "text.txt")
    with open(path, "wb") as f:
        f.write(text)
    sa = H.naive_table(text)
    planted = bytearray(text[22:46])
    planted[5] = ord("d")
    planted[17] = ord("d")
    queries = [text[22:46].decode(), planted.decode(), "abcabc", "ca", "dddd", "b"]
    for k in (0, 1, 2, 3):
        got = _approx(exe, path, queries, k)
        trip, first = H.brute(text, None, [q.encode() for q in queries], k, sa)
        for j, q in enumerate(queries):
            want = sorted((p, c) for _, p, c in trip[first[j]:first[j + 1]])
            assert got[j] == want, (q, k, got[j][:5], want[:5])
    assert len(_approx(exe, path, queries[:2], 2)[1]) == 2 and _approx(exe, path, queries[:2], 1)[1] == []
    # k = 0 against the existing --query report: the same count and the same positions
    exact = _run(exe, path, *[x for q in queries for x in ("--query", q)])
    got = _approx(exe, path, queries, 0)
    for j, q in enumerate(queries):
        m = re.fullmatch(rf'positions\("{re.escape(q)}"\): (\d+)(?: \[(.*)\])?', exact[j])
        assert m and int(m.group(1)) == len(got[j]), (exact[j], len(got[j]))
        assert all(c == 0 for _, c in got[j])
        listed = [int(x) for x in (m.group(2) or "").replace(", ...", "").split(", ") if x]
        assert set(listed) <= {p for p, _ in got[j]} and len(listed) == min(8, len(got[j])), (exact[j], got[j][:8])
    # with --lce the count keeps its meaning there and the queries stay exact
    both = _run(exe, path, "--query", "abcabc", "--lce", "20,100", "--mismatches", "1")
    assert both[0].startswith('positions("abcabc"): ') and re.fullmatch(r"20 100 \d+", both[1]), both
    for args, word in ((["--mismatches", "1"], "--lce"), (["--query", "ab", "--mismatches", "256"], "255"),
                       (["--query", "ab", "--mismatches", "-1"], "--mismatches")):
        bad = subprocess.run([exe, path, *args], capture_output=True, text=True)
        assert bad.returncode == 1 and word in bad.stderr and "Suffixes" not in bad.stdout, (args, bad.stderr)


def test_cli_hamming_on_emulator(tmp_path):
    _exercise(_build(tmp_path, os.path.dirname(H.build_emulator()), "suffix_emu"), tmp_path)


@pytest.mark.gpu
def test_cli_hamming_on_gpu(tmp_path):
    _exercise(_build(tmp_path, os.path.join(ROOT, "suffix_amd"), "suffix_hip"), tmp_path)
