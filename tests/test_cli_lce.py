"""`suffix-array FILE --lce I,J[,I,J...] [--mismatches K]` and `--isa` (tools/suffix_array.cpp over
include/suffix_table.hpp): one `i j len` line per pair, equal to plain byte comparison (tests/_lce.py's `brute`); the
inverse table written by --dump is the inverse of the table written next to it.  CPU: linked against the emulator build
of the ABI; GPU: against libsuffix_hip.so."""
import os
import random
import subprocess

import numpy as np
import pytest

import _lce as L
from test_cli_repeats import _build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("Suffixes: ")
    return lines[1:]


def _exercise(exe, tmp_path):
    rng = random.Random(14)
    text = bytes(rng.choice(b"ab") for _ in range(90)) + b"abcabd" + b"a" * 40
    n = len(text)
    path = os.path.join(str(tmp_path), "text.txt")
    with open(path, "wb") as f:
        f.write(text)
    pairs = [(rng.randrange(n), rng.randrange(n)) for _ in range(40)] + [(90, 93), (0, 0), (n - 1, 5), (n, 3), (n + 1, 0), (100, 120)]
    arg = ",".join(f"{i},{j}" for i, j in pairs)
    for k in (None, 0, 1, 2, 7):
        got = _run(exe, path, "--lce", arg, *([] if k is None else ["--mismatches", str(k)]))
        want = [f"{i} {j} {L.brute(text, i, j, k or 0)}" for i, j in pairs]
        assert got == want, (k, [(g, w) for g, w in zip(got, want) if g != w][:4])
    assert _run(exe, path, "--lce", "90,93") == ["90 93 2"]                                # abcabda.. against abdaaa..: ab
    assert _run(exe, path, "--lce", "90,93", "--mismatches", "1") == ["90 93 4"]          # c against d stepped over, a, then b against a
    # --isa: the summary line, and with --dump the table's inverse
    prefix = os.path.join(str(tmp_path), "dump")
    lines = _run(exe, path, "--isa", "--dump", prefix)
    sa = np.fromfile(prefix + ".sa", dtype=np.uint32)
    isa = np.fromfile(prefix + ".isa", dtype=np.uint32)
    assert sa.tolist() == sorted(range(n), key=lambda p: text[p:]) and np.array_equal(isa, L.expected_isa(sa))
    assert lines == [f"ISA: rank of the whole text {int(isa[0])}, of its last byte {int(isa[-1])}"]
    for args, word in ((["--lce", "1,2,3"], "even"), (["--lce", "1,x"], "--lce"), (["--lce", "1,-2"], "--lce"), (["--lce", ""], "--lce"),
                       (["--mismatches", "2"], "--lce"), (["--lce", "1,2", "--mismatches", "-1"], "--mismatches")):
        bad = subprocess.run([exe, path, *args], capture_output=True, text=True)
        assert bad.returncode == 1 and word in bad.stderr and "Suffixes" not in bad.stdout, (args, bad.stderr)


def test_cli_lce_on_emulator(tmp_path):
    _exercise(_build(tmp_path, os.path.dirname(L.build_emulator()), "suffix_emu"), tmp_path)


@pytest.mark.gpu
def test_cli_lce_on_gpu(tmp_path):
    _exercise(_build(tmp_path, os.path.join(ROOT, "suffix_amd"), "suffix_hip"), tmp_path)
