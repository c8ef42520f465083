"""`suffix-array FILE --match FILE2 --mems L [--unique] [--max-pairs P]` (tools/suffix_array.cpp over
include/suffix_table.hpp): the maximal exact matches between FILE2 and FILE, one `qpos tpos len` line each, equal to the
definition as a double loop (tests/_mem.py).  CPU: linked against the emulator build of the ABI; GPU: against
libsuffix_hip.so."""
import os
import random
import subprocess

import pytest

import _mem as E
from test_cli_repeats import _build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _mems(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("Suffixes: ")
    return lines[1], [tuple(int(x) for x in ln.split()) for ln in lines[2:]]


def _files(tmp_path):
    rng = random.Random(12)
    one = bytes(rng.choice(b"abc") for _ in range(70))
    two = bytearray(rng.choice(b"abcd") for _ in range(50))
    two[10:24] = one[30:44]
    p1, p2 = os.path.join(str(tmp_path), "one.txt"), os.path.join(str(tmp_path), "two.txt")
    with open(p1, "wb") as f:
        f.write(one)
    with open(p2, "wb") as f:
        f.write(bytes(two))
    return p1, p2, one, bytes(two)


def _exercise(exe, tmp_path):
    p1, p2, one, two = _files(tmp_path)
    for L in (1, 3, 6, 14, 40):
        for unique in (False, True):
            want = E.brute(one, two, L, unique=unique)
            head, got = _mems(exe, p1, "--match", p2, "--mems", str(L), *(["--unique"] if unique else []))
            assert got == want, (L, unique, got[:5], want[:5])
            assert head.startswith(f"MEMs with {p2} (>= {L} bytes{', unique' if unique else ''}): {len(want)} matches, "), head
    assert any(l >= 14 for _, _, l in E.brute(one, two, 14)) and E.brute(one, two, 40) == []
    pairs = int(_mems(exe, p1, "--match", p2, "--mems", "2")[0].split()[-2])
    head, got = _mems(exe, p1, "--match", p2, "--mems", "2", "--max-pairs", str(pairs))
    assert got == E.brute(one, two, 2)
    bad = subprocess.run([exe, p1, "--match", p2, "--mems", "2", "--max-pairs", str(pairs - 1)], capture_output=True, text=True)
    assert bad.returncode == 2 and str(pairs) in bad.stderr and "max_pairs" in bad.stderr, (bad.returncode, bad.stderr)
    bad = subprocess.run([exe, p1, "--match", p2, "--mems", "0"], capture_output=True, text=True)
    assert bad.returncode == 1 and "--mems" in bad.stderr
    bad = subprocess.run([exe, p1, "--mems", "3"], capture_output=True, text=True)
    assert bad.returncode == 1 and "--match" in bad.stderr
    for args in (["--match", p2, "--mems", "3", "--min-len", "5"], ["--match", p2, "--unique"], ["--match", p2, "--max-pairs", "9"]):
        bad = subprocess.run([exe, p1, *args], capture_output=True, text=True)
        assert bad.returncode == 1 and "--mems" in bad.stderr and "Suffixes" not in bad.stdout, (args, bad.stderr)


def test_cli_mems_on_emulator(tmp_path):
    _exercise(_build(tmp_path, os.path.dirname(E.build_emulator()), "suffix_emu"), tmp_path)


@pytest.mark.gpu
def test_cli_mems_on_gpu(tmp_path):
    _exercise(_build(tmp_path, os.path.join(ROOT, "suffix_amd"), "suffix_hip"), tmp_path)
