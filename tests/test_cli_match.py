"""`suffix-array FILE --match FILE2 [--min-len L]` (tools/suffix_array.cpp over include/suffix_table.hpp): the spans of
FILE2 that also stand in FILE.  CPU: linked against the emulator build of the ABI; GPU: against libsuffix_hip.so."""
import os
import subprocess

import pytest

import _match as M
from test_cli_repeats import _build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _match(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("Suffixes: ")
    return lines[1], [tuple(int(x) for x in ln.split()) for ln in lines[2:]]


def _exercise(exe, tmp_path):
    one, two, long_, short = M.cli_files(tmp_path)
    head, spans = _match(exe, one, "--match", two)                          # the default: 32 bytes
    assert head == f"Shared with {two} (>= 32 bytes): 1 spans, 100 bytes" and spans == [long_]
    head, spans = _match(exe, one, "--match", two, "--min-len", "31")
    assert head == f"Shared with {two} (>= 31 bytes): 2 spans, 131 bytes" and spans == [long_, short]
    head, spans = _match(exe, one, "--match", two, "--min-len", "101")
    assert head.endswith("0 spans, 0 bytes") and spans == []
    bad = subprocess.run([exe, one, "--match", two, "--min-len", "0"], capture_output=True, text=True)
    assert bad.returncode == 1 and "--min-len" in bad.stderr
    bad = subprocess.run([exe, one, "--match", os.path.join(str(tmp_path), "absent")], capture_output=True, text=True)
    assert bad.returncode == 1 and "cannot read" in bad.stderr


def test_cli_match_on_emulator(tmp_path):
    emu = os.path.join(HERE, "emu")
    subprocess.check_call(["make", "-s", "-j8", "-C", emu])
    _exercise(_build(tmp_path, emu, "suffix_emu"), tmp_path)


@pytest.mark.gpu
def test_cli_match_on_gpu(tmp_path):
    _exercise(_build(tmp_path, os.path.join(ROOT, "suffix_amd"), "suffix_hip"), tmp_path)
