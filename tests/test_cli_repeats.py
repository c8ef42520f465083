"""`suffix-array FILE --repeats L [--earlier]` (tools/suffix_array.cpp over include/suffix_table.hpp): one "begin end" line
per repeated span.  CPU: linked against the emulator build of the ABI; GPU: against libsuffix_hip.so."""
import os
import subprocess

import pytest

import _gen

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "tools", "suffix_array.cpp")


def _build(tmp_path, libdir, libname):
    exe = str(tmp_path / f"suffix-array-{libname}")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), SRC,
                           "-L", libdir, f"-l{libname}", f"-Wl,-rpath,{libdir}", "-o", exe])
    return exe


def _spans(exe, path, *opts):
    out = subprocess.run([exe, str(path), *opts], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("Suffixes: ")
    return [tuple(int(x) for x in ln.split()) for ln in lines[1:]]


def _exercise(exe, tmp_path):
    (tmp_path / "banana.txt").write_bytes(b"banana")
    assert _spans(exe, tmp_path / "banana.txt", "--repeats", "2") == [(1, 6)]
    assert _spans(exe, tmp_path / "banana.txt", "--repeats", "2", "--earlier") == [(3, 6)]
    assert _spans(exe, tmp_path / "banana.txt", "--repeats", "4", "--earlier") == []
    # a text with planted copies (no 100 bytes of it repeat otherwise)
    base = _gen.english_like(3000, seed=12).tobytes()
    text = base + b"#" + base[500:900] + b"%" + base[2000:2100]
    (tmp_path / "copies.txt").write_bytes(text)
    got = _spans(exe, tmp_path / "copies.txt", "--repeats", "100", "--earlier")
    assert got == [(3001, 3401), (3402, 3502)]
    both = _spans(exe, tmp_path / "copies.txt", "--repeats", "100")
    assert both == [(500, 900), (2000, 2100), (3001, 3401), (3402, 3502)]
    bad = subprocess.run([exe, str(tmp_path / "banana.txt"), "--repeats", "0"], capture_output=True, text=True)
    assert bad.returncode == 1 and "--repeats" in bad.stderr


def test_cli_repeats_on_emulator(tmp_path):
    emu = os.path.join(HERE, "emu")
    subprocess.check_call(["make", "-s", "-j8", "-C", emu])
    _exercise(_build(tmp_path, emu, "suffix_emu"), tmp_path)


@pytest.mark.gpu
def test_cli_repeats_on_gpu(tmp_path):
    _exercise(_build(tmp_path, os.path.join(ROOT, "suffix_amd"), "suffix_hip"), tmp_path)
