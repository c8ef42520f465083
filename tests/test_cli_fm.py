"""`suffix-array PREFIX.bwt --fm PREFIX.bwi --query Q...` (tools/suffix_array.cpp over suffix::FmIndex): the queries of
`suffix-array FILE --query Q...` answered from the transform on disk, line for line.  CPU: linked against the emulator
build of the ABI; GPU: against libsuffix_hip.so."""
import os
import subprocess

import pytest

import _bwt as B
import _gen
from test_cli_repeats import _build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _run(exe, *args):
    return subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=600)


def _exercise(exe, tmp_path, orc):
    text = _gen.english_like(50_000).tobytes()
    src, pre = tmp_path / "in.txt", tmp_path / "tr"
    src.write_bytes(text)
    sa = B.table_of(orc, text)
    words = [text[a:a + k].decode("ascii") for a, k in ((100, 3), (2000, 9), (31000, 24), (49990, 10), (0, 1))]
    queries = words + ["zq#zq", words[2] + "#", ""]                     # present, absent, empty
    qargs = [x for q in queries for x in ("--query", q)]
    ref = _run(exe, src, *qargs)
    assert ref.returncode == 0, ref.stderr
    want = [ln for ln in ref.stdout.splitlines() if ln.startswith("positions(")]
    assert len(want) == len(queries)
    # what the table route prints is the oracle's: count and the first eight positions
    for q, ln in zip(queries, want):
        s, e = orc.positions(text, sa, q.encode()) if q else (0, 0)
        assert ln.startswith(f'positions("{q}"): {e - s}'), ln
        if e > s:
            assert ln.split("[")[1].rstrip(".], ").split(", ") == [str(v) for v in sa[s:min(e, s + 8)]], ln
    assert sum(1 for ln in want if ln.endswith(": 0")) == 3 and any("..." in ln for ln in want)
    for step, opts in ((64, ("--step", "64")), (0, ("--step", "0")), (256, ())):
        out = _run(exe, src, "--bwt", pre, *opts)
        assert out.returncode == 0, out.stderr
        for occ in ((), ("--occ-step", "64"), ("--occ-step", "4096")):
            got = _run(exe, tmp_path / "tr.bwt", "--fm", tmp_path / "tr.bwi", *qargs, *occ)
            assert got.returncode == 0, got.stderr
            lines = got.stdout.splitlines()
            assert lines[0] == "Suffixes: 50000" and lines[1:] == want, (step, occ, lines)
    # a sample file that is none, missing files, a bad block size
    (tmp_path / "bad.bwi").write_bytes(b"\x40\x00\x00")
    out = _run(exe, tmp_path / "tr.bwt", "--fm", tmp_path / "bad.bwi", *qargs)
    assert out.returncode == 2 and "corrupted" in out.stderr
    out = _run(exe, tmp_path / "tr.bwt", "--fm", tmp_path / "absent.bwi", *qargs)
    assert out.returncode == 1 and "cannot read" in out.stderr
    out = _run(exe, tmp_path / "tr.bwt", "--fm", tmp_path / "tr.bwi", *qargs, "--occ-step", "48")
    assert out.returncode == 1 and "--occ-step" in out.stderr
    # a transform with the samples of another step: refused by the engine, status 2
    out = _run(exe, src, "--bwt", tmp_path / "other", "--step", "128")
    assert out.returncode == 0
    (tmp_path / "mixed.bwi").write_bytes(b"\x40\x00\x00\x00" + (tmp_path / "other.bwi").read_bytes()[4:])
    out = _run(exe, tmp_path / "tr.bwt", "--fm", tmp_path / "mixed.bwi", *qargs)
    assert out.returncode == 2 and "invalid argument" in out.stderr


def test_cli_fm_on_emulator(tmp_path, oracle):
    import _fm
    emu = os.path.dirname(_fm.build_emulator())
    _exercise(_build(tmp_path, emu, "suffix_emu"), tmp_path, oracle)


@pytest.mark.gpu
def test_cli_fm_on_gpu(tmp_path, oracle):
    _exercise(_build(tmp_path, os.path.join(ROOT, "suffix_amd"), "suffix_hip"), tmp_path, oracle)
