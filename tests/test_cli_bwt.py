"""`suffix-array FILE --bwt PREFIX [--step S]` and `suffix-array PREFIX.bwt --unbwt PREFIX.bwi --out OUT`
(tools/suffix_array.cpp over include/suffix_table.hpp): the transform of a file on disk and the file back from it.
CPU: linked against the emulator build of the ABI; GPU: against libsuffix_hip.so."""
import os
import subprocess

import numpy as np
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
    src, pre, back = tmp_path / "in.txt", tmp_path / "tr", tmp_path / "back.txt"
    src.write_bytes(text)
    sa = B.table_of(orc, text)
    for step, opts in ((256, ()), (64, ("--step", "64")), (0, ("--step", "0"))):
        out = _run(exe, src, "--bwt", pre, *opts)
        assert out.returncode == 0, out.stderr
        wb, ws = B.definition(text, sa, step)
        assert out.stdout.splitlines() == ["Suffixes: 50000", f"BWT: primary {ws[0]}, {ws.size} samples (step {step})"]
        assert (tmp_path / "tr.bwt").read_bytes() == wb.tobytes()
        bwi = np.frombuffer((tmp_path / "tr.bwi").read_bytes(), dtype="<u4")
        assert bwi[0] == step and np.array_equal(bwi[1:], ws)
        out = _run(exe, tmp_path / "tr.bwt", "--unbwt", tmp_path / "tr.bwi", "--out", back)
        assert out.returncode == 0 and out.stdout.splitlines() == ["Restored: 50000 bytes"], out.stderr
        assert back.read_bytes() == text
        back.unlink()
    # (step 64 is on disk) a corrupted .bwi: a changed sample, a changed step, a cut file -> status 2, nothing written
    wb, ws = B.definition(text, sa, 64)
    good = np.concatenate([[64], ws]).astype("<u4")
    bad = tmp_path / "bad.bwi"
    (tmp_path / "tr.bwi").write_bytes(good.tobytes())
    (tmp_path / "tr.bwt").write_bytes(wb.tobytes())
    for k, v in ((5, int(good[5]) ^ 1 or 2), (1, 0), (0, 128), (0, 48)):
        arr = good.copy()
        arr[k] = v
        bad.write_bytes(arr.tobytes())
        out = _run(exe, tmp_path / "tr.bwt", "--unbwt", bad, "--out", back)
        assert out.returncode == 2 and "corrupted" in out.stderr and not back.exists(), (k, v, out.stderr)
    bad.write_bytes(good.tobytes()[:-2])
    out = _run(exe, tmp_path / "tr.bwt", "--unbwt", bad, "--out", back)
    assert out.returncode == 2 and "corrupted" in out.stderr and not back.exists()
    # a corrupted .bwt
    flipped = bytearray(wb.tobytes())
    flipped[12345] ^= 0x20
    (tmp_path / "flip.bwt").write_bytes(bytes(flipped))
    out = _run(exe, tmp_path / "flip.bwt", "--unbwt", tmp_path / "tr.bwi", "--out", back)
    if out.returncode == 0:                                           # (then it IS the transform of what was written)
        got = back.read_bytes()
        vb, vs = B.definition(got, B.table_of(orc, got), 64)
        assert vb.tobytes() == bytes(flipped) and np.array_equal(vs, ws)
    else:
        assert out.returncode == 2 and "corrupted" in out.stderr and not back.exists()
    # missing files, bad options -> status 1
    for args in ((tmp_path / "absent", "--bwt", pre), (tmp_path / "absent.bwt", "--unbwt", tmp_path / "tr.bwi", "--out", back),
                 (tmp_path / "tr.bwt", "--unbwt", tmp_path / "absent.bwi", "--out", back)):
        out = _run(exe, *args)
        assert out.returncode == 1 and "cannot read" in out.stderr, args
    out = _run(exe, src, "--bwt", pre, "--step", "3")
    assert out.returncode == 1 and "--step" in out.stderr
    out = _run(exe, tmp_path / "tr.bwt", "--unbwt", tmp_path / "tr.bwi")
    assert out.returncode == 1 and "--out" in out.stderr


def test_cli_bwt_on_emulator(tmp_path, oracle):
    emu = os.path.join(HERE, "emu")
    subprocess.check_call(["make", "-s", "-j8", "-C", emu])
    _exercise(_build(tmp_path, emu, "suffix_emu"), tmp_path, oracle)


@pytest.mark.gpu
def test_cli_bwt_on_gpu(tmp_path, oracle):
    _exercise(_build(tmp_path, os.path.join(ROOT, "suffix_amd"), "suffix_hip"), tmp_path, oracle)
