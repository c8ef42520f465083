"""`suffix-array FILE --lz PREFIX [--min-len L]` and `suffix-array PREFIX.lz --unlz --out OUT` (tools/suffix_array.cpp
over suffix::SuffixTable::lz77 / suffix::unlz): the round trip on disk, the printed phrase count against
SuffixTable.lz77, and damaged files.  CPU: linked against the emulator build of the ABI; GPU: against libsuffix_hip.so."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _gen
import _lz as Z
from suffix_amd import Engine, SuffixTable, default_engine
from test_cli_repeats import _build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _run(exe, *args):
    return subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=600)


def _exercise(exe, tmp_path, eng, orc):
    text = _gen.english_like(20_000).tobytes() + b"\x00\xff" + _gen.english_like(3_000).tobytes()
    src, pre, back = tmp_path / "in.txt", tmp_path / "f", tmp_path / "back.txt"
    src.write_bytes(text)
    sa, _ = Z.table_of(orc, text)
    for opts, m in (((), 1), (("--min-len", "8"), 8)):
        out = _run(exe, src, "--lz", pre, *opts)
        assert out.returncode == 0, out.stderr
        f = SuffixTable.from_parts(text, sa, engine=eng).lz77(m)
        want = f"LZ77: z {len(f)}, literals {int((f.src == Z.NONE).sum())}, longest {int(f.len.max())}"
        assert out.stdout.splitlines()[-1] == want, (out.stdout, want)
        raw = (tmp_path / "f.lz").read_bytes()
        z = len(f)
        assert raw[:8] == b"SFXLZ1\x00\x00" and struct.unpack("<II", raw[8:16]) == (len(text), z) and len(raw) == 16 + 9 * z
        ln = np.frombuffer(raw, dtype=np.uint32, count=z, offset=16)
        sr = np.frombuffer(raw, dtype=np.uint32, count=z, offset=16 + 4 * z)
        Z.check_phrases(text, Z.lpf(text), m, None, ln, sr, raw[16 + 8 * z:], "cli")
        if back.exists():
            back.unlink()
        got = _run(exe, tmp_path / "f.lz", "--unlz", "--out", back)
        assert got.returncode == 0 and got.stdout.strip() == f"Restored: {len(text)} bytes", (got.stdout, got.stderr)
        assert back.read_bytes() == text
    # damaged files: truncated, a wrong magic, a wrong n, a forward copy, a zero length -- status 2, no output file
    z = struct.unpack("<I", raw[12:16])[0]
    k = next(i for i in range(z) if sr[i] != Z.NONE)
    fwd = bytearray(raw)
    fwd[16 + 4 * z + 4 * k:16 + 4 * z + 4 * k + 4] = struct.pack("<I", len(text) - 1)
    zero = bytearray(raw)
    zero[16 + 4 * k:16 + 4 * k + 4] = struct.pack("<I", 0)
    for name, blob in (("truncated", raw[:-5]), ("short", raw[:11]), ("magic", b"SFXLZ2\x00\x00" + raw[8:]),
                       ("n", raw[:8] + struct.pack("<I", len(text) + 1) + raw[12:]), ("forward", bytes(fwd)), ("zero", bytes(zero))):
        p, o = tmp_path / (name + ".lz"), tmp_path / (name + ".out")
        p.write_bytes(blob)
        got = _run(exe, p, "--unlz", "--out", o)
        assert got.returncode == 2 and "corrupted" in got.stderr and not o.exists(), (name, got.returncode, got.stderr)
    got = _run(exe, tmp_path / "f.lz", "--unlz")
    assert got.returncode == 1 and "--out" in got.stderr
    got = _run(exe, src, "--lz", pre, "--min-len", "0")
    assert got.returncode == 1


def test_cli_lz_on_emulator(tmp_path, oracle):
    lib = Z.build_emulator()
    _exercise(_build(tmp_path, os.path.dirname(lib), "suffix_emu"), tmp_path, Engine(lib), oracle)


@pytest.mark.gpu
def test_cli_lz_on_gpu(tmp_path, oracle):
    _exercise(_build(tmp_path, os.path.join(ROOT, "suffix_amd"), "suffix_hip"), tmp_path, default_engine(), oracle)
