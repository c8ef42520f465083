"""`suffix-array FILE --runs [--min-period P] [--max-period Q] [--min-len L]` and `suffix-array FILE --lyndon`
(tools/suffix_array.cpp over include/suffix_table.hpp): one `begin end period` line per maximal repetition, one line per
Lyndon factor start, line for line equal to the definition (tests/_runs.py's `brute`, Duval's algorithm).  CPU: linked
against the emulator build of the ABI; GPU: against libsuffix_hip.so."""
import os
import random
import subprocess

import pytest

import _runs as R
from test_cli_repeats import _build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _lines(exe, path, *opts):
    out = subprocess.run([exe, str(path), *opts], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("Suffixes: ")
    return lines[1], [tuple(int(x) for x in ln.split()) for ln in lines[2:]]


def duval(text):
    """The starts of the Lyndon factors of `text` (Duval 1983), straight on the bytes."""
    n, i, out = len(text), 0, []
    while i < n:
        j, k = i + 1, i
        while j < n and text[k] <= text[j]:
            k = i if text[k] < text[j] else k + 1
            j += 1
        while i <= k:
            out.append(i)
            i += j - k
    return out


def _exercise(exe, tmp_path):
    rng = random.Random(17)
    texts = [t for t, _ in R.KNOWN] + [b"a", b"\x00\xff\x00\xff\xff"]
    texts += [bytes(rng.randrange(rng.choice((1, 2, 3, 4))) + 97 for _ in range(rng.randint(1, 200))) for _ in range(20)]
    assert duval(b"banana") == [0, 1, 3, 5]
    for i, text in enumerate(texts):
        path = tmp_path / f"t{i}.bin"
        path.write_bytes(text)
        want = R.brute(text)
        head, got = _lines(exe, path, "--runs")
        assert head == f"Runs: {len(want)}" and got == want, (text, got[:5], want[:5])
        head, got = _lines(exe, path, "--lyndon")
        assert head == f"Lyndon factors: {len(duval(text))}" and [g[0] for g in got] == duval(text), text
        if i % 4 == 0 or i < len(R.KNOWN):
            for opts, flt in ((("--min-period", "2"), (2, None, 0)), (("--max-period", "2"), (1, 2, 0)), (("--min-len", "5"), (1, None, 5)),
                              (("--min-period", "2", "--max-period", "5", "--min-len", "6"), (2, 5, 6)),
                              (("--min-period", "4", "--max-period", "3"), (4, 3, 0))):
                want = R.brute(text, *flt)
                head, got = _lines(exe, path, "--runs", *opts)
                assert head == f"Runs: {len(want)}" and got == want, (text, opts, got[:5], want[:5])
    assert [r for t, r in R.KNOWN if t == b"mississippi"][0] == _lines(exe, tmp_path / "t0.bin", "--runs")[1]
    for args in (["--min-period", "2"], ["--max-period", "7"]):
        bad = subprocess.run([exe, str(tmp_path / "t0.bin"), *args], capture_output=True, text=True)
        assert bad.returncode == 1 and "--runs" in bad.stderr and "Suffixes" not in bad.stdout, (args, bad.stderr)
    bad = subprocess.run([exe, str(tmp_path / "t0.bin"), "--runs", "--min-period", "0"], capture_output=True, text=True)
    assert bad.returncode == 1 and "--min-period" in bad.stderr


def test_cli_runs_on_emulator(tmp_path):
    _exercise(_build(tmp_path, os.path.dirname(R.build_emulator()), "suffix_emu"), tmp_path)


@pytest.mark.gpu
def test_cli_runs_on_gpu(tmp_path):
    _exercise(_build(tmp_path, os.path.join(ROOT, "suffix_amd"), "suffix_hip"), tmp_path)
