"""The small launches of the hybrid build (round 10: the alphabet stage inside k_byte_presence, k_hist16_finish's sums without
atomics, the counter lines of the tie kernels) under AddressSanitizer: tests/asan_small_launches.cpp, a stand-alone program (its
own main, the emulator build of the kernels linked in, nothing preloaded), built by tests/emu/asan_small.mk and run as four
child processes -- grid caps 3 (stretches of one row or none) and 24 (three rows per stretch: the summed path), the workgroups
in index order and in reverse (the hooks are read once per process).  It sets the hooks itself and compares every table with a
std::sort of the suffixes."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CASES = {"3": 7, "24": 3}


@pytest.fixture(scope="module")
def program():
    cxx = "clang++" if shutil.which("clang++") else "g++"
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU, "-f", "asan_small.mk", f"ASAN_CXX={cxx}"])
    return os.path.join(EMU, "asan", "cp", "asan_small_launches")


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("cap", sorted(CASES))
def test_small_launches_under_address_sanitizer(program, cap, order):
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD" and not k.startswith("SFX_")}
    r = subprocess.run([program, cap, order], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and f"asan_small_launches ok: cap {cap}, {order}, {CASES[cap]} cases" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
