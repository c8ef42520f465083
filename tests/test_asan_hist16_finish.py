"""k_hist16_finish under AddressSanitizer: tests/asan_hist16_finish.cpp, a stand-alone program (its own main, the emulator build
of the kernels linked in, nothing preloaded), built by tests/emu/asan_hist16.mk and run as two child processes -- the workgroups
in index order and in reverse (the hooks are read once per process).  It sets the hooks itself and compares every table with a
std::sort of the suffixes."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")


@pytest.fixture(scope="module")
def program():
    cxx = "clang++" if shutil.which("clang++") else "g++"
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU, "-f", "asan_hist16.mk", f"ASAN_CXX={cxx}"])
    return os.path.join(EMU, "asan", "cp", "asan_hist16_finish")


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_hist16_finish_under_address_sanitizer(program, order):
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD" and not k.startswith("SFX_")}
    r = subprocess.run([program, order], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and f"asan_hist16_finish ok: {order}, 4 cases" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
