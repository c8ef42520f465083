"""The compact-staging text-fed partition pass under AddressSanitizer: tests/asan_compact_partition.cpp, a stand-alone program
(its own main, the emulator build of the kernels linked in, nothing preloaded), built by tests/emu/asan_compact.mk and run as a
child process.  It sets the hooks itself and compares every table with a std::sort of the suffixes."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")


def test_compact_partition_under_address_sanitizer():
    cxx = "clang++" if shutil.which("clang++") else "g++"
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU, "-f", "asan_compact.mk", f"ASAN_CXX={cxx}"])
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD" and not k.startswith("SFX_")}
    r = subprocess.run([os.path.join(EMU, "asan", "cp", "asan_compact_partition")], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "asan_compact_partition ok: 7 cases" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
