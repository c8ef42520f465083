#!/usr/bin/env python3
"""Out-of-bounds check of the text-fed front half of the hybrid initial sort: the texts of tests/test_emu_front_end.py (every
symbol width, last tiles that are full, one element long or end inside a packed word, stretches that end short or are empty)
through the AddressSanitizer build of the emulator.  The tile loader reads the words behind a thread's positions and requests the
next tile's words ahead of time: a read past the packed text would hide there.  Not part of the pytest suite; run by hand after
changes to k_partition, k_hist16_text or k_hist16_finish:

    make -C tests/emu asan
    LD_PRELOAD=$(clang++ -print-file-name=libclang_rt.asan-x86_64.so) \\
    ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0:halt_on_error=1 \\
    SFX_TINY=0 SFX_HYBRID_MIN=1 SFX_MAX_GRID=3 python tests/asan_front_end.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402

import oracle  # noqa: E402
import test_emu_front_end as fe  # noqa: E402
from suffix_amd import Engine, SuffixTable  # noqa: E402

assert os.environ.get("SFX_HYBRID_MIN") == "1" and os.environ.get("SFX_TINY") == "0", "see the docstring: the hybrid route on small texts"
oracle.build()
eng = Engine(os.path.join(HERE, "emu", "asan", "libsuffix_emu.so"))
for name, t in fe.texts():
    eng.profile(True)
    eng.profile_reset()
    got = SuffixTable(t, engine=eng).table()
    names = set(r["name"] for r in eng.profile_report())
    eng.profile(False)
    assert "radix_hist16_finish" in names and "radix_scatter_text_u32" in names, (name, sorted(names))
    assert np.array_equal(got, oracle.sais(t)), name
    print(name, "ok", flush=True)
print("front end ok")
