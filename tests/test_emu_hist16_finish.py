"""k_hist16_finish on the CPU emulator: 32 columns of 2048 sub-buckets, each finished by whichever of its 8 workgroups arrives
last at the column's ticket, and the whole by whichever column arrives last at the grid's.

The emulator runs workgroups in index order, so without help the last stretch's workgroup would finish every column and column 31
the whole; SFX_FINISH_REVERSE=1 maps workgroup i to the work of grid - 1 - i, and then the FIRST stretch finishes every column
and column 0 the whole.  Every case runs in both orders.  SFX_MAX_GRID=3: three partial histograms, so five of the eight
stretches hold no rows at all.  The hooks are read once per process: one subprocess per setting, started together.

Cases (SA and LCP against the oracle, radix_hist16_text and radix_hist16_finish among the profiled names):
  - uniform texts of 1, 2, 4 and 8 bits per symbol at n = 2 * 16384 + r, r in {0, 1, spw - 1, spw, spw + 1}, and one of
    9 * 16384 + 3 spw + 5 per width;
  - a 4-bit text whose lowest and highest symbol occur once each, as the last two bytes: the first and the last column are
    empty, their neighbours hold one suffix each;
  - skewed DNA on which the route gives way by its statistics and the four-pass sort takes its digit totals from the histogram
    (radix_window_from_hist16: totals_lo and totals_hi);
  - (SFX_HYBRID_CAP=100, a setting of its own) a text with a planted sub-bucket of ~300 suffixes: oversized sub-buckets exist,
    statistics words 2 and 3 steer the route (oversize_gather)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

UNIT = 16384
WIDTHS = {"sigma2": (2, 32), "dna": (4, 16), "sigma16": (16, 8), "bytes8": (200, 4)}   # name -> (sigma, spw)


def lengths(spw):
    return sorted({2 * UNIT + r for r in (0, 1, spw - 1, spw, spw + 1)})


def empty_end_columns():
    sys.path.insert(0, HERE)
    import _gen
    n = 2 * UNIT + 77
    t = _gen.uniform_bytes(n, 14, 1201, base=41).copy()
    t[n - 2] = 40
    t[n - 1] = 55
    return t.tobytes()


def skewed_dna():
    sys.path.insert(0, HERE)
    import _routes
    return _routes.skewed(3 * UNIT + 11, 4, 1301, 0.2).tobytes()


def planted_oversized():
    sys.path.insert(0, HERE)
    import _gen
    base = _gen.dna(40000, seed=5).tobytes()
    tails = _gen.dna(300 * 7, seed=6).tobytes()
    block = b"GATTACAGC"
    return base + b"".join(block + tails[7 * k:7 * k + 7] for k in range(300))


def texts(which):
    """(name, bytes, profile names the build must show) of every case of a setting; deterministic."""
    sys.path.insert(0, HERE)
    import _gen
    hist = ("radix_hist16_text", "radix_hist16_finish")
    if which == "cap":
        return [("planted-oversized", planted_oversized(), hist + ("oversize_gather",))]
    out = []
    for name, (sigma, spw) in WIDTHS.items():
        for i, n in enumerate(lengths(spw)):
            out.append((f"{name}-{n}", _gen.uniform_bytes(n, sigma, 131 + i, base=40).tobytes(), hist))
        n = 9 * UNIT + 3 * spw + 5
        out.append((f"{name}-{n}", _gen.uniform_bytes(n, sigma, 177, base=40).tobytes(), hist))
    out.append(("empty-end-columns", empty_end_columns(), hist))
    out.append(("skewed-dna", skewed_dna(), hist + ("radix_window_from_hist16",)))
    return out


SCRIPT = r"""
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {here!r})
import numpy as np
import torch
import oracle
import test_emu_hist16_finish as hf
from suffix_amd import Engine
from suffix_amd import device as sdev
oracle.build()
eng = Engine(os.path.join({here!r}, "emu", "libsuffix_emu.so"))
for name, t, must in hf.texts(sys.argv[1]):
    exp = oracle.sais(t)
    want = oracle.lcp_kasai(t, exp)
    eng.profile(True); eng.profile_reset()
    sa, lcp = sdev.build_sa_lcp(torch.frombuffer(bytearray(t), dtype=torch.uint8), engine=eng)
    names = set(r["name"] for r in eng.profile_report())
    eng.profile(False)
    assert names >= set(must), (name, sorted(names))
    assert np.array_equal(sa.numpy().view(np.uint32), exp), ("SA", name)
    assert np.array_equal(lcp.numpy().view(np.uint32), want), ("LCP", name)
print("OK")
"""

SETTINGS = {
    "forward": ("all", {}),
    "reverse": ("all", {"SFX_FINISH_REVERSE": "1"}),
    "cap-forward": ("cap", {"SFX_HYBRID_CAP": "100"}),
    "cap-reverse": ("cap", {"SFX_HYBRID_CAP": "100", "SFX_FINISH_REVERSE": "1"}),
}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(HERE, "emu")])
    script = tmp_path_factory.mktemp("hist16_finish") / "finish.py"
    script.write_text(SCRIPT.format(root=ROOT, here=HERE))
    procs = {}
    for name, (which, extra) in SETTINGS.items():
        base = {k: v for k, v in os.environ.items() if not k.startswith("SFX_")}
        env = dict(base, SFX_TINY="0", SFX_HYBRID_MIN="1", SFX_MAX_GRID="3", **extra)
        procs[name] = subprocess.Popen([sys.executable, str(script), which], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    yield procs
    for p in procs.values():
        if p.poll() is None:
            p.kill()


def test_the_texts_are_what_the_cases_say():
    sys.path.insert(0, HERE)
    import _routes
    t = empty_end_columns()
    a = np.frombuffer(t, dtype=np.uint8)
    assert _routes.predict(t)["sigma"] == 16 and (a == 40).sum() == 1 and (a == 55).sum() == 1 and t[-2:] == bytes([40, 55])
    s = skewed_dna()
    largest, slow = _routes.top16_histogram(s)
    assert largest > 4096 and largest < 65536 and slow * 64 > len(s), (largest, slow)        # gives way, and no counter wraps
    p = planted_oversized()
    largest, slow = _routes.top16_histogram(p)
    assert 100 < largest < 400 and slow == 0, (largest, slow)
    for name, (sigma, spw) in WIDTHS.items():
        ns = lengths(spw)
        assert 2 * UNIT in ns and 2 * UNIT + 1 in ns and len(ns) == 5, (name, ns)


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_hist16_finish_on_the_emulator(runs, setting):
    out, err = runs[setting].communicate(timeout=1500)
    assert runs[setting].returncode == 0 and out.strip().endswith("OK"), (out[-2000:], err[-4000:])
