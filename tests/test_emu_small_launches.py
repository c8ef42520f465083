"""The small launches of the hybrid build on the CPU emulator (round 10):
  - k_byte_presence's last workgroup writes the LUT and the 8 flag words of the alphabet (sharded tickets; no make_lut launch);
  - k_hist16_finish's workgroups store their stretch's sums over the stretch's first two rows and the column's last arriver adds
    eight of them (no atomics into the sub-bucket counts, which nobody zeroes any more);
  - k_tie_totals posts its words itself and leaves the counter lines zero, which the histogram sweep zeroed for it.

SFX_TINY=0 SFX_HYBRID_MIN=1 take texts of emulator size down the hybrid route.  The emulator runs workgroups in index order;
SFX_FINISH_REVERSE=1 maps workgroup i to the work of grid - 1 - i in every kernel with a last-arriver stage, so every setting
runs in both orders.  The hooks are read once per process: one subprocess per setting, started together.

Grid caps:
  - SFX_MAX_GRID=3: three partial histograms, stretches of one row or none -- the column stage reads packed rows;
  - SFX_MAX_GRID=24 at n = 24 * 16384 (4-bit symbols: 48 tiles, 24 rows, three per stretch) and at n = 24 * 16384 + 5 (8-bit
    symbols: 97 tiles, 20 rows -- six stretches of three rows, one of two, one empty): the summed path, and both in one column.

Texts under SFX_MAX_GRID=3 (SA and LCP against the oracle; radix_hist16_text and radix_hist16_finish among the profiled names,
make_lut not among them):
  - uniform texts of 1, 2, 4 and 8 bits per symbol at n = 2 * 16384 + r, r in {0, 1, spw - 1, spw, spw + 1}, and one of
    9 * 16384 + 3 spw + 5 per width;
  - a 3-bit alphabet (6 symbols: ten to a word, the generic pack kernel and the run-time sweep);
  - symbols that include the bytes 0x00 and 0xFF (the first and the last flag bit of the posted words);
  - skewed DNA on which the route gives way by its statistics (radix_window_from_hist16);
  - (SFX_HYBRID_CAP=100, a setting of its own) the planted oversized sub-bucket (oversize_gather).
Through the device entry point with guarded buffers (tests/_buffers.py), SA against the oracle:
  - a DNA text one byte behind a 16-byte boundary (the byte-wise presence loop);
  - the same build twice into one workspace, filled with 0xFF before each call: whatever must be zero on entry -- the tickets of
    the alphabet stage, the counter lines -- is zeroed inside the build."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

UNIT = 16384
WIDTHS = {"sigma2": (2, 32), "dna": (4, 16), "sigma16": (16, 8), "bytes8": (200, 4)}   # name -> (sigma, spw)
HIST = ("radix_hist16_text", "radix_hist16_finish")


def lengths(spw):
    return sorted({2 * UNIT + r for r in (0, 1, spw - 1, spw, spw + 1)})


def with_both_ends(n):
    """16 symbols, 0x00 and 0xFF among them."""
    sys.path.insert(0, HERE)
    import _gen
    t = _gen.uniform_bytes(n, 16, 907, base=0).copy()
    t[t == 15] = 0xFF
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
    if which == "cap":
        return [("planted-oversized", planted_oversized(), HIST + ("oversize_gather",))]
    if which == "rows3":
        return [("sigma16-rows3", _gen.uniform_bytes(24 * UNIT, 16, 311, base=40).tobytes(), HIST),
                ("bytes8-rows3-2-0", _gen.uniform_bytes(24 * UNIT + 5, 200, 312, base=40).tobytes(), HIST)]
    out = []
    for name, (sigma, spw) in WIDTHS.items():
        for i, n in enumerate(lengths(spw)):
            out.append((f"{name}-{n}", _gen.uniform_bytes(n, sigma, 231 + i, base=40).tobytes(), HIST))
        n = 9 * UNIT + 3 * spw + 5
        out.append((f"{name}-{n}", _gen.uniform_bytes(n, sigma, 277, base=40).tobytes(), HIST))
    out.append(("sigma6", _gen.uniform_bytes(2 * UNIT + 7, 6, 401, base=40).tobytes(), HIST))
    out.append(("bytes-00-ff", with_both_ends(2 * UNIT + 3), HIST))
    out.append(("skewed-dna", skewed_dna(), HIST + ("radix_window_from_hist16",)))
    return out


def device_texts(which):
    """(name, bytes, byte offset of the text behind a 16-byte boundary) for the calls through the device entry point."""
    sys.path.insert(0, HERE)
    import _gen
    if which == "rows3":
        return [("dna-rows3-twice", _gen.dna(24 * UNIT, seed=9).tobytes(), 0)]
    if which == "cap":
        return []
    return [("dna-unaligned", _gen.dna(2 * UNIT + 21, seed=7).tobytes(), 1), ("sigma16-twice", _gen.uniform_bytes(2 * UNIT + 9, 16, 403, base=40).tobytes(), 0)]


SCRIPT = r"""
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {here!r})
import numpy as np
import torch
import oracle
import _buffers
import test_emu_small_launches as sl
from suffix_amd import Engine
from suffix_amd import device as sdev
oracle.build()
eng = Engine(os.path.join({here!r}, "emu", "libsuffix_emu.so"))
for name, t, must in sl.texts(sys.argv[1]):
    exp = oracle.sais(t)
    want = oracle.lcp_kasai(t, exp)
    eng.profile(True); eng.profile_reset()
    sa, lcp = sdev.build_sa_lcp(torch.frombuffer(bytearray(t), dtype=torch.uint8), engine=eng)
    names = set(r["name"] for r in eng.profile_report())
    eng.profile(False)
    assert names >= set(must), (name, sorted(names))
    assert "make_lut" not in names, (name, sorted(names))
    assert np.array_equal(sa.numpy().view(np.uint32), exp), ("SA", name)
    assert np.array_equal(lcp.numpy().view(np.uint32), want), ("LCP", name)
for name, t, off in sl.device_texts(sys.argv[1]):
    exp = oracle.sais(t)
    eng.profile(True); eng.profile_reset()
    rc, b = _buffers.call_build_sa(eng, t, "cpu", text_off=off, fill=0xFF)
    for again in (0, 1):
        if again:                                   # the same buffers, dirty again: 0xFF over what the first build left
            b["workspace"].fill(0xFF); b["sa"].fill(0xFF)
            rc = eng.lib.sfx_build_sa_u32_dev(b["text"].ptr, len(t), b["sa"].ptr, b["workspace"].ptr, b["workspace"].nbytes, None)
        assert rc == _buffers.OK, (name, again, rc)
        got = b["sa"].host(np.uint32)
        assert np.array_equal(got, exp), ("SA", name, again, np.flatnonzero(got != exp)[:4])
        assert b["text"].host().tobytes() == t
        _buffers.check_all(b)
        assert eng.build_stats()["sigma"] == len(set(t)), (name, again, eng.build_stats())
    names = set(r["name"] for r in eng.profile_report())
    eng.profile(False)
    assert names >= set(sl.HIST) and "make_lut" not in names, (name, sorted(names))
print("OK")
"""

SETTINGS = {
    "forward": ("all", {"SFX_MAX_GRID": "3"}),
    "reverse": ("all", {"SFX_MAX_GRID": "3", "SFX_FINISH_REVERSE": "1"}),
    "cap-forward": ("cap", {"SFX_MAX_GRID": "3", "SFX_HYBRID_CAP": "100"}),
    "cap-reverse": ("cap", {"SFX_MAX_GRID": "3", "SFX_HYBRID_CAP": "100", "SFX_FINISH_REVERSE": "1"}),
    "rows3-forward": ("rows3", {"SFX_MAX_GRID": "24"}),
    "rows3-reverse": ("rows3", {"SFX_MAX_GRID": "24", "SFX_FINISH_REVERSE": "1"}),
}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(HERE, "emu")])
    script = tmp_path_factory.mktemp("small_launches") / "small.py"
    script.write_text(SCRIPT.format(root=ROOT, here=HERE))
    procs = {}
    for name, (which, extra) in SETTINGS.items():
        base = {k: v for k, v in os.environ.items() if not k.startswith("SFX_")}
        env = dict(base, SFX_TINY="0", SFX_HYBRID_MIN="1", **extra)
        procs[name] = subprocess.Popen([sys.executable, str(script), which], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    yield procs
    for p in procs.values():
        if p.poll() is None:
            p.kill()


def test_the_texts_are_what_the_cases_say():
    sys.path.insert(0, HERE)
    import _routes
    t = with_both_ends(2 * UNIT + 3)
    assert 0x00 in t and 0xFF in t and _routes.predict(t)["sigma"] == 16
    assert _routes.predict(texts("all")[-3][1])["bits"] == 3
    s = skewed_dna()
    largest, slow = _routes.top16_histogram(s)
    assert largest > 4096 and largest < 65536 and slow * 64 > len(s), (largest, slow)        # gives way, and no counter wraps
    p = planted_oversized()
    largest, slow = _routes.top16_histogram(p)
    assert 100 < largest < 400 and slow == 0, (largest, slow)
    # the rows of the partial counts under SFX_MAX_GRID=24: as many as fit the element buffer (n / 16384) and the cap, a tile =
    # 1024 packed words; three rows per stretch of eight
    for (name, text, _), spw, rows in zip(texts("rows3"), (8, 4), (24, 20)):
        n = len(text)
        tiles = ((n + spw - 1) // spw + 1023) // 1024
        most = min(n // UNIT, 24)
        per = (tiles + most - 1) // most
        assert (tiles + per - 1) // per == rows and (rows + 7) // 8 == 3, (name, n, tiles, most, per)
    for name, (sigma, spw) in WIDTHS.items():
        ns = lengths(spw)
        assert 2 * UNIT in ns and 2 * UNIT + 1 in ns and len(ns) == 5, (name, ns)


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_small_launches_on_the_emulator(runs, setting):
    out, err = runs[setting].communicate(timeout=1500)
    assert runs[setting].returncode == 0 and out.strip().endswith("OK"), (out[-2000:], err[-4000:])
