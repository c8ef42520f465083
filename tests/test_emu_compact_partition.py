"""The compact-staging text-fed partition pass (k_partition_text) on the CPU emulator: a thread's words in registers and in an LDS
copy of the tile's packed text, digits out of the registers, 16-bit tile-local indices in the stage, elements rebuilt from the
LDS copy on their way out; the short last tile of a stretch with its positions behind the end kept out of masks and counts.

With T the shipped tile (16384 positions: 32 per thread x 512 threads): every symbol width the kernel takes (1, 2, 4 and 8 bits:
32, 16, 8 and 4 symbols per packed word) and one it does not (sigma = 5, 3 bits: the generic k_partition loop), at lengths
n = 2 T + r for r in {0, 1, spw - 1, spw, spw + 1} -- the last tile is full, holds one element, or ends inside a packed word --
and one text of 9 T + 3 spw + 5 positions per width, which fills several stretches and leaves the last one short.
SFX_MAX_GRID=3: a workgroup takes several tiles, so the prefetch crosses the ends of stretches and runs into "no next tile".
One DNA text whose last positions all carry the largest code at n = 2 T + 15: their windows reach the spare words behind the
text, and a window read one word short sorts them wrong.  The key forms: the default (SrcText36, one more symbol in the
element) and SFX_HYBRID_KEY36=0 (SrcText32) -- the hooks are read once per process, so each setting has its own subprocess.

The same kernel under AddressSanitizer: tests/test_asan_compact_partition.py."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

TILE = 16384                     # positions per tile of k_partition_text (kCompactKPT = 32 per thread x 512 threads)
WIDTHS = {"sigma2": (2, 32), "dna": (4, 16), "sigma16": (16, 8), "bytes8": (200, 4), "sigma5": (5, 10)}   # name -> (sigma, spw)


def lengths(spw, k=2):
    return sorted({TILE * k + r for r in (0, 1, spw - 1, spw, spw + 1)})


def _gen():
    sys.path.insert(0, HERE)
    import _gen
    return _gen


def texts():
    """(name, bytes) of every case of the default key form; deterministic."""
    g = _gen()
    out = []
    for name, (sigma, spw) in WIDTHS.items():
        for i, n in enumerate(lengths(spw)):
            out.append((f"{name}-{n}", g.uniform_bytes(n, sigma, 131 + i, base=40).tobytes()))
        # several stretches, the last of them short: 9 full tiles and a partial one
        n = TILE * 9 + 3 * spw + 5
        out.append((f"{name}-{n}", g.uniform_bytes(n, sigma, 177, base=40).tobytes()))
    out.append(tail_text())
    return out


def tail_text():
    """DNA, n = 2 T + 15, the last 40 positions all the largest code: the windows of the last tile's 15 positions read the
    text's last word and the spare words behind it."""
    g = _gen()
    n = TILE * 2 + 15
    t = g.uniform_bytes(n, 4, 211, base=40).copy()
    t[-40:] = t.max()
    return (f"dna-tail-{n}", t.tobytes())


def key32_texts():
    """DNA through SrcText32 (SFX_HYBRID_KEY36=0): a full last tile, a short one that ends inside a word, several stretches."""
    g = _gen()
    out = [(f"dna32-{n}", g.uniform_bytes(n, 4, 251 + i, base=40).tobytes()) for i, n in enumerate((TILE * 2, TILE * 2 + 17))]
    n = TILE * 9 + 3 * 16 + 5
    out.append((f"dna32-{n}", g.uniform_bytes(n, 4, 277, base=40).tobytes()))
    out.append(tail_text())
    return out


SCRIPT = r"""
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {here!r})
import numpy as np
import torch
import oracle
import test_emu_compact_partition as cp
from suffix_amd import Engine
from suffix_amd import device as sdev
oracle.build()
eng = Engine(os.path.join({here!r}, "emu", "libsuffix_emu.so"))
for name, t in getattr(cp, {which!r})():
    exp = oracle.sais(t)
    want = oracle.lcp_kasai(t, exp)
    eng.profile(True); eng.profile_reset()
    sa, lcp = sdev.build_sa_lcp(torch.frombuffer(bytearray(t), dtype=torch.uint8), engine=eng)
    names = set(r["name"] for r in eng.profile_report())
    eng.profile(False)
    assert names >= set(("radix_hist16_text", "radix_hist16_finish", "radix_scatter_text_u32")), (name, sorted(names))
    assert np.array_equal(sa.numpy().view(np.uint32), exp), ("SA", name)
    assert np.array_equal(lcp.numpy().view(np.uint32), want), ("LCP", name)
print("OK")
"""


def run_texts(tmp_path, which, **hooks):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(HERE, "emu")])
    script = tmp_path / f"{which}.py"
    script.write_text(SCRIPT.format(root=ROOT, here=HERE, which=which))
    env = dict(os.environ, SFX_TINY="0", SFX_HYBRID_MIN="1", SFX_MAX_GRID="3", **hooks)
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-2000:], r.stderr[-4000:])


def test_lengths_cover_the_last_tile_shapes():
    for name, (sigma, spw) in WIDTHS.items():
        ns = lengths(spw)
        assert TILE * 2 in ns and TILE * 2 + 1 in ns and any(n % spw not in (0, 1) and n % TILE < spw for n in ns), (name, ns)


def test_tile_is_the_shipped_one():
    """TILE follows the kernel's geometry: 512 threads x kCompactKPT positions."""
    import re
    src = open(os.path.join(ROOT, "suffix_amd", "csrc", "sfx_radix.hip")).read()
    m = re.search(r"constexpr int kCompactKPT = (\d+)", src)
    assert m and int(m.group(1)) * 512 == TILE, m and m.group(0)


def test_compact_partition_every_width_on_the_emulator(tmp_path):
    run_texts(tmp_path, "texts")


def test_compact_partition_32_bit_key_form_on_the_emulator(tmp_path):
    run_texts(tmp_path, "key32_texts", SFX_HYBRID_KEY36="0")
