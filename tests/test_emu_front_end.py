"""The text-fed front half of the hybrid initial sort on the CPU emulator: the tile loader of the first partition pass
(TextTileWords: a thread's 16 consecutive positions from one load of packed words, the next tile's words requested before the
current tile is ranked), the prefetching histogram sweep (k_hist16_text) and the one kernel between them (k_hist16_finish:
sub-bucket starts, digit totals, cursors and statistics).

Every symbol width the loader takes (1, 2, 4 and 8 bits: 32, 16, 8 and 4 symbols per packed word) and one it does not (sigma = 5,
3 bits: the retained src.key() loop), at lengths n = 8192 k + r with k = 2 and r in {0, 1, spw - 1, spw, spw + 1}: the last tile of
8192 positions is full, holds one element, or ends inside a packed word.  At these sizes the stretches of the input
(class_len) are longer than the text, so every stretch but the first is empty; one longer text per width fills several stretches
and leaves the last one short.  SFX_MAX_GRID=3: a workgroup takes several tiles, so the prefetch crosses the ends of stretches
and runs into "no next tile".  The environment hooks are read once per process: one subprocess for all texts.

The same texts run under AddressSanitizer through tests/asan_front_end.py (`make -C tests/emu asan`): a prefetch is where a read
past the packed text would hide."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

TILE = 8192                      # positions per tile of the 8-wave partition pass (16 per thread x 512 threads)
WIDTHS = {"sigma2": (2, 32), "dna": (4, 16), "sigma16": (16, 8), "bytes8": (200, 4), "sigma5": (5, 10)}   # name -> (sigma, spw)


def lengths(spw, k=2):
    return sorted({TILE * k + r for r in (0, 1, spw - 1, spw, spw + 1)})


def texts():
    """(name, bytes) of every case; deterministic."""
    sys.path.insert(0, HERE)
    import _gen
    out = []
    for name, (sigma, spw) in WIDTHS.items():
        for i, n in enumerate(lengths(spw)):
            out.append((f"{name}-{n}", _gen.uniform_bytes(n, sigma, 31 + i, base=40).tobytes()))
        # several stretches, the last of them short: 9 full tiles and a partial one
        n = TILE * 9 + 3 * spw + 5
        out.append((f"{name}-{n}", _gen.uniform_bytes(n, sigma, 77, base=40).tobytes()))
    return out


SCRIPT = r"""
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {here!r})
import numpy as np
import torch
import oracle
import test_emu_front_end as fe
from suffix_amd import Engine
from suffix_amd import device as sdev
oracle.build()
eng = Engine(os.path.join({here!r}, "emu", "libsuffix_emu.so"))
for name, t in fe.texts():
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


def test_lengths_cover_the_last_tile_shapes():
    for name, (sigma, spw) in WIDTHS.items():
        ns = lengths(spw)
        assert TILE * 2 in ns and TILE * 2 + 1 in ns and any(n % spw not in (0, 1) and n % TILE < spw for n in ns), (name, ns)


def test_front_end_every_width_on_the_emulator(tmp_path):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(HERE, "emu")])
    script = tmp_path / "front_end.py"
    script.write_text(SCRIPT.format(root=ROOT, here=HERE))
    env = dict(os.environ, SFX_TINY="0", SFX_HYBRID_MIN="1", SFX_MAX_GRID="3")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-2000:], r.stderr[-4000:])
