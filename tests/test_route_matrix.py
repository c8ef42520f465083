"""The route matrix on the CPU: the ledger (tests/_routes.py's table against REQUIRED, EXEMPT, the plain-Python dispatch rules
and the oracle-side LCP sample -- no engine) and every case of at most 2^19 bytes through the emulator build, hook-free: no
SFX_* variable is set, so the library dispatches as the product does.  Larger cases run in test_gpu_route_matrix.py only, and
the ledger says which.  82 tests in 45 s on an idle machine (about 100 s beside other work): a third the ledger, which generates
and counts the texts of 2^25 bytes, the rest the emulator, its slowest case 8 s."""
import os
import subprocess

import numpy as np
import pytest

import _routes
from suffix_amd import Engine

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
N_CASES = 56
LEDGER_FULL_MAX = 1 << 21           # up to here the ledger runs the oracle for the LCP route; above, the byte counts decide


@pytest.fixture(scope="module")
def emu():
    assert not [k for k in os.environ if k.startswith("SFX_")], "the matrix is about the hook-free dispatch"
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU_DIR])
    return Engine(os.environ.get("SUFFIX_EMU_LIB") or os.path.join(EMU_DIR, "libsuffix_emu.so"))


def test_ledger_required_cells_are_held():
    names = [c.name for c in _routes.CASES]
    # (cells overlap -- direct_b2 is also a 2-bit k32 text on the passes -- so a deleted case need not empty a required cell: the
    # count is pinned, and a case cannot leave the table unnoticed)
    assert len(set(names)) == len(names) == N_CASES, len(names)
    missing = [r for r in _routes.REQUIRED if not _routes.satisfied(r, _routes.CASES)]
    assert not missing, missing
    for r in _routes.REQUIRED:
        assert r[:3] not in _routes.EXEMPT, r
    for c in _routes.CASES:
        assert c.cell[:3] not in _routes.EXEMPT, c.name
        assert (c.where == "emu+gpu") == (c.n <= _routes.EMU_MAX) or c.where.startswith("tests/"), c.name


@pytest.mark.parametrize("case", _routes.CASES, ids=lambda c: c.name)
def test_ledger_declared_cell_is_the_predicted_one(case, oracle):
    text = np.ascontiguousarray(case.make())
    assert len(text) == case.n
    bits, key, sort, lcp_route = case.cell
    p = _routes.predict(text)                     # (asserts the distance to the key rule's threshold)
    assert p["bits"] == bits and p["key"] == key[:3], (p, case.cell)
    if sort.startswith("hybrid"):
        assert p["sort"] == "hybrid", p
        largest, slow = _routes.top16_histogram(text)
        assert slow * 64 <= case.n and (largest > 16384) == (sort == "hybrid_keys"), (largest, slow)
    else:
        assert p["sort"] == sort, (p, case.cell)
    flips = case.tags & {"flip_lo", "flip_hi"}
    if flips:
        assert case.n + ("flip_lo" in flips) == 1 << (case.n.bit_length() - ("flip_hi" in flips)), case.n
        assert key[:3] == ("k32" if "flip_lo" in flips else "k64")
    if lcp_route is None:
        assert case.where.startswith("tests/"), case.name
    elif case.n <= LEDGER_FULL_MAX:
        sa = oracle.sais(text)
        route, window = _routes.lcp_route_of(p["sigma"], oracle.lcp_kasai(text, sa))
        assert route == lcp_route and (window is None or f"w{window}" in case.tags), (route, window, case.cell, case.tags)
    else:
        # (uniform or skewed text without planted repeats: a mean LCP of a few symbols -- checked against the oracle on the GPU run)
        assert lcp_route == ("direct_packed" if p["sigma"] <= 16 else "direct_raw"), case.cell


@pytest.mark.parametrize("case", [c for c in _routes.CASES if c.where == "emu+gpu"], ids=lambda c: c.name)
def test_emulator_takes_the_declared_cell(emu, oracle, case):
    _routes.check_case(emu, oracle, case, "cpu")
