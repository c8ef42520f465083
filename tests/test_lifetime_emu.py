"""CPU tests of what the library holds on to: the product's host code compiled against the fiber
emulator, with `sfx_resource_stats` compared at every checkpoint, field for field, with the ledger that the emulator's HIP
shim keeps on its own.  The cases are tests/_lifetime.py's, shared with test_gpu_lifetime.py."""
import os

import pytest

import _lce
import _lifetime as L
from suffix_amd import Engine

EMU_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "libsuffix_emu.so")


@pytest.fixture(scope="module")
def ctx(oracle):
    return L.Ctx(Engine(_lce.build_emulator()), "cpu", oracle)


def test_no_raw_resource_call_outside_the_wrappers():
    found, wrapped = L.raw_calls()
    assert not found, found
    assert wrapped == 9, wrapped                                        # one per wrapper in sfx_host.hpp


def test_stats_entry_refuses_null_and_zeroes_the_reserved_words(ctx):
    import ctypes
    from suffix_amd._lib import ResourceStats
    assert ctx.lib.sfx_resource_stats(None) == L.ERR_ARG
    s = ResourceStats()
    ctypes.memset(ctypes.byref(s), 0xFF, ctypes.sizeof(s))
    assert ctx.lib.sfx_resource_stats(ctypes.byref(s)) == L.OK and list(s.reserved) == [0] * 7 and ctypes.sizeof(s) == 128
    assert ctx.base["streams"] == 1 and ctx.base["pinned_bytes"] == L.STAGE_BYTES and ctx.base["device_allocs"] == 0, ctx.base


@pytest.mark.parametrize("name", sorted(L.CONSTRUCTORS))
def test_handles(ctx, name):
    L.handles(ctx, name, reps=10)


def test_refusals_after_an_allocation(ctx):
    L.refusals(ctx)


def test_hot_path_allocates_nothing(ctx):
    L.hot_path(ctx)


def test_pool_allocates_once_at_one_size(ctx):
    L.pool_one_size(ctx)


def test_pool_ladder(ctx):
    """(lengths 16 * 2.5^k here, up to 381 KB: the emulator takes minutes for the GPU test's 24 MB)"""
    L.pool_ladder(ctx, 16)


def test_eight_threads_one_after_another(ctx):
    L.threads(ctx, 8, together=False)


def test_long_lived_thread_gives_its_scratch_back(ctx):
    L.long_lived_thread_gives_its_scratch_back(ctx)


def test_steady_state(ctx):
    L.steady_state(ctx, 5003, 20, marks=(10, 20))


@pytest.mark.parametrize("mode", ["normal", "handles_alive", "daemon_parked"])
def test_process_exit(ctx, tmp_path, mode):
    L.process_exit(ctx, mode, EMU_LIB, tmp_path)
