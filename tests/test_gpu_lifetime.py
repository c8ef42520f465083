"""What the library holds on to, on the MI355X: the cases of tests/_lifetime.py through
libsuffix_hip.so.  Only the library's own counters are asserted; the change of `torch.cuda.mem_get_info()` over each case
is printed and put into the assertion messages, never compared (the machines are shared)."""
import pytest

import _lifetime as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(oracle):
    import suffix_amd
    e = suffix_amd.default_engine()
    e.require_device()                      # fail loudly: no CPU fallback
    assert e.path.endswith("libsuffix_hip.so")
    c = L.Ctx(e, "cuda", oracle)
    yield c
    print("mem_get_info deltas (bytes less free than at the baseline, information only):", c.info)


@pytest.mark.parametrize("name", sorted(L.CONSTRUCTORS))
def test_handles(ctx, name):
    L.handles(ctx, name, reps=50)


def test_refusals_after_an_allocation(ctx):
    L.refusals(ctx)


def test_hot_path_allocates_nothing(ctx):
    L.hot_path(ctx)


def test_pool_allocates_once_at_one_size(ctx):
    L.pool_one_size(ctx)


def test_pool_ladder(ctx):
    L.pool_ladder(ctx, 1024)


def test_eight_threads_one_after_another(ctx):
    L.threads(ctx, 8, together=False)


def test_four_threads_together(ctx):
    L.threads(ctx, 4, together=True)


def test_long_lived_thread_gives_its_scratch_back(ctx):
    L.long_lived_thread_gives_its_scratch_back(ctx)


def test_steady_state(ctx):
    L.steady_state(ctx, 20011, 200, marks=(10, 100, 200))


@pytest.mark.parametrize("mode", ["normal", "handles_alive", "daemon_parked"])
def test_process_exit(ctx, tmp_path, mode):
    L.process_exit(ctx, mode, "", tmp_path)
