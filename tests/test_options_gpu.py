"""omc_ctx_set_option and omc_ctx_counter through the real entry points: the frozen expectation of tests/options_expect.py (which
tests/test_options_host.py holds the table to without a device) fed through Engine.set_option, which raises ValueError on a
reject, and the seven counter names and an unknown one through Engine.counter.  No sampling kernel is launched ("reenter_abi_ok"
reads the kernel descriptors back with its one-thread probe when the process has not asked before); every pointer option is back
at 0 before the engine closes."""

import pytest

import options_expect as E

pytestmark = pytest.mark.gpu


def test_options_and_counters_through_the_engine():
    import torch

    from openmcmc_amd.engine import Engine

    eng = Engine(1, seed=1)
    ring = torch.zeros((128, 1, 2), dtype=torch.int64, device=eng.device)  # a live tensor: large enough for every capacity probed

    def status(name, value):
        try:
            eng.set_option(name, value)
        except ValueError:
            return E.INVALID_ARG
        return E.OK

    state = E.defaults()
    probes = E.plain_probes()
    probes += [(n, 0) for n in E.POINTERS]  # a foreign address or event would be used by a later launch: only "none"
    probes += E.clock_probes(ring.data_ptr(), ring.data_ptr())
    probes += [(n, 1) for n in E.UNKNOWN + E.UNKNOWN_WITH_BLANKS]
    for name, value in probes:
        assert status(name, value) == E.apply(state, name, value), (name, value)
    assert state["sweep_times_ptr"] == 0 and state["sweep_times_cap"] == 0 and all(state[n] == 0 for n in E.POINTERS)
    # what the context kept, where a counter shows it: the position the clock's options reset
    assert eng.counter("sweep_times_pos") == 0

    for name in E.COUNTERS:
        v = eng.counter(name)
        assert isinstance(v, int) and v >= 0, (name, v)
    for name in ("tridiag_join_fallbacks", "run_handoff_timeouts", "band_join_fallbacks", "band_join_retries"):
        assert eng.counter(name) == 0, name  # nothing has run
    assert eng.counter("wall_clock_khz") > 0
    assert eng.counter("reenter_abi_ok") in (0, 1)
    with pytest.raises(ValueError):
        eng.counter("no_such_counter")
    eng.check_status()
    eng.close()
