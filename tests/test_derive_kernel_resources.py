"""Compile-time guard for the per-draw reduction kernels (omc_reduce.hip; no GPU needed: hipcc cross-compiles): the long form
with and without an index and the short form, for every one of the seven ops, keep everything in registers -- no scratch, no
spilled VGPRs.  The kernels are named, so a form that is silently dropped fails here."""

import os

import pytest
from kernel_usage import HIPCC, compile_usage, not_in_registers

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

N_OPS = 7  # OMC_REDUCE_SUM .. OMC_REDUCE_SUPNORM (include/omcmc_hip.h)


def test_reduce_kernels_need_no_scratch(tmp_path):
    usage = compile_usage("omc_reduce.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "k_reduce_" in k}
    print(kernels)
    expected = [f"k_reduce_longILi{op}ELb{i}EE" for op in range(N_OPS) for i in (0, 1)] + [f"k_reduce_shortILi{op}EE" for op in range(N_OPS)]
    for piece in expected:
        assert sum(piece in k for k in kernels) == 1, (piece, sorted(usage))
    assert len(kernels) == len(expected) == 3 * N_OPS, sorted(kernels)
    assert not not_in_registers(kernels)
