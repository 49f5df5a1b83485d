"""Compile-time guard for the rank kernels (omc_rank.hip; no GPU needed: hipcc cross-compiles): the quantiles, the bisection
and the combination keep everything in registers -- no scratch, no spilled VGPRs.  (The gather, the sort and the index check they
launch are compiled in omc_store_shared.hip: test_store_shared_kernel_resources.py.)"""

import os

import pytest
from kernel_usage import HIPCC, compile_usage, not_in_registers

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_rank_kernels_need_no_scratch(tmp_path):
    usage = compile_usage("omc_rank.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "k_rank_" in k or "k_store_" in k}
    # quantiles, emit, combine -- and no copy of a shared kernel
    for piece in ("k_rank_stats", "k_rank_emit", "k_rank_combine"):
        assert sum(piece in k for k in kernels) == 1, (piece, sorted(usage))
    assert len(kernels) == 3, sorted(kernels)
    assert not not_in_registers(kernels)
