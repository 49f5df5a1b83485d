"""Compile-time guard for the highest-density-interval kernels (omc_hdi.hip; no GPU needed: hipcc cross-compiles): the gather,
the count and the window-minimum kernels keep everything in registers -- no scratch, no spilled VGPRs.  (The sort and the index
check they launch are compiled in omc_store_shared.hip: test_store_shared_kernel_resources.py.)"""

import os

import pytest
from kernel_usage import HIPCC, compile_usage, not_in_registers

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_hdi_kernels_need_no_scratch(tmp_path):
    usage = compile_usage("omc_hdi.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "k_hdi_" in k or "k_rank_" in k or "k_store_" in k}
    print(kernels)
    # the gather, the window minimum in its two sizes and its second stage, the count -- and no copy of a shared kernel
    for piece in ("k_hdi_gather", "k_hdi_windowILi64E", "k_hdi_windowILi256E", "k_hdi_window_final", "k_hdi_count"):
        assert sum(piece in k for k in kernels) == 1, (piece, sorted(usage))
    assert len(kernels) == 5, sorted(kernels)
    assert not not_in_registers(kernels)
