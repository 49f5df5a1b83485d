"""Compile-time guard for the store histogram kernels (omc_hist.hip; no GPU needed: hipcc cross-compiles): the counting kernel's
four prefetched draws, its edge pointers and its three outside counters stay in registers -- no scratch, no spilled VGPRs -- in
all four instantiations, and so does every other kernel of the file."""

import os

import pytest
from kernel_usage import HIPCC, compile_usage, not_in_registers

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_hist_kernels_need_no_scratch(tmp_path):
    usage = compile_usage("omc_hist.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "k_hist_" in k}
    assert sum("k_hist_count" in k for k in kernels) == 4, sorted(usage)  # shared / per-element edges x guess / bisection
    assert any("k_hist_minmax_part" in k for k in kernels) and any("k_hist_check" in k for k in kernels), sorted(usage)
    assert not not_in_registers(kernels)
