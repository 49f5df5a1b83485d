"""Compile-time guard for the 2-D store histogram kernels (omc_hist2d.hip; no GPU needed: hipcc cross-compiles): the prefetched
draws of four rows, the edge pointers of both axes, the outside counters and -- in the pooled kernel -- the four cell keys of the
occupancy pass stay in registers: no scratch, no spilled VGPRs in any instantiation."""

import os

import pytest
from kernel_usage import HIPCC, compile_usage, not_in_registers

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_hist2d_kernels_need_no_scratch(tmp_path):
    usage = compile_usage("omc_hist2d.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "k_hist2d_" in k}
    assert sum("k_hist2d_pair" in k for k in kernels) == 8, sorted(usage)  # shared / per-pair edges x guess / bisection x LDS / direct
    assert sum("k_hist2d_pool" in k for k in kernels) == 8, sorted(usage)  # guess / bisection x LDS / direct x with / without occupancy
    assert not not_in_registers(kernels)
