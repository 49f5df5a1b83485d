"""Compile-time guard for the joint density kernels (omc_kde2d.hip; no GPU needed: hipcc cross-compiles): the moments, the
convolution with its accumulators, count registers and window of weights, the mode and the level pass stay in registers and LDS --
no scratch, no spilled VGPRs -- in both lane widths of the convolution, and so does the check of the counts."""

import os

import pytest
from kernel_usage import HIPCC, compile_usage, not_in_registers

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_kde2d_kernels_need_no_scratch(tmp_path):
    usage = compile_usage("omc_kde2d.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "k_kde2d" in k}
    assert sum("k_kde2d_convILi" in k for k in kernels) == 2, sorted(usage)  # one and two columns per lane
    for name in ("k_kde2d_check", "k_kde2d_prep", "k_kde2d_mode", "k_kde2d_level"):
        assert any(name in k for k in kernels), (name, sorted(usage))
    assert not not_in_registers(kernels)
