"""Compile-time guard for the kernel density kernels (omc_kde.hip; no GPU needed: hipcc cross-compiles): the bandwidth rules, the
six dependent sums of a Phi evaluation, the convolution and the mode stay in registers and LDS -- no scratch, no spilled VGPRs -- in
the one-wave and the four-wave form, and so does the check of the counts."""

import os

import pytest
from kernel_usage import HIPCC, compile_usage, not_in_registers

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_kde_kernels_need_no_scratch(tmp_path):
    usage = compile_usage("omc_kde.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "k_kde" in k}
    assert sum("k_kdeILi" in k for k in kernels) == 2, sorted(usage)  # 64 and 256 threads
    assert any("k_kde_check" in k for k in kernels), sorted(usage)
    assert not not_in_registers(kernels)
