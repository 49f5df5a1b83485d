"""Compile-time guard for the store covariance kernels (omc_cov.hip; no GPU needed: hipcc cross-compiles): the 128
accumulator registers of the MFMA kernel, its prefetched slab and the column offsets stay in registers -- no scratch, no
spilled VGPRs -- and so does every other kernel of the file."""

import os

import pytest
from kernel_usage import HIPCC, compile_usage, not_in_registers

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_cov_kernels_need_no_scratch(tmp_path):
    usage = compile_usage("omc_cov.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "k_cov_" in k}
    assert any("k_cov_mfma" in k for k in kernels) and any("k_cov_join" in k for k in kernels), sorted(usage)
    assert not not_in_registers(kernels)
