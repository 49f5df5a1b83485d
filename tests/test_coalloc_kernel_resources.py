"""Compile-time guard for the co-allocation kernels (omc_coalloc.hip; no GPU needed: hipcc cross-compiles): the 64 accumulator
registers of the int8 MFMA kernel with its prefetched label bytes, in every instantiation of the padded label count, and the 64
labels the score kernel keeps per lane stay in registers -- no scratch, no spilled VGPRs."""

import os

import pytest
from kernel_usage import HIPCC, compile_usage, not_in_registers

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_coalloc_kernels_need_no_scratch(tmp_path):
    usage = compile_usage("omc_coalloc.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "k_coalloc_" in k or "k_partition_" in k}
    for name in ("k_coalloc_pack", "k_coalloc_join", "k_partition_score", "k_partition_best"):
        assert any(name in k for k in kernels), sorted(usage)
    assert sum("k_coalloc_mfma" in k for k in kernels) == 7, sorted(usage)  # Kp = 1, 2, .., 64
    assert not not_in_registers(kernels)
