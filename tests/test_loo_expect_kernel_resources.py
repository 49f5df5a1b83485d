"""Compile-time guard for the PSIS-LOO expectation kernels of the device store (omc_loo_expect.hip; no GPU needed: hipcc
cross-compiles): the fit that leaves its record, the six forms of the expectation pass
(two load forms x three kinds of f) and the join keep everything in registers -- no scratch, no spilled VGPRs.  (The check of the
tail lengths and the gather are omc_psis.hip's, test_psis_kernel_resources.py; the sort and the index check they launch are
compiled in omc_store_shared.hip: test_store_shared_kernel_resources.py.)"""

import os

import pytest
from kernel_usage import HIPCC, compile_usage, not_in_registers

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_loo_expect_kernels_need_no_scratch(tmp_path):
    usage = compile_usage("omc_loo_expect.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "k_loo_" in k or "k_psis_" in k or "k_rank_" in k or "k_store_" in k}
    print(kernels)
    for piece, count in (("k_loo_check_tail", 0), ("k_loo_gather", 0), ("k_loo_fit", 1), ("k_loo_expect", 6), ("k_loo_join", 1)):
        assert sum(piece in k for k in kernels) == count, (piece, sorted(usage))
    assert len(kernels) == 8, sorted(kernels)
    assert not not_in_registers(kernels)
