"""Compile-time guard for the PSIS kernels of the device store (omc_psis.hip; no GPU needed: hipcc cross-compiles): the check of the
tail lengths, the gather that computes the log-likelihood on the way and the fit keep everything in registers -- no scratch, no
spilled VGPRs.  (The sort and the index check they launch are compiled in omc_store_shared.hip:
test_store_shared_kernel_resources.py.)"""

import os

import pytest
from kernel_usage import HIPCC, compile_usage, not_in_registers

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_psis_kernels_need_no_scratch(tmp_path):
    usage = compile_usage("omc_psis.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "k_psis_" in k or "k_rank_" in k or "k_store_" in k}
    print(kernels)
    for piece in ("k_psis_check_tail", "k_psis_gather", "k_psis_fit"):
        assert sum(piece in k for k in kernels) == 1, (piece, sorted(usage))
    assert len(kernels) == 3, sorted(kernels)
    assert not not_in_registers(kernels)
