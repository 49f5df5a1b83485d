"""Compile-time guard for the indicator-ESS kernels of the device store (omc_essq.hip; no GPU needed: hipcc cross-compiles): the
thresholds, the pack pass with its 64 draws in registers, the two forms of the lag kernel (bits in LDS, bits in global
memory) and the pick of the order statistics keep everything in registers -- no scratch, no spilled VGPRs.  (The gather, the sort and
the index check they launch are compiled in omc_store_shared.hip: test_store_shared_kernel_resources.py.)"""

import os

import pytest
from kernel_usage import HIPCC, compile_usage, not_in_registers

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_essq_kernels_need_no_scratch(tmp_path):
    usage = compile_usage("omc_essq.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "k_essq_" in k or "k_rank_" in k or "k_store_" in k or "k_diag_" in k}
    print(kernels)
    for piece, count in (("k_essq_thresholds", 1), ("k_essq_pack", 1), ("k_essq_lags", 2), ("k_essq_pick", 1)):
        assert sum(piece in k for k in kernels) == count, (piece, sorted(usage))
    assert len(kernels) == 5, sorted(kernels)
    assert not not_in_registers(kernels)
