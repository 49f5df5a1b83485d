"""Compile-time guard for what the store summaries share (omc_store_shared.hip; no GPU needed: hipcc cross-compiles): the split
gather, the two sort kernels, the index check and the column-moments kernels (the slices with and without an index, the join) are
there exactly once and keep everything in registers -- no scratch, no spilled VGPRs."""

import os

import pytest
from kernel_usage import HIPCC, compile_usage, not_in_registers

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_store_shared_kernels_need_no_scratch(tmp_path):
    usage = compile_usage("omc_store_shared.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "k_rank_" in k or "k_store_" in k}
    print(kernels)
    for piece in ("k_rank_gather", "k_rank_sort_tile", "k_rank_sort_global", "k_store_check_index", "k_store_moments_partILb0EE",
                  "k_store_moments_partILb1EE", "k_store_moments_join"):
        assert sum(piece in k for k in kernels) == 1, (piece, sorted(usage))
    assert len(kernels) == 7, sorted(kernels)
    assert not not_in_registers(kernels)
