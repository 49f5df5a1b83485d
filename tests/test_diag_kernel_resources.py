"""Compile-time guard for the store diagnostics kernels (omc_diag.hip; no GPU needed: hipcc cross-compiles): every kernel
keeps its lag accumulators and its ring of lagged operands in registers -- no scratch, no spilled VGPRs."""

import os

import pytest
from kernel_usage import HIPCC, compile_usage, not_in_registers

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_diag_kernels_need_no_scratch(tmp_path):
    usage = compile_usage("omc_diag.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "k_diag_" in k}
    assert len(kernels) >= 4, sorted(usage)  # means, lag blocks, short-series form, Geyer step
    assert not not_in_registers(kernels)
