"""Compile-time guard for the autocorrelation kernels (omc_autocorr.hip; no GPU needed: hipcc cross-compiles): the lag kernel --
32 accumulators and a 32-slot ring of doubles per lane -- in both its instantiations, reading the gathered centred draws and
reading the store where it lies, keeps everything in registers: no scratch, no spilled VGPRs.  So do the kernels around it.  The
kernels are named, so an instantiation that is silently dropped fails here."""

import os

import pytest
from kernel_usage import HIPCC, compile_usage, not_in_registers

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_autocorr_kernels_need_no_scratch(tmp_path):
    usage = compile_usage("omc_autocorr.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "k_acorr_" in k}
    print(kernels)
    expected = [f"k_acorr_lagsILb{i}EE" for i in (0, 1)] + [f"k_acorr_prepassILb{i}EE" for i in (0, 1)] + ["k_acorr_sum", "k_acorr_emit", "k_acorr_tau"]
    for piece in expected:
        assert sum(piece in k for k in kernels) == 1, (piece, sorted(usage))
    assert len(kernels) == len(expected), sorted(kernels)
    assert not not_in_registers(kernels)
