"""Compile-time guard for the log-likelihood kernels of the device store (omc_loglik.hip; no GPU needed: hipcc cross-compiles): the
row pre-pass, the two load forms of the column pass -- 8-byte and 16-byte loads -- and the join keep everything in registers: no
scratch, no spilled VGPRs.  The kernels are named, so a form that is silently dropped fails here."""

import os

import pytest
from kernel_usage import HIPCC, compile_usage, not_in_registers

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_loglik_kernels_need_no_scratch(tmp_path):
    usage = compile_usage("omc_loglik.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "k_loglik_" in k or "k_store_" in k}
    print(kernels)
    for piece in ("k_loglik_head", "k_loglik_partILb0EE", "k_loglik_partILb1EE", "k_loglik_join"):
        assert sum(piece in k for k in kernels) == 1, (piece, sorted(usage))
    assert len(kernels) == 4, sorted(kernels)
    assert not not_in_registers(kernels)
