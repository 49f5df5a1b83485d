"""Compile-time guard for the truncated mixture kernels (no GPU needed: hipcc cross-compiles): the ragged scan and the dense scan
with a per-chain diagonal (omc_truncmix.hip) inline the near-limit truncated-normal quantile, which under a spike component is
the common path, and the log-density with limits (omc_scalar.hip) is a few sums -- none of them uses scratch or spills VGPRs."""

import os

import pytest

from kernel_usage import HIPCC, compile_usage, not_in_registers

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_truncated_mixture_kernels_need_no_scratch(tmp_path):
    usage = {**compile_usage("omc_truncmix.hip", tmp_path), **compile_usage("omc_scalar.hip", tmp_path)}
    # by substring of the (mangled) name; the dense scan and the log-density are template instantiations now, and every
    # instantiation that the two files hold is checked
    wanted = ("k_small_gibbs_truncated", "k_dense_gibbs_truncated", "k_diag_gauss_logpdf")
    kernels = {k: v for k, v in usage.items() if any(w in k for w in wanted)}
    for want in wanted:
        assert any(want in k for k in kernels), sorted(usage)
    # the per-chain-diagonal instantiation <true> of the dense scan and the instantiation <true> (limits) of the log-density
    assert any("k_dense_gibbs_truncatedILb1E" in k for k in kernels), sorted(kernels)
    assert any("k_diag_gauss_logpdfILb1E" in k for k in kernels), sorted(kernels)
    assert not not_in_registers(kernels), not_in_registers(kernels)
