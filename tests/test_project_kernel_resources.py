"""Compile-time guard for the linear-map kernels of the device store (omc_project.hip; no GPU needed: hipcc cross-compiles): the
three load forms of k_project_mfma -- 8-byte loads, 8-byte loads through an index, 16-byte loads --, each in its two tile
shapes, keep everything in registers: no scratch, no spilled VGPRs.  The kernels are named, so a form that is silently dropped fails here."""

import os

import pytest
from kernel_usage import HIPCC, compile_usage, not_in_registers

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_project_kernels_need_no_scratch(tmp_path):
    usage = compile_usage("omc_project.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "k_project_" in k}
    print(kernels)
    expected = [f"k_project_mfmaILb{v}ELb{i}ELb{t}EE" for v, i in ((0, 0), (0, 1), (1, 0)) for t in (0, 1)]
    for piece in expected:
        assert sum(piece in k for k in kernels) == 1, (piece, sorted(usage))
    assert len(kernels) == len(expected), sorted(kernels)
    assert not not_in_registers(kernels)
