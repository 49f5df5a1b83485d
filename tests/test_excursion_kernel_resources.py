"""Compile-time guard for the first-failure kernels (omc_excursion.hip; no GPU needed: hipcc cross-compiles): the long form with and
without an index and the short form, for 1, 2, 4 and 8 slot registers, and the check of the positions keep everything in registers
-- no scratch, no spilled VGPRs.  The kernels are named, so a form that is silently dropped fails here."""

import os

import pytest
from kernel_usage import HIPCC, compile_usage, not_in_registers

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

SLOTS = (1, 2, 4, 8)  # the slot registers of an instantiation: the call's slots rounded up


def test_first_failure_kernels_need_no_scratch(tmp_path):
    usage = compile_usage("omc_excursion.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "k_ff_" in k}
    print(kernels)
    expected = ([f"k_ff_longILi{lt}ELb{i}EE" for lt in SLOTS for i in (0, 1)] + [f"k_ff_shortILi{lt}EE" for lt in SLOTS]
                + ["k_ff_check_pos"])
    for piece in expected:
        assert sum(piece in k for k in kernels) == 1, (piece, sorted(usage))
    assert len(kernels) == len(expected) == 3 * len(SLOTS) + 1, sorted(kernels)
    assert not not_in_registers(kernels)
