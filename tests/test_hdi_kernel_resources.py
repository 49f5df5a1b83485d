"""Compile-time guard for the highest-density-interval kernels (omc_hdi.hip; no GPU needed: hipcc cross-compiles): the gather,
the translation unit's copy of the two sort kernels, the count and the window-minimum kernels keep everything in registers --
no scratch, no spilled VGPRs."""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_hdi_kernels_need_no_scratch(tmp_path):
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", f"-I{ROOT}/include",
           "-mllvm", "-instcombine-max-copied-from-constant-users=100000",  # as openmcmc_amd/csrc/Makefile
           "-c", f"{ROOT}/openmcmc_amd/csrc/omc_hdi.hip", "-o", str(tmp_path / "omc_hdi.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    usage, name = {}, None
    for line in (out.stderr + out.stdout).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    kernels = {k: v for k, v in usage.items() if "k_hdi_" in k or "k_rank_" in k}
    print(kernels)
    # the gather, the two sort kernels, the window minimum in its two sizes and its second stage; besides them the index check
    # and the count
    for piece in ("k_hdi_gather", "k_rank_sort_tile", "k_rank_sort_global", "k_hdi_windowILi64E", "k_hdi_windowILi256E",
                  "k_hdi_window_final", "k_hdi_count", "k_rank_check"):
        assert sum(piece in k for k in kernels) == 1, (piece, sorted(usage))
    assert len(kernels) == 8, sorted(kernels)
    bad = {k: v for k, v in kernels.items() if v.get("ScratchSize [bytes/lane]") != 0 or v.get("VGPRs Spill") != 0}
    assert not bad, bad
