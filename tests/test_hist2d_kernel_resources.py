"""Compile-time guard for the 2-D store histogram kernels (omc_hist2d.hip; no GPU needed: hipcc cross-compiles): the prefetched
draws of four rows, the edge pointers of both axes, the outside counters and -- in the pooled kernel -- the four cell keys of the
occupancy pass stay in registers: no scratch, no spilled VGPRs in any instantiation."""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_hist2d_kernels_need_no_scratch(tmp_path):
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", f"-I{ROOT}/include",
           "-mllvm", "-instcombine-max-copied-from-constant-users=100000",  # as openmcmc_amd/csrc/Makefile
           "-c", f"{ROOT}/openmcmc_amd/csrc/omc_hist2d.hip", "-o", str(tmp_path / "omc_hist2d.o"),
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
    kernels = {k: v for k, v in usage.items() if "k_hist2d_" in k}
    assert sum("k_hist2d_pair" in k for k in kernels) == 8, sorted(usage)  # shared / per-pair edges x guess / bisection x LDS / direct
    assert sum("k_hist2d_pool" in k for k in kernels) == 8, sorted(usage)  # guess / bisection x LDS / direct x with / without occupancy
    bad = {k: v for k, v in kernels.items() if v.get("ScratchSize [bytes/lane]") != 0 or v.get("VGPRs Spill") != 0}
    assert not bad, bad
