"""Compile-time guard for the truncated mixture kernels (omc_truncmix.hip; no GPU needed: hipcc cross-compiles): the
ragged scan inlines the near-limit truncated-normal quantile, which under a spike component is the common path -- no
kernel of the file uses scratch or spills VGPRs."""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_truncated_mixture_kernels_need_no_scratch(tmp_path):
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", f"-I{ROOT}/include",
           "-mllvm", "-instcombine-max-copied-from-constant-users=100000",  # as openmcmc_amd/csrc/Makefile
           "-c", f"{ROOT}/openmcmc_amd/csrc/omc_truncmix.hip", "-o", str(tmp_path / "omc_truncmix.o"),
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
    kernels = {k: v for k, v in usage.items() if "k_" in k}
    names = " ".join(kernels)
    for want in ("k_small_gibbs_truncated", "k_dense_gibbs_truncated_diag", "k_diag_gauss_logpdf_limits"):
        assert want in names, sorted(usage)
    bad = {k: v for k, v in kernels.items() if v.get("ScratchSize [bytes/lane]") != 0 or v.get("VGPRs Spill") != 0}
    assert not bad, bad
