"""Compile-time guard for the per-draw reduction kernels (omc_reduce.hip; no GPU needed: hipcc cross-compiles): the long form
with and without an index and the short form, for every one of the seven ops, keep everything in registers -- no scratch, no
spilled VGPRs.  The kernels are named, so a form that is silently dropped fails here."""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

N_OPS = 7  # OMC_REDUCE_SUM .. OMC_REDUCE_SUPNORM (include/omcmc_hip.h)


def test_reduce_kernels_need_no_scratch(tmp_path):
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", f"-I{ROOT}/include",
           "-mllvm", "-instcombine-max-copied-from-constant-users=100000",  # as openmcmc_amd/csrc/Makefile
           "-c", f"{ROOT}/openmcmc_amd/csrc/omc_reduce.hip", "-o", str(tmp_path / "omc_reduce.o"),
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
    kernels = {k: v for k, v in usage.items() if "k_reduce_" in k}
    print(kernels)
    expected = [f"k_reduce_longILi{op}ELb{i}EE" for op in range(N_OPS) for i in (0, 1)] + [f"k_reduce_shortILi{op}EE" for op in range(N_OPS)]
    for piece in expected:
        assert sum(piece in k for k in kernels) == 1, (piece, sorted(usage))
    assert len(kernels) == len(expected) == 3 * N_OPS, sorted(kernels)
    bad = {k: v for k, v in kernels.items() if v.get("ScratchSize [bytes/lane]") != 0 or v.get("VGPRs Spill") != 0}
    assert not bad, bad
