"""Compile-time guard for the exp-transform kernels (omc_transform.hip; no GPU needed: hipcc cross-compiles).  The fused
ManifoldMALA step keeps a lane's vectors in registers and the matrix it factorises in LDS: no scratch, no spilled registers, no
out-of-line call, and at most 128 VGPRs (the compiler reports 114; allocated in granules of 8) -- 4 waves per SIMD (MI355X: 512
registers per lane and SIMD), which is what the LDS tiles admit at p = 32 (4 workgroups of 4 waves per CU) and more than they
admit above: registers must not cut the residency further than LDS does over the upper half of the orders, where a step costs
most.  Below p = 22 LDS would admit 8 waves per SIMD and registers hold it at 4.  Its LDS is dynamic: the
largest launch (p = 64) must fit the 160 KB of a compute unit."""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

VGPR_MAX = 128  # 4 waves per SIMD


def test_transform_kernels_resources(tmp_path):
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", f"-I{ROOT}/include",
           "-mllvm", "-instcombine-max-copied-from-constant-users=100000",  # as openmcmc_amd/csrc/Makefile
           "-c", f"{ROOT}/openmcmc_amd/csrc/omc_transform.hip", "-o", str(tmp_path / "omc_transform.o"),
           "-Rpass-analysis=kernel-resource-usage", "-save-temps=obj"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=tmp_path)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "warning:" not in out.stderr, out.stderr[-2000:]
    usage, name = {}, None
    for line in (out.stderr + out.stdout).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|VGPRs|AGPRs|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    kernels = {k: v for k, v in usage.items() if "k_transform_" in k or "k_mala_transform_step" in k}
    assert len(kernels) == 3, sorted(usage)
    for k, v in kernels.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
    step = [v for k, v in kernels.items() if "k_mala_transform_step" in k]
    assert len(step) == 1  # one instantiation: p is a run-time argument
    assert step[0]["VGPRs"] + step[0]["AGPRs"] <= VGPR_MAX, step[0]
    assert step[0]["LDS Size [bytes/block]"] == 0  # all of it is dynamic
    # dynamic LDS of the launches, as omc_mala_transform_step sizes them: one tile of p x (p | 1) doubles per wave, 4 waves
    for p in range(1, 65):
        assert 4 * p * (p | 1) * 8 <= 160 * 1024, p
    src = open(os.path.join(ROOT, "openmcmc_amd", "csrc", "omc_transform.hip")).read()
    assert "#define TF_WAVES_MAX 4" in src and "(size_t)waves * p * ld * sizeof(double)" in src  # ... and that is still how
    # no out-of-line call anywhere in the device code of the file
    asm = [f for f in os.listdir(tmp_path) if f.endswith(".s") and "gfx950" in f]
    assert asm, os.listdir(tmp_path)
    text = open(tmp_path / asm[0]).read()
    assert "s_swappc_b64" not in text
