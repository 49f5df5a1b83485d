"""What the compiler reports a translation unit's kernels to use (no GPU needed: hipcc cross-compiles for gfx950).  Shared by the
test_*_kernel_resources.py of the store summaries."""

import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def compile_usage(hip_file, tmp_path):
    """{function name: {"ScratchSize [bytes/lane]": n, "VGPRs Spill": n}} of openmcmc_amd/csrc/<hip_file>, compiled with the
    flags of openmcmc_amd/csrc/Makefile"""
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", f"-I{ROOT}/include",
           "-mllvm", "-instcombine-max-copied-from-constant-users=100000",
           "-c", f"{ROOT}/openmcmc_amd/csrc/{hip_file}", "-o", str(tmp_path / (hip_file + ".o")),
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
    return usage


def not_in_registers(kernels):
    """the kernels of {name: usage} that use scratch or spill VGPRs (or whose usage was not reported)"""
    return {k: v for k, v in kernels.items() if v.get("ScratchSize [bytes/lane]") != 0 or v.get("VGPRs Spill") != 0}
