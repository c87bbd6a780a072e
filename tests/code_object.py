"""Reads the built library's gfx950 code object (test infrastructure): the static LDS the compiler gave every kernel, which the launch-plan
tests add to the dynamic LDS that csrc/launch_plan.h asks for.  The library must have been built (`__graft_entry__.build()`)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "r-vio_amd", "librvio_hip.so")


def _tool(name):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for p in (os.path.join(rocm, "llvm", "bin", name), os.path.join(rocm, "lib", "llvm", "bin", name), shutil.which(name) or ""):
        if p and os.path.exists(p):
            return p
    pytest.fail("%s not found (ROCm's LLVM tools are needed to read the built library's code object)" % name)


def read_static_lds(lib=LIB):
    """{kernel name as c++filt prints it, without return type and arguments: static LDS in bytes}: the .hip_fatbin section -> the gfx950 code
    object -> the kernel descriptors' notes"""
    if not os.path.exists(lib):
        pytest.fail("r-vio_amd/librvio_hip.so has not been built: run __graft_entry__.build() first (this test reads the kernels' static LDS from it)")
    with tempfile.TemporaryDirectory() as t:
        fat, co = os.path.join(t, "fat.bin"), os.path.join(t, "gfx950.co")
        subprocess.check_call([_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
        subprocess.check_call([_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--output=" + co,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"])
        notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    # one YAML map per kernel under amdhsa.kernels: its keys are sorted, .group_segment_fixed_size comes before .name
    for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        name = re.search(r"\n\s*\.name:\s+(\S+)", blk)
        lds = re.search(r"\n\s*\.group_segment_fixed_size:\s+(\d+)", blk)
        assert name and lds, blk[:400]
        out[name.group(1)] = int(lds.group(1))
    assert len(out) > 40, "kernel descriptors not found in the code object's notes"
    dem = subprocess.run([shutil.which("c++filt") or _tool("llvm-cxxfilt")], input="\n".join(out), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(dem) == len(out)
    return {re.sub(r"\(.*", "", re.sub(r"^void ", "", d)): v for d, v in zip(dem, out.values())}
