"""The launch form of the standstill detector (csrc/launch_plan.h standstill_launch), compiled with g++ from
tests/hostemu/standstill_plan_emu.cpp and checked on the CPU at batch 1 / 8 / 128 / 2048: one workgroup of 256 threads per instance, no
dynamic LDS, and the kernel's static LDS — read from the built library's gfx950 code object under the name launch_plan.h gives it — within the
160 KiB of a CU (and no more than the few hundred bytes the four waves' partial sums need)."""
import ctypes as C
import os
import subprocess

import pytest

from test_aux_plan import static_lds  # noqa: F401  (the fixture that reads the code object's notes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "standstill_plan_emu.cpp")
LIMIT = 163840
NAME = "standstill_kernel"


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("standstill_plan") / "standstill_plan_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unused-variable", SRC, "-o", so])
    L = C.CDLL(so)
    L.sp_kernel_name.restype = C.c_char_p
    L.sp_lds_limit.restype = C.c_long
    return L


def test_constants(emu):
    assert emu.sp_lds_limit() == LIMIT and emu.sp_threads() == 256 and emu.sp_waves() == 4


@pytest.mark.parametrize("batch", [1, 8, 128, 2048])
def test_one_workgroup_per_instance_within_a_cu(emu, static_lds, batch):
    names = [emu.sp_kernel_name(k).decode() for k in range(emu.sp_num_kernels())]
    assert NAME in names and NAME in static_lds, "standstill_kernel must be named in kLpKernelName and present in the built library"
    out = (C.c_long * 6)()
    emu.sp_launch(batch, out)
    gx, gy, gz, threads, lds, kern = list(out)
    assert (gx, gy, gz, threads) == (1, 1, batch, 256)
    assert names[kern] == NAME and lds == 0
    st = static_lds[NAME]
    print("batch %d: static LDS of %s = %d B, dynamic 0" % (batch, NAME, st))
    # the four waves' partial sums, nothing else: a few dozen doubles
    assert 8 * emu.sp_red_doubles() <= st <= 1024 and st + lds <= LIMIT
    # the plan sets no dynamic-LDS limit for it and accepts the stock handle with this static part ...
    statics = (C.c_size_t * len(names))(*[static_lds[nm] for nm in names])
    attr = C.c_long(-1)
    assert emu.sp_plan(11, 200, batch, statics, kern, C.byref(attr)) == 0 and attr.value == 0
    # ... and refuses, by name of the limit, a build whose kernel would not fit a CU
    statics[kern] = LIMIT + 8
    assert emu.sp_plan(11, 200, batch, statics, kern, C.byref(attr)) == 1
