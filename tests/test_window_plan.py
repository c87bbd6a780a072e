"""The launch form of the window-pose kernel (csrc/launch_plan.h window_pose_launch), compiled with g++ from tests/hostemu/window_plan_emu.cpp and
checked on the CPU at batch 1 / 8 / 128 and every window: one workgroup of four waves per (instance, age) on a grid (ages, 1, instances), no
dynamic LDS, room for every column that is not zero at the longest chain, and the kernel's static LDS — read from the built library's gfx950
code object under the name launch_plan.h gives it — what the plan counts (chain, J and T staged, the groups' shares, the record) within the
160 KiB of a CU."""
import ctypes as C
import os
import subprocess

import pytest

from test_aux_plan import static_lds  # noqa: F401  (the fixture that reads the code object's notes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "window_plan_emu.cpp")
LIMIT = 163840
NAME = "window_pose_kernel"


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("window_plan") / "window_plan_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unused-variable", SRC, "-o", so])
    L = C.CDLL(so)
    L.wpp_kernel_name.restype = C.c_char_p
    for f in ("wpp_lds_limit", "wpp_lds_doubles", "wpp_chain_doubles"):
        getattr(L, f).restype = C.c_long
    return L


def test_constants(emu):
    import window_cases
    abi = window_cases.abi
    assert emu.wpp_lds_limit() == LIMIT and emu.wpp_threads() == 256
    assert emu.wpp_nmax() == 32 and emu.wpp_nz() == 6 + 6 * 32 == 198           # the columns that are not zero at the longest chain
    assert emu.wpp_nz() > 3 * 64                                                # more than three waves of rows: the row loop is a loop
    assert emu.wpp_groups() * 36 <= emu.wpp_threads()                            # one thread per (group, entry of the 6 x 6)
    assert 8 * emu.wpp_words() == C.sizeof(abi.rvio_window_pose) == 368 and emu.wpp_words() <= emu.wpp_threads()
    assert emu.wpp_chain_doubles() == 12 * (emu.wpp_nmax() + 1)
    assert emu.wpp_lds_doubles() == emu.wpp_chain_doubles() + 2 * 6 * emu.wpp_nz() + 2 * 36 * emu.wpp_groups() + emu.wpp_words()
    # the enum grew at its end
    assert emu.wpp_kernel_id() == emu.wpp_num_kernels() - 1 and emu.wpp_kernel_name(emu.wpp_kernel_id()).decode() == NAME


@pytest.mark.parametrize("batch", [1, 8, 128])
def test_one_workgroup_per_instance_and_age(emu, batch):
    for max_len in range(3, 33):
        n = max_len - 1
        for n_ages in (1, 2, n, n + 1):
            out = (C.c_long * 6)()
            emu.wpp_launch(batch, n_ages, out)
            gx, gy, gz, threads, lds, kern = list(out)
            assert (gx, gy, gz, threads, lds) == (n_ages, 1, batch, 256, 0), (max_len, n_ages)
            assert kern == emu.wpp_kernel_id()
        assert 6 + 6 * n <= emu.wpp_nz()


@pytest.mark.parametrize("batch", [1, 8, 128])
def test_static_lds_within_a_cu(emu, static_lds, batch):  # noqa: F811
    names = [emu.wpp_kernel_name(k).decode() for k in range(emu.wpp_num_kernels())]
    assert NAME in names and NAME in static_lds, "window_pose_kernel must be named in kLpKernelName and present in the built library"
    kern = names.index(NAME)
    st = static_lds[NAME]
    print("batch %d: static LDS of %s = %d B (the plan counts %d B), dynamic 0" % (batch, NAME, st, 8 * emu.wpp_lds_doubles()))
    # what the plan counts and alignment, nothing else
    assert 8 * emu.wpp_lds_doubles() <= st <= 8 * emu.wpp_lds_doubles() + 256 and st <= LIMIT
    # the plan sets no dynamic-LDS limit for it and accepts the stock handle with this static part ...
    statics = (C.c_size_t * len(names))(*[static_lds[nm] for nm in names])
    attr = C.c_long(-1)
    assert emu.wpp_plan(11, 200, batch, statics, kern, C.byref(attr)) == 0 and attr.value == 0
    # ... and refuses a build whose kernel would not fit a CU
    statics[kern] = LIMIT + 8
    assert emu.wpp_plan(11, 200, batch, statics, kern, C.byref(attr)) == 1
