"""The launch form of the relative-pose rows (csrc/launch_plan.h rel_launch), compiled with g++ from tests/hostemu/rel_plan_emu.cpp and checked on
the CPU at batch 1 / 8 / 128: one wave per instance, no dynamic LDS, and the kernel's static LDS — read from the built library's gfx950 code
object under the name launch_plan.h gives it — the chain of 33 rigid transforms and no more (its rows have no head block), within the 160 KiB
of a CU.  The chain covers every window a handle accepts (max_track_len 32: 31 clones)."""
import ctypes as C
import os
import subprocess

import pytest

from test_aux_plan import static_lds  # noqa: F401  (the fixture that reads the code object's notes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "rel_plan_emu.cpp")
LIMIT = 163840
NAME = "rel_rows_kernel"


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rel_plan") / "rel_plan_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unused-variable", SRC, "-o", so])
    L = C.CDLL(so)
    L.rlp_kernel_name.restype = C.c_char_p
    L.rlp_lds_limit.restype = C.c_long
    return L


def test_constants(emu):
    assert emu.rlp_lds_limit() == LIMIT and emu.rlp_threads() == 64
    assert emu.rlp_nmax() == 32 and emu.rlp_chain_doubles() == 33 * 12
    assert 32 - 1 <= emu.rlp_nmax() < emu.rlp_threads()          # the longest window a handle accepts (max_track_len = 32); one lane per clone


@pytest.mark.parametrize("batch", [1, 8, 128])
def test_one_wave_per_instance_within_a_cu(emu, static_lds, batch):
    names = [emu.rlp_kernel_name(k).decode() for k in range(emu.rlp_num_kernels())]
    assert NAME in names and NAME in static_lds, "rel_rows_kernel must be named in kLpKernelName and present in the built library"
    out = (C.c_long * 6)()
    emu.rlp_launch(batch, out)
    gx, gy, gz, threads, lds, kern = list(out)
    assert (gx, gy, gz, threads) == (1, 1, batch, 64)
    assert names[kern] == NAME and lds == 0
    st = static_lds[NAME]
    print("batch %d: static LDS of %s = %d B, dynamic 0" % (batch, NAME, st))
    # the chain, nothing else
    assert 8 * emu.rlp_chain_doubles() <= st <= 8 * emu.rlp_chain_doubles() + 256 and st + lds <= LIMIT
    # the plan sets no dynamic-LDS limit for it and accepts the stock handle with this static part ...
    statics = (C.c_size_t * len(names))(*[static_lds[nm] for nm in names])
    attr = C.c_long(-1)
    assert emu.rlp_plan(11, 200, batch, statics, kern, C.byref(attr)) == 0 and attr.value == 0
    # ... and refuses a build whose kernel would not fit a CU
    statics[kern] = LIMIT + 8
    assert emu.rlp_plan(11, 200, batch, statics, kern, C.byref(attr)) == 1
