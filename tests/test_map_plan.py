"""The launch form of the map-landmark rows (csrc/launch_plan.h map_launch) and the sizes of the block the map calls allocate, compiled with g++
from tests/hostemu/map_plan_emu.cpp and checked on the CPU at batch 1 / 8 / 128 and every window: one workgroup of four waves per instance, no
dynamic LDS, one lane per column that is not zero, and the kernel's static LDS — read from the built library's gfx950 code object under the name
launch_plan.h gives it — what the plan counts (chain, transposed rows, slot records, partial sums) within the 160 KiB of a CU."""
import ctypes as C
import os
import subprocess

import pytest

from test_aux_plan import static_lds  # noqa: F401  (the fixture that reads the code object's notes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "map_plan_emu.cpp")
LIMIT = 163840
NAME = "map_rows_kernel"


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("map_plan") / "map_plan_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unused-variable", SRC, "-o", so])
    L = C.CDLL(so)
    L.mpp_kernel_name.restype = C.c_char_p
    for f in ("mpp_lds_limit", "mpp_lds_doubles", "mpp_H_stride", "mpp_block_bytes"):
        getattr(L, f).restype = C.c_long
    L.mpp_min_depth.restype = C.c_double
    return L


def test_constants(emu):
    assert emu.mpp_lds_limit() == LIMIT and emu.mpp_threads() == 256 and emu.mpp_waves() == 4
    assert emu.mpp_points() == 8 and emu.mpp_rows() == 16 == emu.mpp_aux_rows()
    hdr = open(os.path.join(ROOT, "include", "rvio_hip.h")).read()
    assert "#define RVIO_MAP_MAX_POINTS 8" in hdr
    assert emu.mpp_nmax() == 32 and emu.mpp_nz() == 6 + 6 * 32 <= 64 * emu.mpp_waves()      # one lane per column that is not zero, at the longest chain
    assert emu.mpp_min_depth() == 0.1
    import map_cases
    abi = map_cases.abi
    assert abi.MAP_MIN_DEPTH == emu.mpp_min_depth() and abi.RVIO_MAP_MAX_POINTS == emu.mpp_points()


@pytest.mark.parametrize("batch", [1, 8, 128])
def test_block_sizes_at_every_window(emu, batch):
    for max_len in range(3, 33):
        dmax = 24 + 6 * (max_len - 1)
        assert emu.mpp_H_stride(dmax) == 16 * dmax
        # rows | r | sigma | (gamma, applied) | the record | eight slot records | the flag, per instance
        want = batch * (8 * 16 * dmax + 8 * 16 + 8 * 16 + 16 + 32 + 8 * 40 + 4)
        assert emu.mpp_block_bytes(batch, dmax) == want, (max_len, batch)
        # the flags lie behind everything else: 4-byte aligned whatever the batch
        assert (want - 4 * batch) % 4 == 0 and (8 * 16 * dmax * batch) % 8 == 0


@pytest.mark.parametrize("batch", [1, 8, 128])
def test_four_waves_per_instance_within_a_cu(emu, static_lds, batch):
    names = [emu.mpp_kernel_name(k).decode() for k in range(emu.mpp_num_kernels())]
    assert NAME in names and NAME in static_lds, "map_rows_kernel must be named in kLpKernelName and present in the built library"
    out = (C.c_long * 6)()
    emu.mpp_launch(batch, out)
    gx, gy, gz, threads, lds, kern = list(out)
    assert (gx, gy, gz, threads) == (1, 1, batch, 256)
    assert names[kern] == NAME and lds == 0
    st = static_lds[NAME]
    print("batch %d: static LDS of %s = %d B (the plan counts %d B), dynamic 0" % (batch, NAME, st, 8 * emu.mpp_lds_doubles()))
    # what the plan counts, the eight status words and alignment, nothing else
    assert 8 * emu.mpp_lds_doubles() <= st <= 8 * emu.mpp_lds_doubles() + 256 and st + lds <= LIMIT
    # the plan sets no dynamic-LDS limit for it and accepts the stock handle with this static part ...
    statics = (C.c_size_t * len(names))(*[static_lds[nm] for nm in names])
    attr = C.c_long(-1)
    assert emu.mpp_plan(11, 200, batch, statics, kern, C.byref(attr)) == 0 and attr.value == 0
    # ... and refuses a build whose kernel would not fit a CU
    statics[kern] = LIMIT + 8
    assert emu.mpp_plan(11, 200, batch, statics, kern, C.byref(attr)) == 1
