"""The launch form of the auxiliary measurement update (csrc/launch_plan.h aux_update_launch), compiled with g++ from
tests/hostemu/aux_plan_emu.cpp and swept on the CPU: for every window 0 .. 31 and batch 1 / 8 / 128 the dynamic LDS the launch asks for plus
the kernel's static LDS — read from the built library's gfx950 code object — fits the 160 KiB of a CU, stays within the limit the handle set
when it was created, and the T product's deal of row groups x column ranges fits the workgroup's eight waves."""
import ctypes as C
import os
import subprocess

import pytest

from code_object import read_static_lds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "aux_plan_emu.cpp")
HDR = os.path.join(ROOT, "r-vio_amd", "csrc", "launch_plan.h")
LIMIT = 163840


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("aux_plan") / "aux_plan_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unused-variable", SRC, "-o", so])
    L = C.CDLL(so)
    L.ap_kernel_name.restype = C.c_char_p
    L.ap_lds_limit.restype = C.c_long
    L.ap_attr.restype = C.c_long
    return L


@pytest.fixture(scope="module")
def static_lds():
    """{kernel name as c++filt prints it: static LDS in bytes} of the built library's gfx950 code object (as tests/test_launch_plan.py reads it)"""
    return read_static_lds()


def launch(emu, n, m, batch):
    out = (C.c_long * 6)()
    emu.ap_launch(n, m, batch, out)
    return dict(zip(("gx", "gy", "gz", "threads", "lds", "kernel"), out))


def test_constants(emu):
    assert emu.ap_lds_limit() == LIMIT and emu.ap_max_rows() == 16 and emu.ap_threads() == 512
    hdr = open(os.path.join(ROOT, "include", "rvio_hip.h")).read()
    assert "#define RVIO_AUX_MAX_ROWS 16" in hdr


@pytest.mark.parametrize("batch", [1, 8, 128])
def test_every_window_fits_a_cu(emu, static_lds, batch):
    nk = emu.ap_num_kernels()
    names = [emu.ap_kernel_name(k).decode() for k in range(nk)]
    assert "aux_update_kernel<4>" in names and "aux_update_kernel<16>" in names
    statics = (C.c_size_t * nk)(*[static_lds[nm] for nm in names])
    worst = 0
    for n in range(0, 32):
        d = 24 + 6 * n
        G = (d + 63) // 64
        assert G * emu.ap_splits(G) <= 512 // 64 and G <= 4
        for m in range(1, 17):
            l = launch(emu, n, m, batch)
            name = names[l["kernel"]]
            assert name == ("aux_update_kernel<4>" if m <= 4 else "aux_update_kernel<16>")
            assert (l["gx"], l["gy"], l["gz"], l["threads"]) == (1, 1, batch, 512)      # one workgroup per instance, ONE form at every batch size
            tot = l["lds"] + static_lds[name]
            worst = max(worst, tot)
            assert tot <= LIMIT, (n, m, batch, tot)
            # within the limit create set for the kernel on every handle whose window can hold n clones
            for ml in range(max(3, n + 1), 33):
                attr = emu.ap_attr(ml, 200, batch, statics, l["kernel"])
                assert attr == -1 or l["lds"] <= attr, (n, m, ml, l["lds"], attr)
            assert l["lds"] == launch(emu, n, m, 1)["lds"]
    print("batch %d: worst static + dynamic LDS of the aux launch = %d B (static %d / %d)" % (
        batch, worst, static_lds["aux_update_kernel<4>"], static_lds["aux_update_kernel<16>"]))
    assert worst > 100 * 1024      # (the sweep saw the full window at 16 rows)
