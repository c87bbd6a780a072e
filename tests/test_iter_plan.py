"""The launch form of one pass of the iterated measurement update (csrc/launch_plan.h aux_iter_launch), compiled with g++ from
tests/hostemu/iter_plan_emu.cpp and swept on the CPU: for every window 0 .. 31 and MB 4 / 16 the dynamic LDS the launch asks for plus the
kernel's static LDS — read from the built library's gfx950 code object — fits the 160 KiB of a CU and stays within the limit the handle set
when it was created; it is the plain launch's footprint plus d doubles; the chain's block holds what the kernel indexes."""
import ctypes as C
import os
import subprocess

import pytest

from code_object import read_static_lds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "iter_plan_emu.cpp")
LIMIT = 163840


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("iter_plan") / "iter_plan_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unused-variable", SRC, "-o", so])
    L = C.CDLL(so)
    L.ip_kernel_name.restype = C.c_char_p
    for f in (L.ip_lds_limit, L.ip_attr, L.ip_x0_stride, L.ip_block_bytes):
        f.restype = C.c_long
    return L


@pytest.fixture(scope="module")
def static_lds():
    return read_static_lds()


def launch(emu, n, m, batch, plain=0):
    out = (C.c_long * 6)()
    emu.ip_launch(n, m, batch, plain, out)
    return dict(zip(("gx", "gy", "gz", "threads", "lds", "kernel"), out))


def test_constants(emu):
    assert emu.ip_lds_limit() == LIMIT and emu.ip_max_iters() == 8 and emu.ip_threads() == 512
    hdr = open(os.path.join(ROOT, "include", "rvio_hip.h")).read()
    assert "#define RVIO_MEAS_MAX_ITERS 8" in hdr


@pytest.mark.parametrize("batch", [1, 4])
def test_every_window_fits_a_cu(emu, static_lds, batch):
    nk = emu.ip_num_kernels()
    names = [emu.ip_kernel_name(k).decode() for k in range(nk)]
    assert "aux_iter_kernel<4>" in names and "aux_iter_kernel<16>" in names
    assert names.index("aux_iter_kernel<4>") > names.index("map_rows_kernel")           # appended: the earlier families keep their numbers
    statics = (C.c_size_t * nk)(*[static_lds[nm] for nm in names])
    worst = 0
    for n in range(0, 32):
        d = 24 + 6 * n
        for m in (1, 3, 4, 5, 6, 16):                                                  # MB 4 up to four rows, MB 16 beyond
            l = launch(emu, n, m, batch)
            name = names[l["kernel"]]
            assert name == ("aux_iter_kernel<4>" if m <= 4 else "aux_iter_kernel<16>")
            assert (l["gx"], l["gy"], l["gz"], l["threads"]) == (1, 1, batch, 512)
            assert l["lds"] == launch(emu, n, m, batch, plain=1)["lds"] + 8 * d          # dx of the previous pass beside the plain footprint
            tot = l["lds"] + static_lds[name]
            worst = max(worst, tot)
            assert tot <= LIMIT, (n, m, batch, tot)
            for ml in range(max(3, n + 1), 33):
                attr = emu.ip_attr(ml, 200, batch, statics, l["kernel"])
                assert attr == -1 or l["lds"] <= attr, (n, m, ml, l["lds"], attr)
    print("batch %d: worst static + dynamic LDS of a pass = %d B (static %d / %d)" % (
        batch, worst, static_lds["aux_iter_kernel<4>"], static_lds["aux_iter_kernel<16>"]))
    assert 120000 < worst <= LIMIT        # (the sweep saw the full window at 16 rows: about 122.3 KB)


def test_the_block_holds_what_the_kernel_indexes(emu):
    for nmax in (2, 10, 31):
        dmax = 24 + 6 * nmax
        xs = emu.ip_x0_stride(nmax)
        assert xs == 26 + 7 * nmax + 7                                                  # the state, then the pose line
        for B in (1, 4, 2048):
            assert emu.ip_block_bytes(B, nmax, dmax) == B * (8 * xs + 8 * dmax + 24 + 4)  # snapshots | dx | records | running flags
