"""The arithmetic of the device's gray conversion (r-vio_amd/csrc/gray.h: what gray_kernel and gray_kernel4 compute per pixel), compiled with
g++ (tests/hostemu/gray_emu.cpp) and run over ALL 2^24 (R, G, B) triples, in both channel orders, with three and four bytes per pixel and
through both kernel forms (byte by byte / four pixels from the dwords that hold them), against the NumPy form of OpenCV's 8-bit fixed-point
cvtColor (Tracker.cc:182-196): Y = (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14 — the form tests/test_host.py pins for the host's to_gray.
Integers in, integers out: every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostemu", "gray_emu.cpp")
HDR = os.path.join(HERE, "..", "r-vio_amd", "csrc", "gray.h")
LIB = os.path.join(HERE, "hostemu", "libgray_emu.so")


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", SRC, "-o", LIB])
    L = C.CDLL(LIB)
    L.gray_emu_bytes.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p]
    L.gray_emu_bytes.restype = None
    L.gray_emu_wide.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p]
    L.gray_emu_wide.restype = C.c_int
    return L


@pytest.fixture(scope="module")
def triples():
    """every (R, G, B), shuffled so that the four pixels of a dword group are unrelated, and the NumPy gray of each"""
    v = np.arange(1 << 24, dtype=np.uint32)
    np.random.default_rng(24).shuffle(v)
    r, g, b = (v >> 16) & 255, (v >> 8) & 255, v & 255
    y = ((r.astype(np.int64) * 4899 + g.astype(np.int64) * 9617 + b.astype(np.int64) * 1868 + 8192) >> 14)
    assert y.min() == 0 and y.max() == 255
    return r.astype(np.uint8), g.astype(np.uint8), b.astype(np.uint8), y.astype(np.uint8)


@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("bgr", [0, 1])
def test_all_triples_both_forms(emu, triples, ch, bgr):
    r, g, b, want = triples
    n = len(want)
    px = np.empty((n, ch), np.uint8)
    px[:, 0], px[:, 1], px[:, 2] = (b, g, r) if bgr else (r, g, b)
    if ch == 4:
        px[:, 3] = np.random.default_rng(ch + bgr).integers(0, 256, n, dtype=np.uint8)     # alpha: ignored
    got = np.full(n, 0x5A, np.uint8)
    emu.gray_emu_bytes(px.ctypes.data, n, ch, bgr, got.ctypes.data)
    assert np.array_equal(got, want), "byte form: %d of 2^24 triples differ" % int((got != want).sum())
    got4 = np.full(n, 0xA5, np.uint8)
    assert emu.gray_emu_wide(px.ctypes.data, n, ch, bgr, got4.ctypes.data) == 0
    assert np.array_equal(got4, want), "wide form: %d of 2^24 triples differ" % int((got4 != want).sum())


def test_the_two_orders_differ_and_alpha_does_not_matter(emu):
    px = np.array([[200, 100, 50, 0], [200, 100, 50, 255], [0, 0, 0, 77], [255, 255, 255, 3]], np.uint8)
    out = {}
    for bgr in (0, 1):
        o = np.zeros(4, np.uint8)
        emu.gray_emu_bytes(px.ctypes.data, 4, 4, bgr, o.ctypes.data)
        out[bgr] = o
        assert o[0] == o[1] and o[2] == 0 and o[3] == 255
    assert out[0][0] == (200 * 4899 + 100 * 9617 + 50 * 1868 + 8192) >> 14
    assert out[1][0] == (50 * 4899 + 100 * 9617 + 200 * 1868 + 8192) >> 14 and out[0][0] != out[1][0]
