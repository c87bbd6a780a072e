"""The arithmetic of the device's raw-sensor gray conversion (r-vio_amd/csrc/raw.h: what raw16_kernel / raw16_kernel4 / bayer_kernel /
bayer_kernel4 compute), compiled with g++ (tests/hostemu/raw_emu.cpp) and walked the way each kernel form walks an image, against NumPy:
the depth step over all 65 536 values, 16-bit colour against int64 sums, the mosaics against tests/raw_model.py (padded-array slices and one
mask per site kind — not a transliteration of the header).  Integers in, integers out: every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import raw_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostemu", "raw_emu.cpp")
HDRS = [os.path.join(HERE, "..", "r-vio_amd", "csrc", f) for f in ("raw.h", "gray.h")]
LIB = os.path.join(HERE, "hostemu", "libraw_emu.so")
SIZES = [(3, 3), (4, 5), (5, 4), (7, 9), (258, 6), (8, 3), (260, 5), (516, 4)]     # W x H; the last three: whole groups of four for the wide walk


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", SRC, "-o", LIB])
    L = C.CDLL(LIB)
    L.raw_emu_depth.argtypes = [C.c_void_p, C.c_long, C.c_void_p]
    L.raw_emu_depth.restype = None
    L.raw_emu_px16.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p]
    L.raw_emu_px16.restype = None
    L.raw_emu_wide16.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p]
    L.raw_emu_wide16.restype = C.c_int
    for f in (L.raw_emu_bayer, L.raw_emu_bayer_wide):
        f.argtypes = [C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_int, C.c_int, C.c_void_p]
        f.restype = C.c_int
    return L


def test_depth_step_over_all_values(emu):
    v = np.arange(65536, dtype=np.uint16)
    got = np.full(65536, 0x5A, np.uint8)
    emu.raw_emu_depth(v.ctypes.data, 65536, got.ctypes.data)
    want = (v.astype(np.int64) + 128) // 257
    assert want.max() == 255 and want.min() == 0
    assert np.array_equal(got, want)
    assert np.array_equal(got, np.rint(v.astype(np.float64) * (255. / 65535.)))
    assert np.array_equal(got, np.rint(v.astype(np.float32) * np.float32(255. / 65535.)))
    assert np.array_equal(got, np.rint(v.astype(np.float64) * 255 / 65535))
    assert np.array_equal(got, np.rint(v.astype(np.float32) * np.float32(255) / np.float32(65535)))
    got4 = np.zeros(65536, np.uint8)                  # ... and as raw16_kernel4<1> sees them: four samples in two dwords
    assert emu.raw_emu_wide16(v.ctypes.data, 65536, 1, 0, got4.ctypes.data) == 0
    assert np.array_equal(got4, want)


def triples16(n=1 << 20):
    rng = np.random.default_rng(16)
    t = rng.integers(0, 65536, (n, 3), dtype=np.uint16)
    corners = np.array([[r, g, b] for r in (0, 65535) for g in (0, 65535) for b in (0, 65535)], np.uint16)
    t[:8] = corners
    t[8:16] = corners[::-1]
    return t


@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("bgr", [0, 1])
def test_16_bit_colour_both_forms(emu, ch, bgr):
    t = triples16()
    n = len(t)
    r, g, b = (t[:, i].astype(np.int64) for i in range(3))
    y16 = (r * 4899 + g * 9617 + b * 1868 + 8192) >> 14
    assert y16.max() == 65535 and y16.min() == 0
    want = ((y16 + 128) // 257).astype(np.uint8)
    px = np.empty((n, ch), np.uint16)
    px[:, 0], px[:, 1], px[:, 2] = (t[:, 2], t[:, 1], t[:, 0]) if bgr else (t[:, 0], t[:, 1], t[:, 2])
    if ch == 4:
        px[:, 3] = np.random.default_rng(ch + bgr).integers(0, 65536, n, dtype=np.uint16)     # alpha: ignored
    got = np.full(n, 0x5A, np.uint8)
    emu.raw_emu_px16(px.ctypes.data, n, ch, bgr, got.ctypes.data)
    assert np.array_equal(got, want), int((got != want).sum())
    got4 = np.full(n, 0xA5, np.uint8)
    assert emu.raw_emu_wide16(px.ctypes.data, n, ch, bgr, got4.ctypes.data) == 0
    assert np.array_equal(got4, want), int((got4 != want).sum())
    assert np.array_equal(M.gray16(px.reshape(1, n, ch), not bgr)[0], want)                   # the shared model says the same


def images(w, h, bits):
    """random, all-zero, all-max, and one with a single saturated colour plane of the RGGB layout (every pattern reads it as some plane)"""
    top = (1 << bits) - 1
    dt = np.uint8 if bits == 8 else np.uint16
    rng = np.random.default_rng(w * 1000 + h * 10 + bits)
    out = [rng.integers(0, top + 1, (h, w)).astype(dt), np.zeros((h, w), dt), np.full((h, w), top, dt)]
    for plane in ((0, 0), (1, 0), (1, 1)):
        one = np.zeros((h, w), dt)
        one[plane[1]::2, plane[0]::2] = top
        out.append(one)
    return out


def run_bayer(emu, img, pat, wide=False, pad=0):
    h, w = img.shape
    bits = 8 * img.dtype.itemsize
    buf = np.full((h, w + pad), 0x33, img.dtype)     # a padded row stride, in samples
    buf[:, :w] = img
    got = np.full((h, w), 0x5A, np.uint8)
    rc = (emu.raw_emu_bayer_wide if wide else emu.raw_emu_bayer)(buf.ctypes.data, bits, w + pad, w, h, pat, got.ctypes.data)
    assert rc == 0
    return got


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_bayer_against_the_numpy_model(emu, size, bits):
    w, h = size
    for img in images(w, h, bits):
        for pat, name in enumerate(M.PATTERNS):
            want = M.bayer_gray(img, name)
            got = run_bayer(emu, img, pat, pad=3)
            assert np.array_equal(got, want), (name, np.argwhere(got != want)[:4])
            if w % 4 == 0:
                got4 = run_bayer(emu, img, pat, wide=True, pad=4)
                assert np.array_equal(got4, want), (name, np.argwhere(got4 != want)[:4])


def test_the_wide_walk_refuses_what_the_plan_never_gives_it(emu):
    img = np.zeros((5, 6), np.uint8)
    got = np.zeros((5, 6), np.uint8)
    assert emu.raw_emu_bayer_wide(img.ctypes.data, 8, 6, 6, 5, 0, got.ctypes.data) == -1
    assert emu.raw_emu_bayer(img.ctypes.data, 8, 6, 2, 5, 0, got.ctypes.data) == -1


@pytest.mark.parametrize("bits", [8, 16])
def test_a_constant_colour_gives_its_gray_everywhere(emu, bits):
    """a mosaic sampled from one colour gives gray_px(R, G, B) at every pixel, borders included — and read with any other pattern it does not"""
    top = (1 << bits) - 1
    dt = np.uint8 if bits == 8 else np.uint16
    w, h = 12, 7
    for rgb in ((top, top // 3, top // 9), (top // 9, top, top // 2), (top // 2, 3, top)):
        colour = np.broadcast_to(np.array(rgb, dt), (h, w, 3))
        y = int(M.gray_px(*rgb))
        want = y if bits == 8 else (y + 128) // 257
        for pat, name in enumerate(M.PATTERNS):
            m = M.mosaic(colour, name)
            for wide in (False, True):
                got = run_bayer(emu, m, pat, wide=wide)
                assert (got == want).all(), (name, rgb, wide)
            for other, oname in enumerate(M.PATTERNS):
                if other != pat:
                    assert not (run_bayer(emu, m, other) == want).all(), (name, oname)


@pytest.mark.parametrize("bits", [8, 16])
def test_swapping_the_pattern_rows_or_columns_shifts_the_image(emu, bits):
    top = (1 << bits) - 1
    img = np.random.default_rng(bits).integers(0, top + 1, (9, 12)).astype(np.uint8 if bits == 8 else np.uint16)
    h, w = img.shape
    idx = {n: i for i, n in enumerate(M.PATTERNS)}
    for name in M.PATTERNS:
        a = run_bayer(emu, img, idx[name])
        rows = run_bayer(emu, np.ascontiguousarray(img[1:]), idx[M.ROW_SWAP[name]])       # the image without its first row: every site changes row parity
        assert np.array_equal(rows[1:h - 2], a[2:h - 1]), name                            # (rows that are interior in both)
        cols = run_bayer(emu, np.ascontiguousarray(img[:, 1:]), idx[M.COL_SWAP[name]])
        assert np.array_equal(cols[:, 1:w - 2], a[:, 2:w - 1]), name
        assert not np.array_equal(run_bayer(emu, np.ascontiguousarray(img[1:]), idx[name])[1:h - 2], a[2:h - 1])
