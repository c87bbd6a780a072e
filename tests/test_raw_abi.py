"""CPU-side checks of the raw-sensor surface of the C-ABI (16-bit and Bayer image formats, added within ABI 6, purely additive): the header's
new rvio_pixel_format values against the Python mirror, the entry points, NULL handles, and the wrapper's packing of uint16 and mosaic
images.  No compute is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O

abi = O.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = {"MONO16": 16, "RGB16": 17, "BGR16": 18, "RGBA16": 19, "BGRA16": 20,
         "BAYER_RGGB8": 32, "BAYER_BGGR8": 33, "BAYER_GBRG8": 34, "BAYER_GRBG8": 35,
         "BAYER_RGGB16": 48, "BAYER_BGGR16": 49, "BAYER_GBRG16": 50, "BAYER_GRBG16": 51}


@pytest.fixture(scope="module")
def lib():
    from rvio_amd import build, hip
    build.build()
    return hip.load()


def test_constants_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "rvio_hip.h")).read()
    for name, val in TABLE.items():
        m = re.search(r"\bRVIO_PIX_%s\s*=\s*(\d+)" % name, hdr)
        assert m and int(m.group(1)) == val == getattr(abi, "RVIO_PIX_" + name), name
    for name, val in (("MONO8", 0), ("RGB8", 1), ("BGR8", 2), ("RGBA8", 3), ("BGRA8", 4)):      # the old five keep their numbers
        m = re.search(r"\bRVIO_PIX_%s\s*=\s*(\d+)" % name, hdr)
        assert m and int(m.group(1)) == val == getattr(abi, "RVIO_PIX_" + name), name
    assert abi.PIX_CHANNELS == {0: 1, 1: 3, 2: 3, 3: 4, 4: 4}                                   # ... and their table is what it was
    assert len(re.findall(r"\bRVIO_PIX_[A-Z0-9_]+\s*=\s*\d+", hdr)) == 18
    assert "within 6" in hdr.lower()


def test_the_layout_table():
    L = abi.PIX_LAYOUT
    assert sorted(L) == sorted(list(range(5)) + list(TABLE.values()))
    for fmt, (bpp, dtype, last) in L.items():
        bits16, bayer = bool(fmt & 16), bool(fmt & 32)                   # the bit coding of the values
        assert dtype == ("uint16" if bits16 else "uint8"), fmt
        samples = 1 if bayer or fmt & 15 == 0 else 3 if fmt & 15 <= 2 else 4
        assert bpp == samples * (2 if bits16 else 1) and last == (None if samples == 1 else samples), fmt
    for fmt in range(5):
        assert L[fmt][0] == abi.PIX_CHANNELS[fmt]
    assert sorted(abi.PIX_ENCODING.values()) == sorted(L)
    assert abi.PIX_ENCODING["bayer_gbrg16"] == 50 and abi.PIX_ENCODING["bgra16"] == 20 and abi.PIX_ENCODING["mono8"] == 0


def test_symbols_and_null_handle(lib):
    from rvio_amd import hip
    assert abi.ABI_VERSION == 6 and lib.rvio_hip_abi_version() == 6
    for s in ("rvio_hip_set_image_format", "rvio_hip_get_image_format"):
        assert s in hip.SYMBOLS and hasattr(lib, s)
    for fmt in TABLE.values():
        assert lib.rvio_hip_set_image_format(None, fmt) == -1
    assert lib.rvio_hip_get_image_format(None) == -1


def bare(fmt):
    """a wrapper object without a device: only its host-side packing, set up as set_image_format would"""
    from rvio_amd import hip
    h = hip.RvioHip.__new__(hip.RvioHip)
    h.h, h.cfg = None, abi.config_named("B", width=8, height=6)
    bpp, h.sample_dtype, ch = abi.PIX_LAYOUT[fmt]
    h.channels = ch or 1
    return h, bpp


def test_wrapper_packs_every_family():
    from rvio_amd import hip
    for fmt in sorted(TABLE.values()):
        h, bpp = bare(fmt)
        _, dtype, last = abi.PIX_LAYOUT[fmt]
        good = (6, 8) if last is None else (6, 8, last)
        img, stride = h._img(np.zeros(good, dtype))
        assert stride == 8 * bpp and img.dtype == np.dtype(dtype) and img.shape == good, fmt
        bad_shapes = [(6, 8, 3)] if last is None else [(6, 8), (6, 8, 7 - last)]
        for bad in bad_shapes:
            with pytest.raises(hip.RvioHipError):
                h._img(np.zeros(bad, dtype))
        if dtype == "uint16":                       # 8-bit samples are not silently widened
            with pytest.raises(hip.RvioHipError):
                h._img(np.zeros(good, np.uint8))


def test_row_padded_views_go_over_as_they_are():
    h, _ = bare(abi.RVIO_PIX_MONO16)
    buf = np.zeros((6, 8 + 3), np.uint16)
    img, stride = h._img(buf[:, :8])
    assert stride == 2 * (8 + 3) and img.ctypes.data == buf.ctypes.data
    h, _ = bare(abi.RVIO_PIX_RGB16)
    buf = np.zeros((6, 8 * 3 + 2), np.uint16)
    img, stride = h._img(buf[:, : 8 * 3].reshape(6, 8, 3))
    assert stride == 2 * (8 * 3 + 2) and img.ctypes.data == buf.ctypes.data
    h, _ = bare(abi.RVIO_PIX_BAYER_GRBG8)
    buf = np.zeros((6, 8 + 5), np.uint8)
    img, stride = h._img(buf[:, :8])
    assert stride == 13 and img.ctypes.data == buf.ctypes.data
    img, stride = h._img(np.zeros((6, 8, 1), np.uint8)[:, :, 0][:, ::1].T.copy().T)      # a view that is not row-major is packed
    assert stride == 8 and img.flags.c_contiguous


def test_an_object_with_only_channels_set_still_works():
    from rvio_amd import hip
    h = hip.RvioHip.__new__(hip.RvioHip)
    h.h, h.cfg, h.channels = None, abi.config_named("B", width=8, height=6), 3
    img, stride = h._img(np.zeros((6, 8, 3), np.uint8))
    assert stride == 24
