"""CPU-side checks of the colour-input surface of the C-ABI (added within ABI 6, purely additive): the two entry points are declared,
exported and listed, they refuse a NULL handle, the Python mirror carries the format constants, and the wrapper refuses an image whose
shape does not match the handle's format.  No compute is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O

abi = O.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rvio_hip_set_image_format", "rvio_hip_get_image_format")


@pytest.fixture(scope="module")
def lib():
    from rvio_amd import build, hip
    build.build()
    return hip.load()


def test_abi_6_exports_the_image_format(lib):
    from rvio_amd import hip
    assert abi.ABI_VERSION == 6 and lib.rvio_hip_abi_version() == 6
    assert C.sizeof(abi.rvio_config) == 312
    hdr = open(os.path.join(ROOT, "include", "rvio_hip.h")).read()
    declared = set(re.findall(r"\b(rvio_(?:hip_)?[a-z_]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in hip.SYMBOLS and hasattr(lib, s), s
    assert "within 6" in hdr.lower()            # the header says that the ABI number did not move


def test_null_handle_is_invalid(lib):
    assert lib.rvio_hip_set_image_format(None, abi.RVIO_PIX_RGB8) == -1
    assert lib.rvio_hip_get_image_format(None) == -1


def test_constants_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "rvio_hip.h")).read()
    for name in ("MONO8", "RGB8", "BGR8", "RGBA8", "BGRA8"):
        m = re.search(r"\bRVIO_PIX_%s\s*=\s*(\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(abi, "RVIO_PIX_" + name), name
    assert abi.PIX_CHANNELS == {0: 1, 1: 3, 2: 3, 3: 4, 4: 4}


def test_wrapper_refuses_a_shape_that_does_not_match_the_format():
    from rvio_amd import hip
    h = hip.RvioHip.__new__(hip.RvioHip)        # no device here: only the host-side packing of the wrapper
    h.h, h.cfg = None, abi.config_named("B", width=8, height=6)
    for ch, good, bad in ((1, (6, 8), (6, 8, 3)), (3, (6, 8, 3), (6, 8)), (3, (6, 8, 3), (6, 8, 4)), (4, (6, 8, 4), (6, 8, 3))):
        h.channels = ch
        img, stride = h._img(np.zeros(good, np.uint8))
        assert stride == 8 * ch
        with pytest.raises(hip.RvioHipError):
            h._img(np.zeros(bad, np.uint8))
    h.channels = 3                              # a row-padded colour view goes over as it is, with its stride in bytes
    buf = np.zeros((6, 8 * 3 + 5), np.uint8)
    view = buf[:, : 8 * 3].reshape(6, 8, 3)
    img, stride = h._img(view)
    assert stride == 8 * 3 + 5 and img.ctypes.data == buf.ctypes.data
