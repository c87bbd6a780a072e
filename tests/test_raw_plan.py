"""The launch form of the raw-sensor gray conversion: front_forms() of r-vio_amd/csrc/launch_plan.h compiled with g++
(tests/hostemu/raw_plan_emu.cpp) and swept over every new image format x W % 4 x aligned / unaligned source x batch 1 / 8.

What DESIGN.md section 3 documents: each family has a wide form (a lane converts four adjacent pixels from aligned dwords), taken exactly when
W % 4 == 0 and base address, row stride and instance stride of the source are multiples of four bytes, and a plain form for everything else;
both are launched as one wave per 256 pixels of a row, four rows per workgroup, one grid layer per instance, without dynamic LDS.  The five
8-bit formats keep the forms (and enum values) they had before raw input existed."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostemu", "raw_plan_emu.cpp")
HDR = os.path.join(HERE, "..", "r-vio_amd", "csrc", "launch_plan.h")
LIB = os.path.join(HERE, "hostemu", "libraw_plan_emu.so")

# format value -> (samples per pixel, bits, bayer, family of its LpGray names)
NEW = {16: (1, 16, 0, "16_1"), 17: (3, 16, 0, "16_3"), 18: (3, 16, 0, "16_3"), 19: (4, 16, 0, "16_4"), 20: (4, 16, 0, "16_4")}
NEW.update({f: (1, 8, 1, "BAYER8") for f in (32, 33, 34, 35)})
NEW.update({f: (1, 16, 1, "BAYER16") for f in (48, 49, 50, 51)})


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unused-variable", SRC, "-o", LIB])
    L = C.CDLL(LIB)
    L.rp_form.argtypes = [C.c_char_p]
    return L


def front(emu, batch, W, H, channels, bits=8, bayer=0, src_dword=1, throughput=0, equalizer=0):
    vin = (C.c_long * 9)(batch, throughput, W, H, equalizer, channels, bits, bayer, src_dword)
    out = (C.c_long * 8)()
    assert emu.rp_front(vin, out) == 0
    return dict(zip(("gray", "gx", "gy", "gz", "threads", "lds", "kernel", "clahe_interp"), out))


def form_name(family, wide):
    return (("W" if wide else "P") + family) if family[0] == "1" else family + ("_W" if wide else "_P")


@pytest.mark.parametrize("fmt", sorted(NEW))
def test_every_new_format_gets_the_documented_form(emu, fmt):
    ch, bits, bayer, family = NEW[fmt]
    seen = set()
    for B in (1, 8):
        for H in (240, 243):
            for W in (376, 377, 378, 379, 768, 769):
                for aligned in (0, 1):
                    f = front(emu, B, W, H, ch, bits, bayer, aligned, throughput=int(B >= 8))
                    wide = W % 4 == 0 and aligned == 1
                    assert f["gray"] == emu.rp_form(form_name(family, wide).encode()) and f["gray"] > 4, (B, W, H, aligned, f)
                    seen.add(f["gray"])
                    # the grid covers W x H: a wave per 256 pixels of a row, four rows per workgroup, a layer per instance
                    assert f["threads"] == 256 and f["gx"] * 256 >= W > (f["gx"] - 1) * 256, f
                    assert f["gy"] * 4 >= H > (f["gy"] - 1) * 4 and f["gz"] == B, f
                    assert 0 <= f["lds"] <= emu.rp_lds_limit() == 163840 and f["lds"] == 0 and f["kernel"] == -1, f
    assert len(seen) == 2


def test_the_new_forms_are_all_different(emu):
    names = ["W16_1", "P16_1", "W16_3", "P16_3", "W16_4", "P16_4", "BAYER8_W", "BAYER8_P", "BAYER16_W", "BAYER16_P"]
    vals = [emu.rp_form(n.encode()) for n in names]
    assert len(set(vals)) == 10 and min(vals) == 5


def test_the_old_formats_give_what_they_gave(emu):
    """LPGR_NONE = 0 without a launch for mono, gray_kernel4<3> = 1, gray_kernel<3> = 2, gray_kernel4<4> = 3, gray_kernel<4> = 4"""
    for B in (1, 8):
        for W in (376, 377, 378, 379):
            for aligned in (0, 1):
                wide = W % 4 == 0 and aligned == 1
                m = front(emu, B, W, 240, 1, src_dword=aligned)
                assert (m["gray"], m["gx"], m["threads"], m["lds"]) == (0, 0, 0, 0), m
                for ch, forms in ((3, (2, 1)), (4, (4, 3))):
                    f = front(emu, B, W, 240, ch, src_dword=aligned)
                    assert f["gray"] == forms[wide], (B, W, aligned, ch, f)
                    assert (f["gx"], f["gy"], f["gz"], f["threads"], f["lds"], f["kernel"]) == ((W + 255) // 256, 60, B, 256, 0, -1), f


def test_a_mosaic_of_one_byte_per_pixel_is_converted(emu):
    """"is a conversion launched" is not "more than one byte per pixel": behind an 8-bit mosaic CLAHE reads the handle's gray buffer (rows of W
    bytes), so its four-pixel form follows from W alone — behind a mono image from the caller's alignment"""
    px4, px1 = emu.rp_form(b"PX4"), emu.rp_form(b"PX1")
    for aligned in (0, 1):
        b = front(emu, 8, 376, 240, 1, 8, 1, aligned, throughput=1, equalizer=1)
        assert b["gx"] > 0 and b["clahe_interp"] == px4
        m = front(emu, 8, 376, 240, 1, 8, 0, aligned, throughput=1, equalizer=1)
        assert m["gx"] == 0 and m["clahe_interp"] == (px4 if aligned else px1)
    assert front(emu, 8, 378, 240, 1, 8, 1, 1, throughput=1, equalizer=1)["clahe_interp"] == px1
