"""CPU-side checks of the per-instance calibration surface of the C-ABI (added within ABI 6, purely additive): the five entry points are
exported and declared, rvio_calibration has the layout a C compiler gives the header's struct and the ctypes mirror has the same one,
rvio_calibration_from_config copies the calibration members of a config, NULL handles are refused, and the header names what stays common
to all instances of a handle.  No compute is launched here."""
import ctypes as C
import os
import re
import subprocess

import pytest

import oracle as O

abi = O.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rvio_calibration_from_config", "rvio_hip_set_calibration_at", "rvio_hip_set_calibrations", "rvio_hip_get_calibration_at",
       "rvio_hip_initialize_at")
FIELDS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "fisheye", "T_bc")


@pytest.fixture(scope="module")
def lib():
    from rvio_amd import build, hip
    build.build()
    return hip.load()


def header():
    return open(os.path.join(ROOT, "include", "rvio_hip.h")).read()


def test_symbols_exported_and_declared_within_abi_6(lib):
    from rvio_amd import hip
    assert abi.ABI_VERSION == 6 and lib.rvio_hip_abi_version() == 6
    hdr = header()
    declared = set(re.findall(r"\b(rvio_(?:hip_)?[a-z_]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in hip.SYMBOLS and hasattr(lib, s), s
    assert "#define RVIO_HIP_ABI_VERSION 6" in hdr and "within 6" in hdr.lower()
    # additive: the structs that existed keep their sizes
    assert C.sizeof(abi.rvio_config) == 312 and C.sizeof(abi.rvio_odom) == 464 and C.sizeof(abi.rvio_frame_info) == 64


def test_struct_layout_matches_a_c_compiler(tmp_path):
    assert C.sizeof(abi.rvio_calibration) == 168
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rvio_hip.h"\nint main(void) {\n  printf("%zu", sizeof(rvio_calibration));\n'
                   + "".join('  printf(" %%zu", offsetof(rvio_calibration, %s));\n' % f for f in FIELDS) + '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == 168
    assert got[1:] == [getattr(abi.rvio_calibration, f).offset for f in FIELDS]
    assert got[1:] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40]        # no padding: 9 floats + one int32 + 16 doubles = 40 + 128
    assert [n for n, _ in abi.rvio_calibration._fields_] == list(FIELDS)


def test_from_config_round_trips_the_stock_config(lib):
    cfg = abi.rvio_config()
    lib.rvio_config_euroc(C.byref(cfg))
    k = abi.rvio_calibration()
    C.memset(C.byref(k), 0xff, C.sizeof(k))                           # every byte is written
    lib.rvio_calibration_from_config.restype = None
    lib.rvio_calibration_from_config(C.byref(cfg), C.byref(k))
    assert bytes(k) == bytes(abi.calibration_from_config(cfg)) == bytes(abi.calibration_from_config(abi.config_euroc()))
    for f in FIELDS[:-1]:
        assert getattr(k, f) == getattr(cfg, f), f
    assert list(k.T_bc) == list(cfg.T_bc) and k.T_bc[3] == -0.0216401454975 and k.fx == C.c_float(458.654).value
    # ... and back: a config given these members is the stock config again
    back = abi.config_euroc(fx=1.0, fy=1.0, cx=0.0, cy=0.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=1.0, fisheye=1)
    for i in range(16):
        back.T_bc[i] = 0.0
    for f in FIELDS[:-1]:
        setattr(back, f, getattr(k, f))
    for i in range(16):
        back.T_bc[i] = k.T_bc[i]
    assert bytes(back) == bytes(cfg)
    # another camera: the fisheye flag and a different extrinsic arrive as they are
    other = abi.config_euroc(fisheye=1, k1=-0.0137, k3=0.25, fx=300.0)
    other.T_bc[7] = 0.125
    lib.rvio_calibration_from_config(C.byref(other), C.byref(k))
    assert k.fisheye == 1 and k.k3 == 0.25 and k.fx == 300.0 and k.T_bc[7] == 0.125
    assert bytes(k) == bytes(abi.calibration_from_config(other))
    lib.rvio_calibration_from_config(None, C.byref(k))                # NULL arguments: nothing happens
    lib.rvio_calibration_from_config(C.byref(other), None)
    assert k.fx == 300.0


def test_null_arguments_are_invalid(lib):
    k = abi.calibration_from_config(abi.config_euroc())
    w = (C.c_double * 3)(0, 0, 0)
    a = (C.c_double * 3)(0, 0, 9.8)
    assert lib.rvio_hip_set_calibration_at(None, 0, C.byref(k)) == -1
    assert lib.rvio_hip_set_calibrations(None, C.byref(k)) == -1
    assert lib.rvio_hip_get_calibration_at(None, 0, C.byref(k)) == -1
    assert lib.rvio_hip_initialize_at(None, 0, w, a, 10) == -1


def test_header_names_every_handle_wide_exception():
    """what a fleet canNOT bind per robot is stated where the entry points are declared"""
    hdr = header()
    a = hdr.index("per-instance calibration ---")
    doc = hdr[a: hdr.index("int rvio_hip_get_calibration_at", a)]
    assert "HANDLE-WIDE" in doc
    for word in ("width, height", "sigma_px", "sigma_py", "Tracker.*", "IMU.*", "INI.*"):
        assert word in doc, word
    for key in ("n_features", "max_track_len", "min_track_len", "min_dist", "qual_lvl", "block_x", "block_y", "enable_equalizer", "use_sampson",
                "inlier_thr", "imu_rate", "gravity", "small_angle"):
        assert key in doc, key
    # the semantics a caller relies on
    for phrase in ("drains the handle", "BEFORE THE FIRST FRAME", "tracking history", "rvio_hip_debug_poison", "instance 0 only", "non-finite"):
        assert phrase in doc, phrase
    batch_doc = hdr[hdr.index("--- batched instances"): hdr.index("int rvio_hip_create_batch")]
    assert "replays of the same sensor" not in batch_doc and "rvio_hip_set_calibration_at" in batch_doc
    assert "RVIO_ERR_STATE when the window is not empty" in hdr


def test_wrapper_refuses_a_wrong_number_of_calibrations():
    from rvio_amd import hip
    h = hip.RvioHip.__new__(hip.RvioHip)
    h.h, h.batch = None, 3
    with pytest.raises(hip.RvioHipError):
        h.set_calibrations([abi.calibration_from_config(abi.config_euroc())] * 2)
