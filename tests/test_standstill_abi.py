"""CPU-side checks of standstill detection (added within ABI 6): the five entry points are exported, declared and named on the ABI-version
line; the two structs have the layout a C++ compiler gives the header's; rvio_standstill_config_default follows its formulas; NULL handles are
refused; and abi.standstill_model — the NumPy model the device is held to — has the properties the statistic is used for.  No compute is
launched here.  The thresholds are the tests' own (tests/standstill_cases.py), not the library's defaults."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import standstill_cases as Z

abi = Z.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rvio_standstill_config_default", "rvio_hip_set_standstill", "rvio_hip_standstill", "rvio_hip_standstill_dev", "rvio_hip_get_standstill")
CFG_FIELDS = ("sigma_a", "sigma_w", "imu_thr", "disp_thr_px", "sigma_v", "sigma_bg", "min_pairs", "bias_rows", "gate", "reserved")
REC_FIELDS = ("T", "disparity", "gamma", "n_pairs", "flags", "m", "img_count")


@pytest.fixture(scope="module")
def lib():
    from rvio_amd import build, hip
    build.build()
    return hip.load()


def state0():
    x = np.zeros(26)
    x[3] = x[13] = 1.0
    x[20:23] = [0.002, -0.001, 0.0005]
    x[23:26] = [0.03, 0.01, -0.02]
    return x


def test_symbols_exported_and_declared_within_abi_6(lib):
    from rvio_amd import hip
    assert abi.ABI_VERSION == 6 and lib.rvio_hip_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "rvio_hip.h")).read()
    declared = set(re.findall(r"\b(rvio_(?:hip_)?[a-z_]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in hip.SYMBOLS and hasattr(lib, s), s
    version_line = [l for l in hdr.splitlines() if l.startswith("#define RVIO_HIP_ABI_VERSION")][0]
    assert "#define RVIO_HIP_ABI_VERSION 6" in version_line
    assert all(s in version_line for s in NEW + ("rvio_standstill_config", "rvio_standstill"))


def test_struct_layouts_match_a_cxx_compiler(tmp_path):
    src = tmp_path / "layout.cpp"
    body = '  std::printf("%zu", sizeof(rvio_standstill_config));\n' + "".join('  std::printf(" %%zu", offsetof(rvio_standstill_config, %s));\n' % f for f in CFG_FIELDS)
    body += '  std::printf("\\n%zu", sizeof(rvio_standstill));\n' + "".join('  std::printf(" %%zu", offsetof(rvio_standstill, %s));\n' % f for f in REC_FIELDS)
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "rvio_hip.h"\nint main() {\n' + body + '  std::printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a, b = ([int(v) for v in line.split()] for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert a[0] == C.sizeof(abi.rvio_standstill_config) == 64
    assert a[1:] == [getattr(abi.rvio_standstill_config, f).offset for f in CFG_FIELDS] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60]
    assert b[0] == C.sizeof(abi.rvio_standstill) == 40
    assert b[1:] == [getattr(abi.rvio_standstill, f).offset for f in REC_FIELDS] == [0, 8, 16, 24, 28, 32, 36]


def test_defaults_follow_their_formulas(lib):
    for cfg in (abi.config_euroc(), abi.config_euroc(imu_rate=100, sigma_a=5e-3, sigma_g=3e-4)):
        c = abi.rvio_standstill_config()
        lib.rvio_standstill_config_default.restype = None
        lib.rvio_standstill_config_default(C.byref(cfg), C.byref(c))
        assert c.sigma_a == cfg.sigma_a * math.sqrt(cfg.imu_rate) and c.sigma_w == cfg.sigma_g * math.sqrt(cfg.imu_rate)
        assert (c.imu_thr, c.disp_thr_px, c.sigma_v, c.sigma_bg) == (12.0, 0.5, 0.05, c.sigma_w)
        assert (c.min_pairs, c.bias_rows, c.gate, c.reserved) == (20, 0, 1, 0)
        p = abi.standstill_config_default(cfg)
        assert all(getattr(p, f) == getattr(c, f) for f in CFG_FIELDS)


def test_null_handle_is_invalid(lib):
    c = Z.ss_config()
    imu = Z.imu_batch(state0(), 4)
    ip = imu.ctypes.data_as(C.POINTER(abi.rvio_imu))
    r = abi.rvio_standstill()
    assert lib.rvio_hip_set_standstill(None, C.byref(c)) == -1
    assert lib.rvio_hip_standstill(None, ip, 4, 0) == -1 and lib.rvio_hip_standstill_dev(None, ip, 0, 4, 0) == -1
    assert lib.rvio_hip_get_standstill(None, 0, C.byref(r)) == -1


@pytest.mark.parametrize("m", [10, 200])
def test_model_at_rest_and_in_motion(m):
    x, c = state0(), Z.ss_config()
    T, w_mean, disp, n_pairs, flags = abi.standstill_model(x, Z.imu_batch(x, m, seed=0), None, None, 460.0, 460.0, Z.G, c)
    print("m = %d: T at rest %.3f" % (m, T))
    assert 4.0 <= T <= 8.0
    assert flags == 7 and n_pairs == 0 and disp == 0.0
    assert np.max(np.abs(w_mean - x[20:23])) < 4 * Z.SIGMA_W / math.sqrt(m)
    for kind in ("accel", "turn"):
        Tm, _, _, _, fm = abi.standstill_model(x, Z.imu_batch(x, m, seed=0, kind=kind), None, None, 460.0, 460.0, Z.G, c)
        print("m = %d: T with %s %.1f" % (m, kind, Tm))
        assert Tm > 100.0 and fm == abi.SS_IMG_STATIC


def test_model_has_no_attitude_in_it():
    x, c = state0(), Z.ss_config()
    imu = Z.imu_batch(x, 50, seed=3)
    T0 = abi.standstill_model(x, imu, None, None, 460.0, 460.0, Z.G, c)[0]
    for seed in range(4):
        q = np.random.default_rng(seed).standard_normal(4)
        R = abi.quat_to_rot(q / np.linalg.norm(q))
        rot = imu.copy()
        rot["a"] = (imu["a"] - x[23:26]) @ R.T + x[23:26]        # a common rotation of the bias-free specific forces
        T1 = abi.standstill_model(x, rot, None, None, 460.0, 460.0, Z.G, c)[0]
        assert abs(T1 - T0) <= 1e-9 * T0, (T0, T1)


def test_model_image_statistic_and_veto():
    x = state0()
    imu = Z.imu_batch(x, 10, seed=1)
    rng = np.random.default_rng(5)
    prev = rng.uniform(-0.5, 0.5, (30, 2))
    step = np.tile([3.0 / 460.0, 4.0 / 450.0], (30, 1))        # (3, 4) px: 5 px each
    for thr, min_pairs, want_img in ((0.5, 5, 0), (6.0, 5, 1), (0.5, 31, 1), (0.0, 5, 1), (-1.0, 5, 1)):
        c = Z.ss_config(disp_thr_px=thr, min_pairs=min_pairs)
        T, _, disp, n_pairs, flags = abi.standstill_model(x, imu, prev, prev + step, 460.0, 450.0, Z.G, c)
        assert n_pairs == 30 and abs(disp - 5.0) < 1e-12
        assert flags == (abi.SS_IMU_STATIC | (abi.SS_IMG_STATIC | abi.SS_IS_STATIC if want_img else 0)), (thr, min_pairs, flags)
    # a degenerate batch: the mean specific force vanishes
    z = np.zeros(2, abi.IMU_DTYPE)
    z["a"], z["w"] = x[23:26], x[20:23]
    T, _, _, _, flags = abi.standstill_model(x, z, None, None, 460.0, 460.0, Z.G, Z.ss_config())
    assert not np.isfinite(T) and not flags & abi.SS_IMU_STATIC


@pytest.mark.parametrize("n", [0, 1, 10, 31])
@pytest.mark.parametrize("bias_rows", [0, 1])
def test_measurement_passes_the_value_mode_check(n, bias_rows):
    """rvio_hip_update_aux refuses a VALUE-mode H with a non-zero entry in a rotation column (xi is 0 there): the standstill rows have none"""
    d = 24 + 6 * n
    c = Z.ss_config(bias_rows=bias_rows, sigma_v=0.07, sigma_bg=0.003)
    w_mean = np.array([0.01, -0.02, 0.03])
    H, z, sigma = abi.standstill_measurement(d, w_mean, c)
    rows = 6 if bias_rows else 3
    assert H.shape == (rows, d) and z.shape == sigma.shape == (rows,)
    rot = [col for col in range(d) if col < 3 or 9 <= col < 12 or (col >= 24 and (col - 24) % 6 < 3)]
    assert not H[:, rot].any() and np.all(np.isfinite(H)) and np.all(sigma > 0)
    want = np.zeros((rows, d))
    want[np.arange(rows), 15 + np.arange(rows)] = 1.0
    assert np.array_equal(H, want)
    assert np.array_equal(z[:3], np.zeros(3)) and np.array_equal(sigma[:3], np.full(3, 0.07))
    if bias_rows:
        assert np.array_equal(z[3:], w_mean) and np.array_equal(sigma[3:], np.full(3, 0.003))
    # VALUE mode forms z - H xi(x): the velocity and the bias of the state
    x = np.arange(26 + 7 * n, dtype=float)
    r = z - H @ abi.aux_xi(x)
    assert np.array_equal(r[:3], -x[17:20]) and (not bias_rows or np.array_equal(r[3:], w_mean - x[20:23]))
