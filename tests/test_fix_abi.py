"""CPU-side checks of the absolute fixes (added within ABI 6): the entry points are exported, declared and named on the ABI-version line; the
two structs have the layout a C++ compiler gives the header's; NULL handles are refused; and abi.fix_model — the NumPy model the device is held
to — is held to finite differences of the predicted measurement abi.fix_h through the reference's state injection, to the pose-covariance
Jacobian the IMU-rate odometry already uses, and to what an update with it must do: pull the state onto the fix.  No compute is launched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fix_cases as F

abi, A = F.abi, F.A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rvio_hip_update_fix", "rvio_hip_update_fix_dev", "rvio_hip_get_fix", "rvio_hip_get_fix_rows")
FIX_FIELDS, DIAG_FIELDS = ("z", "sigma", "lever"), ("r", "gamma", "applied", "kind", "m", "img_count")
CPU_STATES = ("window10", "moved", "zero_qk")
EPS = 1e-5


@pytest.fixture(scope="module")
def lib():
    from rvio_amd import build, hip
    build.build()
    return hip.load()


def test_symbols_exported_and_declared_within_abi_6(lib):
    from rvio_amd import hip
    assert abi.ABI_VERSION == 6 and lib.rvio_hip_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "rvio_hip.h")).read()
    declared = set(re.findall(r"\b(rvio_(?:hip_)?[a-z_]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in hip.SYMBOLS and hasattr(lib, s), s
    version_line = [l for l in hdr.splitlines() if l.startswith("#define RVIO_HIP_ABI_VERSION")][0]
    assert "#define RVIO_HIP_ABI_VERSION 6" in version_line and all(s in version_line for s in NEW + ("rvio_fix", "rvio_fix_diag"))
    assert re.search(r"RVIO_FIX_POSITION\s*=\s*0\s*,\s*RVIO_FIX_ATTITUDE\s*=\s*1\s*,\s*RVIO_FIX_POSE\s*=\s*2\s*,\s*RVIO_FIX_GRAVITY\s*=\s*3", hdr)
    assert (abi.RVIO_FIX_POSITION, abi.RVIO_FIX_ATTITUDE, abi.RVIO_FIX_POSE, abi.RVIO_FIX_GRAVITY) == (0, 1, 2, 3)
    assert abi.FIX_ROWS == {0: 3, 1: 3, 2: 6, 3: 3}


def test_struct_layout_matches_a_cxx_compiler(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "rvio_hip.h"\nint main() {\n  std::printf("%zu", sizeof(rvio_fix));\n'
                   + "".join('  std::printf(" %%zu", offsetof(rvio_fix, %s));\n' % f for f in FIX_FIELDS)
                   + '  std::printf(" %zu", sizeof(rvio_fix_diag));\n'
                   + "".join('  std::printf(" %%zu", offsetof(rvio_fix_diag, %s));\n' % f for f in DIAG_FIELDS) + '  std::printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == C.sizeof(abi.rvio_fix) == abi.FIX_DTYPE.itemsize == 128
    assert got[1:4] == [getattr(abi.rvio_fix, f).offset for f in FIX_FIELDS] == [0, 56, 104]
    assert got[4] == C.sizeof(abi.rvio_fix_diag) == 72
    assert got[5:] == [getattr(abi.rvio_fix_diag, f).offset for f in DIAG_FIELDS] == [0, 48, 56, 60, 64, 68]


def test_null_arguments_are_invalid(lib):
    f = abi.make_fix((0, 0, 0), (0, 0, 0, 1), 1.0, 1.0)
    out = abi.rvio_fix_diag()
    m, d = C.c_int32(0), C.c_int32(0)
    assert lib.rvio_hip_update_fix(None, 0, 0, 0, C.byref(f)) == -1
    assert lib.rvio_hip_update_fix_dev(None, 0, 0, C.byref(f), C.c_size_t(0), None) == -1
    assert lib.rvio_hip_get_fix(None, 0, C.byref(out)) == -1
    assert lib.rvio_hip_get_fix_rows(None, 0, C.byref(m), C.byref(d), None, None) == -1


# ---------------------------------------------------------------- the NumPy model against finite differences
def _measure(cfg, x, kind, fix):
    """what is differenced: the predicted position / accelerometer reading, and MINUS the attitude residual against the fixed z"""
    out = []
    if kind != abi.RVIO_FIX_ATTITUDE:
        out.append(abi.fix_h(cfg, x, kind, fix.lever)[0:3])
    if kind in (abi.RVIO_FIX_ATTITUDE, abi.RVIO_FIX_POSE):
        out.append(-abi.fix_model(cfg, x, kind, fix)[1][-3:])
    return np.concatenate(out)


@pytest.mark.parametrize("lever", F.LEVERS, ids=["lever", "nolever"])
@pytest.mark.parametrize("kind", F.KINDS, ids=[F.KIND_NAMES[k] for k in F.KINDS])
@pytest.mark.parametrize("name", CPU_STATES)
def test_jacobian_against_central_differences(name, kind, lever):
    cfg = A.K.config()
    x, P = F.cpu_state(name)
    d = P.shape[0]
    h = abi.fix_h(cfg, x, kind, lever)
    fix = abi.make_fix(h[0:3], h[3:7] if h[3:7].any() else (0, 0, 0, 1), 1.0, 1.0, lever)   # (z = the state's own prediction: the attitude residual is linear around 0 only)
    H, r, sigma = abi.fix_model(cfg, x, kind, fix)
    assert H.shape == (abi.FIX_ROWS[kind], d) and np.max(np.abs(r)) < 1e-12
    Hfd = np.zeros_like(H)
    for c in range(d):
        e = np.zeros(d)
        e[c] = EPS
        Hfd[:, c] = (_measure(cfg, abi.inject_state(x, e), kind, fix) - _measure(cfg, abi.inject_state(x, -e), kind, fix)) / (2 * EPS)
    g = x[7:10]
    want = H.copy()
    want[:, 6:9] = H[:, 6:9] @ (np.eye(3) - np.outer(g, g))      # (inject_state re-normalises g: only the tangent part of a step is taken)
    s = x[14:17] - x[4:7] + abi.quat_to_rot(x[10:14]).T @ np.asarray(lever)
    bar = 1e-8 * max(1.0, float(np.linalg.norm(s)), cfg.gravity)
    worst = float(np.max(np.abs(Hfd - want)))
    print("%s %s lever %s: max|H - FD| = %.3e (bar %.3e, max|H| %.3g)" % (name, F.KIND_NAMES[kind], lever, worst, bar, np.max(np.abs(H))))
    assert worst <= bar
    used = np.abs(H).sum(axis=0) > 0
    assert not used[24:].any() and used[:24].any()          # no clone column, and not an all-zero Jacobian


@pytest.mark.parametrize("name", CPU_STATES)
def test_pose_rows_without_lever_are_the_odometry_jacobian(name):
    cfg = A.K.config()
    x, P = F.cpu_state(name)
    fix = F.fix_near(cfg, x, abi.RVIO_FIX_POSE)
    H = abi.fix_model(cfg, x, abi.RVIO_FIX_POSE, fix)[0]
    qk = x[10:14] if x[10:14].any() else np.array([0.0, 0.0, 0.0, 1.0])
    J = abi.imu_pose_cov_jacobian(x[0:4], x[4:7], qk, x[14:17])
    want = np.zeros_like(H)
    want[:, list(abi.IMU_COV_COLS)] = J
    worst = float(np.max(np.abs(H - want)))
    print("%s: max|H_pose - imu_pose_cov_jacobian| = %.3e" % (name, worst))
    assert worst <= 1e-14 * max(1.0, float(np.max(np.abs(J))))


@pytest.mark.parametrize("lever", F.LEVERS, ids=["lever", "nolever"])
@pytest.mark.parametrize("kind", F.KINDS, ids=[F.KIND_NAMES[k] for k in F.KINDS])
@pytest.mark.parametrize("name", ["window10", "moved"])
def test_the_update_pulls_the_state_onto_the_fix(name, kind, lever):
    cfg = A.K.config()
    x, P = F.cpu_state(name)
    fix = F.fix_near(cfg, x, kind, lever, dp=0.05, dth=0.01, sigma_p=1e-4, sigma_q=1e-4)
    H, r, sigma = abi.fix_model(cfg, x, kind, fix)
    want = {abi.RVIO_FIX_POSE: [0.05, 0.01]}.get(kind, [0.01 if kind == abi.RVIO_FIX_ATTITUDE else 0.05])
    got = [float(np.linalg.norm(r[3 * i: 3 * i + 3])) for i in range(len(r) // 3)]
    assert np.allclose(got, want, rtol=1e-3), (got, want)
    x1 = abi.aux_update_model(x, P, H, r, sigma)[0]
    r1 = abi.fix_model(cfg, x1, kind, fix)[1]
    ratio = float(np.linalg.norm(r1) / np.linalg.norm(r))
    print("%s %s lever %s: |r| %.3e -> %.3e (ratio %.3e)" % (name, F.KIND_NAMES[kind], lever, np.linalg.norm(r), np.linalg.norm(r1), ratio))
    assert ratio < 0.1
