"""CPU-side checks of the odometry ring's C-ABI surface (added within ABI 6): the four entry points are exported and declared, rvio_odom has
the layout a C compiler gives the header's struct, NULL handles are refused, and abi.odom_pose_cov — the NumPy mirror of the kernel's pose
covariance — uses the Jacobian that central differences of the reference's own injection rule give.  No compute is launched here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O

abi = O.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rvio_hip_set_odometry", "rvio_hip_get_odometry", "rvio_hip_get_odometry_all", "rvio_hip_get_pose_at")
FIELDS = ("seq", "img_count", "n_clones", "reserved", "p", "q", "v", "pose_cov", "vel_cov")


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
    assert "#define RVIO_HIP_ABI_VERSION 6" in hdr and "within 6" in hdr.lower()


def test_record_layout_matches_a_c_compiler(tmp_path):
    assert C.sizeof(abi.rvio_odom) == 464 and abi.ODOM_DTYPE.itemsize == 464
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rvio_hip.h"\nint main(void) {\n  printf("%zu", sizeof(rvio_odom));\n'
                   + "".join('  printf(" %%zu", offsetof(rvio_odom, %s));\n' % f for f in FIELDS) + '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == 464
    assert got[1:] == [getattr(abi.rvio_odom, f).offset for f in FIELDS]
    assert got[1:] == [abi.ODOM_DTYPE.fields[f][1] for f in FIELDS]
    assert got[1:] == [0, 8, 12, 16, 24, 48, 80, 104, 392]          # no padding: 8 + 4 + 4 + 8 + 8 * (3 + 4 + 3 + 36 + 9) = 464


def test_null_handle_is_invalid(lib):
    n, seq = C.c_int32(0), C.c_int64(0)
    rec = abi.rvio_odom()
    p, q = (C.c_double * 3)(), (C.c_double * 4)()
    assert lib.rvio_hip_set_odometry(None, 16) == -1
    assert lib.rvio_hip_get_odometry(None, 0, C.c_int64(1), 1, C.byref(rec), C.byref(n)) == -1
    assert lib.rvio_hip_get_odometry_all(None, C.byref(rec), C.byref(seq)) == -1
    assert lib.rvio_hip_get_pose_at(None, 0, p, q) == -1


# ---------------------------------------------------------------- the Jacobian behind pose_cov
def inject(q, p, dth, dp):
    """the reference's injection (Updater.cc:549-566): dq = [dth / 2; sqrt(1 - |dth|^2 / 4)], q <- dq (x) q, p <- p + dp"""
    dq = np.concatenate([0.5 * dth, [np.sqrt(1.0 - 0.25 * float(dth @ dth))]])
    return O.quat_mul(dq, q), p + dp


def published(q, p):
    """what the pose line carries: pGk = -R^T p (System.cc:341) and the attitude R_wb = R^T"""
    R = O.quat_to_rot(q)
    return -R.T @ p, R.T


def numeric_jacobian(q, p, step=1e-6):
    pG0, Rwb0 = published(q, p)
    J = np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = step
        col = []
        for s in (+1.0, -1.0):
            qs, ps = inject(q, p, s * d[:3], s * d[3:])
            pG, Rwb = published(qs, ps)
            E = Rwb @ Rwb0.T                                    # ~ I + [phi x]
            phi = 0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
            col.append(np.concatenate([pG - pG0, phi]))
        J[:, k] = (col[0] - col[1]) / (2 * step)
    return J


def test_pose_cov_jacobian_against_central_differences_of_the_injection():
    rng = np.random.default_rng(7)
    worst = 0.0
    for t in range(20):
        q = rng.standard_normal(4)
        q /= np.linalg.norm(q)
        if q[3] < 0:
            q = -q
        p = rng.standard_normal(3)
        p *= (0.5 * (t + 1)) / np.linalg.norm(p)                # |p| = 0.5, 1, ..., 10
        J, Jn = abi.odom_pose_jacobian(q, p), numeric_jacobian(q, p)
        err = float(np.max(np.abs(J - Jn)))
        worst = max(worst, err / max(1.0, np.linalg.norm(p)))
        assert err <= 1e-7 * max(1.0, np.linalg.norm(p)), (t, err)
        # the mirror itself: (C + C^T) / 2 of J P6 J^T for a random SPD covariance, exactly symmetric
        A = rng.standard_normal((24, 24))
        P = A @ A.T * 1e-4
        x = np.concatenate([q, p, rng.standard_normal(19)])
        Cm = J @ P[:6, :6] @ J.T
        got = abi.odom_pose_cov(x, P)
        assert np.array_equal(got, 0.5 * (Cm + Cm.T)) and np.array_equal(got, got.T)
    print("odom_pose_jacobian vs central differences: worst |dJ| / max(1, |p|) = %.2e" % worst)


def test_replay_usage_lists_odometry():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host")], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(ROOT, "host", "rvio_replay")], capture_output=True, text=True)
    assert r.returncode == 2 and "--odometry FILE" in r.stderr and "--odometry-ring N" in r.stderr, r.stderr
