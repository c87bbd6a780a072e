"""CPU-side checks of the fixed-lag smoothed trajectory's C-ABI surface (added within ABI 6): the five entry points are exported and declared,
rvio_window_pose has the layout a C++ compiler gives the header's struct (tests/hostemu/window_pose_layout.cpp), NULL handles are refused, and
abi.window_pose_model — the NumPy statement of csrc/window_pose.hip — uses the Jacobian that central differences of the reference's own
injection rule give when they are pushed through abi.fix_past_h, equals the odometry record's mirror and the pose line at age 0, and agrees
with its extended-precision twin.  The smoothed ring's read window goes through csrc/ring_span.h.  No compute is launched here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
import window_cases as W
from test_ring_span import emu, span  # noqa: F401  (the g++ build of csrc/ring_span.h)

abi = O.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rvio_hip_get_window", "rvio_hip_get_window_dev", "rvio_hip_set_smoothed_odometry", "rvio_hip_get_smoothed_odometry",
       "rvio_hip_get_smoothed_odometry_all")
FIELDS = ("seq", "img_count", "age", "n_clones", "reserved", "p", "q", "pose_cov")


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
    # what is not done is said in the header
    for phrase in ("NOT done: cross-covariances between frames of the window", "just left the window", "time stamps in the record", "interpolation between frames"):
        assert phrase in hdr, phrase


def test_record_layout_matches_a_cxx_compiler(tmp_path):
    assert C.sizeof(abi.rvio_window_pose) == 368 and abi.WINDOW_POSE_DTYPE.itemsize == 368
    exe = str(tmp_path / "layout")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "hostemu", "window_pose_layout.cpp"), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got[0] == 368
    assert got[1:] == [getattr(abi.rvio_window_pose, f).offset for f in FIELDS]
    assert got[1:] == [abi.WINDOW_POSE_DTYPE.fields[f][1] for f in FIELDS]
    assert got[1:] == [0, 8, 12, 16, 20, 24, 48, 80]          # no padding: 8 + 4 * 4 + 8 * (3 + 4 + 36) = 368


def test_null_handle_is_invalid(lib):
    n, seq = C.c_int32(0), C.c_int64(0)
    rec = abi.rvio_window_pose()
    assert lib.rvio_hip_get_window(None, 0, 1, C.byref(rec), C.byref(n)) == -1
    assert lib.rvio_hip_get_window_dev(None, 0, 1, C.byref(rec), C.c_size_t(1)) == -1
    assert lib.rvio_hip_set_smoothed_odometry(None, 16, 0) == -1
    assert lib.rvio_hip_get_smoothed_odometry(None, 0, C.c_int64(1), 1, C.byref(rec), C.byref(n)) == -1
    assert lib.rvio_hip_get_smoothed_odometry_all(None, C.byref(rec), C.byref(seq)) == -1


# ---------------------------------------------------------------- the Jacobian behind pose_cov
def published(x, age):
    """what a record carries, from abi.fix_past_h: the world position of the IMU at that image and the attitude R_wb = R(q)^T"""
    z = abi.fix_past_h(x, age)
    return z[0:3], abi.quat_to_rot(z[3:7]).T


def numeric_jacobian(x, age, step=1e-6):
    """central differences of the reference's injection (Updater.cc:549-566: q <- dq (x) q, p <- p + dp on (qG, pG) and on every clone; the
    other slots additive), every column of the error state"""
    n = (len(x) - 26) // 7
    d = 24 + 6 * n
    p0, Rwb0 = published(x, age)
    J = np.zeros((6, d))
    for k in range(d):
        dx = np.zeros(d)
        dx[k] = step
        col = []
        for s in (+1.0, -1.0):
            p, Rwb = published(abi.inject_state(x, s * dx), age)
            E = Rwb @ Rwb0.T                                    # ~ I + [phi x]
            col.append(np.concatenate([p - p0, 0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])]))
        J[:, k] = (col[0] - col[1]) / (2 * step)
    return J


@pytest.mark.parametrize("n", [2, 10, 31])
def test_jacobian_against_central_differences_of_the_injection(n):
    x, _ = W.built_state(n)
    for age in sorted({0, 1, n}):
        J, Jn = abi.window_pose_jacobian(x, age), numeric_jacobian(np.array(x), age)
        p = abi.window_pose_model(x, np.zeros((24 + 6 * n,) * 2), age)[0]
        err = float(np.max(np.abs(J - Jn)))
        print("n = %d, age %d: |dJ| = %.2e, |p| = %.2f" % (n, age, err, np.linalg.norm(p)))
        assert err <= 1e-7 * max(1.0, np.linalg.norm(p)), (n, age, err)
        # the columns the kernel never reads are exactly zero: 6 .. 23 and every clone older than n - age
        nz = np.zeros(24 + 6 * n, bool)
        nz[0:6] = True
        nz[24 + 6 * (n - age): 24 + 6 * n] = True
        assert not J[:, ~nz].any() and not Jn[:, ~nz].any() and J[:, nz].any(axis=0).all()


@pytest.mark.parametrize("n", [2, 10, 31])
def test_age_0_is_the_odometry_mirror_and_the_pose_line(n):
    x, P = W.built_state(n)
    p, q, cov = abi.window_pose_model(x, P, 0)
    assert np.array_equal(abi.window_pose_jacobian(x, 0)[:, :6], abi.odom_pose_jacobian(x[0:4], x[4:7]))
    ref = abi.odom_pose_cov(x, P)
    assert np.max(np.abs(cov - ref)) <= 64 * W.EPS * np.max(np.abs(ref)) and np.array_equal(cov, cov.T)
    pl, ql = abi.pose_line(x)                                   # (qk, pk) = identity behind augment / compose
    assert np.max(np.abs(p - pl)) <= 1e-12 * max(1.0, np.linalg.norm(pl)) and W.quat_close(q, ql, 1e-12)
    assert np.array_equal(q, x[0:4])


@pytest.mark.parametrize("n", [2, 10, 31])
def test_model_against_its_extended_precision_twin(n):
    x, P = W.built_state(n)
    for age in W.ages_of(n):
        p, q, cov = abi.window_pose_model(x, P, age)
        pt, qt, ct = W.truth(n, age)
        assert ct.dtype == np.longdouble
        # the twin in float64 is the model, to rounding
        p64, q64, c64 = abi.window_pose_model_as(x, P, age, np.float64)
        assert np.max(np.abs(p64 - p)) <= 1e-13 * max(1.0, np.linalg.norm(p)) and W.quat_close(q64, q, 1e-13)
        assert np.max(np.abs(p - pt.astype(float))) <= 1e-12 * max(1.0, np.linalg.norm(p)) and W.quat_close(q, qt.astype(float), 1e-12)
        e = W.cov_err(cov, ct)
        print("n = %d, age %d: float64 model e = %.2e (the floor the device is compared with), twin in float64 e = %.2e" % (n, age, e, W.cov_err(c64, ct)))
        assert e <= 1e-11 and np.array_equal(cov, cov.T)
        assert np.min(np.linalg.eigvalsh(cov)) > 0


# ---------------------------------------------------------------- the ring
def test_ring_read_window_goes_through_ring_span(emu):  # noqa: F811
    """lag 3, capacity 4, 12 frames of a window that grows by one clone per frame up to 10: records exist from the frame at which n_clones
    reaches 3, seq counts them, and the getter's two spans (csrc/ring_span.h) serve the last four, oldest first"""
    lag, cap = 3, 4
    written = []                                               # (seq, img_count of the described frame)
    for frame in range(1, 13):
        n_clones = min(frame - 1, 10)
        if n_clones >= lag:
            written.append((len(written) + 1, frame - lag))
    assert [w[0] for w in written] == list(range(1, 10)) and written[0][1] == 1 and written[-1][1] == 9
    newest = len(written)
    ring = [None] * cap
    for seq, ic in written:
        ring[(seq - 1) % cap] = (seq, ic)
    first, count, slot0, n0 = span(emu, newest, cap, 1, cap)
    assert (first, count) == (6, 4) and 0 < n0 < count           # wrapped
    got = [ring[slot0 + j] if j < n0 else ring[j - n0] for j in range(count)]
    assert got == written[5:9]
    assert span(emu, 0, cap, 1, cap)[1] == 0                    # nothing before the window has grown to the lag


def test_replay_usage_lists_smoothed():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host")], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(ROOT, "host", "rvio_replay")], capture_output=True, text=True)
    assert r.returncode == 2 and "--smoothed FILE" in r.stderr and "--smoothed-lag L" in r.stderr and "--smoothed-ring N" in r.stderr, r.stderr
