"""CPU-side checks of the relative-pose measurements (added within ABI 6): the entry points are exported, declared and named on the ABI-version
line; NULL handles are refused; and abi.rel_model — the NumPy model the device is held to — is held to central differences of abi.rel_h through
the reference's state injection, to the pose lines the oracle recorded, to what an update with it must do (pull the window's delta pose onto the
measurement), and to what it must not read (anything outside the span's clones).  No compute is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rel_cases as R

abi, A = R.abi, R.A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rvio_hip_update_rel", "rvio_hip_update_rel_dev")
EPS = 1e-5
P_, A_, Q_ = abi.RVIO_REL_POSITION, abi.RVIO_REL_ATTITUDE, abi.RVIO_REL_POSE


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
    assert "#define RVIO_HIP_ABI_VERSION 6" in version_line and all(s in version_line for s in NEW)
    assert (abi.RVIO_REL_POSITION, abi.RVIO_REL_ATTITUDE, abi.RVIO_REL_POSE) == (16, 17, 18)
    for name, v in (("RVIO_REL_POSITION", 16), ("RVIO_REL_ATTITUDE", 17), ("RVIO_REL_POSE", 18)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, v), hdr), name
    assert callable(abi.rel_h) and callable(abi.rel_model)


def test_null_arguments_are_invalid(lib):
    f = abi.make_fix((0, 0, 0), (0, 0, 0, 1), 1.0, 1.0)
    a, b = C.c_int(0), C.c_int(1)
    assert lib.rvio_hip_update_rel(None, 0, P_, 0, 0, 1, C.byref(f)) == -1
    assert lib.rvio_hip_update_rel_dev(None, P_, 0, C.byref(f), C.c_size_t(0), C.byref(a), C.byref(b), None) == -1


# ---------------------------------------------------------------- the NumPy model against finite differences
def _measure(x, kind, meas, a, b):
    """what is differenced: the predicted displacement, and MINUS the attitude residual against the fixed z"""
    out = []
    if kind != A_:
        out.append(abi.rel_h(x, a, b, meas.lever[:])[0:3])
    if kind != P_:
        out.append(-abi.rel_model(x, kind, meas, a, b)[1][-3:])
    return np.concatenate(out)


@pytest.mark.parametrize("lever", R.LEVERS, ids=["lever", "nolever"])
@pytest.mark.parametrize("n", R.WINDOWS)
def test_jacobian_against_central_differences(n, lever):
    x, P = A.window_state(n)
    d = P.shape[0]
    for kind, a, b in R.combos(n):
        h = abi.rel_h(x, a, b, lever)
        meas = abi.make_fix(h[0:3], h[3:7], 1.0, 1.0, lever)      # (z = the state's own prediction: the attitude residual is linear around 0 only)
        H, r, sigma = abi.rel_model(x, kind, meas, a, b)
        assert H.shape == (abi.REL_ROWS[kind], d) and np.max(np.abs(r)) < 1e-12
        Hfd = np.zeros_like(H)
        for c in range(d):
            e = np.zeros(d)
            e[c] = EPS
            Hfd[:, c] = (_measure(abi.inject_state(x, e), kind, meas, a, b) - _measure(abi.inject_state(x, -e), kind, meas, a, b)) / (2 * EPS)
        bar = 1e-8 * max(1.0, float(np.max(np.abs(H))))
        worst = float(np.max(np.abs(Hfd - H)))
        print("n=%d %s span (%d, %d) lever %s: max|H - FD| = %.3e (bar %.3e, max|H| %.3g)" % (n, R.KIND_NAMES[kind], a, b, lever, worst, bar, np.max(np.abs(H))))
        assert worst <= bar
        for blk_i, zero in enumerate(R.zero_cols(n, kind, a, b)):
            blk = H[3 * blk_i: 3 * blk_i + 3]
            assert not blk[:, zero].any() and not Hfd[3 * blk_i: 3 * blk_i + 3][:, zero].any(), "a column the table lists as 0"
            assert set(range(0, 24)) <= set(zero) and np.abs(blk).sum() > 1.0


@pytest.mark.parametrize("n", R.WINDOWS)
def test_one_step_without_a_lever_is_the_clone_itself(n):
    x, P = A.window_state(n)
    for a in sorted({0, n // 2, n - 1}):
        i = n - a - 1
        h = abi.rel_h(x, a, a + 1)
        q = x[26 + 7 * i: 30 + 7 * i]
        assert np.max(np.abs(h[0:3] - x[30 + 7 * i: 33 + 7 * i])) <= 1e-15
        assert np.max(np.abs(abi.quat_to_rot(h[3:7]) - abi.quat_to_rot(q))) <= 1e-15
        H, r, sigma = abi.rel_model(x, Q_, abi.make_fix(h[0:3], h[3:7], 1.0, 1.0), a, a + 1)
        want = np.zeros_like(H)
        want[0:3, 27 + 6 * i: 30 + 6 * i] = np.eye(3)
        want[3:6, 24 + 6 * i: 27 + 6 * i] = np.eye(3)
        print("n=%d age %d: max|H - identity blocks| %.3e" % (n, a, np.max(np.abs(H - want))))
        assert np.max(np.abs(H - want)) <= 1e-15


# ---------------------------------------------------------------- what the ages mean: the oracle's recorded pose lines
def test_the_delta_between_two_frames_is_that_of_the_recorded_pose_lines_where_no_update_ran():
    seq, recs = A.long_recorded()
    j = 0
    while j + 1 < len(recs) and not recs[j + 1]["did_update"]:
        j += 1
    assert not any(r["did_update"] for r in recs[: j + 1]) and j >= 2
    x3 = recs[j]["x3"]
    n = (len(x3) - 26) // 7
    worst_p = worst_q = 0.0
    for b in range(1, min(j, n) + 1):
        for a in range(b):
            h = abi.rel_h(x3, a, b)
            ra, rb = recs[j - a], recs[j - b]
            Ra, Rb = abi.quat_to_rot(ra["pose_q"]), abi.quat_to_rot(rb["pose_q"])
            ep = float(np.max(np.abs(h[0:3] - Rb @ (np.asarray(ra["pose_p"]) - np.asarray(rb["pose_p"])))))
            eq = float(np.max(np.abs(abi.quat_to_rot(h[3:7]) - Ra @ Rb.T)))
            worst_p, worst_q = max(worst_p, ep), max(worst_q, eq)
            assert ep <= 1e-12 and eq <= 1e-12, (a, b, ep, eq)
    print("frame %d, %d clones: worst |dp - recorded| %.3e  |dR - recorded| %.3e" % (j + 1, n, worst_p, worst_q))


# ---------------------------------------------------------------- the update pulls the window's delta onto the measurement
def _left(x, meas, a, b):
    """(displacement, angle) between the measurement and the state's prediction, re-evaluated with rel_h"""
    h = abi.rel_h(x, a, b, meas.lever[:])
    E = abi.quat_to_rot(h[3:7]) @ abi.quat_to_rot(np.array(meas.z[3:7])).T
    return float(np.linalg.norm(np.array(meas.z[0:3]) - h[0:3])), float(np.linalg.norm(0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])))


@pytest.mark.parametrize("lever", R.LEVERS, ids=["lever", "nolever"])
@pytest.mark.parametrize("n", R.WINDOWS)
def test_the_update_pulls_the_window_onto_the_measurement(n, lever):
    x, P = A.window_state(n)
    for a, b in R.spans(n):
        meas = R.meas_near(x, Q_, a, b, lever, dp=0.05, dth=0.01, sigma_p=1e-6, sigma_q=1e-7, seed=n + a + b)
        H, r, sigma = abi.rel_model(x, Q_, meas, a, b)
        p0, q0 = _left(x, meas, a, b)
        assert np.isclose(p0, 0.05, rtol=1e-3) and np.isclose(q0, 0.01, rtol=1e-3)
        p1, q1 = _left(abi.aux_update_model(x, P, H, r, sigma)[0], meas, a, b)
        pw, qw = _left(abi.aux_update_model(x, P, -H, r, sigma)[0], meas, a, b)          # a wrong sign pushes away
        print("n=%d span (%d, %d): left %.3f %% of 0.05 m, %.3f %% of 0.01 rad (a wrong sign: %.0f %%, %.0f %%)" % (n, a, b, 100 * p1 / p0, 100 * q1 / q0, 100 * pw / p0, 100 * qw / q0))
        assert p1 <= 0.05 * p0 and q1 <= 0.05 * q0
        assert pw >= p0 and qw >= q0


# ---------------------------------------------------------------- what the model must not read
@pytest.mark.parametrize("n", R.WINDOWS)
def test_nothing_outside_the_span_enters(n):
    x, P = A.window_state(n)
    for kind, a, b in R.combos(n):
        meas = R.meas_near(x, kind, a, b, R.LEVER, seed=n + a)
        y = R.outside_replaced(x, a, b, seed=n + b)
        assert np.max(np.abs(y[0:26] - x[0:26])) > 1e-3
        H0, r0, s0 = abi.rel_model(x, kind, meas, a, b)
        H1, r1, s1 = abi.rel_model(y, kind, meas, a, b)
        assert np.array_equal(H0, H1) and np.array_equal(r0, r1) and np.array_equal(s0, s1)
        assert np.array_equal(abi.rel_h(x, a, b, R.LEVER), abi.rel_h(y, a, b, R.LEVER))
