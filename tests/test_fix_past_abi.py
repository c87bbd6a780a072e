"""CPU-side checks of the past-frame fixes (added within ABI 6): the entry points are exported, declared and named on the ABI-version line; NULL
handles are refused; and abi.fix_past_model — the NumPy model the device is held to — is held to central differences of abi.fix_past_h through the
reference's state injection, to the pose lines the oracle recorded at the frames the ages point to, and to what an update with it must do: pull
the state's PAST pose onto the fix.  No compute is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fix_past_cases as FP

abi, A, F = FP.abi, FP.A, FP.F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rvio_hip_update_fix_past", "rvio_hip_update_fix_past_dev", "rvio_hip_frame_age")
EPS = 1e-5
WINDOWS = (0, 1, 3, 10, 31)


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
    assert callable(abi.fix_past_h) and callable(abi.fix_past_model)


def test_null_arguments_are_invalid(lib):
    f = abi.make_fix((0, 0, 0), (0, 0, 0, 1), 1.0, 1.0)
    age = C.c_int(0)
    assert lib.rvio_hip_update_fix_past(None, 0, 0, 0, 0, C.c_double(0.0), C.byref(f)) == -1
    assert lib.rvio_hip_update_fix_past_dev(None, 0, 0, C.byref(f), C.c_size_t(0), C.byref(age), None, None) == -1
    assert lib.rvio_hip_frame_age(None, 0, C.byref(age)) == -1


# ---------------------------------------------------------------- the NumPy model against finite differences
def _measure(x, kind, fix, age, frac):
    """what is differenced: the predicted position, and MINUS the attitude residual against the fixed z"""
    out = []
    if kind != abi.RVIO_FIX_ATTITUDE:
        out.append(abi.fix_past_h(x, age, fix.lever[:], frac)[0:3])
    if kind != abi.RVIO_FIX_POSITION:
        out.append(-abi.fix_past_model(x, kind, fix, age, frac)[1][-3:])
    return np.concatenate(out)


@pytest.mark.parametrize("lever", FP.LEVERS, ids=["lever", "nolever"])
@pytest.mark.parametrize("n", WINDOWS)
def test_jacobian_against_central_differences(n, lever):
    x, P = A.window_state(n)
    d = P.shape[0]
    for kind, age, frac in FP.combos(n):
        h = abi.fix_past_h(x, age, lever, frac)
        fix = abi.make_fix(h[0:3], h[3:7], 1.0, 1.0, lever)      # (z = the state's own prediction: the attitude residual is linear around 0 only)
        H, r, sigma = abi.fix_past_model(x, kind, fix, age, frac)
        assert H.shape == (abi.FIX_ROWS[kind], d) and np.max(np.abs(r)) < 1e-12
        Hfd = np.zeros_like(H)
        for c in range(d):
            e = np.zeros(d)
            e[c] = EPS
            Hfd[:, c] = (_measure(abi.inject_state(x, e), kind, fix, age, frac) - _measure(abi.inject_state(x, -e), kind, fix, age, frac)) / (2 * EPS)
        s = abi.quat_to_rot(x[0:4]) @ h[0:3]                      # s_a = R_G h
        bar = 1e-8 * max(1.0, float(np.linalg.norm(s)))
        worst = float(np.max(np.abs(Hfd - H)))
        print("n=%d %s age %d frac %.2f lever %s: max|H - FD| = %.3e (bar %.3e, max|H| %.3g)" % (n, FP.KIND_NAMES[kind], age, frac, lever, worst, bar, np.max(np.abs(H))))
        assert worst <= bar
        for b, zero in enumerate(FP.zero_cols(n, kind, age, frac)):
            blk = H[3 * b: 3 * b + 3]
            assert not blk[:, zero].any(), "a column the table lists as 0"
            assert set(range(6, 24)) <= set(zero) and all(c in zero for c in range(24, 24 + 6 * (n - age - (1 if frac > 0 else 0))))
            assert np.abs(blk).sum() > 1.0


def test_age_zero_without_clone_columns_is_todays_fix_at_an_identity_pose():
    """age 0 reads (qG, pG) only: against abi.fix_model on the same state with (qk, pk) at the identity — the state right behind a composition"""
    cfg = A.long_config()
    x, P = A.window_state(10)
    x = x.copy()
    x[10:17] = [0, 0, 0, 1, 0, 0, 0]
    for kind in FP.KINDS:
        fix = FP.fix_near(x, kind, 0, 0.0, FP.LEVER)
        Hp, rp, sp = abi.fix_past_model(x, kind, fix, 0)
        Hn, rn, sn = abi.fix_model(cfg, x, kind, fix)
        keep = [c for c in range(Hn.shape[1]) if not 9 <= c < 15]
        assert np.max(np.abs(Hp[:, keep] - Hn[:, keep])) <= 1e-15 and np.max(np.abs(rp - rn)) <= 1e-15 and np.array_equal(sp, sn)
        assert not Hp[:, 9:15].any()


# ---------------------------------------------------------------- what the ages mean: the oracle's recorded pose lines
def _last_frame_without_an_update(recs):
    j = 0
    while j + 1 < len(recs) and not recs[j + 1]["did_update"]:
        j += 1
    assert not any(r["did_update"] for r in recs[: j + 1]) and j >= 2
    return j


def test_the_rebuilt_past_pose_is_the_recorded_pose_line_where_no_update_ran():
    seq, recs = A.long_recorded()
    j = _last_frame_without_an_update(recs)
    x3 = recs[j]["x3"]
    for a in range(j + 1):
        h = abi.fix_past_h(x3, a, 0)
        ep, eq = float(np.max(np.abs(h[0:3] - recs[j - a]["pose_p"]))), float(np.max(np.abs(h[3:7] - recs[j - a]["pose_q"])))
        print("frame %d, age %d: |p - recorded| %.3e  |q - recorded| %.3e" % (j + 1, a, ep, eq))
        assert ep <= 1e-12 and eq <= 1e-12


def test_at_frame_20_the_past_poses_are_the_recorded_ones_and_the_current_state_is_not():
    cfg = A.long_config()
    seq, recs = A.long_recorded()
    j = 19
    x3 = recs[j]["x3"]
    assert (len(x3) - 26) // 7 == 19
    for a in range(j + 1):
        h = abi.fix_past_h(x3, a, 0)
        ep = float(np.linalg.norm(h[0:3] - recs[j - a]["pose_p"]))
        eq = FP.rot_angle(h[3:7], recs[j - a]["pose_q"])
        # the same delayed fix against the CURRENT state (abi.fix_h): off by the motion since
        now = float(np.linalg.norm(abi.fix_h(cfg, x3, abi.RVIO_FIX_POSITION)[0:3] - recs[j - a]["pose_p"]))
        print("age %2d: past form %.3e m %.3e rad; fused at the current state %.3f m" % (a, ep, eq, now))
        assert ep <= 6e-3 and eq <= 3e-4
        if a >= 1:
            assert now >= 0.05


# ---------------------------------------------------------------- the update pulls the PAST pose onto the fix
@pytest.mark.parametrize("kind", [abi.RVIO_FIX_POSITION, abi.RVIO_FIX_ATTITUDE], ids=["position", "attitude"])
@pytest.mark.parametrize("n", [1, 3, 10, 31])
def test_the_update_pulls_the_past_pose_onto_the_fix(n, kind):
    x, P = A.window_state(n)
    for age in FP.ages(n):
        fix = FP.fix_near(x, kind, age, 0.0, FP.LEVER, dp=0.05, dth=0.01, sigma_p=1e-4, sigma_q=1e-4, seed=n + age)
        H, r, sigma = abi.fix_past_model(x, kind, fix, age)
        assert np.isclose(np.linalg.norm(r), 0.05 if kind == abi.RVIO_FIX_POSITION else 0.01, rtol=1e-3)
        x1 = abi.aux_update_model(x, P, H, r, sigma)[0]
        ratio = float(np.linalg.norm(abi.fix_past_model(x1, kind, fix, age)[1]) / np.linalg.norm(r))
        xn = abi.aux_update_model(x, P, -H, r, sigma)[0]          # a wrong sign pushes away
        wrong = float(np.linalg.norm(abi.fix_past_model(xn, kind, fix, age)[1]) / np.linalg.norm(r))
        print("n=%d %s age %d: |r| -> %.2f %% (a wrong sign: %.0f %%)" % (n, FP.KIND_NAMES[kind], age, 100 * ratio, 100 * wrong))
        assert ratio <= 0.05 and wrong >= 1.0
