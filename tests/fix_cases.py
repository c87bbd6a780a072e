"""Inputs shared by the absolute-fix tests (test infrastructure): start states from tests/aux_update_cases.py (every window of the
max_track_len = 32 sequence) and tests/imu_pose_cases.py ("moved": qk, pk off identity), the state right behind initialisation (qk all zero),
and fixes placed a given distance from a state's own predicted measurement."""
import numpy as np

import aux_update_cases as A

abi, K = A.abi, A.K
LEVER = (0.3, -0.2, 0.1)
LEVERS = (LEVER, (0.0, 0.0, 0.0))
KINDS = abi.FIX_KINDS
KIND_NAMES = {abi.RVIO_FIX_POSITION: "position", abi.RVIO_FIX_ATTITUDE: "attitude", abi.RVIO_FIX_POSE: "pose", abi.RVIO_FIX_GRAVITY: "gravity"}


def zero_qk(x):
    """the state with qk all zero, pk = 0: what System::initialize leaves until the first composition (QuatToRot reads it as I)"""
    x = np.array(x, float)
    x[10:17] = 0.0
    return x


def cpu_state(name):
    """(x, P) for the CPU tests: 'window10', 'moved' (tests/imu_pose_cases.py) and 'zero_qk' (the initial state, qk all zero)"""
    if name == "zero_qk":
        x, P = K.state("empty")
        return zero_qk(x), P
    return K.state(name)


def moved_window(n):
    """(x, P) with n clones of the max_track_len = 32 sequence, qk and pk moved off identity (the head of 'moved'); P stays the window's"""
    x, P = A.window_state(n)
    x = x.copy()
    x[10:17] = K.state("moved")[0][10:17]
    return x, P


def rot_quat(axis_angle):
    """the JPL quaternion of a rotation vector, exact (not the small-angle form)"""
    a = np.asarray(axis_angle, float)
    th = float(np.linalg.norm(a))
    if th == 0.0:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.concatenate([np.sin(th / 2) * a / th, [np.cos(th / 2)]])


def fix_near(cfg, x, kind, lever=(0.0, 0.0, 0.0), dp=0.05, dth=0.01, sigma_p=1e-2, sigma_q=1e-3, seed=0):
    """an rvio_fix whose position / accelerometer part lies dp (m, m/s^2) and whose attitude lies dth (rad) from the state's own prediction, in
    directions drawn from `seed`.  GRAVITY: the offset is drawn ORTHOGONAL to the predicted gravity direction R_k g (a tilt).  The filter carries
    g as three coordinates whose covariance is not confined to the tangent plane, and injection re-normalises g (Updater.cc:566-568): the share
    of a correction ALONG g that the gain hands to g's length (about 90 % of it at these states: sd(g) G = 0.015 against sd(ba) = 0.005) is
    discarded there, by the reference's parameterisation and not by the rows, so an offset along g is not a measure of the rows' signs"""
    rng = np.random.default_rng(77 + seed)
    u, w = rng.standard_normal(3), rng.standard_normal(3)
    if kind == abi.RVIO_FIX_GRAVITY:
        gk = abi.quat_to_rot(np.asarray(x[10:14], float)) @ np.asarray(x[7:10], float)
        u = u - gk * float(u @ gk) / float(gk @ gk)
    u, w = u / np.linalg.norm(u), w / np.linalg.norm(w)
    h = abi.fix_h(cfg, x, kind, lever)
    p = h[0:3] + dp * u
    q = abi.quat_mul(rot_quat(dth * w), h[3:7]) if h[3:7].any() else None
    return abi.make_fix(p, q, sigma_p, sigma_q, lever)
