"""Inputs shared by the past-frame fix tests (test infrastructure): the window states of tests/aux_update_cases.py, the ages each window is tested
at, and fixes placed a given distance from the prediction the state makes for a PAST frame (abi.fix_past_h)."""
import numpy as np

import fix_cases as F

abi, A, K = F.abi, F.A, F.K
LEVER, LEVERS = F.LEVER, F.LEVERS
KINDS = (abi.RVIO_FIX_POSITION, abi.RVIO_FIX_ATTITUDE, abi.RVIO_FIX_POSE)
KIND_NAMES = F.KIND_NAMES
FRAC = 0.25


def ages(n):
    """0, 1, n / 2 (rounded down), n — those the window holds, once each"""
    return sorted({a for a in (0, 1, n // 2, n) if a <= n})


def combos(n):
    """(kind, age, frac) of every case at a window of n clones: the three kinds at every age, POSITION also at frac 0.25 where age + 1 <= n"""
    out = [(k, a, 0.0) for k in KINDS for a in ages(n)]
    out += [(abi.RVIO_FIX_POSITION, a, FRAC) for a in ages(n) if a + 1 <= n]
    return out


def zero_cols(n, kind, age, frac):
    """per block of three rows: the columns the table of include/rvio_hip.h lists as exactly 0"""
    reach = age + (1 if frac > 0 else 0)
    d = 24 + 6 * n
    live_clones = [i for i in range(n - reach, n)]
    pos = set(range(0, 6)) | {24 + 6 * i + c for i in live_clones for c in range(6)}
    att = set(range(0, 3)) | {24 + 6 * i + c for i in live_clones[len(live_clones) - age:] for c in range(3)}
    blocks = {abi.RVIO_FIX_POSITION: (pos,), abi.RVIO_FIX_ATTITUDE: (att,), abi.RVIO_FIX_POSE: (pos, att)}[kind]
    return [[c for c in range(d) if c not in b] for b in blocks]


def fix_near(x, kind, age, frac=0.0, lever=(0.0, 0.0, 0.0), dp=0.05, dth=0.01, sigma_p=1e-2, sigma_q=1e-3, seed=0):
    """an rvio_fix whose position lies dp (m) and whose attitude lies dth (rad) from what the state predicts for the frame `age` back, in
    directions drawn from `seed`"""
    rng = np.random.default_rng(177 + seed)
    u, w = rng.standard_normal(3), rng.standard_normal(3)
    u, w = u / np.linalg.norm(u), w / np.linalg.norm(w)
    h = abi.fix_past_h(x, age, lever, frac)
    return abi.make_fix(h[0:3] + dp * u, abi.quat_mul(F.rot_quat(dth * w), h[3:7]), sigma_p, sigma_q, lever)


def rot_angle(qa, qb):
    """the angle between two JPL quaternions' rotations"""
    E = abi.quat_to_rot(np.asarray(qa, float)) @ abi.quat_to_rot(np.asarray(qb, float)).T
    return float(np.linalg.norm(0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])))
