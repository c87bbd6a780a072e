"""Inputs shared by the relative-pose measurement tests (test infrastructure): the window states of tests/aux_update_cases.py, the spans
(age_new, age_old) each window is tested at, and measurements placed a given distance from the delta pose the state predicts between the two
frames (abi.rel_h)."""
import numpy as np

import fix_cases as F

abi, A, K = F.abi, F.A, F.K
LEVER, LEVERS = F.LEVER, F.LEVERS
KINDS = abi.REL_KINDS
KIND_NAMES = {abi.RVIO_REL_POSITION: "rel_position", abi.RVIO_REL_ATTITUDE: "rel_attitude", abi.RVIO_REL_POSE: "rel_pose"}
WINDOWS = (1, 3, 10, 31)


def spans(n):
    """(0, 1), (0, n), (n - 1, n), (n / 2, n), (0, max(1, n / 2)) — once each"""
    out = []
    for s in ((0, 1), (0, n), (n - 1, n), (n // 2, n), (0, max(1, n // 2))):
        if s not in out:
            out.append(s)
    return out


def combos(n):
    """(kind, age_new, age_old) of every case at a window of n clones"""
    return [(k, a, b) for k in KINDS for a, b in spans(n)]


def span_cols(n, a, b):
    """the columns of the clones n - b .. n - a - 1"""
    return [24 + 6 * i + c for i in range(n - b, n - a) for c in range(6)]


def zero_cols(n, kind, a, b):
    """per block of three rows: the columns the table of include/rvio_hip.h lists as exactly 0 — all of 0 .. 23, every clone outside the span,
    and in the attitude rows the position columns of the span's clones too"""
    d = 24 + 6 * n
    pos = set(span_cols(n, a, b))
    att = {c for c in pos if (c - 24) % 6 < 3}
    blocks = {abi.RVIO_REL_POSITION: (pos,), abi.RVIO_REL_ATTITUDE: (att,), abi.RVIO_REL_POSE: (pos, att)}[kind]
    return [[c for c in range(d) if c not in blk] for blk in blocks]


def meas_near(x, kind, a, b, lever=(0.0, 0.0, 0.0), dp=0.05, dth=0.01, sigma_p=1e-2, sigma_q=1e-3, seed=0):
    """an rvio_fix whose displacement lies dp (m) and whose rotation lies dth (rad) from what the state predicts between the frames b and a
    images back, in directions drawn from `seed`"""
    rng = np.random.default_rng(277 + seed)
    u, w = rng.standard_normal(3), rng.standard_normal(3)
    u, w = u / np.linalg.norm(u), w / np.linalg.norm(w)
    h = abi.rel_h(x, a, b, lever)
    return abi.make_fix(h[0:3] + dp * u, abi.quat_mul(F.rot_quat(dth * w), h[3:7]), sigma_p, sigma_q, lever)


def outside_replaced(x, a, b, seed=0):
    """the state with entries 0 - 25 and every clone outside the span n - b .. n - a - 1 replaced by other valid values (unit quaternions, a unit
    gravity direction)"""
    rng = np.random.default_rng(377 + seed)
    x = np.array(x, float)
    n = (len(x) - 26) // 7

    def quat():
        q = rng.standard_normal(4)
        return q / np.linalg.norm(q)
    x[0:4], x[4:7] = quat(), rng.standard_normal(3)
    g = rng.standard_normal(3)
    x[7:10] = g / np.linalg.norm(g)
    x[10:14], x[14:17] = quat(), 0.1 * rng.standard_normal(3)
    x[17:26] = 0.1 * rng.standard_normal(9)
    for i in list(range(0, n - b)) + list(range(n - a, n)):
        x[26 + 7 * i: 30 + 7 * i], x[30 + 7 * i: 33 + 7 * i] = quat(), 0.1 * rng.standard_normal(3)
    return x
