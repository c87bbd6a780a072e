"""States for the window-pose tests (tests/test_window_pose_abi.py on the CPU, tests/test_gpu_window_pose.py on the device): a composed state
of n clones with an SPD covariance, built once per (n, seed), and the error measure the covariance is held to."""
import functools

import numpy as np

import oracle as O

abi = O.abi
EPS = np.finfo(float).eps
WINDOWS = (3, 11, 32)                       # max_track_len: n = 2, 10, 31 clones (k = 6 + 6 n = 18, 66, 192 columns at the oldest age)


def ages_of(n):
    return sorted({0, 1, n - 1, n})


def unit_quat(rng, angle=None):
    """a unit quaternion (JPL xyzw, w >= 0): uniform, or a rotation by `angle` about a random axis"""
    if angle is None:
        q = rng.standard_normal(4)
    else:
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        q = np.concatenate([np.sin(0.5 * angle) * ax, [np.cos(0.5 * angle)]])
    q /= np.linalg.norm(q)
    return -q if q[3] < 0 else q


@functools.lru_cache(maxsize=None)
def built_state(n, seed=0):
    """(x, P) of a composed state with n clones: the reference frame some metres from the world origin, clones of ~6 degrees and ~0.2 m per
    image, (qk, pk) = identity as behind augment / compose; P = SPD, symmetric bit for bit, with correlations between every pair of blocks"""
    rng = np.random.default_rng(1000 * n + seed)
    x = np.zeros(26 + 7 * n)
    x[0:4] = unit_quat(rng)
    x[4:7] = 3.0 * rng.standard_normal(3)
    g = rng.standard_normal(3)
    x[7:10] = g / np.linalg.norm(g)
    x[10:14] = [0.0, 0.0, 0.0, 1.0]
    x[17:20] = rng.standard_normal(3)
    x[20:26] = 0.01 * rng.standard_normal(6)
    for i in range(n):
        x[26 + 7 * i: 30 + 7 * i] = unit_quat(rng, 0.1 * (1 + rng.random()))
        x[30 + 7 * i: 33 + 7 * i] = 0.2 * rng.standard_normal(3)
    d = 24 + 6 * n
    A = rng.standard_normal((d, d))
    M = 1e-4 * (A @ A.T) / d + 1e-6 * np.eye(d)
    P = 0.5 * (M + M.T)
    x.setflags(write=False)
    P.setflags(write=False)
    return x, P


@functools.lru_cache(maxsize=None)
def truth(n, age, seed=0):
    """(p, q, cov) of built_state(n, seed) at `age` in np.longdouble"""
    x, P = built_state(n, seed)
    return abi.window_pose_model_as(x, P, age, np.longdouble)


def cov_err(C, C_true):
    """e = max_ij |C - C_true|_ij / sqrt(C_true,ii C_true,jj), evaluated in the truth's precision"""
    C_true = np.asarray(C_true)
    dg = np.sqrt(np.diag(C_true))
    return float(np.max(np.abs(np.asarray(C, C_true.dtype) - C_true) / np.outer(dg, dg)))


def quat_close(q, q_ref, tol):
    """equal up to sign"""
    q, q_ref = np.asarray(q, float), np.asarray(q_ref, float)
    return min(float(np.max(np.abs(q - q_ref))), float(np.max(np.abs(q + q_ref)))) <= tol
