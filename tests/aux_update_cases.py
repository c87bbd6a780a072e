"""Inputs and truth shared by the auxiliary-update tests (test infrastructure): start states at every window from ONE recorded sequence of the
longest window (max_track_len = 32: the state in front of frame k holds k - 1 clones while the window fills) and from tests/imu_pose_cases.py,
random measurements (H ~ N(0, 1), sigma in [1e-3, 1e-1]) and the truth — abi.aux_update_model everywhere, the CPU oracle on the sub-class it
covers: an H whose first 24 columns are zero is, with the rows rescaled to the image noise, exactly oracle.update_from_stack (no compression
runs on a stack that is not tall, ekf_apply does the rest)."""
import functools

import numpy as np

import imu_pose_cases as K
import oracle as O
import scenarios as S

abi, rv = O.abi, O.rv
X_TOL = K.X_TOL
WINDOWS = (0, 3, 4, 10, 17, 31)       # d = 24, 42, 48, 84, 126, 210: the empty window, 48 a multiple of 16, both sides of 6n = 96, the longest
COND_MAX = 1e6


def p_bar(Pref):
    """the project's covariance bar (tests/test_gpu_filter.py:18)"""
    return 1e-9 * float(np.max(np.abs(Pref))) + 1e-15


@functools.lru_cache(maxsize=None)
def long_config():
    return abi.config_named("B", enable_equalizer=0, max_track_len=32)


@functools.lru_cache(maxsize=None)
def long_recorded():
    return S.record_sequence(long_config(), n_frames=33, duration=6.0)


def window_state(n):
    """(x, P) with n clones: the composed state in front of a frame of the max_track_len = 32 sequence"""
    seq, recs = long_recorded()
    r = recs[n + 1] if n > 0 else recs[0]
    x, P = r["x0"].copy(), r["P0"].copy()
    assert (len(x) - 26) // 7 == n and P.shape == (24 + 6 * n, 24 + 6 * n)
    return x, P


def chi2_95(m):
    O.lib().orc_chi2_95.restype = O.C.c_double
    return float(O.lib().orc_chi2_95(int(m)))


def whitened_S(P, H, sigma):
    Hw = H / sigma[:, None]
    return Hw @ P @ Hw.T + np.eye(len(sigma))


def measurement(P, m, seed, kind="full", gamma_target=None):
    """(H, v, sigma): kind 'full' = dense rows over all d columns, 'clone' = the first 24 columns zero.  gamma_target: the residual is a random
    direction scaled so that v~^T S^-1 v~ = gamma_target (the gated cases put it a factor 4 on either side of the table); None: v ~ sigma N(0, 1).
    Asserts cond(S) <= 1e6."""
    rng = np.random.default_rng(1000 * seed + 17 * m + P.shape[0])
    d = P.shape[0]
    H = rng.standard_normal((m, d))
    if kind == "clone":
        assert d > 24 and m <= d - 24
        H[:, :24] = 0.0
    sigma = 10.0 ** rng.uniform(-3, -1, m)
    Sw = whitened_S(P, H, sigma)
    assert np.linalg.cond(Sw) <= COND_MAX, np.linalg.cond(Sw)
    u = rng.standard_normal(m)
    if gamma_target is None:
        v = sigma * u
    else:
        L = np.linalg.cholesky(0.5 * (Sw + Sw.T))
        v = sigma * (L @ (u * np.sqrt(gamma_target / float(u @ u))))
    return H, v, sigma


def oracle_update(cfg, x, P, H, v, sigma):
    """the oracle on a clone-only H: rows rescaled to the image noise sigma_im, handed over as a stack that is not tall"""
    assert not H[:, :24].any() and H.shape[0] <= H.shape[1] - 24
    sim = float(np.float32(max(cfg.sigma_px, cfg.sigma_py)))
    s = sim / sigma
    xo, Po, info = O.update_from_stack(cfg, x, P, (H * s[:, None])[:, 24:], v * s, n_good=3)
    assert info["updated"] == 1 and info["rank"] == -1, info
    return xo, Po


def zupt(d, z=(0.0, 0.0, 0.0), sigma=0.05):
    """the zero-velocity / velocity measurement in VALUE mode: H = I at columns 15..17"""
    H = np.zeros((3, d))
    H[0, 15] = H[1, 16] = H[2, 17] = 1.0
    return H, np.asarray(z, float), np.full(3, float(sigma))
