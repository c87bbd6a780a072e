"""Inputs shared by the standstill tests (test infrastructure): IMU batches drawn at rest or in motion around a given state's biases, with the
detector's own noises, and the thresholds the tests use — their own, far from the library's defaults (those are tuning values)."""
import numpy as np

from pkgload import load_pkg

abi = load_pkg().abi
import math

_CFG = abi.config_euroc()
G = _CFG.gravity
# the detector noises of the tests: the discrete-time form of the configured densities (m/s^2, rad/s per sample)
SIGMA_A, SIGMA_W = _CFG.sigma_a * math.sqrt(_CFG.imu_rate), _CFG.sigma_g * math.sqrt(_CFG.imu_rate)
IMU_THR = 40.0                           # at rest T ~ 6 (at most 6 + a few sqrt(12 / m)); the moving batches below give T > 100


def ss_config(**over):
    c = abi.rvio_standstill_config(SIGMA_A, SIGMA_W, IMU_THR, 0.5, 0.05, SIGMA_W, 5, 0, 1, 0)
    for k, v in over.items():
        setattr(c, k, v)
    return c


def _rot(seed):
    q = np.random.default_rng(900 + seed).standard_normal(4)
    q /= np.linalg.norm(q)
    return abi.quat_to_rot(q)


def imu_batch(x, m, seed=0, kind="rest", gravity=G, sigma_a=SIGMA_A, sigma_w=SIGMA_W):
    """m samples at 200 Hz around the biases of x.  'rest': a = ba + R g + noise, w = bg + noise (R: a random attitude);
    'accel': + a sinusoidal acceleration of 0.2 m/s^2 RMS ON EACH AXIS (0.04 / sigma_a^2 = 50 per axis: T ~ 156; a sinusoid of 0.2 m/s^2 peak on ONE axis
    would give 0.02 / sigma_a^2 + 6 = 31 under the configured noise and could not be told from rest by a factor); at m = 1, where a sinusoid has no meaning,
    the same 0.2 * sqrt(3) as a constant along gravity.  'turn': + 0.05 rad/s of rotation"""
    rng = np.random.default_rng(1234 + 31 * seed + m)
    imu = np.zeros(m, abi.IMU_DTYPE)
    up = _rot(seed) @ np.array([0.0, 0.0, gravity])
    t = np.arange(m) / 200.0
    imu["t"], imu["dt"] = t, 1.0 / 200.0
    imu["a"] = x[23:26] + up + sigma_a * rng.standard_normal((m, 3))
    imu["w"] = x[20:23] + sigma_w * rng.standard_normal((m, 3))
    if kind == "accel":
        if m == 1:
            imu["a"] += 0.2 * np.sqrt(3.0) * up / gravity
        else:
            ph = 2 * np.pi * (np.arange(m) + 0.5) / m          # whole periods over the batch: the mean stays where it was
            imu["a"] += 0.2 * np.sqrt(2.0) * np.sin(ph)[:, None] * np.array([1.0, 1.0, 1.0])
    elif kind == "turn":
        imu["w"] += np.array([0.05, 0.0, 0.0])
    else:
        assert kind == "rest"
    return imu
