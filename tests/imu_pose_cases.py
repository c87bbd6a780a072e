"""Inputs and truth shared by the IMU-rate odometry tests (test infrastructure): synthetic IMU batches, start states from the recorded cfg-B
sequence, and the oracle's records — prefix propagation: PreIntegrator::propagate's sample loop is prefix-exact, so the state behind sample j
is oracle.propagate(cfg, x, P, imu[:j + 1]), and the pose line behind it is System.cc:339-341 on that state."""
import functools

import numpy as np

import oracle as O
import scenarios as S

abi, rv = O.abi, O.rv
X_TOL = 1e-9          # the project's state bar (tests/test_gpu_filter.py)
MS_CPU = (1, 2, 10, 65)
MS_GPU = (1, 2, 10, 63, 64, 65, 200)


@functools.lru_cache(maxsize=None)
def config():
    return abi.config_named("B", enable_equalizer=0)


@functools.lru_cache(maxsize=None)
def recorded():
    return S.record_sequence(config(), n_frames=12)


@functools.lru_cache(maxsize=None)
def _imu_all(seed):
    return rv.synth.SynthSequence(config(), duration=8.0, seed=seed).imu_all()


def state(name):
    """(x, P): 'empty' = the initial state (empty window, qk = identity, pk = 0); 'window10' = the composed state in front of frame 12 (10 clones);
    'moved' = that frame's PROPAGATED state (10 clones, non-identity qk, non-zero pk: the loop starts from QuatToRot(qk) and rebuilds pk)"""
    seq, recs = recorded()
    if name == "empty":
        return recs[0]["x0"].copy(), recs[0]["P0"].copy()
    if name == "window10":
        assert (len(recs[11]["x0"]) - 26) // 7 == 10
        return recs[11]["x0"].copy(), recs[11]["P0"].copy()
    assert name == "moved"
    x = recs[11]["x1"].copy()
    assert abs(x[13]) < 1 - 1e-9 and np.linalg.norm(x[14:17]) > 1e-4
    return x, recs[11]["P1"].copy()


STATES = ("empty", "window10", "moved")


def batch(m, seed=0, special=False, x=None):
    """m consecutive samples of a moving stretch of the synthetic sequence `seed`.  special (needs the start state x, m >= 2): the LAST sample
    turns slower than small_angle after the bias is removed (the nSmallAngle branch), the one before it has dt = 0."""
    imu = _imu_all(seed)[600 + 37 * seed: 600 + 37 * seed + m].copy()
    assert len(imu) == m
    if special:
        assert m >= 2 and x is not None
        imu["w"][m - 1] = x[20:23] + np.array([2e-4, -1e-4, 3e-4])
        imu["dt"][m - 2] = 0.0
        assert np.linalg.norm(imu["w"][m - 1] - x[20:23]) < config().small_angle
    return imu


def oracle_records(x, P, imu):
    """(p [m, 3], q [m, 4], v [m, 3]) by oracle prefix propagation"""
    cfg = config()
    m = len(imu)
    p, q, v = np.zeros((m, 3)), np.zeros((m, 4)), np.zeros((m, 3))
    RG = O.quat_to_rot(x[0:4])
    for j in range(m):
        xj = O.propagate(cfg, x, P, imu[:j + 1])[0]
        q[j] = O.quat_mul(xj[10:14], x[0:4])
        p[j] = RG.T @ (xj[14:17] - x[4:7])
        v[j] = xj[17:20]
    return p, q, v


@functools.lru_cache(maxsize=None)
def case(state_name, m, seed, special=False):
    """(x, P, imu, (p, q, v) of the oracle), computed once per session"""
    x, P = state(state_name)
    imu = batch(m, seed, special, x)
    # (the state path of the loop reads neither P nor the clones: the 24 x 24 head keeps the m (m + 1) / 2 oracle steps of a long batch cheap)
    return x, P, imu, oracle_records(x[:26], P[:24, :24], imu)


def worst_delta(rec, truth):
    p, q, v = truth
    return max(float(np.max(np.abs(rec["p"] - p))), float(np.max(np.abs(rec["q"] - q))), float(np.max(np.abs(rec["v"] - v))))
