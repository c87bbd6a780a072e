"""Truth shared by the tests of IMU-rate odometry with covariance (test infrastructure), on the states, batches and config of imu_pose_cases.py:
the covariance record behind sample j is what the oracle's own frame gives when an image arrives there and runs no update — prefix propagation
of the 24 x 24 head (the marginal of the head does not depend on the clones), composition without augmentation, the odometry record's map."""
import functools

import numpy as np

import imu_pose_cases as K
import oracle as O

abi = O.abi
REL_TOL = 1e-11       # the project's bar for this quantity (tests/test_gpu_odometry.py): max|got - want| <= 1e-11 max|want| per record
MS_CPU = (1, 2, 10, 65)
MS_GPU = (1, 2, 10, 63, 64, 65, 129)
M_GROW = 193          # plain handle only: the host staging grows


def oracle_cov_records(x, P, imu):
    """(pose_cov [m, 6, 6], vel_cov [m, 3, 3]) by oracle prefix propagation + composition"""
    cfg = K.config()
    m = len(imu)
    pose_cov, vel_cov = np.zeros((m, 6, 6)), np.zeros((m, 3, 3))
    x, P = np.ascontiguousarray(x[:26]), np.ascontiguousarray(P[:24, :24])
    for j in range(m):
        xj, Pj = O.propagate(cfg, x, P, imu[:j + 1])
        xc, Pc = O.augment_compose(cfg, xj, Pj, False)[:2]
        pose_cov[j] = abi.odom_pose_cov(xc, Pc)
        vel_cov[j] = Pc[15:18, 15:18]
    return pose_cov, vel_cov


@functools.lru_cache(maxsize=None)
def case(state_name, m, seed=0, special=False):
    """(x, P, imu, (pose_cov, vel_cov) of the oracle), computed once per session"""
    x, P = K.state(state_name)
    imu = K.batch(m, seed, special, x)
    return x, P, imu, oracle_cov_records(x, P, imu)


def rel_delta(rec, truth):
    """the worst max|got - want| / max|want| over the records, for pose_cov and vel_cov"""
    worst = 0.0
    for got, want in ((rec["pose_cov"], truth[0]), (rec["vel_cov"], truth[1])):
        for g, w in zip(got, want):
            d, s = float(np.max(np.abs(g - w))), float(np.max(np.abs(w)))
            # (an all-zero block — the velocity covariance of the initial state behind a sample with dt = 0 — admits no deviation at all)
            worst = max(worst, d / s if s > 0 else (0.0 if d == 0 else np.inf))
    return worst


def exactly_symmetric(rec):
    return np.array_equal(rec["pose_cov"], np.swapaxes(rec["pose_cov"], 1, 2)) and np.array_equal(rec["vel_cov"], np.swapaxes(rec["vel_cov"], 1, 2))
