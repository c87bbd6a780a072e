"""RANSAC's gyro prior (gyro_dR in csrc/frontend_kernels.hip, Ransac.cc:120-155) at the IMU batches the suite never sent it: one sample; 191, 192
and 193 samples — the first RVIO_MAX_IMU = 192 delta rotations come one per thread, the rest are formed inside the product loop —; irregular dt
with zero-dt duplicates; scattered samples slower than small_angle (the prior integrates the RAW gyro: no bias is removed); and one run at
small_angle = 0.5 with dt = 0.05 (every other sample in the branch at |w| = 0.4; the two forms of the delta rotation differ by about 5e-6 per
sample there — 0.02 px over the batch, which the inlier sets do not resolve on the CPU: 66 inliers either way; that run checks that the device
takes a branch the oracle agrees with bit for bit, the others that the prior as a whole decides).

Direct-track mode against O.Tracker, as tests/test_gpu_branches.py's candidate-count test: about 80 point pairs that obey a known rotation plus
translation, 20 % gross outliers; the IMU batch integrates to that rotation (a NumPy product of the per-sample rotations, written here).  Winner,
inlier count, flags (the surviving points) and the tracker tables are bit-exact.  Each case first shows on the CPU that the prior matters to it:
with the gyro batch zeroed the oracle keeps another set of points."""
import numpy as np
import pytest

import oracle as O
from test_gpu_edges import _same_tracker

abi, rv = O.abi, O.rv
pytestmark = pytest.mark.gpu

N_PTS = 80
#        (m, small_angle or None for the stock one, dt or None for irregular)
CASES = [(1, None, None), (191, None, None), (192, None, None), (193, None, None), (10, 0.5, 0.05)]


def _skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def gyro_batch(cfg, m, dt, seed):
    """the IMU batch and the rotation Rci (dR_{m-1} ... dR_0) Ric it integrates to"""
    rng = np.random.default_rng([3, m, seed])
    imu = np.zeros(m, abi.IMU_DTYPE)
    if dt is None:
        while True:
            imu["dt"] = 0.005 * rng.choice([0.0, 0.6, 1.0, 1.0, 1.4, 2.0, 3.0], size=m)
            if imu["dt"].sum() > 0 and (m < 8 or (imu["dt"] == 0).any()):
                break
        # a steady turn of 0.06 rad over the batch with scatter per sample, about a fifth of the samples nearly at rest (raw |w| < small_angle),
        # the samples around RVIO_MAX_IMU among them
        mean = rng.normal(size=3)
        mean *= 0.06 / imu["dt"].sum() / np.linalg.norm(mean)
        imu["w"] = mean + 0.3 * np.linalg.norm(mean) * rng.normal(size=(m, 3))
        slow = [s for s in (0, 5, 187, 188) if s < m and m > 1] + [int(s) for s in rng.permutation(min(m, 186))[: m // 5]]
        for s in slow:
            imu["w"][s] = rng.normal(0.0, 3e-4, 3)
        assert m == 1 or all(np.linalg.norm(imu["w"][s]) < cfg.small_angle for s in slow)
        # the samples on either side of RVIO_MAX_IMU each turn by 0.01 rad about an axis of their own (4.6 px at this focal length): a delta rotation
        # lost or taken twice at the edge changes the inlier set (asserted on the CPU below)
        for s in range(189, m):
            d = rng.normal(size=3)
            imu["dt"][s] = 0.01
            imu["w"][s] = d / np.linalg.norm(d)
    else:
        imu["dt"] = dt
        for s in range(m):
            d = rng.normal(size=3)
            imu["w"][s] = (0.4 if s % 2 == 0 else 0.6) * d / np.linalg.norm(d)
    imu["a"] = np.array([0.0, 0.0, 9.81])
    imu["t"] = np.cumsum(imu["dt"])
    R, I = np.eye(3), np.eye(3)
    for u in imu:
        w1, dts = np.linalg.norm(u["w"]), u["dt"]
        wx = _skew(u["w"])
        if w1 < cfg.small_angle:
            dR = I - dts * wx + .5 * dts ** 2 * (wx @ wx)
        else:
            dR = I - np.sin(w1 * dts) / w1 * wx + (1 - np.cos(w1 * dts)) / w1 ** 2 * (wx @ wx)
        R = dR @ R
    Ric = np.array(list(cfg.T_bc)).reshape(4, 4)[:3, :3]
    return imu, Ric.T @ R @ Ric


def point_pairs(cfg, R, seed):
    """pixels of N_PTS landmarks in two ideal pinhole views related by X2 = R X1 + t; every fifth pair is a gross outlier"""
    rng = np.random.default_rng([5, seed])
    p0 = np.stack([rng.uniform(40, cfg.width - 40, N_PTS), rng.uniform(40, cfg.height - 40, N_PTS)], 1)
    X1 = np.stack([(p0[:, 0] - cfg.cx) / cfg.fx, (p0[:, 1] - cfg.cy) / cfg.fy, np.ones(N_PTS)], 1) * rng.uniform(2.0, 8.0, (N_PTS, 1))
    X2 = X1 @ R.T + np.array([0.08, -0.03, 0.05])
    p1 = np.stack([cfg.fx * X2[:, 0] / X2[:, 2] + cfg.cx, cfg.fy * X2[:, 1] / X2[:, 2] + cfg.cy], 1)
    bad = np.arange(N_PTS) % 5 == 2
    p1[bad] += np.array([37.0, -23.0])
    return np.ascontiguousarray(p0, np.float32), np.ascontiguousarray(p1, np.float32), bad


def run(tr, p0, p1, imu):
    none = np.zeros((0, 2), np.float32)
    tr.track_points(none, np.zeros(0, np.uint8), np.zeros(0, abi.IMU_DTYPE), p0)          # first image: seed the slots with p0
    return tr.track_points(p1, np.ones(len(p1), np.uint8), imu, none)


@pytest.mark.parametrize("m,small_angle,dt", CASES, ids=lambda v: str(v))
def test_gyro_prior_batches(gpu_required, m, small_angle, dt):
    from rvio_amd import hip
    kw = {} if small_angle is None else dict(small_angle=small_angle)
    cfg = abi.config_named("B", enable_equalizer=0, k1=0.0, k2=0.0, p1=0.0, p2=0.0, **kw)      # an ideal pinhole: the pairs obey the model exactly
    imu, R = gyro_batch(cfg, m, dt, 0)
    p0, p1, bad = point_pairs(cfg, R, m)
    # the prior matters: without the gyro batch the oracle keeps other points, with it the inliers are the consistent pairs
    t, t0 = O.Tracker(cfg), O.Tracker(cfg)
    oi = run(t, p0, p1, imu)
    still = imu.copy()
    still["w"] = 0.0
    oi0 = run(t0, p0, p1, still)
    kept, kept0 = t.get_points()[0], t0.get_points()[0]
    assert N_PTS - int(bad.sum()) <= oi["n_ransac_inliers"] < N_PTS - int(bad.sum()) // 2, oi      # (an offset along a point's epipolar line survives)
    assert oi0["n_ransac_inliers"] != oi["n_ransac_inliers"] or not np.array_equal(kept, kept0), (oi, oi0)
    if m > 189:                     # the batch's last sample matters too: the one a wrong edge at RVIO_MAX_IMU = 192 would lose
        tl = O.Tracker(cfg)
        oil = run(tl, p0, p1, imu[:-1])
        assert oil["n_ransac_inliers"] != oi["n_ransac_inliers"] or not np.array_equal(kept, tl.get_points()[0]), (oi, oil)
    if small_angle is not None:     # (printed, not asserted: at the stock small_angle every sample takes the other branch)
        tb = O.Tracker(abi.config_named("B", enable_equalizer=0, k1=0.0, k2=0.0, p1=0.0, p2=0.0))
        oib = run(tb, p0, p1, imu)
        print("small_angle 0.5 / stock: inliers %d / %d" % (oi["n_ransac_inliers"], oib["n_ransac_inliers"]))
    h = hip.RvioHip(cfg)
    try:
        run(h, p0, p1, imu)
        gi = h.frame_info()
        for key in ("n_tracked_in", "n_klt_ok", "n_ransac_inliers", "ransac_winner", "n_tracked_out", "n_feat_update"):
            assert gi[key] == oi[key], (m, key, gi, oi)
        n_pts, _ = _same_tracker(h, t, m)
        assert n_pts == oi["n_ransac_inliers"] and gi["device_error"] == 0
        print("m %d: %d inliers with the prior, %d with the gyro zeroed" % (m, oi["n_ransac_inliers"], oi0["n_ransac_inliers"]))
    finally:
        h.close()
