"""GPU: standstill detection and the automatic zero-velocity update (rvio_hip_standstill*, csrc/standstill.hip in front of csrc/aux_update.hip)
against abi.standstill_model / abi.aux_update_model and against a twin handle that is handed the same update through rvio_hip_update_aux.
Bars: the statistic 1e-12 relative (a sum of m <= 4096 non-negative doubles in any order: m 2^-53 ~ 4.5e-13, a few ulps per term on top); the
disparity 1e-3 px (float32 rounding of normalised coordinates <= 1: f 2^-23 ~ 6e-5 px per coordinate at f ~ 460); the update: BITS against the
twin (the same kernel on the same inputs), the aux test's own bars against the model where z comes from a device mean.  Every threshold is the
test's own (tests/standstill_cases.py) and every case asserts on the CPU, beforehand, that the model is a factor 1.5 away from it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import aux_update_cases as A
import oracle as O
import scenarios as S
import standstill_cases as Z

abi, rv = O.abi, O.rv
K = A.K
pytestmark = pytest.mark.gpu
MS = (1, 2, 63, 64, 65, 192, 193, 1000)     # the wave and workgroup edges of the strided loops
K0 = 38
NODIST = dict(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)


def cfg_direct(dist):
    return K.config() if dist else abi.config_named("B", enable_equalizer=0, **NODIST)


def rec(h, i=0):
    return h.get_standstill(i).asdict()


@pytest.fixture(scope="module")
def hP(gpu_required):
    from rvio_amd import hip
    h = hip.RvioHip(K.config())
    yield h
    assert h.frame_info()["device_error"] == 0
    h.close()


# ---------------------------------------------------------------- 1. the statistic
@pytest.mark.parametrize("m", MS)
def test_statistic_against_the_model(hP, m):
    c = Z.ss_config()
    hP.set_standstill(c)
    for si, name in enumerate(K.STATES):
        x, P = K.state(name)
        hP.set_state(x, P)
        for kind in ("rest", "accel", "turn"):
            imu = Z.imu_batch(x, m, seed=si, kind=kind)
            T, w_mean, _, _, flags = abi.standstill_model(x, imu, None, None, 1.0, 1.0, K.config().gravity, c)
            assert T <= c.imu_thr / 1.5 or T >= 1.5 * c.imu_thr, (name, kind, m, T)      # far from the threshold on the CPU first
            assert (kind == "rest") == bool(flags & abi.SS_IMU_STATIC)
            hP.standstill(imu, apply=0)
            r = rec(hP)
            print("%s %s m=%d: T %.15g (model %.15g, rel %.2e) flags %d" % (name, kind, m, r["T"], T, abs(r["T"] - T) / T, r["flags"]))
            assert abs(r["T"] - T) <= 1e-12 * T
            assert r["flags"] == flags and r["m"] == m and r["n_pairs"] == 0 and r["disparity"] == 0.0 and r["gamma"] == 0.0
            xd, Pd = hP.get_state()
            assert np.array_equal(xd, x) and np.array_equal(Pd, P)
    # a degenerate batch: the mean specific force vanishes — not static, whatever T is
    z = np.zeros(3, abi.IMU_DTYPE)
    z["a"], z["w"] = x[23:26], x[20:23]
    hP.standstill(z, apply=0)
    assert not rec(hP)["flags"] & abi.SS_IMU_STATIC


# ---------------------------------------------------------------- 2. the disparity
def run_direct(h, seq, n_frames, each=None, init=True):
    """frame_points on the synthetic direct-track sequence; each(k, inp, pts_before, pts, hist_len) behind every frame"""
    drv = rv.synth.DirectTrackDriver(seq)
    if init:
        h.initialize(*seq.init_from_static(K0))
    prev = np.zeros((0, 2), np.float32)
    for k in range(K0 + 1, K0 + 1 + n_frames):
        inp = drv.inputs(k)
        h.frame_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])
        pts, hl = h.get_points()
        drv.after(pts)
        if each:
            each(k, inp, prev, pts, hl)
        prev = pts


def pairs_px(inp, prev, pts, hl):
    """(previous, current) PIXEL of every live point with two observations: a survivor carries the bits of the tracked_xy that was handed in,
    and tracked_xy[j] continues the live point j of the frame before"""
    where = {inp["tracked"][j].tobytes(): j for j in range(len(inp["tracked"])) if inp["status"][j]}
    a, b = [], []
    for i in np.flatnonzero(hl >= 2):
        j = where[pts[i].tobytes()]
        a.append(prev[j]); b.append(pts[i])
    return np.array(a, float).reshape(-1, 2), np.array(b, float).reshape(-1, 2)


def seq_of(cfg, motion):
    # (stationary: 0.02 px of pixel noise — a mean step of 0.02 sqrt(2) sqrt(pi / 2) = 0.035 px, not the exact zero of identical projections)
    return rv.synth.SynthSequence(cfg, duration=8.0, seed=0, motion=motion, pixel_noise=None if motion == "sinus" else 0.02)


@pytest.mark.parametrize("motion", ["sinus", "stationary"])
def test_disparity_against_the_model(gpu_required, motion):
    from rvio_amd import hip
    cfg = cfg_direct(False)
    # (the sinus sequence and its inputs as scenarios.record_sequence records them; the stationary one built from synth directly)
    seq, recs = S.record_sequence(cfg, n_frames=5) if motion == "sinus" else (seq_of(cfg, motion), None)
    h = hip.RvioHip(cfg)
    c = Z.ss_config(disp_thr_px=0.5, min_pairs=5)
    h.set_standstill(c)
    imu = Z.imu_batch(np.zeros(26), 10)
    seen = []

    def each(k, inp, prev, pts, hl):
        if recs is not None:
            r = recs[k - K0 - 1]
            assert np.array_equal(r["inp"]["tracked"], inp["tracked"]) and np.array_equal(r["inp"]["cand"], inp["cand"])
        a, b = pairs_px(inp, prev, pts, hl)
        _, _, disp, n_pairs, flags = abi.standstill_model(np.zeros(26), imu, a, b, 1.0, 1.0, cfg.gravity, c)
        assert n_pairs == int(np.sum(hl >= 2))
        h.standstill(imu, apply=0)
        r = rec(h)
        print("%s frame %d: n_pairs %d disparity %.6f px (model %.6f)" % (motion, k, r["n_pairs"], r["disparity"], disp))
        assert r["n_pairs"] == n_pairs and abs(r["disparity"] - disp) <= 1e-3
        if n_pairs == 0:
            assert k == K0 + 1 and r["flags"] & abi.SS_IMG_STATIC and r["disparity"] == 0.0
        else:
            assert n_pairs >= 50 and (disp > 1.5 * c.disp_thr_px if motion == "sinus" else disp < c.disp_thr_px / 1.5)
            assert bool(r["flags"] & abi.SS_IMG_STATIC) == (motion == "stationary")
        # too few pairs for an opinion: the image test does not veto, and the record says how many there were
        h.set_standstill(Z.ss_config(disp_thr_px=0.5, min_pairs=len(pts) + 1))
        h.standstill(imu, apply=0)
        r2 = rec(h)
        assert r2["n_pairs"] == n_pairs and r2["flags"] & abi.SS_IMG_STATIC and r2["disparity"] == r["disparity"]
        h.set_standstill(c)
        seen.append(n_pairs)
    run_direct(h, seq, 5, each)
    assert seen[0] == 0 and min(seen[1:]) >= 50
    # the frame behind initialize starts over
    seen.clear()
    run_direct(h, seq, 1, each)
    assert seen == [0]
    assert h.frame_info()["device_error"] == 0
    h.close()


def test_disparity_with_the_stock_distortion(gpu_required):
    """the device measures fx, fy times the step of the UNDISTORTED normalised coordinates, the model here the raw pixel step: held to the two
    sides of the decision only — on the model first"""
    from rvio_amd import hip
    cfg = cfg_direct(True)
    c = Z.ss_config()
    imu = Z.imu_batch(np.zeros(26), 10)
    for motion in ("stationary", "sinus"):
        h = hip.RvioHip(cfg)
        h.set_standstill(c)
        out = []

        def each(k, inp, prev, pts, hl):
            if k == K0 + 1:
                return
            a, b = pairs_px(inp, prev, pts, hl)
            disp = abi.standstill_model(np.zeros(26), imu, a, b, 1.0, 1.0, cfg.gravity, c)[2]
            assert disp < 0.05 if motion == "stationary" else disp > 1.0
            h.standstill(imu, apply=0)
            out.append(rec(h)["disparity"])
        run_direct(h, seq_of(cfg, motion), 4, each)
        h.close()
        print("%s, stock distortion: %s px" % (motion, np.round(out, 4)))
        assert len(out) == 3 and all(d < 0.05 if motion == "stationary" else d > 1.0 for d in out)


# ---------------------------------------------------------------- 3. decision and update
def snapshot(h):
    """everything a call that does not apply must leave alone"""
    x, P = h.get_state()
    return dict(x=x, P=P, pose=np.concatenate(h.pose()), info=repr(sorted(h.frame_info().items())), odom=h.odometry().tobytes(),
                imuo=h.get_imu_odometry().tobytes(), imuc=h.get_imu_odometry_cov().tobytes(), pts=h.get_points()[0].tobytes(), hl=h.get_points()[1].tobytes())


def same(a, b):
    return all(np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)


def history_handle(motion, frames=4):
    from rvio_amd import hip
    cfg = cfg_direct(True)
    h = hip.RvioHip(cfg)
    h.set_odometry(16); h.set_imu_odometry(256); h.set_imu_odometry_cov(1)
    run_direct(h, seq_of(cfg, motion), frames)
    return h


@pytest.fixture(scope="module")
def hStat(gpu_required):
    h = history_handle("stationary")
    yield h
    assert h.frame_info()["device_error"] == 0
    h.close()


def twin_update(x, P, H, z, sigma, gate):
    from rvio_amd import hip
    t = hip.RvioHip(cfg_direct(True))
    t.set_state(x, P)
    t.update_aux(H, z, sigma, abi.RVIO_AUX_VALUE, gate)
    xt, Pt = t.get_state()
    d = t.aux_diag()
    pose = np.concatenate(t.pose())
    t.close()
    return xt, Pt, d, pose


def test_applied_update_equals_the_twins_bits(hStat):
    h = hStat
    c = Z.ss_config(min_pairs=5, bias_rows=0, gate=1)
    h.set_standstill(c)
    x, P = h.get_state()
    imu = Z.imu_batch(x, 10, seed=1)
    T, w_mean, _, _, f = abi.standstill_model(x, imu, None, None, 1.0, 1.0, K.config().gravity, c)
    assert T <= c.imu_thr / 1.5
    H, z, sigma = abi.standstill_measurement(P.shape[0], w_mean, c)
    xm, Pm, gm = abi.aux_update_model(x, P, H, z, sigma, abi.RVIO_AUX_VALUE)
    assert gm < A.chi2_95(3) / 2                                   # the gate lets it through, on the CPU first
    before = snapshot(h)
    # detect only: nothing but the record changes
    h.standstill(imu, apply=0)
    r0 = rec(h)
    assert r0["flags"] == 0b0111 and r0["gamma"] == 0.0 and r0["n_pairs"] >= 50 and r0["disparity"] < c.disp_thr_px / 1.5
    assert same(before, snapshot(h))
    # applied
    h.standstill(imu, apply=1)
    r = rec(h)
    xd, Pd = h.get_state()
    xt, Pt, (gt, at), pose_t = twin_update(x, P, H, z, sigma, 1)
    print("applied: flags %s gamma %.6g (twin %.6g, model %.6g)  |v| %.3e -> %.3e" % (bin(r["flags"]), r["gamma"], gt, gm, np.linalg.norm(x[17:20]), np.linalg.norm(xd[17:20])))
    assert r["flags"] == 0b1111 and at == 1 and r["gamma"] == gt
    assert np.array_equal(xd, xt) and np.array_equal(Pd, Pt) and np.array_equal(np.concatenate(h.pose()), pose_t)
    assert abs(r["gamma"] - gm) <= 1e-7 * gm
    # the effect, as the model says: the velocity and its covariance have shrunk
    after = snapshot(h)
    assert after["odom"] == before["odom"] and after["imuo"] == before["imuo"] and after["imuc"] == before["imuc"] and after["pts"] == before["pts"]
    assert S.state_delta(xd, xm) <= A.X_TOL and float(np.max(np.abs(Pd - Pm))) <= A.p_bar(Pm)
    assert np.linalg.norm(xm[17:20]) < np.linalg.norm(x[17:20]) and np.linalg.norm(xd[17:20]) < np.linalg.norm(x[17:20])
    assert np.all(np.diag(Pm)[15:18] < np.diag(P)[15:18]) and np.all(np.diag(Pd)[15:18] < np.diag(P)[15:18])
    h.set_state(x, P)


def test_bias_rows_against_the_model(hStat):
    h = hStat
    c = Z.ss_config(min_pairs=5, bias_rows=1, gate=0, sigma_bg=1e-3)
    h.set_standstill(c)
    x, P = h.get_state()
    imu = Z.imu_batch(x, 65, seed=2)
    T, w_mean, _, _, f = abi.standstill_model(x, imu, None, None, 1.0, 1.0, K.config().gravity, c)
    assert T <= c.imu_thr / 1.5
    H, z, sigma = abi.standstill_measurement(P.shape[0], w_mean, c)
    xm, Pm, gm = abi.aux_update_model(x, P, H, z, sigma, abi.RVIO_AUX_VALUE)
    h.standstill(imu, apply=1)
    r = rec(h)
    xd, Pd = h.get_state()
    dxw, dpw = S.state_delta(xd, xm), float(np.max(np.abs(Pd - Pm)))
    print("bias rows: state %.3e (bar %.0e)  P %.3e (bar %.3e)  gamma %.6g vs %.6g" % (dxw, A.X_TOL, dpw, A.p_bar(Pm), r["gamma"], gm))
    assert r["flags"] == 0b1111
    assert dxw <= A.X_TOL and dpw <= A.p_bar(Pm) and abs(r["gamma"] - gm) <= 1e-7 * gm
    assert np.max(np.abs(xd[20:23] - x[20:23])) > 1e-10 and np.array_equal(Pd, Pd.T)
    h.set_state(x, P)


def test_moving_imu_and_gate_leave_everything_alone(hStat):
    h = hStat
    c = Z.ss_config(min_pairs=5, gate=1)
    h.set_standstill(c)
    x, P = h.get_state()
    for kind in ("turn", "accel"):
        imu = Z.imu_batch(x, 10, seed=3, kind=kind)
        assert abi.standstill_model(x, imu, None, None, 1.0, 1.0, K.config().gravity, c)[0] >= 1.5 * c.imu_thr
        before = snapshot(h)
        h.standstill(imu, apply=1)
        r = rec(h)
        assert r["flags"] == abi.SS_IMG_STATIC and r["gamma"] == 0.0
        assert same(before, snapshot(h))
    # the gate: a velocity 10 sigma off in every axis
    x2 = x.copy()
    x2[17:20] += 10.0 * np.sqrt(np.diag(P)[15:18] + c.sigma_v ** 2)
    H, z, sigma = abi.standstill_measurement(P.shape[0], np.zeros(3), c)
    assert abi.aux_update_model(x2, P, H, z, sigma, abi.RVIO_AUX_VALUE)[2] >= 2 * A.chi2_95(3)
    h.set_state(x2, P)
    imu = Z.imu_batch(x2, 10, seed=4)
    before = snapshot(h)
    h.standstill(imu, apply=1)
    r = rec(h)
    assert r["flags"] == 0b0111 and r["gamma"] == 0.0
    assert same(before, snapshot(h))
    # the same call without the gate is applied
    h.set_standstill(Z.ss_config(min_pairs=5, gate=0))
    h.standstill(imu, apply=1)
    assert rec(h)["flags"] == 0b1111
    h.set_state(x, P)


def test_moving_image_vetoes(gpu_required):
    h = history_handle("sinus")
    c = Z.ss_config(min_pairs=5)
    h.set_standstill(c)
    x, P = h.get_state()
    imu = Z.imu_batch(x, 10, seed=5)
    assert abi.standstill_model(x, imu, None, None, 1.0, 1.0, K.config().gravity, c)[0] <= c.imu_thr / 1.5
    before = snapshot(h)
    h.standstill(imu, apply=1)
    r = rec(h)
    print("moving image: disparity %.3f px over %d pairs, flags %s" % (r["disparity"], r["n_pairs"], bin(r["flags"])))
    assert r["flags"] == abi.SS_IMU_STATIC and r["disparity"] > 1.5 * c.disp_thr_px and r["n_pairs"] >= 50 and r["gamma"] == 0.0
    assert same(before, snapshot(h))
    assert h.frame_info()["device_error"] == 0
    h.close()


# ---------------------------------------------------------------- 4. batch handles
def imu_device(torch, batches, stride):
    buf = np.zeros((len(batches), stride), abi.IMU_DTYPE)
    for i, b in enumerate(batches):
        buf[i, :len(b)] = b
    t = torch.from_numpy(buf.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("B,front", [(3, False), (3, True), (128, False), (128, True)])
def test_batch_handles(hP, gpu_required, B, front):
    import torch
    from rvio_amd import hip
    c = Z.ss_config(bias_rows=1, gate=0, sigma_bg=1e-3)
    x, P = K.state("window10")
    m = 10
    static = [Z.imu_batch(x, m, seed=10 + s) for s in range(4)]
    moving = Z.imu_batch(x, m, seed=20, kind="turn")
    for b in static:
        assert abi.standstill_model(x, b, None, None, 1.0, 1.0, K.config().gravity, c)[0] <= c.imu_thr / 1.5
    assert abi.standstill_model(x, moving, None, None, 1.0, 1.0, K.config().gravity, c)[0] >= 1.5 * c.imu_thr
    # the plain handle's result for each static batch
    hP.set_standstill(c)
    plain = []
    for b in static:
        hP.set_state(x, P)
        hP.standstill(b, apply=1)
        r = rec(hP)
        assert r["flags"] == 0b1111
        plain.append(hP.get_state() + (r, np.concatenate(hP.pose())))
    assert not np.array_equal(plain[0][0], plain[1][0])            # (the bias rows make the result depend on the batch)
    hb = hip.RvioHip(S.small_image_config() if front else K.config(), batch=B, front_end=front)
    hb.set_standstill(c)
    hb.set_state(x, P)
    moves = [i % 3 == 2 for i in range(B)]
    d_imu = imu_device(torch, [moving if moves[i] else static[i % 4] for i in range(B)], m + 3)
    hb.standstill_dev(d_imu.data_ptr(), m + 3, m, apply=1)
    hb.sync()
    for i in range(B):
        xd, Pd = hb.get_state_at(i)
        r = rec(hb, i)
        if moves[i]:
            assert r["flags"] == abi.SS_IMG_STATIC and r["gamma"] == 0.0 and np.array_equal(xd, x) and np.array_equal(Pd, P), i
        else:
            px, pP, pr, ppose = plain[i % 4]
            assert r == pr and np.array_equal(xd, px) and np.array_equal(Pd, pP) and np.array_equal(np.concatenate(hb.get_pose_at(i)), ppose), i
    # imu_stride = 0: every instance sees the same batch
    hb.set_state(x, P)
    hb.standstill_dev(d_imu.data_ptr(), 0, m, apply=1)
    for i in range(B):
        xd, Pd = hb.get_state_at(i)
        assert rec(hb, i) == plain[0][2] and np.array_equal(xd, plain[0][0]) and np.array_equal(Pd, plain[0][1]), i
    hb.close()
    hP.set_standstill(Z.ss_config())


def test_batch_front_end_reads_each_instances_own_tracks(gpu_required):
    """three camera streams behind one batch handle — 0 and 2 stand still, 1 moves — with a calibration table (the config's values: cam_of reads the
    table) and per-instance IMU batches that are all static: the image statistic of every instance is its own, instance 1 is vetoed and untouched,
    and each instance equals a plain handle fed the same stream and handed the batch instance's state"""
    import torch
    from rvio_amd import hip
    cfg = S.small_image_config()
    still = rv.synth.SynthSequence(cfg, duration=6.0, seed=0, motion="stationary")
    moves = rv.synth.SynthSequence(cfg, duration=6.0, seed=0)
    k0, n_frames, B = 70, 4, 3
    img_still = still.render(k0)
    seqs = [still, moves, still]
    imgs = [np.stack([img_still, moves.render(k0 + f), img_still]) for f in range(n_frames)]
    hb = hip.RvioHip(cfg, batch=B, front_end=True)
    hb.set_calibrations([abi.calibration_from_config(cfg)] * B)
    hs = [hip.RvioHip(cfg) for _ in range(B)]
    c = Z.ss_config(min_pairs=5, gate=0)
    for h in hs + [hb]:
        h.set_standstill(c)
    for i, q in enumerate(seqs):
        w, a, n = q.init_from_static(k0 - 1)
        hs[i].initialize(w, a, n)
        if i == 0:
            hb.initialize(w, a, n)
        hb.set_state_at(i, *hs[i].get_state())
    keep = []
    for f in range(n_frames):
        imu = np.stack([q.imu_between(k0 + f) for q in seqs])
        m = imu.shape[1]
        d_img, d_imu = torch.from_numpy(imgs[f]).cuda(), torch.from_numpy(imu.view(np.uint8).reshape(B, -1)).cuda()
        keep += [d_img, d_imu]
        torch.cuda.synchronize()
        hb.frame_batch_dev(d_img.data_ptr(), cfg.width, cfg.width * cfg.height, d_imu.data_ptr(), m, m)
        for i in range(B):
            hs[i].frame_dev(d_img[i].data_ptr(), cfg.width, d_imu[i].data_ptr(), m, 0, 0)
    states = [hb.get_state_at(i) for i in range(B)]
    for i in range(B):
        assert np.array_equal(hb.get_points_at(i)[0], hs[i].get_points()[0]) and np.array_equal(hb.get_points_at(i)[1], hs[i].get_points()[1])
        hs[i].set_state(*states[i])          # the batch instance's bits (a batch handle's filter agrees with a plain one to rounding only)
    batches = [Z.imu_batch(states[i][0], 10, seed=30 + i) for i in range(B)]
    for i in range(B):
        assert abi.standstill_model(states[i][0], batches[i], None, None, 1.0, 1.0, cfg.gravity, c)[0] <= c.imu_thr / 1.5
    d_b = imu_device(torch, batches, 10)
    hb.standstill_dev(d_b.data_ptr(), 10, 10, apply=1)
    for i in range(B):
        hs[i].standstill(batches[i], apply=1)
        r, rp = rec(hb, i), rec(hs[i])
        print("instance %d: %s" % (i, r))
        assert r == rp, (i, r, rp)
        xa, Pa = hb.get_state_at(i)
        xb, Pb = hs[i].get_state()
        assert np.array_equal(xa, xb) and np.array_equal(Pa, Pb), i
        assert r["n_pairs"] >= 20
        if i == 1:
            assert r["flags"] == abi.SS_IMU_STATIC and r["disparity"] > 1.5 * c.disp_thr_px and np.array_equal(xa, states[i][0]) and np.array_equal(Pa, states[i][1])
        else:
            assert r["flags"] == 0b1111 and r["disparity"] < c.disp_thr_px / 1.5 and not np.array_equal(xa, states[i][0])
    hb.close()
    for h in hs:
        assert h.frame_info()["device_error"] == 0
        h.close()


# ---------------------------------------------------------------- 5. windows and padding
@pytest.mark.parametrize("n", [0, 1, 9, 10, 31])
def test_every_window_with_poisoned_padding(gpu_required, n):
    from rvio_amd import hip
    h = hip.RvioHip(A.long_config())
    c = Z.ss_config(bias_rows=1, gate=0, sigma_bg=1e-3)
    h.set_standstill(c)
    x0, P0 = A.window_state(n)
    h.set_state(x0, P0)
    h.poison(7)
    h.propagate(K.batch(10, seed=0))        # writes the poisoned buffer's d x d block and makes it current: NaN in the padding up to ld = 210
    x, P = h.get_state()
    imu = Z.imu_batch(x, 64, seed=n)
    T, w_mean, _, _, f = abi.standstill_model(x, imu, None, None, 1.0, 1.0, A.long_config().gravity, c)
    assert T <= c.imu_thr / 1.5
    H, z, sigma = abi.standstill_measurement(24 + 6 * n, w_mean, c)
    xm, Pm, gm = abi.aux_update_model(x, P, H, z, sigma, abi.RVIO_AUX_VALUE)
    h.standstill(imu, apply=1)
    r = rec(h)
    xd, Pd = h.get_state()
    err = h.frame_info()["device_error"]
    h.close()
    dxw, dpw = S.state_delta(xd, xm), float(np.max(np.abs(Pd - Pm)))
    print("n=%d: state %.3e  P %.3e (bar %.3e)  gamma %.6g vs %.6g" % (n, dxw, dpw, A.p_bar(Pm), r["gamma"], gm))
    assert r["flags"] == 0b1111 and err == 0 and Pd.shape == (24 + 6 * n, 24 + 6 * n) and np.all(np.isfinite(Pd))
    assert dxw <= A.X_TOL and dpw <= A.p_bar(Pm) and abs(r["gamma"] - gm) <= 1e-7 * gm


# ---------------------------------------------------------------- 6. ordering
def ordering_inputs():
    cfg = S.small_image_config()
    seq = rv.synth.SynthSequence(cfg, duration=4.0, seed=0, motion="stationary", pixel_noise=0.02)
    img = seq.render(K0 + 1)                  # the platform never moves: one image
    return cfg, seq, img


def ordering_run(mode, sync):
    """12 whole frames with rvio_hip_standstill(apply = 1) behind each one; mode 'images' (rvio_hip_frame, the pipelined path) or 'points'
    (rvio_hip_frame_points); sync: rvio_hip_sync in front of and behind every standstill call"""
    from rvio_amd import hip
    cfg, seq, img = ordering_inputs()
    h = hip.RvioHip(cfg)
    h.set_standstill(Z.ss_config(min_pairs=5))
    h.initialize(*seq.init_from_static(K0))
    drv = rv.synth.DirectTrackDriver(seq)
    recs = []
    for k in range(K0 + 1, K0 + 13):
        imu = seq.imu_between(k)
        if mode == "images":
            h.frame(img, imu, None)
        else:
            inp = drv.inputs(k)
            h.frame_points(inp["tracked"], inp["status"], imu, inp["cand"])
        if sync:
            h.sync()
        h.standstill(imu, apply=1)
        if sync:
            h.sync()
        if mode == "points":
            drv.after(h.get_points()[0])      # (a getter of the tracker's points: it waits for the front end, not for the filter stream)
            r = h.get_standstill()
            recs.append((r.T, r.disparity, r.gamma, r.n_pairs, r.flags, r.m, r.img_count))
        else:
            recs.append(None)
    if mode == "images":                      # flat out: the records of the last call only (reading one waits for the filter stream)
        r = h.get_standstill()
        recs[-1] = (r.T, r.disparity, r.gamma, r.n_pairs, r.flags, r.m, r.img_count)
    x, P = h.get_state()
    pts, hl = h.get_points()
    err = h.frame_info()["device_error"]
    h.close()
    return dict(x=x, P=P, pts=pts, hl=hl, recs=np.array([r for r in recs if r is not None], float), err=np.array(err))


@pytest.mark.parametrize("mode", ["images", "points"])
def test_flat_out_equals_synchronised_and_paranoid(gpu_required, tmp_path, mode):
    a, b = ordering_run(mode, False), ordering_run(mode, True)
    print("%s: last record %s" % (mode, a["recs"][-1]))
    assert a["err"] == 0 and b["err"] == 0
    assert int(a["recs"][-1][4]) == 0b1111 and a["recs"][-1][3] >= 20      # the updates really apply
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    np.savez(str(tmp_path / "flat.npz"), **a)
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import test_gpu_standstill as T\n"
            "r = T.ordering_run(%r, False)\n"
            "ref = np.load(%r)\n"
            "assert all(np.array_equal(r[k], ref[k]) for k in r), [k for k in r if not np.array_equal(r[k], ref[k])]\n"
            "print('PARANOID_OK')\n") % (os.path.dirname(os.path.abspath(__file__)), mode, str(tmp_path / "flat.npz"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, RVIO_PARANOID="1"))
    assert out.returncode == 0 and "PARANOID_OK" in out.stdout, out.stderr[-2000:]


# ---------------------------------------------------------------- 7. errors
def test_argument_and_state_errors(gpu_required):
    import torch
    from rvio_amd import hip
    cfg = S.small_image_config()
    h = hip.RvioHip(cfg)
    L = h.L
    c = Z.ss_config()
    imu = Z.imu_batch(np.zeros(26), 8)
    ip = imu.ctypes.data_as(C.POINTER(abi.rvio_imu))
    d_imu = torch.from_numpy(imu.view(np.uint8)).cuda()
    torch.cuda.synchronize()
    dp = C.c_void_p(d_imu.data_ptr())
    r = abi.rvio_standstill()
    assert L.rvio_hip_get_standstill(h.h, 0, C.byref(r)) == -4                          # before the first call
    assert L.rvio_hip_set_standstill(h.h, C.byref(c)) == 0
    assert L.rvio_hip_standstill(h.h, ip, 8, 0) == -4 and L.rvio_hip_standstill_dev(h.h, dp, 0, 8, 0) == -4      # no state yet
    seq = rv.synth.SynthSequence(cfg, duration=3.0, seed=0)
    h.initialize(*seq.init_from_static(K0))
    assert L.rvio_hip_set_standstill(h.h, None) == 0
    assert L.rvio_hip_standstill(h.h, ip, 8, 0) == -4 and b"rvio_hip_set_standstill" in L.rvio_hip_last_error(h.h)      # switched off
    # bad configuration members, each named
    for name, val in (("sigma_a", 0.0), ("sigma_a", np.nan), ("sigma_w", -1.0), ("sigma_w", np.inf), ("imu_thr", 0.0), ("disp_thr_px", np.nan),
                      ("sigma_v", 0.0), ("sigma_bg", np.inf), ("min_pairs", 0), ("bias_rows", 2), ("gate", -1)):
        assert L.rvio_hip_set_standstill(h.h, C.byref(Z.ss_config(**{name: val}))) == -1, name
        assert name.encode() in L.rvio_hip_last_error(h.h), name
    assert L.rvio_hip_standstill(h.h, ip, 8, 0) == -4                                   # a refused configuration switches nothing on
    assert L.rvio_hip_set_standstill(h.h, C.byref(Z.ss_config(disp_thr_px=-1.0))) == 0 and L.rvio_hip_set_standstill(h.h, C.byref(c)) == 0
    assert L.rvio_hip_standstill(h.h, ip, 8, 0) == 0 and L.rvio_hip_standstill_dev(h.h, dp, 0, 8, 1) == 0 and L.rvio_hip_standstill_dev(h.h, dp, 8, 8, 0) == 0
    assert L.rvio_hip_get_standstill(h.h, 0, C.byref(r)) == 0 and r.m == 8 and r.img_count == 0
    assert L.rvio_hip_standstill(h.h, ip, 0, 0) == -1 and L.rvio_hip_standstill(h.h, ip, -1, 0) == -1 and L.rvio_hip_standstill(h.h, None, 8, 0) == -1
    assert L.rvio_hip_standstill(h.h, ip, 8, 2) == -1 and L.rvio_hip_standstill(h.h, ip, 8, -1) == -1
    assert L.rvio_hip_standstill_dev(h.h, dp, 7, 8, 0) == -1 and L.rvio_hip_standstill_dev(h.h, dp, -1, 8, 0) == -1 and L.rvio_hip_standstill_dev(h.h, None, 0, 8, 0) == -1
    assert L.rvio_hip_standstill_dev(h.h, dp, 0, 0, 0) == -1 and L.rvio_hip_standstill_dev(h.h, dp, 0, 8, 3) == -1
    assert L.rvio_hip_get_standstill(h.h, 1, C.byref(r)) == -1 and L.rvio_hip_get_standstill(h.h, -1, C.byref(r)) == -1 and L.rvio_hip_get_standstill(h.h, 0, None) == -1
    # inside an open frame
    img, fimu = seq.render(K0 + 1), seq.imu_between(K0 + 1)
    d_img, d_fimu = torch.from_numpy(img).cuda(), torch.from_numpy(fimu.view(np.uint8)).cuda()
    torch.cuda.synchronize()
    h.frame_begin_dev(d_img.data_ptr(), img.shape[1], d_fimu.data_ptr(), len(fimu), 0, 0)
    rc_open, rc_open_dev = L.rvio_hip_standstill(h.h, ip, 8, 1), L.rvio_hip_standstill_dev(h.h, dp, 0, 8, 1)
    do_update, do_augment = h.frame_plan()
    if do_update:
        h.update_tracked()
    h.augment_compose(do_augment)
    h.frame_end()
    assert rc_open == -4 and rc_open_dev == -4
    assert L.rvio_hip_standstill(h.h, ip, 8, 1) == 0                                    # behind the frame, on the pipelined handle
    assert L.rvio_hip_get_standstill(h.h, 0, C.byref(r)) == 0 and r.img_count == 1
    h.sync()
    assert h.frame_info()["device_error"] == 0
    h.close()
