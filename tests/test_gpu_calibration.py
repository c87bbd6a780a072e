"""Per-instance camera calibration (rvio_hip_set_calibration_at / rvio_hip_set_calibrations / rvio_hip_get_calibration_at) and
rvio_hip_initialize_at: every instance of a handle computes with its own intrinsics, distortion model and camera-IMU extrinsic.

The arithmetic does not change, only where its constants come from — so the bar throughout is BIT-FOR-BIT against a handle created with
that calibration in its config, and every case carries a control (the same inputs under the common calibration must give other bits), or
a kernel that still read the common copy would pass.

Three calibrations: c0 the stock config; c1 rad-tan with another focal length and centre, k3 != 0 and a T_BC0 turned by 35 degrees with
another lever arm; c2 fisheye (the coefficients of test_gpu_edges.py::test_fisheye_camera) with a T_BC0 turned by -50 degrees.  cfg_i is
cfg B with calibration c_i, a window of 6 clones (max_track_len 7) and min_track_len 2: the first update is the fourth frame's."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import scenarios as S
from test_gpu_batch import pack_inputs, same_filter_state

abi, rv = O.abi, O.rv
pytestmark = pytest.mark.gpu
ML, MIN_LEN = 7, 2


def _rot(axis, deg):
    a = np.asarray(axis, float)
    a /= np.linalg.norm(a)
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def _T(axis, deg, t):
    T0 = np.array(abi._T_BC0).reshape(4, 4)
    M = np.eye(4)
    M[:3, :3] = T0[:3, :3] @ _rot(axis, deg)
    M[:3, 3] = t
    return M


CALS = [dict(),
        dict(fx=420.5, fy=431.25, cx=351.0, cy=262.5, k1=-0.25, k2=0.06, p1=0.0004, p2=-0.0003, k3=0.01,
             T=_T([1, 2, 3], 35.0, [0.05, -0.03, 0.08])),
        dict(fisheye=1, k1=-0.0137, k2=0.0207, p1=-0.0128, p2=0.0025, T=_T([-2, 1, 0.5], -50.0, [-0.04, 0.06, -0.02]))]


def cfg_i(i, **over):
    kw = dict(CALS[i])
    Tm = kw.pop("T", None)
    kw.update(max_track_len=ML, min_track_len=MIN_LEN)
    kw.update(over)
    c = abi.config_named("B", **kw)
    if Tm is not None:
        for k, v in enumerate(Tm.reshape(-1)):
            c.T_bc[k] = v
    return c


class FisheyeSequence(rv.synth.SynthSequence):
    """the synthetic scene seen through the camera model Camera.Fisheye: 1 undistorts (cv::fisheye, equidistant: theta_d = theta (1 + k1 theta^2
    + k2 theta^4 + k3 theta^6 + k4 theta^8) with D = (k1, k2, p1, p2) of the config) — SynthSequence.project is the rad-tan model only, and a
    stream rendered with it but normalised as a fisheye image gives the chi^2 gate nothing to accept"""

    def project(self, k, noise=True):
        c = self.cfg
        R_wb, p_w = self.pose(self.frame_time(k))
        pc = ((self.landmarks - p_w) @ R_wb - self.t_bc) @ self.R_bc
        z = pc[:, 2]
        ok = z > 0.5
        zs = np.where(ok, z, 1.0)
        x, y = pc[:, 0] / zs, pc[:, 1] / zs
        r = np.sqrt(x * x + y * y)
        th = np.arctan(r)
        th2 = th * th
        th_d = th * (1 + th2 * (float(c.k1) + th2 * (float(c.k2) + th2 * (float(c.p1) + th2 * float(c.p2)))))
        sc = np.where(r > 1e-8, th_d / np.maximum(r, 1e-8), 1.0)
        u = float(c.fx) * x * sc + float(c.cx)
        v = float(c.fy) * y * sc + float(c.cy)
        ok &= r * r < 1.2
        if noise and self.pixel_noise > 0:
            nr = np.random.default_rng(1000003 * (self.seed + 1) + k).standard_normal((len(u), 2))
            u = u + self.pixel_noise * nr[:, 0]
            v = v + self.pixel_noise * nr[:, 1]
        margin = 20.0
        ok &= (u > margin) & (u < c.width - margin) & (v > margin) & (v < c.height - margin)
        return np.stack([u, v], 1).astype(np.float32), ok


def make_seq(cfg, seed):
    return (FisheyeSequence if cfg.fisheye else rv.synth.SynthSequence)(cfg, duration=8.0, seed=seed)


def cal_i(i):
    return abi.calibration_from_config(cfg_i(i))


def same_cal(a, b):
    return bytes(a) == bytes(b)


def to_dev(torch, arrays):
    return [torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda() for a in arrays]


def bind(h, B):
    """c1 through the _at call, c2 through the bulk call (which hands the others back as the getter returned them)"""
    h.set_calibration_at(1, cal_i(1))
    cals = [h.get_calibration_at(j) for j in range(B)]
    for j in range(B):
        if j % 3 == 2:
            cals[j] = cal_i(2)
        elif j % 3 == 1 and j > 1:
            cals[j] = cal_i(1)
    h.set_calibrations(cals)


# ---------------------------------------------------------------- 1. filter only
@pytest.fixture(scope="module")
def recs3():
    cfgs = [cfg_i(i, enable_equalizer=0) for i in range(3)]
    seqs_recs = [S.record_sequence(cfgs[i], n_frames=10, seed=i) for i in range(3)]
    return cfgs, [sr[0] for sr in seqs_recs], [sr[1] for sr in seqs_recs]


@pytest.mark.parametrize("B", [3, 128])
def test_filter_only_batch_with_mixed_calibrations(gpu_required, recs3, B):
    """rvio_hip_frame_tracks_dev, instance j under calibration j % 3, on hand-over tables the oracle recorded under cfg_(j % 3): every
    instance within 1e-9 of its oracle state per frame, bit-identical to the same instance of a handle created with cfg_(j % 3), and NOT
    the bits of a handle left at c0.  Calibration is read by geom4_kernel and feat_build_kernel<4> here (every batch handle with
    max_track_len <= 16).  update_forms() at this window (6n <= 36), for reference — none of the forms below reads calibration:
      B = 3:    LPC_NONE, LPG_REDUCE (gram_finish), LPT_GEMM, LPS_SOLVE6_1, LPD_INSIDE, LPJ_STRIPS
      B = 128:  LPC_NONE, LPG_BATCH4 + lit_batch, LPT_GEMM_LDS, LPS_SOLVE6_1, LPD_INSIDE, LPJ_BATCH
    (B = 128, a multiple of 8, also takes the XCD-aware workgroup order of batch_remap() in the kernels that use it: the calibrated kernels
    keep the plain order, and their table index is blockIdx.z.)  Frames 4-7, 9, 10 hand over at most 24 features (the literal path's
    export in feat_build_kernel), frame 8 the first full-length tracks (71-78 features)."""
    from rvio_amd import hip
    import torch
    cfgs, _, recs = recs3
    nfr = len(recs[0])
    hm = hip.RvioHip(cfgs[0], batch=B)
    whole = [hip.RvioHip(cfgs[i], batch=B) for i in range(3)]          # whole[0] is also the control: a handle left at c0
    for j in range(B):
        assert same_cal(hm.get_calibration_at(j), cal_i(0))
    bind(hm, B)
    for j in range(B):
        assert same_cal(hm.get_calibration_at(j), cal_i(j % 3)), j
    for h in [hm] + whole:
        h.set_state(recs[0][0]["x0"], recs[0][0]["P0"])
        for j in range(B):
            h.set_state_at(j, recs[j % 3][0]["x0"], recs[j % 3][0]["P0"])
    n_upd, worst = 0, 0.0
    for f in range(nfr):
        rf = [recs[j % 3][f] for j in range(B)]
        n_feat, types, lens, meas, imu, m = pack_inputs(cfgs[0], rf)
        d = to_dev(torch, (imu, n_feat, types, lens, meas))
        torch.cuda.synchronize()
        for h in [hm] + whole:
            h.frame_tracks_dev(d[0].data_ptr(), m, m, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr())
        for h in [hm] + whole:
            h.sync()
        for j in range(B):
            xa, Pa = hm.get_state_at(j)
            dlt = S.state_delta(xa, rf[j]["x3"])
            worst = max(worst, dlt)
            assert dlt <= 1e-9, (f, j, dlt)
            xw, Pw = whole[j % 3].get_state_at(j)
            assert np.array_equal(xa, xw) and np.array_equal(Pa, Pw), (f, j)
            n_upd += int(bool(rf[j]["did_update"]) and rf[j]["diag"]["updated"])
        if rf[0]["did_update"]:
            assert hm.frame_info()["updated"] == rf[0]["diag"]["updated"] == 1, f
    print("B = %d: worst |state - oracle| = %.3e, %d updates applied" % (B, worst, n_upd))
    assert n_upd == 7 * B                                               # frames 4 .. 10 of every sequence (within 1e-9 of the oracle's: applied)
    # the control: the same inputs under the common calibration are other bits
    for j in (1, 2):
        assert not np.array_equal(hm.get_state_at(j)[0], whole[0].get_state_at(j)[0]), j
    assert np.array_equal(hm.get_state_at(0)[0], whole[0].get_state_at(0)[0])
    for h in [hm] + whole:
        h.close()


# ---------------------------------------------------------------- 2. with the front end
@pytest.fixture(scope="module")
def scenes3():
    cfgs = [cfg_i(i) for i in range(3)]                                # stock front end: CLAHE on, corners from the device detector
    n_frames, k0 = 14, 60
    seqs = [make_seq(cfgs[i], i) for i in range(3)]
    imgs = np.stack([[q.render(k0 + f) for q in seqs] for f in range(n_frames)])       # [frame][instance][H][W]
    imus = [[q.imu_between(k0 + f) for q in seqs] for f in range(n_frames)]
    return cfgs, seqs, imgs, imus


def test_front_end_batch_with_mixed_calibrations(gpu_required, scenes3):
    """rvio_hip_frame_batch_dev, B = 3, stream i rendered under cfg_i: the undistortion of the tracked points and of the refilled corners
    (ransac_book_kernel / ransac_book_a_kernel + bookkeep_b_kernel), RANSAC's gyro prior, geom4_kernel, feat_build_kernel<4> and
    landmark_kernel all index the table.  Against three plain handles created with cfg_i (tracker tables bit for bit, states to the
    batch-against-plain rounding bar of test_gpu_batch.py) and against whole-cfg_i batch handles fed the same three streams (bit for bit,
    the landmark cloud included).  Every instance is initialised by rvio_hip_initialize_at from its own stationary IMU average."""
    from rvio_amd import hip
    import torch
    cfgs, seqs, imgs, imus = scenes3
    B, n_frames = 3, len(imgs)
    hb = hip.RvioHip(cfgs[0], batch=B, front_end=True)
    whole = [hip.RvioHip(cfgs[i], batch=B, front_end=True) for i in range(3)]
    hs = [hip.RvioHip(cfgs[i]) for i in range(3)]
    bind(hb, B)
    inits = [q.init_from_static(38) for q in seqs]
    for h in [hb] + whole:
        h.set_landmarks(True)
        h.initialize(*inits[0])
        for i in range(B):
            h.initialize_at(i, *inits[i])
    for i in range(B):
        hs[i].initialize(*inits[i])
        xa, Pa = hb.get_state_at(i)
        xb, Pb = hs[i].get_state()
        assert np.array_equal(xa, xb) and np.array_equal(Pa, Pb), i
    keep, n_upd, n_pts = [], [0] * B, 0
    for f in range(n_frames):
        m = len(imus[f][0])
        assert all(len(u) == m for u in imus[f])
        d_img = torch.from_numpy(imgs[f]).cuda()
        d_imu = torch.from_numpy(np.stack(imus[f]).view(np.uint8).reshape(B, -1)).cuda()
        keep += [d_img, d_imu]
        torch.cuda.synchronize()
        W, H = cfgs[0].width, cfgs[0].height
        for h in [hb] + whole:
            h.frame_batch_dev(d_img.data_ptr(), W, W * H, d_imu.data_ptr(), m, m)
        for i in range(B):
            hs[i].frame_dev(d_img[i].data_ptr(), W, d_imu[i].data_ptr(), m, 0, 0)
        for h in [hb] + whole + hs:
            h.sync()
        for i in range(B):
            xa, Pa = hb.get_state_at(i)
            xb, Pb = hs[i].get_state()
            assert same_filter_state(xa, Pa, xb, Pb), (f, i)
            pa, la = hb.get_points_at(i)
            pb, lb = hs[i].get_points()
            assert len(pa) > 50 and np.array_equal(pa, pb) and np.array_equal(la, lb), (f, i)
            xw, Pw = whole[i].get_state_at(i)
            assert np.array_equal(xa, xw) and np.array_equal(Pa, Pw), (f, i)
            la_, lw = hb.landmarks_at(i), whole[i].landmarks_at(i)
            assert la_["frame"] == lw["frame"] and la_["n"] == lw["n"], (f, i)
            for key in ("feat", "p_r", "p_world"):
                assert np.array_equal(la_[key], lw[key]), (f, i, key)
            n_upd[i] += hs[i].frame_info()["updated"]
            n_pts += la_["n"]
    assert min(n_upd) >= 3 and n_pts > 30, (n_upd, n_pts)
    # the control: streams 1 and 2 under the common calibration are other bits (and another tracker table: other normalised coordinates, other inliers)
    for i in (1, 2):
        assert not np.array_equal(hb.get_state_at(i)[0], whole[0].get_state_at(i)[0]), i
    assert np.array_equal(hb.get_state_at(0)[0], whole[0].get_state_at(0)[0])
    for h in [hb] + whole + hs:
        h.close()


# ---------------------------------------------------------------- 3. plain handles
def test_plain_handle_recalibrated_through_frame_points(gpu_required, recs3):
    """a plain handle created with cfg_0 and given c1 (instance 0) against one created with cfg_1, through rvio_hip_frame_points on the
    direct-track inputs recorded under cfg_1: ransac_kernel and bookkeep_b_kernel (LPB_PLAIN), feat_prop_kernel / feat_build_kernel<16> and
    landmark_kernel index a table of one entry.  update_forms() of one stream at 6n <= 36: LPC_ROLE, LPG_REDUCE, LPS_SMALL (the factor
    comes from the role workgroup), LPD_ROLES, LPJ_LDS."""
    from rvio_amd import hip
    cfgs, seqs, recs = recs3
    ha, hb, h0 = hip.RvioHip(cfgs[0]), hip.RvioHip(cfgs[1]), hip.RvioHip(cfgs[0])
    ha.set_calibration_at(0, cal_i(1))
    assert same_cal(ha.get_calibration_at(0), cal_i(1)) and same_cal(hb.get_calibration_at(0), cal_i(1))
    w, a, n = seqs[1].init_from_static(38)
    for h in (ha, hb, h0):
        h.set_landmarks(True)
        h.initialize(w, a, n)
    n_upd, n_pts, worst = 0, 0, 0.0
    for f, r in enumerate(recs[1]):
        inp = r["inp"]
        for h in (ha, hb, h0):
            h.frame_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])
        xa, Pa = ha.get_state()
        xb, Pb = hb.get_state()
        assert np.array_equal(xa, xb) and np.array_equal(Pa, Pb), f
        worst = max(worst, S.state_delta(xa, r["x3"]))
        if len(inp["tracked"]):
            ua, ub = ha.debug_tracked(len(inp["tracked"])), hb.debug_tracked(len(inp["tracked"]))
            assert np.array_equal(ua[0], ub[0]) and np.array_equal(ua[1], ub[1]), f
            assert not np.array_equal(ua[1], h0.debug_tracked(len(inp["tracked"]))[1]), f          # control: c0 normalises differently
        la, lb = ha.landmarks(), hb.landmarks()
        assert la["frame"] == lb["frame"] and np.array_equal(la["feat"], lb["feat"]) and np.array_equal(la["p_r"], lb["p_r"]), f
        assert np.array_equal(la["p_world"], lb["p_world"]), f
        pa, hla = ha.get_points()
        assert np.array_equal(pa, r["pts"]) and np.array_equal(hla, r["hist_len"]), f
        n_upd += ha.frame_info()["updated"]
        n_pts += la["n"]
    assert n_upd == 7 and n_pts > 30 and worst <= 1e-6, (n_upd, n_pts, worst)      # (1e-6: the front end's bar against the oracle, test_gpu_edges.py)
    assert not np.array_equal(ha.get_state()[0], h0.get_state()[0])
    for h in (ha, hb, h0):
        h.close()


class _DA:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}


@pytest.mark.parametrize("load", ["above24", "upto24"])
def test_sharded_ranks_recalibrated(gpu_required, recs3, load):
    """rvio_hip_update_local / rvio_hip_update_global at world 2 on one GPU: both ranks created with cfg_0 and set to c1 against ranks
    created with cfg_1 — states and each rank's landmark cloud bit for bit.  (Up to 24 features every rank builds every feature, above
    that rank r builds the features f % 2 == r: feat_build_kernel<16> with shard_world = 2.)"""
    import torch
    from rvio_amd import hip
    cfgs, seqs, recs = recs3
    r = recs[1][-1]
    assert r["did_update"]
    if load == "above24":
        types, lens, meas = S.worst_case_tracks(cfgs[1], r, seqs[1], n_feat=60)
    else:
        types, lens, meas = r["types"][:20], r["lens"][:20], r["meas"][:20]
    world = 2

    def run(make):
        hs = [make() for _ in range(world)]
        blocks = []
        for rk, h in enumerate(hs):
            h.set_landmarks(True)
            h.set_state(r["x1"], r["P1"])
            ptr, n = h.update_local(types, lens, meas, rk, world)
            h.sync()
            blocks.append(torch.as_tensor(_DA(ptr, n), device="cuda").clone())
        allb = torch.cat(blocks).contiguous()
        torch.cuda.synchronize()
        out = []
        for h in hs:
            h.update_global(allb.data_ptr(), world)
            out.append((h.get_state(), h.landmarks(), h.frame_info()["updated"]))
            h.close()
        return out

    def recalibrated():
        h = hip.RvioHip(cfgs[0])
        h.set_calibration_at(0, cal_i(1))
        return h

    got, want, ctrl = run(recalibrated), run(lambda: hip.RvioHip(cfgs[1])), run(lambda: hip.RvioHip(cfgs[0]))
    for rk in range(world):
        (xa, Pa), la, ua = got[rk]
        (xb, Pb), lb, ub = want[rk]
        assert ua == ub == 1 and la["n"] >= 3, (rk, ua, ub, la["n"])
        assert np.array_equal(xa, xb) and np.array_equal(Pa, Pb), rk
        for key in ("feat", "p_r", "p_world"):
            assert np.array_equal(la[key], lb[key]), (rk, key)
        assert not np.array_equal(xa, ctrl[rk][0][0]), rk
    assert np.array_equal(got[0][0][0], got[1][0][0])                   # the update is replicated


# ---------------------------------------------------------------- 4. book-keeping
def test_table_bookkeeping_and_invalid_arguments(gpu_required, recs3):
    from rvio_amd import hip
    import torch
    cfgs, _, recs = recs3
    B = 3
    hb, hw = hip.RvioHip(cfgs[0], batch=B), hip.RvioHip(cfgs[1], batch=B)
    L = hb.L
    for j in range(B):
        assert same_cal(hb.get_calibration_at(j), cal_i(0)) and same_cal(hw.get_calibration_at(j), cal_i(1))
    hb.set_calibration_at(1, cal_i(1))
    assert [same_cal(hb.get_calibration_at(j), cal_i(0)) for j in range(B)] == [True, False, True]      # untouched instances: the config's
    assert same_cal(hb.get_calibration_at(1), cal_i(1))
    # every RVIO_ERR_INVALID case; none of them changes the table
    k = cal_i(2)
    out = abi.rvio_calibration()
    assert L.rvio_hip_set_calibration_at(None, 0, C.byref(k)) == -1
    assert L.rvio_hip_set_calibration_at(hb.h, 0, None) == -1
    assert L.rvio_hip_set_calibrations(None, C.byref(k)) == -1
    assert L.rvio_hip_set_calibrations(hb.h, None) == -1
    assert L.rvio_hip_get_calibration_at(None, 0, C.byref(out)) == -1
    assert L.rvio_hip_get_calibration_at(hb.h, 0, None) == -1
    for bad in (-1, B, B + 5):
        assert L.rvio_hip_set_calibration_at(hb.h, bad, C.byref(k)) == -1
        assert L.rvio_hip_get_calibration_at(hb.h, bad, C.byref(out)) == -1

    def broken(**kw):
        c = cal_i(2)
        for name, v in kw.items():
            if name.startswith("T"):
                c.T_bc[int(name[1:])] = v
            else:
                setattr(c, name, v)
        return c
    bads = [broken(fx=0.0), broken(fy=0.0), broken(fx=float("nan")), broken(cy=float("inf")), broken(k3=float("-inf")), broken(p1=float("nan")),
            broken(T5=float("nan")), broken(T3=float("inf")), broken(T15=float("nan"))]
    for c in bads:
        assert L.rvio_hip_set_calibration_at(hb.h, 2, C.byref(c)) == -1
        arr = (abi.rvio_calibration * B)(cal_i(2), cal_i(2), c)
        assert L.rvio_hip_set_calibrations(hb.h, arr) == -1               # one bad entry refuses the whole call
    assert b"instance 2" in L.rvio_hip_last_error(hb.h)
    assert [same_cal(hb.get_calibration_at(j), cal_i(i)) for j, i in enumerate((0, 1, 0))] == [True] * 3
    assert L.rvio_hip_set_calibration_at(hb.h, 2, C.byref(broken(fx=-300.0, k1=0.0))) == 0      # negative focal length, zero distortion: finite, accepted
    hb.set_calibration_at(2, cal_i(0))
    hp = hip.RvioHip(cfgs[0])
    assert L.rvio_hip_set_calibration_at(hp.h, 1, C.byref(k)) == -1       # a plain handle has instance 0 only
    assert L.rvio_hip_get_calibration_at(hp.h, 1, C.byref(out)) == -1
    hp.close()
    # the table survives rvio_hip_initialize, rvio_hip_set_state* and rvio_hip_debug_poison(7): one update from a recorded state, instance 1 under c1
    r = recs[1][7]
    assert r["did_update"] and len(r["lens"]) > 24
    hb.initialize(np.zeros(3), np.array([0.0, 0.0, 9.8]), 20)
    for h in (hb, hw):
        h.set_state(r["x0"], r["P0"])
        h.set_state_at(1, r["x0"], r["P0"])
        h.L.rvio_hip_frame_plan(h.h, None, None)
        h.L.rvio_hip_frame_plan(h.h, None, None)
    hb.poison(7)
    assert same_cal(hb.get_calibration_at(1), cal_i(1)) and same_cal(hb.get_calibration_at(0), cal_i(0))
    n_feat, types, lens, meas, imu, m = pack_inputs(cfgs[0], [r] * B)
    d = to_dev(torch, (imu, n_feat, types, lens, meas))
    torch.cuda.synchronize()
    for h in (hb, hw):
        h.frame_tracks_dev(d[0].data_ptr(), m, m, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr())
        h.sync()
    xa, Pa = hb.get_state_at(1)
    xw, Pw = hw.get_state_at(1)
    assert np.array_equal(xa, xw) and np.array_equal(Pa, Pw)
    assert S.state_delta(xa, r["x3"]) <= 1e-9
    assert not np.array_equal(xa, hb.get_state_at(0)[0])                  # instance 0 (c0) on the same inputs: other bits
    hb.close()
    hw.close()


def test_initialize_at(gpu_required, recs3):
    from rvio_amd import hip
    import torch
    cfgs, seqs, recs = recs3
    B = 3
    inits = [q.init_from_static(38) for q in seqs]
    hb, hp = hip.RvioHip(cfgs[0], batch=B), hip.RvioHip(cfgs[0])
    hb.initialize(*inits[0])
    x0, P0 = hb.get_state_at(0)
    hb.initialize_at(1, *inits[1])
    hp.initialize(*inits[1])
    xa, Pa = hb.get_state_at(1)
    xb, Pb = hp.get_state()
    assert xa.shape == (26,) and Pa.shape == (24, 24)
    assert np.array_equal(xa, xb) and np.array_equal(Pa, Pb)              # the code rvio_hip_initialize runs, bit for bit
    assert not np.array_equal(xa, x0)
    for j in (0, 2):                                                       # the other instances keep their states
        xj, Pj = hb.get_state_at(j)
        assert np.array_equal(xj, x0) and np.array_equal(Pj, P0), j
    hp.initialize_at(0, *inits[2])                                         # a plain handle: instance 0
    hb.initialize_at(2, *inits[2])
    assert np.array_equal(hp.get_state()[0], hb.get_state_at(2)[0])
    w = (C.c_double * 3)(*inits[1][0])
    a = (C.c_double * 3)(*inits[1][1])
    L = hb.L
    assert L.rvio_hip_initialize_at(None, 0, w, a, 10) == -1
    assert L.rvio_hip_initialize_at(hb.h, 0, None, a, 10) == -1 and L.rvio_hip_initialize_at(hb.h, 0, w, None, 10) == -1
    assert L.rvio_hip_initialize_at(hb.h, -1, w, a, 10) == -1 and L.rvio_hip_initialize_at(hb.h, B, w, a, 10) == -1
    assert L.rvio_hip_initialize_at(hp.h, 1, w, a, 10) == -1
    # a non-empty window: RVIO_ERR_STATE, and nothing is stored
    for f in range(3):
        n_feat, types, lens, meas, imu, m = pack_inputs(cfgs[0], [recs[0][f]] * B)
        d = to_dev(torch, (imu, n_feat, types, lens, meas))
        torch.cuda.synchronize()
        hb.frame_tracks_dev(d[0].data_ptr(), m, m, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr())
        hb.sync()
    before = hb.get_state_at(1)
    assert len(before[0]) > 26
    assert L.rvio_hip_initialize_at(hb.h, 1, w, a, 10) == -4
    assert b"empty window" in L.rvio_hip_last_error(hb.h)
    after = hb.get_state_at(1)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    hb.close()
    hp.close()
