"""GPU: relative-pose measurements between two frames of the clone window (rvio_hip_update_rel*, csrc/rel_rows.hip in front of
csrc/aux_update.hip).  The rows the device forms against abi.rel_model (bar 1e-12 max(1, max|H|), the columns the header's table lists as 0
exactly 0.0, all of 0 - 23 among them); the applied update against abi.aux_update_model on the model's rows at the bars of
tests/test_gpu_fix_past.py; a twin handle handed the device's own rows through rvio_hip_update_aux ends with the same bits; nothing outside the
span's clones enters; the gate; batch handles with per-instance spans, strides and flags, a span outside the window among them; frames flat out
against synchronised; the record and every refusal.  One handle of the longest window (max_track_len = 32, leading dimension 210) takes the
states of every window."""
import ctypes as C

import numpy as np
import pytest

import rel_cases as R
import scenarios as S
from test_gpu_aux_update import GAMMA_RTOL
from test_gpu_fix import diag_of, place

abi, A, K = R.abi, R.A, R.K
rv = A.rv
pytestmark = pytest.mark.gpu
K0 = 38
P_, A_, Q_ = abi.RVIO_REL_POSITION, abi.RVIO_REL_ATTITUDE, abi.RVIO_REL_POSE


@pytest.fixture(scope="module")
def hL(gpu_required):
    from rvio_amd import hip
    h = hip.RvioHip(A.long_config())
    yield h
    assert h.frame_info()["device_error"] == 0
    h.close()


def run(h, kind, meas, a, b, gate=0):
    h.update_rel(kind, meas, a, b, gate)
    xd, Pd = h.get_state()
    return dict(x=xd, P=Pd, diag=diag_of(h), pose=h.pose(), rows=h.get_fix_rows())


def check_rows(tag, x, kind, meas, a, b, out):
    H, r, sigma = abi.rel_model(x, kind, meas, a, b)
    Hd, sd = out["rows"]
    dg = out["diag"]
    m, n = abi.REL_ROWS[kind], (len(x) - 26) // 7
    bar = 1e-12 * max(1.0, float(np.max(np.abs(H))))
    eh, er = float(np.max(np.abs(Hd - H))), float(np.max(np.abs(dg["r"][:m] - r)))
    print("%s: max|H - model| %.3e  max|r - model| %.3e (bar %.1e, max|H| %.3g)" % (tag, eh, er, bar, np.max(np.abs(H))))
    assert Hd.shape == H.shape and eh <= bar and er <= bar
    assert np.array_equal(sd, sigma) and not dg["r"][m:].any() and (dg["kind"], dg["m"]) == (kind, m)
    for blk_i, zero in enumerate(R.zero_cols(n, kind, a, b)):
        blk = Hd[3 * blk_i: 3 * blk_i + 3][:, zero]
        assert set(range(24)) <= set(zero)
        assert not blk.any() and not np.signbit(blk).any(), "a column the table lists as 0"
        assert np.abs(Hd[3 * blk_i: 3 * blk_i + 3]).sum() > 1.0
    return eh, er


# ---------------------------------------------------------------- 1. the rows
@pytest.mark.parametrize("n", R.WINDOWS)
def test_rows_against_the_model(hL, n):
    x0, P0 = A.window_state(n)
    worst = [0.0, 0.0]
    for kind, a, b in R.combos(n):
        for li, lever in enumerate(R.LEVERS):
            x, P = place(hL, x0, P0, n != 31)      # (padding where the window leaves some: behind a poisoned propagation)
            meas = R.meas_near(x, kind, a, b, lever, sigma_p=(0.02, 0.03, 0.04), sigma_q=(0.005, 0.006, 0.007), seed=n + a + b + li)
            out = run(hL, kind, meas, a, b)
            eh, er = check_rows("%s n=%d span=(%d, %d) lever=%d" % (R.KIND_NAMES[kind], n, a, b, 1 - li), x, kind, meas, a, b, out)
            worst = [max(worst[0], eh), max(worst[1], er)]
            assert out["diag"]["applied"] == 1 and out["rows"][0].shape[1] == 24 + 6 * n and out["diag"]["img_count"] == -a
    print("n=%d: worst max|H - model| %.3e, worst max|r - model| %.3e" % (n, worst[0], worst[1]))


# ---------------------------------------------------------------- 2. the applied update
@pytest.mark.parametrize("n", R.WINDOWS)
def test_applied_update_against_the_model(hL, n):
    x0, P0 = A.window_state(n)
    worst = [0.0, 0.0]
    for kind, a, b in R.combos(n):
        x, P = place(hL, x0, P0, n != 31)
        meas = R.meas_near(x, kind, a, b, R.LEVER, sigma_p=0.02, sigma_q=0.005, seed=3 + n + a + b)
        out = run(hL, kind, meas, a, b)
        H, r, sigma = abi.rel_model(x, kind, meas, a, b)
        xw, Pw, gw = abi.aux_update_model(x, P, H, r, sigma)
        xd, Pd, dg = out["x"], out["P"], out["diag"]
        dxw, dpw = S.state_delta(xd, xw), float(np.max(np.abs(Pd - Pw)))
        worst = [max(worst[0], dxw), max(worst[1], dpw / float(np.max(np.abs(Pw))))]
        print("%s n=%d span=(%d, %d): state %.3e (bar %.0e)  P %.3e (bar %.3e)  gamma %.6g vs %.6g" % (R.KIND_NAMES[kind], n, a, b, dxw, A.X_TOL, dpw, A.p_bar(Pw), dg["gamma"], gw))
        assert dg["applied"] == 1 and np.all(np.isfinite(Pd))
        assert dxw <= A.X_TOL and dpw <= A.p_bar(Pw)
        assert np.array_equal(Pd, Pd.T)
        assert abs(dg["gamma"] - gw) <= GAMMA_RTOL * abs(gw)
        wp, wq = abi.pose_line(xd)
        assert np.max(np.abs(out["pose"][0] - wp)) <= 1e-12 and np.max(np.abs(out["pose"][1] - wq)) <= 1e-12
        assert np.max(np.abs(xd - x)) > 1e-10
        # the window's delta pose moved onto the measurement
        assert np.linalg.norm(abi.rel_model(xd, kind, meas, a, b)[1]) < np.linalg.norm(r)
    print("n=%d: worst state distance %.3e, worst |P - model| / max|P| %.3e" % (n, worst[0], worst[1]))


# ---------------------------------------------------------------- 3. the bits of a twin
@pytest.mark.parametrize("kind", [P_, Q_], ids=["m3", "m6"])
def test_a_twin_handed_the_devices_rows_ends_with_the_same_bits(hL, kind):
    from rvio_amd import hip
    twin = hip.RvioHip(A.long_config())
    for n in (3, 10):
        x, P = A.window_state(n)
        a, b = n // 2, n
        meas = R.meas_near(x, kind, a, b, R.LEVER, sigma_p=0.02, sigma_q=0.005, seed=n)
        hL.set_state(x, P)
        out = run(hL, kind, meas, a, b)
        m = abi.REL_ROWS[kind]
        twin.set_state(x, P)
        twin.update_aux(out["rows"][0], out["diag"]["r"][:m], out["rows"][1], abi.RVIO_AUX_RESIDUAL, 0)
        xt, Pt = twin.get_state()
        pt = twin.pose()
        gt, at = twin.aux_diag()
        assert at == 1 and out["diag"]["applied"] == 1 and gt == out["diag"]["gamma"]
        assert np.array_equal(xt, out["x"]) and np.array_equal(Pt, out["P"])
        assert np.array_equal(pt[0], out["pose"][0]) and np.array_equal(pt[1], out["pose"][1])
        assert np.max(np.abs(xt - x)) > 1e-10
    assert twin.frame_info()["device_error"] == 0
    twin.close()


# ---------------------------------------------------------------- 4. nothing outside the span enters
def test_states_that_differ_outside_the_span_give_the_same_bits(hL):
    from rvio_amd import hip
    twin = hip.RvioHip(A.long_config())
    for n in (3, 10, 31):
        x, P = A.window_state(n)
        for kind, a, b in R.combos(n):
            meas = R.meas_near(x, kind, a, b, R.LEVER, sigma_p=0.02, sigma_q=0.005, seed=n + a)
            y = R.outside_replaced(x, a, b, seed=n + b)
            assert np.max(np.abs(y[0:26] - x[0:26])) > 1e-3
            hL.set_state(x, P)
            twin.set_state(y, P)
            o0, o1 = run(hL, kind, meas, a, b), run(twin, kind, meas, a, b)
            assert np.array_equal(o0["rows"][0], o1["rows"][0]) and np.array_equal(o0["rows"][1], o1["rows"][1])
            assert np.array_equal(o0["diag"]["r"], o1["diag"]["r"]) and o0["diag"]["r"][:3].any()
    assert twin.frame_info()["device_error"] == 0
    twin.close()


# ---------------------------------------------------------------- 5. the gate
def meas_with_gamma(x, P, kind, a, b, target, seed):
    s = 1.0
    for _ in range(8):
        meas = R.meas_near(x, kind, a, b, R.LEVER, dp=0.01 * s, dth=0.002 * s, sigma_p=0.02, sigma_q=0.005, seed=seed)
        g = abi.aux_update_model(x, P, *abi.rel_model(x, kind, meas, a, b))[2]
        s *= np.sqrt(target / g)
    return meas, g


@pytest.mark.parametrize("kind", R.KINDS, ids=[R.KIND_NAMES[k] for k in R.KINDS])
def test_gate_accepts_and_rejects(hL, kind):
    n, a, b = 10, 2, 7
    x, P = A.window_state(n)
    chi = A.chi2_95(abi.REL_ROWS[kind])
    meas, gw = meas_with_gamma(x, P, kind, a, b, chi / 4, seed=5)
    assert gw <= chi / 2
    hL.set_state(x, P)
    out = run(hL, kind, meas, a, b, gate=1)
    xw, Pw, _ = abi.aux_update_model(x, P, *abi.rel_model(x, kind, meas, a, b))
    print("gate/accept %s: gamma %.6g vs %.6g (table %.6g)" % (R.KIND_NAMES[kind], out["diag"]["gamma"], gw, chi))
    assert out["diag"]["applied"] == 1 and abs(out["diag"]["gamma"] - gw) <= GAMMA_RTOL * gw
    assert S.state_delta(out["x"], xw) <= A.X_TOL and float(np.max(np.abs(out["P"] - Pw))) <= A.p_bar(Pw)
    meas, gw = meas_with_gamma(x, P, kind, a, b, 4 * chi, seed=6)
    assert gw >= 2 * chi
    hL.set_state(x, P)
    pose0 = hL.pose()
    out = run(hL, kind, meas, a, b, gate=1)
    print("gate/reject %s: gamma %.6g vs %.6g (table %.6g)" % (R.KIND_NAMES[kind], out["diag"]["gamma"], gw, chi))
    assert out["diag"]["applied"] == 0 and abs(out["diag"]["gamma"] - gw) <= GAMMA_RTOL * gw
    assert np.array_equal(out["x"], x) and np.array_equal(out["P"], P)
    assert np.array_equal(out["pose"][0], pose0[0]) and np.array_equal(out["pose"][1], pose0[1])
    check_rows("gate/reject rows", x, kind, meas, a, b, out)          # the rows were formed all the same
    assert run(hL, kind, meas, a, b, gate=0)["diag"]["applied"] == 1


# ---------------------------------------------------------------- 6. batch handles
def test_batch_per_instance_spans_strides_and_flags(hL, gpu_required):
    import torch
    from rvio_amd import hip
    cfg = A.long_config()
    n, kind = 10, Q_
    xw, Pw = A.window_state(n)
    states = [R.F.moved_window(n), (xw, Pw), (R.F.zero_qk(xw), Pw)]
    spans = [(0, 2), (1, 3), (2, 2)]
    meass = [R.meas_near(states[i][0], kind, spans[i][0], max(spans[i][1], spans[i][0] + 1), R.LEVERS[i % 2], sigma_p=0.02, sigma_q=0.005, seed=40 + i) for i in range(3)]
    single = []
    for i in range(2):
        hL.set_state(*states[i])
        single.append(run(hL, kind, meass[i], *spans[i]))
    hb = hip.RvioHip(cfg, batch=3, front_end=False)

    def load():
        hb.set_state(*states[0])                    # (the window length is handle-wide: set it, then the instances' own states)
        for i in range(3):
            hb.set_state_at(i, *states[i])
    load()
    recs = np.zeros(6, abi.FIX_DTYPE)               # a stride of two records: the odd ones hold NaN, which nobody may read
    recs["z"], recs["sigma"], recs["lever"] = np.nan, np.nan, np.nan
    for i in range(3):
        recs[2 * i] = np.frombuffer(bytes(meass[i]), abi.FIX_DTYPE)[0]
    d_meas = torch.from_numpy(recs.view(np.uint8)).cuda()
    d_new = torch.tensor([s[0] for s in spans], dtype=torch.int32).cuda()
    d_old = torch.tensor([s[1] for s in spans], dtype=torch.int32).cuda()
    d_act = torch.tensor([1, 0, 1], dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    pose2 = hb.get_pose_at(2)
    hb.update_rel_dev(kind, 0, d_meas.data_ptr(), 2, d_new.data_ptr(), d_old.data_ptr(), None)
    for i in range(3):
        xd, Pd = hb.get_state_at(i)
        pp, pq = hb.get_pose_at(i)
        dg = diag_of(hb, i)
        if i == 2:                                  # outside the window: neither launch wrote it, and the record says so
            assert (dg["m"], dg["applied"], dg["img_count"], dg["gamma"]) == (0, 0, -1, 0.0) and not dg["r"].any() and dg["kind"] == kind
            assert np.array_equal(xd, states[2][0]) and np.array_equal(Pd, states[2][1])
            assert np.array_equal(pp, pose2[0]) and np.array_equal(pq, pose2[1])
        else:
            s = single[i]
            assert dg["applied"] == 1 and dg["gamma"] == s["diag"]["gamma"] and np.array_equal(dg["r"], s["diag"]["r"]) and dg["img_count"] == -spans[i][0]
            assert np.array_equal(xd, s["x"]) and np.array_equal(Pd, s["P"])
            assert np.array_equal(pp, s["pose"][0]) and np.array_equal(pq, s["pose"][1])
            Hd, sd = hb.get_fix_rows(i)
            assert np.array_equal(Hd, s["rows"][0]) and np.array_equal(sd, s["rows"][1])
    # the caller's flags: instance 1 is left alone, instance 0 runs as before
    load()
    hb.update_rel_dev(kind, 0, d_meas.data_ptr(), 2, d_new.data_ptr(), d_old.data_ptr(), d_act.data_ptr())
    xd, Pd = hb.get_state_at(1)
    assert diag_of(hb, 1)["applied"] == 0 and np.array_equal(xd, states[1][0]) and np.array_equal(Pd, states[1][1])
    xd, Pd = hb.get_state_at(0)
    assert np.array_equal(xd, single[0]["x"]) and np.array_equal(Pd, single[0]["P"])
    xd, Pd = hb.get_state_at(2)
    assert np.array_equal(xd, states[2][0]) and np.array_equal(Pd, states[2][1]) and diag_of(hb, 2)["img_count"] == -1
    # the host form on ONE instance: the others stay as they are
    load()
    hb.update_rel(kind, meass[1], spans[1][0], spans[1][1], 0, instance=1)
    for i in range(3):
        xd, Pd = hb.get_state_at(i)
        if i == 1:
            assert diag_of(hb, 1)["applied"] == 1 and np.array_equal(xd, single[1]["x"]) and np.array_equal(Pd, single[1]["P"])
        else:
            assert diag_of(hb, i)["applied"] == 0 and np.array_equal(xd, states[i][0]) and np.array_equal(Pd, states[i][1])
    assert hb.frame_info()["device_error"] == 0
    hb.close()


def test_batch_of_128_with_a_shared_record_and_span(gpu_required):
    import torch
    from rvio_amd import hip
    cfg, B, kind, n, a, b = A.long_config(), 128, Q_, 10, 1, 5
    x, P = A.window_state(n)
    meas = R.meas_near(x, kind, a, b, R.LEVER, sigma_p=0.02, sigma_q=0.005, seed=9)
    h1 = hip.RvioHip(cfg)
    h1.set_state(x, P)
    one = run(h1, kind, meas, a, b)
    h1.close()
    hb = hip.RvioHip(cfg, batch=B, front_end=False)
    hb.set_state(x, P)
    d_meas = torch.from_numpy(np.frombuffer(bytes(meas), np.uint8).copy()).cuda()
    d_new = torch.full((B,), a, dtype=torch.int32).cuda()
    d_old = torch.full((B,), b, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    hb.update_rel_dev(kind, 0, d_meas.data_ptr(), 0, d_new.data_ptr(), d_old.data_ptr(), None)
    for i in (0, 1, 63, 64, 127):
        xd, Pd = hb.get_state_at(i)
        dg = diag_of(hb, i)
        assert dg["applied"] == 1 and dg["gamma"] == one["diag"]["gamma"] and np.array_equal(xd, one["x"]) and np.array_equal(Pd, one["P"])
        assert np.array_equal(hb.get_fix_rows(i)[0], one["rows"][0])
    hb.set_state(x, P)
    hb.update_rel(kind, meas, a, b, 0, instance=-1)      # host form, every instance
    for i in (0, 77, 127):
        xd, Pd = hb.get_state_at(i)
        assert np.array_equal(xd, one["x"]) and np.array_equal(Pd, one["P"])
    assert hb.frame_info()["device_error"] == 0
    hb.close()


# ---------------------------------------------------------------- 7. between frames, flat out
def frames_run(sync):
    """a first direct-track frame, then 8 with a one-step POSE measurement (the newest clone) behind each; sync: rvio_hip_sync in front of and
    behind every measurement"""
    from rvio_amd import hip
    cfg = K.config()
    seq = rv.synth.SynthSequence(cfg, duration=8.0, seed=0)
    h = hip.RvioHip(cfg)
    h.initialize(*seq.init_from_static(K0))
    drv = rv.synth.DirectTrackDriver(seq)
    for k in range(K0 + 1, K0 + 10):
        inp = drv.inputs(k)
        h.frame_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])
        if k > K0 + 1:                            # (the window holds its first clone behind the second frame)
            if sync:
                h.sync()
            j = k - K0
            h.update_rel(Q_, abi.make_fix((0.002 * j, -0.001 * j, 0.0005 * j), (0.0, 0.0, 0.0, 1.0), 0.05, 0.02, R.LEVER), 0, 1, 0)
            if sync:
                h.sync()
        drv.after(h.get_points()[0])      # (a getter of the tracker's points: it waits for the front end, not for the filter stream)
    x, P = h.get_state()
    pts, hl = h.get_points()
    dg = diag_of(h)
    err = h.frame_info()["device_error"]
    h.close()
    return dict(x=x, P=P, pts=pts, hl=hl, r=dg["r"], ga=np.array([dg["gamma"], dg["applied"], dg["img_count"], dg["kind"]]), err=np.array(err))


def test_frames_flat_out_equal_synchronised(gpu_required):
    a, b = frames_run(False), frames_run(True)
    print("flat out: last record r %s gamma/applied/img_count/kind %s" % (a["r"], a["ga"]))
    assert a["err"] == 0 and b["err"] == 0 and a["ga"][1] == 1 and a["ga"][2] == 9 and a["ga"][3] == Q_
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------- 8. the record, the refusals
def test_record_and_refusals(gpu_required):
    import torch
    from rvio_amd import hip
    cfg = S.small_image_config()
    h = hip.RvioHip(cfg)
    L = h.L
    INVALID, STATE = -1, -4
    vp, dbl = C.c_void_p, C.c_double

    def call(kind, meas, a=0, b=1, gate=0, inst=-1):
        return L.rvio_hip_update_rel(h.h, inst, kind, gate, a, b, C.byref(meas))
    def mk(**kw):
        f = abi.make_fix((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0), 0.5, 0.5, (0.1, 0.0, 0.0))
        for name, (i, v) in kw.items():
            getattr(f, name)[i] = v
        return f
    good = mk()
    d_meas = torch.from_numpy(np.frombuffer(bytes(good), np.uint8).copy()).cuda()
    d_new = torch.zeros(1, dtype=torch.int32).cuda()
    d_old = torch.ones(1, dtype=torch.int32).cuda()
    torch.cuda.synchronize()

    def call_dev(kind=P_, gate=0, measp=None, newp=None, oldp=None):
        return L.rvio_hip_update_rel_dev(h.h, kind, gate, vp(d_meas.data_ptr()) if measp is None else measp, C.c_size_t(0),
                                         vp(d_new.data_ptr()) if newp is None else newp, vp(d_old.data_ptr()) if oldp is None else oldp, None)
    assert call(P_, good) == STATE and call_dev() == STATE                      # no state yet
    seq = rv.synth.SynthSequence(cfg, duration=3.0, seed=0)
    h.initialize(*seq.init_from_static(38))
    for kind in R.KINDS:                                                         # the empty window right behind initialisation holds no pair of frames
        assert call(kind, good) == INVALID
    for k in (39, 40, 41):
        img, imu = seq.render(k), seq.imu_between(k)
        d_img, d_imu = torch.from_numpy(img).cuda(), torch.from_numpy(imu.view(np.uint8)).cuda()
        torch.cuda.synchronize()
        h.frame_begin_dev(d_img.data_ptr(), img.shape[1], d_imu.data_ptr(), len(imu), 0, 0)
        assert call(P_, good) == STATE and call_dev() == STATE                  # inside a frame
        do_update, do_augment = h.frame_plan()
        if do_update:
            h.update_tracked()
        h.augment_compose(do_augment)
        h.frame_end()
    n = h.frame_info()["n_clones"]
    assert n == 2
    # the record: the family's kind, the NEWER frame's count
    for kind in R.KINDS:
        for a, b in ((0, 1), (1, 2), (0, 2)):
            assert call(kind, good, a, b) == 0
            dg = diag_of(h)
            assert (dg["kind"], dg["m"], dg["applied"], dg["img_count"]) == (kind, abi.REL_ROWS[kind], 1, 3 - a)
            assert h.get_fix_rows()[0].shape == (abi.REL_ROWS[kind], 24 + 6 * n)
    assert call_dev() == 0 and diag_of(h)["applied"] == 1 and diag_of(h)["kind"] == P_
    # the ages
    assert call(P_, good, 1, 1) == INVALID and call(P_, good, 2, 1) == INVALID and call(P_, good, 0, 0) == INVALID      # age_new >= age_old
    assert call(P_, good, 0, 3) == INVALID and call(P_, good, 2, 3) == INVALID                                            # age_old > n
    assert call(P_, good, -1, 1) == INVALID
    # out of range
    for kind in (-1, 0, 1, 2, 3, 15, 19):
        assert call(kind, good) == INVALID and call_dev(kind=kind) == INVALID, kind
    assert call(P_, good, gate=2) == INVALID and call(P_, good, gate=-1) == INVALID and call(P_, good, inst=1) == INVALID and call(P_, good, inst=-2) == INVALID
    assert L.rvio_hip_update_rel(h.h, 0, P_, 0, 0, 1, None) == INVALID
    assert call_dev(measp=vp(None)) == INVALID and call_dev(newp=vp(None)) == INVALID and call_dev(oldp=vp(None)) == INVALID and call_dev(gate=2) == INVALID
    # the fix families keep refusing the new kinds
    d_age = torch.zeros(1, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    for kind in R.KINDS:
        assert L.rvio_hip_update_fix(h.h, -1, kind, 0, C.byref(good)) == INVALID
        assert L.rvio_hip_update_fix_dev(h.h, kind, 0, vp(d_meas.data_ptr()), C.c_size_t(0), None) == INVALID
        assert L.rvio_hip_update_fix_past(h.h, -1, kind, 0, 0, dbl(0.0), C.byref(good)) == INVALID
        assert L.rvio_hip_update_fix_past_dev(h.h, kind, 0, vp(d_meas.data_ptr()), C.c_size_t(0), vp(d_age.data_ptr()), None, None) == INVALID
    # the record's checks are those of rvio_hip_update_fix
    for bad, refused, taken in ((mk(z=(1, np.nan)), (P_, Q_), (A_,)), (mk(z=(4, np.inf)), (A_, Q_), (P_,)), (mk(sigma=(2, 0.0)), (P_, Q_), (A_,)),
                                (mk(sigma=(4, 0.0)), (A_, Q_), (P_,)), (mk(lever=(2, np.nan)), (P_, Q_), (A_,)), (mk(z=(6, 1.0 + 1e-5)), (A_, Q_), (P_,))):
        for kind in refused:
            assert call(kind, bad) == INVALID, kind
        for kind in taken:
            assert call(kind, bad) == 0, kind
    # a device span outside the window: the record says so, the state stays
    h.sync()
    x0, P0 = h.get_state()
    d_old.fill_(3)
    torch.cuda.synchronize()
    assert call_dev() == 0
    dg = diag_of(h)
    assert (dg["m"], dg["applied"], dg["img_count"]) == (0, 0, -1) and not dg["r"].any()
    x1, P1 = h.get_state()
    assert np.array_equal(x0, x1) and np.array_equal(P0, P1)
    h.sync()
    assert h.frame_info()["device_error"] == 0
    h.close()
