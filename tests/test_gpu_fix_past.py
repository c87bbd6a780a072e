"""GPU: past-frame fixes (rvio_hip_update_fix_past*, csrc/fix_past.hip in front of csrc/aux_update.hip).  The rows the device forms against
abi.fix_past_model (bar 1e-12 max(1, max|H|), the columns the header's table lists as 0 exactly 0.0); the applied update against
abi.aux_update_model on the model's rows at the bars of tests/test_gpu_aux_update.py; a twin handle handed the device's own rows through
rvio_hip_update_aux ends with the same bits; age 0 against rvio_hip_update_fix behind whole frames; the gate; batch handles with per-instance
ages, strides and flags, an age outside the window among them; frames flat out against synchronised; the long window; every error and
rvio_hip_frame_age.  One handle of the longest window (max_track_len = 32, leading dimension 210) takes the states of every window."""
import ctypes as C

import numpy as np
import pytest

import fix_past_cases as FP
import scenarios as S
from test_gpu_aux_update import GAMMA_RTOL, feed, feed_staged
from test_gpu_fix import diag_of, place

abi, A, K, F = FP.abi, FP.A, FP.K, FP.F
rv = A.rv
pytestmark = pytest.mark.gpu
WINDOWS = (1, 3, 10, 31)
K0 = 38
P_, A_, Q_ = abi.RVIO_FIX_POSITION, abi.RVIO_FIX_ATTITUDE, abi.RVIO_FIX_POSE


@pytest.fixture(scope="module")
def hL(gpu_required):
    from rvio_amd import hip
    h = hip.RvioHip(A.long_config())
    yield h
    assert h.frame_info()["device_error"] == 0
    h.close()


def run(h, kind, fix, age, frac=0.0, gate=0):
    h.update_fix_past(kind, fix, age, frac, gate)
    xd, Pd = h.get_state()
    return dict(x=xd, P=Pd, diag=diag_of(h), pose=h.pose(), rows=h.get_fix_rows())


def check_rows(tag, x, kind, fix, age, frac, out):
    H, r, sigma = abi.fix_past_model(x, kind, fix, age, frac)
    Hd, sd = out["rows"]
    dg = out["diag"]
    m, n = abi.FIX_ROWS[kind], (len(x) - 26) // 7
    bar = 1e-12 * max(1.0, float(np.max(np.abs(H))))
    eh, er = float(np.max(np.abs(Hd - H))), float(np.max(np.abs(dg["r"][:m] - r)))
    print("%s: max|H - model| %.3e  max|r - model| %.3e (bar %.1e, max|H| %.3g)" % (tag, eh, er, bar, np.max(np.abs(H))))
    assert Hd.shape == H.shape and eh <= bar and er <= bar
    assert np.array_equal(sd, sigma) and not dg["r"][m:].any() and (dg["kind"], dg["m"]) == (kind, m)
    for b, zero in enumerate(FP.zero_cols(n, kind, age, frac)):
        blk = Hd[3 * b: 3 * b + 3][:, zero]
        assert not blk.any() and not np.signbit(blk).any(), "a column the table lists as 0"
        assert np.abs(Hd[3 * b: 3 * b + 3]).sum() > 1.0
    return eh, er


# ---------------------------------------------------------------- 1. the rows
@pytest.mark.parametrize("n", WINDOWS)
def test_rows_against_the_model(hL, n):
    x0, P0 = A.window_state(n)
    worst = [0.0, 0.0]
    for kind, age, frac in FP.combos(n):
        for li, lever in enumerate(FP.LEVERS):
            x, P = place(hL, x0, P0, n != 31)      # (padding where the window leaves some: behind a poisoned propagation)
            fix = FP.fix_near(x, kind, age, frac, lever, sigma_p=(0.02, 0.03, 0.04), sigma_q=(0.005, 0.006, 0.007), seed=n + age + li)
            out = run(hL, kind, fix, age, frac)
            eh, er = check_rows("%s n=%d age=%d frac=%.2f lever=%d" % (FP.KIND_NAMES[kind], n, age, frac, 1 - li), x, kind, fix, age, frac, out)
            worst = [max(worst[0], eh), max(worst[1], er)]
            assert out["diag"]["applied"] == 1 and out["rows"][0].shape[1] == 24 + 6 * n and out["diag"]["img_count"] == -age
    print("n=%d: worst max|H - model| %.3e, worst max|r - model| %.3e" % (n, worst[0], worst[1]))


# ---------------------------------------------------------------- 2. the applied update
@pytest.mark.parametrize("n", WINDOWS)
def test_applied_update_against_the_model(hL, n):
    x0, P0 = A.window_state(n)
    for kind, age, frac in FP.combos(n):
        x, P = place(hL, x0, P0, n != 31)
        fix = FP.fix_near(x, kind, age, frac, FP.LEVER, sigma_p=0.02, sigma_q=0.005, seed=3 + n + age)
        out = run(hL, kind, fix, age, frac)
        H, r, sigma = abi.fix_past_model(x, kind, fix, age, frac)
        xw, Pw, gw = abi.aux_update_model(x, P, H, r, sigma)
        xd, Pd, dg = out["x"], out["P"], out["diag"]
        dxw, dpw = S.state_delta(xd, xw), float(np.max(np.abs(Pd - Pw)))
        print("%s n=%d age=%d frac=%.2f: state %.3e (bar %.0e)  P %.3e (bar %.3e)  gamma %.6g vs %.6g" % (FP.KIND_NAMES[kind], n, age, frac, dxw, A.X_TOL, dpw, A.p_bar(Pw), dg["gamma"], gw))
        assert dg["applied"] == 1 and np.all(np.isfinite(Pd))
        assert dxw <= A.X_TOL and dpw <= A.p_bar(Pw)
        assert np.array_equal(Pd, Pd.T)
        assert abs(dg["gamma"] - gw) <= GAMMA_RTOL * abs(gw)
        wp, wq = abi.pose_line(xd)
        assert np.max(np.abs(out["pose"][0] - wp)) <= 1e-12 and np.max(np.abs(out["pose"][1] - wq)) <= 1e-12
        assert np.max(np.abs(xd - x)) > 1e-10
        # the state's PAST pose moved onto the fix
        assert np.linalg.norm(abi.fix_past_model(xd, kind, fix, age, frac)[1]) < np.linalg.norm(r)


# ---------------------------------------------------------------- 3. the bits of a twin
@pytest.mark.parametrize("kind", [P_, Q_], ids=["m3", "m6"])
def test_a_twin_handed_the_devices_rows_ends_with_the_same_bits(hL, kind):
    from rvio_amd import hip
    twin = hip.RvioHip(A.long_config())
    for n in (3, 10):
        x, P = A.window_state(n)
        age = n // 2
        fix = FP.fix_near(x, kind, age, 0.0, FP.LEVER, sigma_p=0.02, sigma_q=0.005, seed=n)
        hL.set_state(x, P)
        out = run(hL, kind, fix, age)
        m = abi.FIX_ROWS[kind]
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


# ---------------------------------------------------------------- 4. age 0 against today's fix
def test_age_zero_behind_whole_frames_is_todays_fix(gpu_required):
    """behind a composition (qk, pk) = identity and rows / columns 9 - 14 of P are exactly zero: today's rows differ from the age-0 rows in those
    columns only, so the two are the same update in exact arithmetic"""
    from rvio_amd import hip
    cfg = K.config()
    seq = rv.synth.SynthSequence(cfg, duration=8.0, seed=0)
    hs = [hip.RvioHip(cfg), hip.RvioHip(cfg)]
    for h in hs:
        h.initialize(*seq.init_from_static(K0))
        drv = rv.synth.DirectTrackDriver(seq)
        for k in range(K0 + 1, K0 + 7):
            inp = drv.inputs(k)
            h.frame_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])
            drv.after(h.get_points()[0])
    x, P = hs[0].get_state()
    assert np.array_equal(x, hs[1].get_state()[0]) and (len(x) - 26) // 7 == 5
    assert not P[9:15, :].any() and not P[:, 9:15].any()
    for kind in FP.KINDS:
        fix = FP.fix_near(x, kind, 0, 0.0, FP.LEVER, dp=0.02, dth=0.004, sigma_p=0.02, sigma_q=0.005, seed=kind)
        for h in hs:
            h.set_state(x, P)
        hs[0].update_fix_past(kind, fix, 0, 0.0, 0)
        hs[1].update_fix(kind, fix, 0)
        (xa, Pa), (xb, Pb) = hs[0].get_state(), hs[1].get_state()
        da, db = diag_of(hs[0]), diag_of(hs[1])
        dx, dp = S.state_delta(xa, xb), float(np.max(np.abs(Pa - Pb)))
        print("%s: past(age 0) against update_fix: state %.3e (bar %.0e)  P %.3e (bar %.3e)" % (FP.KIND_NAMES[kind], dx, A.X_TOL, dp, A.p_bar(Pb)))
        assert da["applied"] == 1 and db["applied"] == 1 and np.max(np.abs(da["r"] - db["r"])) <= 1e-12
        assert dx <= A.X_TOL and dp <= A.p_bar(Pb) and abs(da["gamma"] - db["gamma"]) <= GAMMA_RTOL * db["gamma"]
        assert np.max(np.abs(xa - x)) > 1e-10
    for h in hs:
        assert h.frame_info()["device_error"] == 0
        h.close()


# ---------------------------------------------------------------- 5. the gate
def fix_with_gamma(x, P, kind, age, target, seed):
    s = 1.0
    for _ in range(8):
        fix = FP.fix_near(x, kind, age, 0.0, FP.LEVER, dp=0.01 * s, dth=0.002 * s, sigma_p=0.02, sigma_q=0.005, seed=seed)
        g = abi.aux_update_model(x, P, *abi.fix_past_model(x, kind, fix, age))[2]
        s *= np.sqrt(target / g)
    return fix, g


@pytest.mark.parametrize("kind", FP.KINDS, ids=[FP.KIND_NAMES[k] for k in FP.KINDS])
def test_gate_accepts_and_rejects(hL, kind):
    n, age = 10, 5
    x, P = A.window_state(n)
    chi = A.chi2_95(abi.FIX_ROWS[kind])
    fix, gw = fix_with_gamma(x, P, kind, age, chi / 4, seed=5)
    assert gw <= chi / 2
    hL.set_state(x, P)
    out = run(hL, kind, fix, age, gate=1)
    xw, Pw, _ = abi.aux_update_model(x, P, *abi.fix_past_model(x, kind, fix, age))
    print("gate/accept %s: gamma %.6g vs %.6g (table %.6g)" % (FP.KIND_NAMES[kind], out["diag"]["gamma"], gw, chi))
    assert out["diag"]["applied"] == 1 and abs(out["diag"]["gamma"] - gw) <= GAMMA_RTOL * gw
    assert S.state_delta(out["x"], xw) <= A.X_TOL and float(np.max(np.abs(out["P"] - Pw))) <= A.p_bar(Pw)
    fix, gw = fix_with_gamma(x, P, kind, age, 4 * chi, seed=6)
    assert gw >= 2 * chi
    hL.set_state(x, P)
    pose0 = hL.pose()
    out = run(hL, kind, fix, age, gate=1)
    print("gate/reject %s: gamma %.6g vs %.6g (table %.6g)" % (FP.KIND_NAMES[kind], out["diag"]["gamma"], gw, chi))
    assert out["diag"]["applied"] == 0 and abs(out["diag"]["gamma"] - gw) <= GAMMA_RTOL * gw
    assert np.array_equal(out["x"], x) and np.array_equal(out["P"], P)
    assert np.array_equal(out["pose"][0], pose0[0]) and np.array_equal(out["pose"][1], pose0[1])
    check_rows("gate/reject rows", x, kind, fix, age, 0.0, out)          # the rows were formed all the same
    assert run(hL, kind, fix, age, gate=0)["diag"]["applied"] == 1


# ---------------------------------------------------------------- 6. batch handles
def test_batch_per_instance_ages_strides_and_flags(hL, gpu_required):
    import torch
    from rvio_amd import hip
    cfg = A.long_config()
    n, kind = 10, Q_
    xw, Pw = A.window_state(n)
    states = [F.moved_window(n), (xw, Pw), (F.zero_qk(xw), Pw)]
    ages = [0, 2, n + 1]
    fixes = [FP.fix_near(states[i][0], kind, min(ages[i], n), 0.0, FP.LEVERS[i % 2], sigma_p=0.02, sigma_q=0.005, seed=40 + i) for i in range(3)]
    single = []
    for i in range(2):
        hL.set_state(*states[i])
        single.append(run(hL, kind, fixes[i], ages[i]))
    hb = hip.RvioHip(cfg, batch=3, front_end=False)

    def load():
        hb.set_state(*states[0])                    # (the window length is handle-wide: set it, then the instances' own states)
        for i in range(3):
            hb.set_state_at(i, *states[i])
    load()
    recs = np.zeros(6, abi.FIX_DTYPE)               # a stride of two records: the odd ones hold NaN, which nobody may read
    recs["z"], recs["sigma"], recs["lever"] = np.nan, np.nan, np.nan
    for i in range(3):
        recs[2 * i] = np.frombuffer(bytes(fixes[i]), abi.FIX_DTYPE)[0]
    d_fix = torch.from_numpy(recs.view(np.uint8)).cuda()
    d_age = torch.tensor(ages, dtype=torch.int32).cuda()
    d_frac = torch.zeros(3, dtype=torch.float64).cuda()
    d_act = torch.tensor([1, 0, 1], dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    pose2 = hb.get_pose_at(2)
    hb.update_fix_past_dev(kind, 0, d_fix.data_ptr(), 2, d_age.data_ptr(), None, None)
    for i in range(3):
        xd, Pd = hb.get_state_at(i)
        pp, pq = hb.get_pose_at(i)
        dg = diag_of(hb, i)
        if i == 2:                                  # outside the window: neither launch wrote it, and the record says so
            assert (dg["m"], dg["applied"], dg["img_count"], dg["gamma"]) == (0, 0, -1, 0.0) and not dg["r"].any()
            assert np.array_equal(xd, states[2][0]) and np.array_equal(Pd, states[2][1])
            assert np.array_equal(pp, pose2[0]) and np.array_equal(pq, pose2[1])
        else:
            s = single[i]
            assert dg["applied"] == 1 and dg["gamma"] == s["diag"]["gamma"] and np.array_equal(dg["r"], s["diag"]["r"]) and dg["img_count"] == -ages[i]
            assert np.array_equal(xd, s["x"]) and np.array_equal(Pd, s["P"])
            assert np.array_equal(pp, s["pose"][0]) and np.array_equal(pq, s["pose"][1])
            Hd, sd = hb.get_fix_rows(i)
            assert np.array_equal(Hd, s["rows"][0]) and np.array_equal(sd, s["rows"][1])
    # the caller's flags (with d_frac given): instance 1 is left alone, instance 0 runs as before
    load()
    hb.update_fix_past_dev(kind, 0, d_fix.data_ptr(), 2, d_age.data_ptr(), d_frac.data_ptr(), d_act.data_ptr())
    xd, Pd = hb.get_state_at(1)
    assert diag_of(hb, 1)["applied"] == 0 and np.array_equal(xd, states[1][0]) and np.array_equal(Pd, states[1][1])
    xd, Pd = hb.get_state_at(0)
    assert np.array_equal(xd, single[0]["x"]) and np.array_equal(Pd, single[0]["P"])
    xd, Pd = hb.get_state_at(2)
    assert np.array_equal(xd, states[2][0]) and np.array_equal(Pd, states[2][1]) and diag_of(hb, 2)["img_count"] == -1
    # the host form on ONE instance: the others stay as they are
    load()
    hb.update_fix_past(kind, fixes[1], ages[1], 0.0, 0, instance=1)
    for i in range(3):
        xd, Pd = hb.get_state_at(i)
        if i == 1:
            assert diag_of(hb, 1)["applied"] == 1 and np.array_equal(xd, single[1]["x"]) and np.array_equal(Pd, single[1]["P"])
        else:
            assert diag_of(hb, i)["applied"] == 0 and np.array_equal(xd, states[i][0]) and np.array_equal(Pd, states[i][1])
    assert hb.frame_info()["device_error"] == 0
    hb.close()


def test_batch_of_128_with_a_shared_fix_and_age(gpu_required):
    import torch
    from rvio_amd import hip
    cfg, B, kind, n, age = A.long_config(), 128, P_, 10, 4
    x, P = A.window_state(n)
    fix = FP.fix_near(x, kind, age, FP.FRAC, FP.LEVER, sigma_p=0.02, seed=9)
    h1 = hip.RvioHip(cfg)
    h1.set_state(x, P)
    one = run(h1, kind, fix, age, FP.FRAC)
    h1.close()
    hb = hip.RvioHip(cfg, batch=B, front_end=False)
    hb.set_state(x, P)
    d_fix = torch.from_numpy(np.frombuffer(bytes(fix), np.uint8).copy()).cuda()
    d_age = torch.full((B,), age, dtype=torch.int32).cuda()
    d_frac = torch.full((B,), FP.FRAC, dtype=torch.float64).cuda()
    torch.cuda.synchronize()
    hb.update_fix_past_dev(kind, 0, d_fix.data_ptr(), 0, d_age.data_ptr(), d_frac.data_ptr(), None)
    for i in (0, 1, 63, 64, 127):
        xd, Pd = hb.get_state_at(i)
        dg = diag_of(hb, i)
        assert dg["applied"] == 1 and dg["gamma"] == one["diag"]["gamma"] and np.array_equal(xd, one["x"]) and np.array_equal(Pd, one["P"])
        assert np.array_equal(hb.get_fix_rows(i)[0], one["rows"][0])
    hb.set_state(x, P)
    hb.update_fix_past(kind, fix, age, FP.FRAC, 0, instance=-1)      # host form, every instance
    for i in (0, 77, 127):
        xd, Pd = hb.get_state_at(i)
        assert np.array_equal(xd, one["x"]) and np.array_equal(Pd, one["P"])
    assert hb.frame_info()["device_error"] == 0
    hb.close()


# ---------------------------------------------------------------- 7. between frames, flat out
def frames_run(sync):
    """8 direct-track frames with a POSITION fix of the PREVIOUS frame behind each; sync: rvio_hip_sync in front of and behind every fix"""
    from rvio_amd import hip
    cfg = K.config()
    seq = rv.synth.SynthSequence(cfg, duration=8.0, seed=0)
    h = hip.RvioHip(cfg)
    h.initialize(*seq.init_from_static(K0))
    drv = rv.synth.DirectTrackDriver(seq)
    for k in range(K0 + 1, K0 + 9):
        inp = drv.inputs(k)
        h.frame_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])
        if sync:
            h.sync()
        age = h.frame_age(k - K0 - 1) if k > K0 + 1 else 0
        assert age == (1 if k > K0 + 1 else 0)
        h.update_fix_past(P_, abi.make_fix((0.002 * (k - K0), -0.001 * (k - K0), 0.0), None, 0.05, 0.0, FP.LEVER), age, 0.5 if k > K0 + 2 else 0.0, 0)      # (frac > 0 needs age + 1 <= n: from the third frame on)
        if sync:
            h.sync()
        drv.after(h.get_points()[0])      # (a getter of the tracker's points: it waits for the front end, not for the filter stream)
    x, P = h.get_state()
    pts, hl = h.get_points()
    dg = diag_of(h)
    err = h.frame_info()["device_error"]
    h.close()
    return dict(x=x, P=P, pts=pts, hl=hl, r=dg["r"], ga=np.array([dg["gamma"], dg["applied"], dg["img_count"]]), err=np.array(err))


def test_frames_flat_out_equal_synchronised(gpu_required):
    a, b = frames_run(False), frames_run(True)
    print("flat out: last record r %s gamma/applied/img_count %s" % (a["r"], a["ga"]))
    assert a["err"] == 0 and b["err"] == 0 and a["ga"][1] == 1 and a["ga"][2] == 7
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------- 8. the long window
def pipeline(cfg, recs, seq, mode):
    """whole frames with a POSITION fix two frames old behind every second one.  'flat': nothing between the calls; 'staged': the stage entry
    points, and the state round-trips through the host behind every fix — which drops whatever factor of the clone block the handle kept"""
    from rvio_amd import hip
    h = hip.RvioHip(cfg)
    h.initialize(*seq.init_from_static(38))
    for k, r in enumerate(recs):
        (feed_staged if mode == "staged" else feed)(h, r)
        if k % 2 == 1 and k >= 3:
            h.update_fix_past(P_, abi.make_fix((0.001 * k, 0.0, -0.001 * k), None, 0.05, 0.0, FP.LEVER), 2, 0.0, 0)
            if mode == "staged":
                h.set_state(*h.get_state())
    x, P = h.get_state()
    info = h.frame_info()
    pose = h.pose()
    h.close()
    assert info["device_error"] == 0
    return x, P, pose


def test_long_window_does_not_use_a_stale_clone_block_factor(gpu_required):
    """6n = 102 > 96: the factor of the clone block for the NEXT visual update starts on the side queue behind augment / compose — the covariance
    the fix then changes (a past fix changes the clone block directly).  The whole-frame run must equal the staged run that cannot have kept one."""
    cfg = abi.config_named("B", enable_equalizer=0, max_track_len=18)
    seq, recs = S.record_sequence(cfg, n_frames=24, duration=6.0)
    assert (len(recs[-1]["x0"]) - 26) // 7 == 17 and sum(1 for r in recs if (len(r["x0"]) - 26) // 7 == 17) >= 5
    a, c = pipeline(cfg, recs, seq, "flat"), pipeline(cfg, recs, seq, "staged")
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    assert np.array_equal(a[2][0], c[2][0]) and np.array_equal(a[2][1], c[2][1])
    from rvio_amd import hip
    h = hip.RvioHip(cfg)
    h.initialize(*seq.init_from_static(38))
    for r in recs:
        feed(h, r)
    x0 = h.get_state()[0]
    h.close()
    assert np.max(np.abs(x0 - a[0])) > 1e-6          # the fixes did something


# ---------------------------------------------------------------- 9. errors, rvio_hip_frame_age
def test_argument_and_state_errors_and_frame_age(gpu_required):
    import torch
    from rvio_amd import hip
    cfg = S.small_image_config()
    h = hip.RvioHip(cfg)
    L = h.L
    INVALID, STATE = -1, -4
    vp, dbl = C.c_void_p, C.c_double

    def call(kind, fix, age=0, frac=0.0, gate=0, inst=-1):
        return L.rvio_hip_update_fix_past(h.h, inst, kind, gate, age, dbl(frac), C.byref(fix))
    def mk(**kw):
        f = abi.make_fix((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0), 0.5, 0.5, (0.1, 0.0, 0.0))
        for name, (i, v) in kw.items():
            getattr(f, name)[i] = v
        return f
    good = mk()
    age = C.c_int(-7)
    d_fix = torch.from_numpy(np.frombuffer(bytes(good), np.uint8).copy()).cuda()
    d_age = torch.zeros(1, dtype=torch.int32).cuda()
    torch.cuda.synchronize()

    def call_dev(kind=0, gate=0, fixp=None, agep=None):
        return L.rvio_hip_update_fix_past_dev(h.h, kind, gate, vp(d_fix.data_ptr()) if fixp is None else fixp, C.c_size_t(0), vp(d_age.data_ptr()) if agep is None else agep, None, None)
    assert call(0, good) == STATE and call_dev() == STATE                       # no state yet
    assert L.rvio_hip_frame_age(h.h, 0, C.byref(age)) == INVALID
    seq = rv.synth.SynthSequence(cfg, duration=3.0, seed=0)
    h.initialize(*seq.init_from_static(38))
    for kind in FP.KINDS:                                                        # the empty window right behind initialisation: age 0 only
        assert call(kind, good) == 0 and diag_of(h)["applied"] == 1 and diag_of(h)["kind"] == kind and diag_of(h)["img_count"] == 0
        assert call(kind, good, age=1) == INVALID
    assert call(P_, good, frac=0.25) == INVALID                                  # age + 1 > n
    assert L.rvio_hip_frame_age(h.h, 0, C.byref(age)) == 0 and age.value == 0
    assert L.rvio_hip_frame_age(h.h, 1, C.byref(age)) == INVALID and L.rvio_hip_frame_age(h.h, -1, C.byref(age)) == INVALID
    assert L.rvio_hip_frame_age(h.h, 0, None) == INVALID
    # out of range
    assert call(-1, good) == INVALID and call(abi.RVIO_FIX_GRAVITY, good) == INVALID and call(4, good) == INVALID
    assert call(0, good, gate=2) == INVALID and call(0, good, gate=-1) == INVALID and call(0, good, inst=1) == INVALID and call(0, good, inst=-2) == INVALID
    assert call(0, good, age=-1) == INVALID
    for frac in (-0.1, 1.0, 1.5, np.nan, np.inf):
        assert call(P_, good, frac=frac) == INVALID, frac
    assert L.rvio_hip_update_fix_past(h.h, 0, 0, 0, 0, dbl(0.0), None) == INVALID
    assert call_dev(fixp=vp(None)) == INVALID and call_dev(agep=vp(None)) == INVALID
    assert call_dev(kind=abi.RVIO_FIX_GRAVITY) == INVALID and call_dev(kind=-1) == INVALID and call_dev(gate=2) == INVALID
    assert call_dev() == 0 and diag_of(h)["applied"] == 1
    # the record's checks are those of rvio_hip_update_fix
    for bad, refused, taken in ((mk(z=(1, np.nan)), (P_, Q_), (A_,)), (mk(z=(4, np.inf)), (A_, Q_), (P_,)), (mk(sigma=(2, 0.0)), (P_, Q_), (A_,)),
                                (mk(sigma=(4, 0.0)), (A_, Q_), (P_,)), (mk(lever=(2, np.nan)), (P_, Q_), (A_,)), (mk(z=(6, 1.0 + 1e-5)), (A_, Q_), (P_,))):
        for kind in refused:
            assert call(kind, bad) == INVALID, kind
        for kind in taken:
            assert call(kind, bad) == 0, kind
    # frames through the stage entry points: the count runs ahead of the composed frame between frame_plan and augment_compose
    seen = []
    for k in (39, 40, 41):
        img, imu = seq.render(k), seq.imu_between(k)
        d_img, d_imu = torch.from_numpy(img).cuda(), torch.from_numpy(imu.view(np.uint8)).cuda()
        torch.cuda.synchronize()
        h.frame_begin_dev(d_img.data_ptr(), img.shape[1], d_imu.data_ptr(), len(imu), 0, 0)
        rc_open, rc_open_dev = call(0, good), call_dev()
        do_update, do_augment = h.frame_plan()
        c = k - 38                                                              # this frame's count
        rc_new = L.rvio_hip_frame_age(h.h, c, C.byref(age))                     # counted, not composed yet
        rc_prev = L.rvio_hip_frame_age(h.h, c - 1, C.byref(age))
        seen.append((rc_open, rc_open_dev, rc_new, rc_prev, age.value))
        if do_update:
            h.update_tracked()
        h.augment_compose(do_augment)
        h.frame_end()
        assert L.rvio_hip_frame_age(h.h, c, C.byref(age)) == 0 and age.value == 0
    assert seen == [(STATE, STATE, INVALID, 0, 0)] * 3, seen
    n = h.frame_info()["n_clones"]
    assert n == 2
    for c, want in ((3, 0), (2, 1), (1, 2)):
        assert L.rvio_hip_frame_age(h.h, c, C.byref(age)) == 0 and age.value == want
    assert L.rvio_hip_frame_age(h.h, 0, C.byref(age)) == INVALID and L.rvio_hip_frame_age(h.h, 4, C.byref(age)) == INVALID      # left the window / not yet there
    assert call(Q_, good, age=2) == 0 and diag_of(h)["img_count"] == 1
    assert call(P_, good, age=1, frac=0.5) == 0 and call(P_, good, age=2, frac=0.5) == INVALID and call(Q_, good, age=3) == INVALID
    assert call(A_, good, age=1, frac=0.5) == INVALID and call(Q_, good, age=1, frac=0.5) == INVALID
    assert h.get_fix_rows()[0].shape == (3, 24 + 6 * n)
    h.sync()
    assert h.frame_info()["device_error"] == 0
    h.close()
