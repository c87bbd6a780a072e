"""GPU: map landmarks — pixel observations of known world points at a past image (rvio_hip_update_map*, csrc/map_rows.hip in front of
csrc/aux_update.hip).  The rows the device forms against abi.map_model (bar 1e-12 max(1, max|H|), the columns the header's table lists as 0
exactly 0.0, sigma bit for bit); pixel units against a twin handed the oracle's undistortion of the same float pixels; the per-point gamma and
gate on a stack with two gross outliers and a point behind the camera; the applied update against abi.aux_update_model; a twin handle handed
the device's own rows through rvio_hip_update_aux ends with the same bits; nothing outside the chain's clones enters; batch handles with
per-instance ages, counts, strides, flags and calibrations; frames flat out against synchronised; every refusal; the fix getters keep
reporting the fix family.  One handle of the longest window (max_track_len = 32: 31 clones, leading dimension 210) takes the states of every
window a handle can hold."""
import ctypes as C

import numpy as np
import pytest

import map_cases as M
import oracle as O
import scenarios as S
from test_gpu_aux_update import GAMMA_RTOL
from test_gpu_fix import place

abi, A, K, F = M.abi, M.A, M.K, M.F
rv = A.rv
pytestmark = pytest.mark.gpu
K0 = 38
NORM, PIX = abi.RVIO_MAP_NORMALISED, abi.RVIO_MAP_PIXELS
CALS = M.calibrations()


@pytest.fixture(scope="module")
def hL(gpu_required):
    from rvio_amd import hip
    h = hip.RvioHip(A.long_config())
    yield h
    assert h.frame_info()["device_error"] == 0
    h.close()


def rec_of(h, i=0):
    rec, pts = h.get_map(i)
    return dict(gamma=rec.gamma, applied=rec.applied, m=rec.m, n_used=rec.n_used, n_obs=rec.n_obs, img_count=rec.img_count,
                status=[p.status for p in pts], pgamma=np.array([p.gamma for p in pts]), pr=np.array([p.r[:] for p in pts]),
                depth=np.array([p.depth for p in pts]))


def run(h, pts, age, units=NORM, gate=0, gate_each=0):
    h.update_map(abi.make_map_obs(pts), age, units, gate, gate_each)
    xd, Pd = h.get_state()
    return dict(x=xd, P=Pd, rec=rec_of(h), pose=h.pose(), rows=h.get_map_rows())


def zero_cols(n, age):
    live = set(range(0, 6)) | {24 + 6 * i + c for i in range(n - age, n) for c in range(6)}
    return [c for c in range(24 + 6 * n) if c not in live]


def cfg_of(cal):
    """an rvio_config with the calibration's members (what tests/oracle.py undistort reads)"""
    cfg = abi.config_named("B", enable_equalizer=0, max_track_len=32)
    for name, _ in abi.rvio_calibration._fields_:
        if name != "T_bc":
            setattr(cfg, name, getattr(cal, name))
    for i in range(16):
        cfg.T_bc[i] = cal.T_bc[i]
    return cfg


# ---------------------------------------------------------------- 1. the rows
@pytest.mark.parametrize("n", M.GPU_WINDOWS)
def test_rows_against_the_model(hL, n):
    x0, P0 = M.state(n)
    worst = [0.0, 0.0]
    for cal in sorted(CALS):
        hL.set_calibration_at(0, CALS[cal])
        for nn, a, k, cname, seed in M.row_cases((n,), M.gpu_ages):
            if cname != cal:
                continue
            x, P = place(hL, x0, P0, n != 31)      # (padding where the window leaves some: behind a poisoned propagation)
            pts = M.observations(CALS[cal], x, a, [M.GOOD] * k, seed)
            out = run(hL, pts, a)
            H, r, sg, gamma, status = abi.map_model(CALS[cal], x, P, abi.make_map_obs(pts), a, NORM, 0)
            Hd, rd, sd = out["rows"]
            bar = 1e-12 * max(1.0, float(np.max(np.abs(H))))
            eh, er = float(np.max(np.abs(Hd - H))), float(np.max(np.abs(rd - r)))
            worst = [max(worst[0], eh), max(worst[1], er)]
            print("n=%d age=%d points=%d %s: max|H - model| %.3e  max|r - model| %.3e (bar %.1e, max|H| %.3g)" % (n, a, k, cal, eh, er, bar, np.max(np.abs(H))))
            assert Hd.shape == H.shape == (2 * k, 24 + 6 * n) and eh <= bar and er <= bar
            assert np.array_equal(sd, sg) and np.all(sd == M.SIGMA)
            zc = zero_cols(n, a)
            assert not Hd[:, zc].any() and not np.signbit(Hd[:, zc]).any(), "a column the table lists as 0"
            assert np.abs(Hd).sum() > 0.1
            rc = out["rec"]
            assert (rc["applied"], rc["m"], rc["n_used"], rc["n_obs"], rc["img_count"]) == (1, 2 * k, k, k, -a)
            assert rc["status"] == [0] * k + [3] * (8 - k)
            assert np.max(np.abs(rc["pgamma"][:k] - gamma)) <= GAMMA_RTOL * max(1e-3, float(np.max(gamma)))
    print("n=%d: worst max|H - model| %.3e, worst max|r - model| %.3e" % (n, worst[0], worst[1]))


# ---------------------------------------------------------------- 2. pixel units
@pytest.mark.parametrize("cal", sorted(CALS))
def test_pixels_equal_a_normalised_twin_handed_the_oracles_undistortion(hL, cal):
    from rvio_amd import hip
    k = CALS[cal]
    assert k.fx == k.fy
    twin = hip.RvioHip(A.long_config())
    twin.set_calibration_at(0, k)
    hL.set_calibration_at(0, k)
    for n in (3, 10):
        x, P = M.state(n)
        a = n // 2
        pix = M.pixel_observations(k, x, a, 8, seed=n)
        px32 = np.array([p[1] for p in pix], np.float32)
        un = O.undistort(cfg_of(k), px32).astype(float)
        hL.set_state(x, P)
        twin.set_state(x, P)
        o0 = run(hL, pix, a, units=PIX)
        o1 = run(twin, [(p[0], un[j], p[2] / abs(float(k.fx))) for j, p in enumerate(pix)], a, units=NORM)
        for key in (0, 1, 2):
            assert np.array_equal(o0["rows"][key], o1["rows"][key]), key
        assert np.array_equal(o0["x"], o1["x"]) and np.array_equal(o0["P"], o1["P"]) and o0["rec"]["gamma"] == o1["rec"]["gamma"]
        want = np.tile([pix[0][2] / abs(float(k.fx)), pix[0][2] / abs(float(k.fy))], 8)
        assert np.array_equal(o0["rows"][2], want) and o0["rec"]["applied"] == 1 and o0["rec"]["n_used"] == 8
        H, r, sg, gamma, status = abi.map_model(k, x, P, abi.make_map_obs(pix), a, PIX, 0, uv_n=un)
        assert np.max(np.abs(o0["rows"][1] - r)) <= 1e-12 and np.max(np.abs(o0["x"] - x)) > 1e-10
        print("%s n=%d: pixel rows equal the twin's bit for bit; max|r| %.3e" % (cal, n, np.max(np.abs(r))))
    assert twin.frame_info()["device_error"] == 0
    twin.close()


# ---------------------------------------------------------------- 3. the per-point gamma and gate
def test_per_point_gate_on_a_stack_with_outliers(hL):
    cal, x, P, age, pts = M.gate_case()
    hL.set_calibration_at(0, cal)
    hL.set_state(x, P)
    out = run(hL, pts, age, gate_each=1)
    H, r, sg, gamma, status = abi.map_model(cal, x, P, abi.make_map_obs(pts), age, NORM, 1)
    g_all = abi.map_model(cal, x, P, abi.make_map_obs(pts), age, NORM, 0)[3]
    rc = out["rec"]
    print("statuses %s  gamma_j device %s model %s" % (rc["status"], np.array2string(rc["pgamma"], precision=6), np.array2string(g_all, precision=6)))
    assert tuple(rc["status"]) == M.GATE_STATUS == tuple(status) and rc["n_used"] == 5 and rc["n_obs"] == 8 and rc["applied"] == 1 and rc["m"] == 16
    for j in range(8):
        if M.GATE_STATUS[j] != 2:
            assert abs(rc["pgamma"][j] - g_all[j]) <= GAMMA_RTOL * g_all[j], j
            assert g_all[j] > 100 if M.GATE_STATUS[j] == 1 else g_all[j] < 5
        else:
            assert rc["depth"][j] <= -0.5 and rc["pgamma"][j] == 0.0
    Hd, rd, sd = out["rows"]
    for j in range(8):
        rows = slice(2 * j, 2 * j + 2)
        if M.GATE_STATUS[j]:
            assert not Hd[rows].any() and not np.signbit(Hd[rows]).any() and not rd[rows].any() and np.all(sd[rows] == 1.0)
        else:
            assert np.abs(Hd[rows]).sum() > 0.1 and np.all(sd[rows] == M.SIGMA)
    good = [p for p, s in zip(pts, M.GATE_STATUS) if s == 0]
    H5, r5, s5, _, st5 = abi.map_model(cal, x, P, abi.make_map_obs(good), age, NORM, 0)
    assert not st5.any()
    xw, Pw, gw = abi.aux_update_model(x, P, H5, r5, s5)
    dxw, dpw = S.state_delta(out["x"], xw), float(np.max(np.abs(out["P"] - Pw)))
    print("against the 5 good points alone: state %.3e (bar %.0e)  P %.3e (bar %.3e)  gamma %.6g vs %.6g" % (dxw, A.X_TOL, dpw, A.p_bar(Pw), rc["gamma"], gw))
    assert dxw <= A.X_TOL and dpw <= A.p_bar(Pw) and abs(rc["gamma"] - gw) <= GAMMA_RTOL * gw
    # the same call from the same state: the same bits
    hL.set_state(x, P)
    again = run(hL, pts, age, gate_each=1)
    assert np.array_equal(again["x"], out["x"]) and np.array_equal(again["P"], out["P"]) and np.array_equal(again["rec"]["pgamma"], rc["pgamma"])
    assert all(np.array_equal(p, q) for p, q in zip(again["rows"], out["rows"])) and again["rec"]["gamma"] == rc["gamma"]
    # what the per-point gate buys: the stack gate alone refuses everything
    hL.set_state(x, P)
    pose0 = hL.pose()                     # (the pose line is whatever the last update left: a refused call must not rewrite it)
    whole = run(hL, pts, age, gate=1, gate_each=0)
    rw = whole["rec"]
    print("stack gate alone: gamma %.6g against chi2(16) %.6g" % (rw["gamma"], A.chi2_95(16)))
    assert rw["applied"] == 0 and rw["n_used"] == 7 and rw["status"] == [0, 0, 0, 0, 2, 0, 0, 0] and rw["gamma"] > A.chi2_95(16)
    assert np.array_equal(whole["x"], x) and np.array_equal(whole["P"], P)
    assert np.array_equal(whole["pose"][0], pose0[0]) and np.array_equal(whole["pose"][1], pose0[1])
    assert np.array_equal(whole["rec"]["pgamma"], rc["pgamma"])           # gamma_j is computed and reported all the same


# ---------------------------------------------------------------- 4. the applied update
@pytest.mark.parametrize("n", M.GPU_WINDOWS)
def test_applied_update_against_the_model(hL, n):
    x0, P0 = M.state(n)
    cal = CALS["radtan"]
    hL.set_calibration_at(0, cal)
    worst = [0.0, 0.0]
    for a in M.ages(n):
        for k in (2, 8):
            x, P = place(hL, x0, P0, n != 31)
            pts = M.observations(cal, x, a, [M.GOOD] * k, seed=7 + n + a + k)
            out = run(hL, pts, a, gate_each=1)
            H, r, sg, gamma, status = abi.map_model(cal, x, P, abi.make_map_obs(pts), a, NORM, 1)
            xw, Pw, gw = abi.aux_update_model(x, P, H, r, sg)
            xd, Pd, rc = out["x"], out["P"], out["rec"]
            dxw, dpw = S.state_delta(xd, xw), float(np.max(np.abs(Pd - Pw)))
            worst = [max(worst[0], dxw), max(worst[1], dpw / float(np.max(np.abs(Pw))))]
            print("n=%d age=%d points=%d: state %.3e (bar %.0e)  P %.3e (bar %.3e)  gamma %.6g vs %.6g" % (n, a, k, dxw, A.X_TOL, dpw, A.p_bar(Pw), rc["gamma"], gw))
            assert rc["applied"] == 1 and rc["n_used"] == k and np.all(np.isfinite(Pd))
            assert dxw <= A.X_TOL and dpw <= A.p_bar(Pw)
            assert np.array_equal(Pd, Pd.T)
            assert abs(rc["gamma"] - gw) <= GAMMA_RTOL * abs(gw)
            wp, wq = abi.pose_line(xd)
            assert np.max(np.abs(out["pose"][0] - wp)) <= 1e-12 and np.max(np.abs(out["pose"][1] - wq)) <= 1e-12
            assert np.max(np.abs(xd - x)) > 1e-10
            r1 = abi.map_model(cal, xd, Pd, abi.make_map_obs(pts), a, NORM, 0)[1]
            assert np.linalg.norm(r1) < np.linalg.norm(r)
    print("n=%d: worst state distance %.3e, worst |P - model| / max|P| %.3e" % (n, worst[0], worst[1]))


# ---------------------------------------------------------------- 5. the bits of a twin
@pytest.mark.parametrize("k", [2, 8], ids=["m4", "m16"])
def test_a_twin_handed_the_devices_rows_ends_with_the_same_bits(hL, k):
    from rvio_amd import hip
    twin = hip.RvioHip(A.long_config())
    cal = CALS["fisheye"]
    hL.set_calibration_at(0, cal)
    for n in (3, 10):
        x, P = M.state(n)
        a = n // 2
        pts = M.observations(cal, x, a, [M.GOOD] * k, seed=n + k)
        hL.set_state(x, P)
        out = run(hL, pts, a, gate_each=1)
        Hd, rd, sd = out["rows"]
        assert Hd.shape[0] == 2 * k
        twin.set_state(x, P)
        twin.update_aux(Hd, rd, sd, abi.RVIO_AUX_RESIDUAL, 0)
        xt, Pt = twin.get_state()
        pt = twin.pose()
        gt, at = twin.aux_diag()
        assert at == 1 and out["rec"]["applied"] == 1 and gt == out["rec"]["gamma"]
        assert np.array_equal(xt, out["x"]) and np.array_equal(Pt, out["P"])
        assert np.array_equal(pt[0], out["pose"][0]) and np.array_equal(pt[1], out["pose"][1])
        assert np.max(np.abs(xt - x)) > 1e-10
    assert twin.frame_info()["device_error"] == 0
    twin.close()


# ---------------------------------------------------------------- 6. nothing else enters
def test_states_that_differ_elsewhere_give_the_same_rows(hL):
    from rvio_amd import hip
    twin = hip.RvioHip(A.long_config())
    cal = CALS["radtan"]
    hL.set_calibration_at(0, cal)
    twin.set_calibration_at(0, cal)
    for n in (3, 10, 31):
        x, P = M.state(n)
        for a in M.ages(n):
            pts = M.observations(cal, x, a, [M.GOOD] * 3, seed=n + a)
            y = M.replaced_outside(x, a, seed=n + a)
            assert np.max(np.abs(y[7:26] - x[7:26])) > 1e-3 and np.array_equal(y[0:7], x[0:7])
            hL.set_state(x, P)
            twin.set_state(y, P)
            o0, o1 = run(hL, pts, a), run(twin, pts, a)
            for key in (0, 1, 2):
                assert np.array_equal(o0["rows"][key], o1["rows"][key]), (n, a, key)
            assert np.array_equal(o0["rec"]["pgamma"], o1["rec"]["pgamma"]) and o0["rows"][1].any()
    assert twin.frame_info()["device_error"] == 0
    twin.close()


# ---------------------------------------------------------------- 7. batch handles
def test_batch_per_instance_ages_counts_strides_flags_and_calibrations(hL, gpu_required):
    import torch
    from rvio_amd import hip
    cfg, n = A.long_config(), 10
    xw, Pw = M.state(n)
    states = [F.moved_window(n), (xw, Pw), (F.zero_qk(xw), Pw)]
    cals = [CALS["radtan"], CALS["fisheye"], CALS["radtan"]]
    hb = hip.RvioHip(cfg, batch=3, front_end=False)
    hb.set_calibrations(cals)

    def load(sts=states):
        hb.set_state(*sts[0])
        for i in range(3):
            hb.set_state_at(i, *sts[i])

    def dev_obs(per_instance):
        recs = np.zeros((len(per_instance), 8), abi.MAP_OBS_DTYPE)
        recs["p_w"], recs["uv"], recs["sigma"] = np.nan, np.nan, np.nan          # what nobody may read
        for i, pts in enumerate(per_instance):
            for j, (p_w, uv, s) in enumerate(pts):
                recs[i, j] = (tuple(p_w), tuple(uv), s)
        return torch.from_numpy(recs.reshape(-1).view(np.uint8)).cuda()

    def i32(v):
        return torch.tensor(v, dtype=torch.int32).cuda()

    # (a) per-instance ages, one outside the window; per-instance counts, one below n_max; a stride of 8 records
    ages, counts = [2, 11, 5], [8, 8, 7]
    obs = [M.observations(cals[i], states[i][0], min(ages[i], n), [M.GOOD] * counts[i], seed=60 + i) for i in range(3)]
    d_obs, d_age, d_cnt = dev_obs(obs), i32(ages), i32(counts)
    torch.cuda.synchronize()
    load()
    pose1 = hb.get_pose_at(1)
    hb.update_map_dev(NORM, 0, 1, 8, d_obs.data_ptr(), 8, d_cnt.data_ptr(), d_age.data_ptr(), None)
    hL.set_calibration_at(0, cals[0])
    hL.set_state(*states[0])
    single0 = run(hL, obs[0], ages[0], gate_each=1)
    for i in range(3):
        xd, Pd = hb.get_state_at(i)
        rc = rec_of(hb, i)
        if i == 1:                                  # outside the window: neither launch wrote it, and the record says so
            assert (rc["m"], rc["applied"], rc["n_used"], rc["img_count"], rc["gamma"]) == (0, 0, 0, -1, 0.0) and rc["status"] == [3] * 8
            assert np.array_equal(xd, states[1][0]) and np.array_equal(Pd, states[1][1])
            pp, pq = hb.get_pose_at(1)
            assert np.array_equal(pp, pose1[0]) and np.array_equal(pq, pose1[1])
        elif i == 0:                                # the plain handle's bits
            assert rc["applied"] == 1 and rc["gamma"] == single0["rec"]["gamma"] and rc["img_count"] == -ages[0] and rc["n_used"] == 8
            assert np.array_equal(xd, single0["x"]) and np.array_equal(Pd, single0["P"])
            assert all(np.array_equal(p, q) for p, q in zip(hb.get_map_rows(0), single0["rows"]))
        else:                                       # seven points in a stack of eight slots: the last slot is empty, its NaN record unread
            H, r, sg, gamma, status = abi.map_model(cals[2], states[2][0], states[2][1], abi.make_map_obs(obs[2]), ages[2], NORM, 1)
            xm, Pm, gm = abi.aux_update_model(states[2][0], states[2][1], H, r, sg)
            Hd, rd, sd = hb.get_map_rows(2)
            assert (rc["applied"], rc["m"], rc["n_used"], rc["n_obs"], rc["img_count"]) == (1, 16, 7, 7, -ages[2]) and rc["status"] == [0] * 7 + [3]
            assert Hd.shape[0] == 16 and not Hd[14:].any() and not rd[14:].any() and np.all(sd[14:] == 1.0) and np.all(np.isfinite(Hd))
            assert np.max(np.abs(Hd[:14] - H)) <= 1e-12 * max(1.0, float(np.max(np.abs(H))))
            assert S.state_delta(xd, xm) <= A.X_TOL and float(np.max(np.abs(Pd - Pm))) <= A.p_bar(Pm)
    # (b) one inactive instance, one whose points are all behind the camera
    obs_b = [obs[0], M.observations(cals[1], states[1][0], 3, [M.BEHIND] * 8, seed=70), obs[2]]
    d_obs_b, d_age_b, d_act = dev_obs(obs_b), i32([2, 3, 5]), i32([1, 1, 0])
    torch.cuda.synchronize()
    load()
    hb.update_map_dev(NORM, 0, 1, 8, d_obs_b.data_ptr(), 8, d_cnt.data_ptr(), d_age_b.data_ptr(), d_act.data_ptr())
    xd, Pd = hb.get_state_at(0)
    assert np.array_equal(xd, single0["x"]) and np.array_equal(Pd, single0["P"])
    xd, Pd = hb.get_state_at(1)
    rc = rec_of(hb, 1)
    assert (rc["m"], rc["applied"], rc["n_used"], rc["n_obs"], rc["img_count"]) == (0, 0, 0, 8, -3) and rc["status"] == [2] * 8 and np.all(rc["depth"] <= -0.5)
    assert np.array_equal(xd, states[1][0]) and np.array_equal(Pd, states[1][1])
    xd, Pd = hb.get_state_at(2)
    assert np.array_equal(xd, states[2][0]) and np.array_equal(Pd, states[2][1]) and rec_of(hb, 2)["applied"] == 0
    # (c) shared records (a stride of 0), no counts: instances 0 and 2 hold the same state and calibration and end with the plain handle's bits
    same = [states[0], states[1], states[0]]
    d_one, d_age_c = dev_obs([obs[0]]), i32([2, 2, 2])
    torch.cuda.synchronize()
    load(same)
    hb.update_map_dev(NORM, 0, 1, 8, d_one.data_ptr(), 0, None, d_age_c.data_ptr(), None)
    for i in (0, 2):
        xd, Pd = hb.get_state_at(i)
        assert np.array_equal(xd, single0["x"]) and np.array_equal(Pd, single0["P"]) and rec_of(hb, i)["gamma"] == single0["rec"]["gamma"]
    # the host form on ONE instance: the others stay as they are
    load()
    hb.update_map(abi.make_map_obs(obs[0]), ages[0], NORM, 0, 1, instance=0)
    for i in range(3):
        xd, Pd = hb.get_state_at(i)
        if i == 0:
            assert rec_of(hb, 0)["applied"] == 1 and np.array_equal(xd, single0["x"]) and np.array_equal(Pd, single0["P"])
        else:
            assert rec_of(hb, i)["applied"] == 0 and np.array_equal(xd, states[i][0]) and np.array_equal(Pd, states[i][1])
    assert hb.frame_info()["device_error"] == 0
    hb.close()


# ---------------------------------------------------------------- 8. between frames, flat out
def frames_run(sync, script=None):
    """a first direct-track frame, then 8 with a map call of four points seen one image back behind each; sync: rvio_hip_sync in front of and
    behind every call.  script: the observations of every call (None: formed here from the state, which needs the synchronised run)"""
    from rvio_amd import hip
    cfg = K.config()
    seq = rv.synth.SynthSequence(cfg, duration=8.0, seed=0)
    h = hip.RvioHip(cfg)
    h.initialize(*seq.init_from_static(K0))
    drv = rv.synth.DirectTrackDriver(seq)
    made = []
    for k in range(K0 + 1, K0 + 10):
        inp = drv.inputs(k)
        h.frame_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])
        if k > K0 + 1:                            # (the window holds its first clone behind the second frame)
            if sync:
                h.sync()
            pts = script[len(made)] if script is not None else M.observations(cfg, h.get_state()[0], 1, [M.GOOD] * 4, seed=k)
            made.append(pts)
            h.update_map(abi.make_map_obs(pts), 1, NORM, 0, 1)
            if sync:
                h.sync()
        drv.after(h.get_points()[0])      # (a getter of the tracker's points: it waits for the front end, not for the filter stream)
    x, P = h.get_state()
    pts, hl = h.get_points()
    rc = rec_of(h)
    err = h.frame_info()["device_error"]
    h.close()
    return dict(x=x, P=P, pts=pts, hl=hl, ga=np.array([rc["gamma"], rc["applied"], rc["n_used"], rc["img_count"]]), pg=rc["pgamma"], err=np.array(err)), made


def test_frames_flat_out_equal_synchronised(gpu_required):
    b, script = frames_run(True)
    a, _ = frames_run(False, script)
    print("flat out: last record gamma/applied/n_used/img_count %s" % (a["ga"],))
    assert a["err"] == 0 and b["err"] == 0 and a["ga"][1] == 1 and a["ga"][2] == 4 and a["ga"][3] == 8
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------- 9. every refusal, 10. the other getters
def test_refusals_and_the_fix_getters(gpu_required):
    import torch
    from rvio_amd import hip
    cfg = S.small_image_config()
    h = hip.RvioHip(cfg)
    L = h.L
    INVALID, STATE = -1, -4
    vp = C.c_void_p

    def mk(**kw):
        o = abi.make_map_obs([((0.5, 0.2, 4.0), (0.01, -0.02), 0.01), ((-0.5, 0.1, 5.0), (0.0, 0.03), 0.01)])
        for name, (j, i, v) in kw.items():
            if name == "sigma":
                o[j].sigma = v
            else:
                getattr(o[j], name)[i] = v
        return o

    def call(obs, units=NORM, gate=0, gate_each=1, age=0, n_obs=2, inst=-1):
        return L.rvio_hip_update_map(h.h, inst, units, gate, gate_each, age, n_obs, obs)
    good = mk()
    d_obs = torch.from_numpy(np.frombuffer(bytes(good), np.uint8).copy()).cuda()
    d_age = torch.zeros(1, dtype=torch.int32).cuda()
    torch.cuda.synchronize()

    def call_dev(units=NORM, gate=0, gate_each=1, n_max=2, obsp=None, stride=0, agep=None):
        return L.rvio_hip_update_map_dev(h.h, units, gate, gate_each, n_max, vp(d_obs.data_ptr()) if obsp is None else obsp, C.c_size_t(stride), None,
                                         vp(d_age.data_ptr()) if agep is None else agep, None)

    def err():
        return h.last_error() if hasattr(h, "last_error") else L.rvio_hip_last_error(h.h).decode()
    assert call(good) == STATE and "rvio_hip_update_map before the first" in err()
    assert call_dev() == STATE                                                   # no state yet
    rec = abi.rvio_map_diag()
    m, d = C.c_int32(0), C.c_int32(0)
    assert L.rvio_hip_get_map(h.h, 0, C.byref(rec), None) == STATE and "rvio_hip_get_map before" in err()
    assert L.rvio_hip_get_map_rows(h.h, 0, C.byref(m), C.byref(d), None, None, None) == STATE
    seq = rv.synth.SynthSequence(cfg, duration=3.0, seed=0)
    h.initialize(*seq.init_from_static(38))
    for k in (39, 40, 41):
        img, imu = seq.render(k), seq.imu_between(k)
        d_img, d_imu = torch.from_numpy(img).cuda(), torch.from_numpy(imu.view(np.uint8)).cuda()
        torch.cuda.synchronize()
        h.frame_begin_dev(d_img.data_ptr(), img.shape[1], d_imu.data_ptr(), len(imu), 0, 0)
        assert call(good) == STATE and "between rvio_hip_frame_begin_dev" in err() and call_dev() == STATE      # inside a frame
        do_update, do_augment = h.frame_plan()
        if do_update:
            h.update_tracked()
        h.augment_compose(do_augment)
        h.frame_end()
    n = h.frame_info()["n_clones"]
    assert n == 2
    # a fix first: its getters must keep reporting it
    fix = abi.make_fix(abi.fix_h(cfg, h.get_state()[0], abi.RVIO_FIX_POSITION)[0:3] + 0.01, None, 0.05, 0.0)
    h.update_fix(abi.RVIO_FIX_POSITION, fix)
    fix_rec, fix_rows = bytes(h.get_fix()), h.get_fix_rows()
    # the record of a good call at every age of the window
    x = h.get_state()[0]
    for a in (0, 1, 2):
        pts = M.observations(cfg, x, a, [M.GOOD] * 2, seed=a)
        assert call(abi.make_map_obs(pts), age=a) == 0
        rc = rec_of(h)
        assert (rc["applied"], rc["m"], rc["n_used"], rc["n_obs"], rc["img_count"]) == (1, 4, 2, 2, 3 - a) and rc["status"] == [0, 0] + [3] * 6
        Hd, rd, sd = h.get_map_rows()
        assert Hd.shape == (4, 24 + 6 * n)
        x = h.get_state()[0]
    assert call_dev() == 0
    assert bytes(h.get_fix()) == fix_rec and all(np.array_equal(p, q) for p, q in zip(h.get_fix_rows(), fix_rows))      # 10. the fix block is another
    # the ages
    assert call(good, age=-1) == INVALID and "age" in err()
    assert call(good, age=3) == INVALID and "age" in err()
    # out of range
    for nb in (0, -1, 9):
        assert call(good, n_obs=nb) == INVALID and call_dev(n_max=nb) == INVALID, nb
    for bad in (-1, 2):
        assert call(good, units=bad) == INVALID and call(good, gate=bad) == INVALID and call(good, gate_each=bad) == INVALID
        assert call_dev(units=bad) == INVALID and call_dev(gate=bad) == INVALID and call_dev(gate_each=bad) == INVALID
    assert call(good, inst=1) == INVALID and call(good, inst=-2) == INVALID
    assert call(None) == INVALID and call_dev(obsp=vp(None)) == INVALID and call_dev(agep=vp(None)) == INVALID
    assert call_dev(stride=1) == INVALID and call_dev(stride=2) == 0 and call_dev(n_max=1, stride=1) == 0
    assert L.rvio_hip_get_map(h.h, 1, C.byref(rec), None) == INVALID and L.rvio_hip_get_map(h.h, 0, None, None) == INVALID
    assert L.rvio_hip_get_map_rows(h.h, 0, None, C.byref(d), None, None, None) == INVALID
    # the host form checks the records
    for bad, word in ((mk(p_w=(1, 2, np.nan)), "finite"), (mk(uv=(0, 1, np.inf)), "finite"), (mk(sigma=(1, 0, np.nan)), "finite"),
                      (mk(sigma=(0, 0, 0.0)), "sigma"), (mk(sigma=(1, 0, -0.01)), "sigma")):
        assert call(bad) == INVALID and word in err(), word
    assert call(mk(p_w=(1, 2, np.nan)), n_obs=1) == 0          # (the second record is not part of a call of one)
    # a device age outside the window: the record says so, the state stays
    h.sync()
    x0, P0 = h.get_state()
    d_age.fill_(3)
    torch.cuda.synchronize()
    assert call_dev() == 0
    rc = rec_of(h)
    assert (rc["m"], rc["applied"], rc["n_used"], rc["img_count"]) == (0, 0, 0, -1) and rc["status"] == [3] * 8
    x1, P1 = h.get_state()
    assert np.array_equal(x0, x1) and np.array_equal(P0, P1)
    h.sync()
    assert h.frame_info()["device_error"] == 0
    h.close()
