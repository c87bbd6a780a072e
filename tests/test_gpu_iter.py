"""GPU: the iterated measurement updates (rvio_hip_set_meas_iterations: the fix, past-fix, rel and map calls relinearised max_iters times on the
device — the rows kernels and aux_iter_kernel of csrc/aux_update.hip in a fixed sequence, no read-back).  max_iters = 1 against a twin that
never touched the setter, bit for bit; a fixed number of passes and the early exit against abi.iter_update_model at the bars of
test_gpu_map.py's applied update; a batch of four with four fates in one call; the map statuses pass 0 decided; an indefinite covariance; frames
flat out against synchronised; every refusal.  One handle of the longest window (31 clones, leading dimension 210) takes every state: n = 0
(d = 24, one row group), 10 (d = 84, two groups, four column splits), 31 (d = 210, four groups, two splits); m = 3 (MB 4), 6 and 16 (MB 16)."""
import ctypes as C

import numpy as np
import pytest

import iter_cases as I
import map_cases as M
import scenarios as S

abi, A, K = M.abi, M.A, M.K
rv = A.rv
pytestmark = pytest.mark.gpu
NORM = abi.RVIO_MAP_NORMALISED
FAR = {c.family: c for c in I.cases() if c.name.endswith("far-n10")}
NEAR = {c.family: c for c in I.cases() if c.name.endswith("near-n10")}
MODEL_CASES = [FAR[f] for f in I.FAMILIES] + [I.build("map", I.FAR, 0), I.build("map", I.FAR, 31)]


@pytest.fixture(scope="module")
def hL(gpu_required):
    from rvio_amd import hip
    h = hip.RvioHip(A.long_config())
    h.set_calibration_at(0, I.CAL)
    yield h
    assert h.frame_info()["device_error"] == 0
    h.close()


def rows_of(h, c):
    return h.get_map_rows() if c.family == "map" else h.get_fix_rows()


def run(h, c, gate=0):
    h.set_state(c.x0, c.P0)
    c.call(h, -1, gate)
    xd, Pd = h.get_state()
    it = h.get_meas_iter()
    return dict(x=xd, P=Pd, pose=h.pose(), rec=bytes(c.rec(h)), rows=rows_of(h, c), it=it,
                iters=(it.iterations, it.converged), step=it.step, gamma0=it.gamma0, applied=c.rec(h).applied)


def check_against(tag, out, want, c):
    xw, Pw, info = want
    Pw = np.asarray(Pw, float)
    dxw, dpw = S.state_delta(out["x"], xw), float(np.max(np.abs(out["P"] - Pw)))
    wp, wq = abi.pose_line(out["x"])
    dpose = max(float(np.max(np.abs(out["pose"][0] - wp))), float(np.max(np.abs(out["pose"][1] - wq))))
    print("%s: state %.3e (bar %.0e)  P %.3e (bar %.3e)  pose line %.3e  passes %d (model %d)  last step %.3e (model %.3e)  gamma0 %.6g (model %.6g)"
          % (tag, dxw, A.X_TOL, dpw, A.p_bar(Pw), dpose, out["it"].iterations, info["iterations"], out["step"], info["steps"][-1], out["gamma0"], info["gamma0"]))
    assert out["applied"] == 1 and np.all(np.isfinite(out["P"]))
    assert dxw <= A.X_TOL and dpw <= A.p_bar(Pw)
    assert np.array_equal(out["P"], out["P"].T)
    assert dpose <= 1e-12
    assert out["it"].iterations == info["iterations"] and out["it"].converged == int(info["converged"])
    assert abs(out["gamma0"] - info["gamma0"]) <= 1e-7 * info["gamma0"]
    assert abs(out["step"] - info["steps"][-1]) <= 1e-9
    assert np.max(np.abs(out["x"] - c.x0)) > 1e-10


# ---------------------------------------------------------------- 1. max_iters = 1 is the plain update
@pytest.mark.parametrize("family", I.FAMILIES)
def test_one_iteration_equals_a_handle_that_never_set_it(hL, family):
    from rvio_amd import hip
    c = FAR[family]
    twin = hip.RvioHip(A.long_config())
    twin.set_calibration_at(0, I.CAL)
    hL.set_meas_iterations(1, 0.0)
    assert hL.get_meas_iterations() == (1, 0.0) and twin.get_meas_iterations() == (1, 0.0)
    a, b = run(hL, c), run(twin, c)
    assert twin.frame_info()["device_error"] == 0
    twin.close()
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["P"], b["P"]) and a["rec"] == b["rec"]
    assert np.array_equal(a["pose"][0], b["pose"][0]) and np.array_equal(a["pose"][1], b["pose"][1])
    assert all(np.array_equal(p, q) for p, q in zip(a["rows"], b["rows"]))
    assert a["iters"] == b["iters"] == (1, 0) and a["gamma0"] == b["gamma0"] == c.rec(hL).gamma and a["applied"] == 1
    xw, Pw, gw = c.one_shot()
    assert S.state_delta(a["x"], xw) <= A.X_TOL and float(np.max(np.abs(a["P"] - Pw))) <= A.p_bar(Pw)


# ---------------------------------------------------------------- 2. a fixed number of passes against the model
@pytest.mark.parametrize("iters", [2, 5])
@pytest.mark.parametrize("c", MODEL_CASES, ids=[c.name for c in MODEL_CASES])
def test_fixed_passes_against_the_model(hL, c, iters):
    hL.set_meas_iterations(iters, 0.0)
    out = run(hL, c)
    check_against("%s K=%d" % (c.name, iters), out, c.model(iters, 0.0), c)
    # what the passes buy: the measurement's whitened residuals at the posterior against the one-shot posterior's
    print("   whitened residual sum: one shot %.4g, %d passes %.4g" % (c.whitened_ss(c.one_shot()[0]), iters, c.whitened_ss(out["x"])))


# ---------------------------------------------------------------- 3. the early exit
@pytest.mark.parametrize("c", [NEAR["map"], FAR["map"], NEAR["fix"], FAR["past"], FAR["rel"]], ids=lambda c: c.name)
def test_early_exit_takes_the_passes_the_model_takes(hL, c):
    hL.set_meas_iterations(8, 1e-6)
    want = c.model(8, 1e-6)
    assert 1 < want[2]["iterations"] < 8 and want[2]["converged"]
    out = run(hL, c)
    check_against("%s tol=1e-6" % c.name, out, want, c)
    assert out["it"].converged == 1 and out["step"] < 1e-6


# ---------------------------------------------------------------- 4. a batch of four, one call, four fates
def test_batch_of_four_with_four_fates(hL, gpu_required):
    import torch
    from rvio_amd import hip
    near, far = NEAR["map"], FAR["map"]
    xt, Pt = M.state(I.N)
    outl = M.observations(I.CAL, xt, near.age, [M.OUTLIER] * 8, seed=9)
    states = [(near.x0, near.P0), (far.x0, far.P0), (far.x0, far.P0), (xt, Pt)]
    recs = np.zeros((4, 8), abi.MAP_OBS_DTYPE)
    for i, pts in enumerate([near.pts, far.pts, far.pts, outl]):
        for j, (p_w, uv, s) in enumerate(pts):
            recs[i, j] = (tuple(p_w), tuple(uv), s)
    d_obs = torch.from_numpy(recs.reshape(-1).view(np.uint8)).cuda()
    d_age = torch.tensor([near.age] * 4, dtype=torch.int32).cuda()
    d_act = torch.tensor([1, 1, 0, 1], dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    hb = hip.RvioHip(A.long_config(), batch=4, front_end=False)
    hb.set_calibrations([I.CAL] * 4)
    hb.set_state(*states[0])
    for i in range(4):
        hb.set_state_at(i, *states[i])
    hb.set_meas_iterations(8, 1e-6)
    hb.update_map_dev(NORM, 1, 0, 8, d_obs.data_ptr(), 8, None, d_age.data_ptr(), d_act.data_ptr())
    got = [(hb.get_state_at(i), hb.get_meas_iter(i), hb.get_map(i)[0]) for i in range(4)]
    assert hb.frame_info()["device_error"] == 0
    hb.close()
    wn, wf = near.model(8, 1e-6)[2], far.model(8, 1e-6)[2]
    print("passes: near %d far %d inactive %d gated %d (model: %d, %d); gated gamma %.4g against chi2(16) %.4g"
          % (got[0][1].iterations, got[1][1].iterations, got[2][1].iterations, got[3][1].iterations, wn["iterations"], wf["iterations"], got[3][2].gamma, A.chi2_95(16)))
    assert wn["iterations"] != wf["iterations"]
    assert (got[0][1].iterations, got[0][1].converged) == (wn["iterations"], 1) and (got[1][1].iterations, got[1][1].converged) == (wf["iterations"], 1)
    assert (got[2][1].iterations, got[2][1].converged, got[2][2].applied) == (0, 0, 0)
    assert (got[3][1].iterations, got[3][1].converged, got[3][2].applied) == (1, 0, 0) and got[3][2].gamma > A.chi2_95(16) and got[3][1].gamma0 == got[3][2].gamma
    for i in (2, 3):        # nothing of them was written
        assert np.array_equal(got[i][0][0], states[i][0]) and np.array_equal(got[i][0][1], states[i][1]), i
    # the near instance was finished passes before the call was: it is what the same case gives alone
    hL.set_meas_iterations(8, 1e-6)
    alone = run(hL, near, gate=1)
    assert np.array_equal(got[0][0][0], alone["x"]) and np.array_equal(got[0][0][1], alone["P"]) and got[0][1].step == alone["step"]
    xf, Pf, _ = far.model(8, 1e-6)
    assert S.state_delta(got[1][0][0], xf) <= A.X_TOL and float(np.max(np.abs(got[1][0][1] - Pf))) <= A.p_bar(Pf)


# ---------------------------------------------------------------- 5. the map statuses pass 0 decided are held
def test_map_statuses_and_gammas_of_pass_0_are_held(hL):
    cal, x, P, age, pts = M.gate_case()
    obs = abi.make_map_obs(pts)

    def call(iters):
        hL.set_meas_iterations(iters, 0.0)
        hL.set_state(x, P)
        hL.update_map(obs, age, NORM, 0, 1)
        rec, p = hL.get_map()
        return rec, [q.status for q in p], np.array([q.gamma for q in p]), hL.get_meas_iter(), hL.get_state()
    rec1, st1, g1, it1, s1 = call(1)
    rec4, st4, g4, it4, s4 = call(4)
    print("statuses %s  n_used %d  passes %d  last step %.3e" % (st4, rec4.n_used, it4.iterations, it4.step))
    assert tuple(st4) == M.GATE_STATUS == tuple(st1) and rec4.n_used == 5 and rec4.applied == 1 and it4.iterations == 4
    assert np.array_equal(g4, g1) and rec4.gamma == rec1.gamma
    good = [p for p, s in zip(pts, M.GATE_STATUS) if s == 0]
    og = abi.make_map_obs(good)
    held = {}

    def lin(xx, i):
        H, r, sg, g, st = abi.map_model(cal, xx, P, og, age, NORM, 0, hold=None if i == 0 else held["h"])
        held["h"] = (g, st) if i == 0 else (held["h"][0], st)
        return H, r, sg
    xw, Pw, info = abi.iter_update_model(x, P, lin, 4, 0.0)
    assert S.state_delta(s4[0], xw) <= A.X_TOL and float(np.max(np.abs(s4[1] - Pw))) <= A.p_bar(Pw)


# ---------------------------------------------------------------- 6. an indefinite covariance
def test_indefinite_covariance_sets_bit_8_and_leaves_the_state(gpu_required):
    from rvio_amd import hip
    c = FAR["fix"]           # (a map call would refuse every point at its own 2 x 2 first, and never reach the stack update)
    h = hip.RvioHip(A.long_config())
    h.set_meas_iterations(3, 0.0)
    Pbad = c.P0.copy()
    Pbad[3, 3] = Pbad[4, 4] = Pbad[5, 5] = -1e3
    assert np.min(np.linalg.eigvalsh(A.whitened_S(Pbad, *c.lin(c.x0, 0)[0::2]))) < -1.0
    h.set_state(c.x0, Pbad)
    pose0 = h.pose()
    c.call(h)
    xd, Pd = h.get_state()
    it, rec, err, pose1 = h.get_meas_iter(), c.rec(h), h.frame_info()["device_error"], h.pose()
    h.close()
    assert err & 8 and rec.applied == 0 and (it.iterations, it.converged) == (1, 0)
    assert np.array_equal(xd, c.x0) and np.array_equal(Pd, Pbad)
    assert np.array_equal(pose0[0], pose1[0]) and np.array_equal(pose0[1], pose1[1])


# ---------------------------------------------------------------- 7. between frames, flat out
def frames_run(sync, script=None):
    """a first direct-track frame, then three with an iterated map call of four points seen one image back behind each; sync: rvio_hip_sync in
    front of and behind every call.  script: the observations of every call (None: formed here from the state: the synchronised run)"""
    from rvio_amd import hip
    cfg = K.config()
    seq = rv.synth.SynthSequence(cfg, duration=8.0, seed=0)
    h = hip.RvioHip(cfg)
    h.set_meas_iterations(3, 0.0)
    h.initialize(*seq.init_from_static(38))
    drv = rv.synth.DirectTrackDriver(seq)
    made = []
    for k in range(39, 43):
        inp = drv.inputs(k)
        h.frame_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])
        if k > 39:
            if sync:
                h.sync()
            pts = script[len(made)] if script is not None else M.observations(cfg, h.get_state()[0], 1, [M.GOOD] * 4, seed=k)
            made.append(pts)
            h.update_map(abi.make_map_obs(pts), 1, NORM, 0, 0)
            if sync:
                h.sync()
        drv.after(h.get_points()[0])
    x, P = h.get_state()
    it, rec = h.get_meas_iter(), h.get_map()[0]
    err = h.frame_info()["device_error"]
    h.close()
    return dict(x=x, P=P, it=np.array([it.iterations, it.converged, it.step, it.gamma0]), ga=np.array([rec.gamma, rec.applied, rec.n_used]), err=np.array(err)), made


def test_frames_flat_out_equal_synchronised(gpu_required):
    b, script = frames_run(True)
    a, _ = frames_run(False, script)
    print("flat out: passes/converged/step/gamma0 %s" % (a["it"],))
    assert a["err"] == 0 and b["err"] == 0 and a["it"][0] == 3 and a["ga"][1] == 1 and a["ga"][2] == 4
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------- 8. every refusal
def test_refusals(gpu_required):
    from rvio_amd import hip
    h = hip.RvioHip(S.small_image_config())
    L = h.L
    INVALID, STATE = -1, -4

    def err():
        return L.rvio_hip_last_error(h.h).decode()

    def setit(k, t):
        return L.rvio_hip_set_meas_iterations(h.h, int(k), C.c_double(t))
    for k in (0, 9, -1):
        assert setit(k, 0.0) == INVALID and "max_iters" in err(), k
    for t in (-1e-9, float("nan"), float("inf")):
        assert setit(4, t) == INVALID and "tol" in err(), t
    assert h.get_meas_iterations() == (1, 0.0)                       # a refused call changes nothing
    assert setit(8, 0.0) == 0 and setit(1, 1e-3) == 0 and h.get_meas_iterations() == (1, 1e-3)
    rec = abi.rvio_meas_iter()
    assert L.rvio_hip_get_meas_iter(h.h, 0, C.byref(rec)) == STATE and "before the first" in err()
    assert L.rvio_hip_get_meas_iter(h.h, 1, C.byref(rec)) == INVALID and L.rvio_hip_get_meas_iter(h.h, 0, None) == INVALID
    assert L.rvio_hip_set_meas_iterations(None, 2, C.c_double(0.0)) == INVALID
    assert h.frame_info()["device_error"] == 0
    h.close()
