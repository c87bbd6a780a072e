"""GPU: the auxiliary measurement update (rvio_hip_update_aux*, csrc/aux_update.hip) against abi.aux_update_model at every window and row
count, and against the CPU oracle on the sub-class the oracle covers (clone-only H: tests/aux_update_cases.py).  Bars: the project's own —
states 1e-9 per component, covariance 1e-9 max|P| + 1e-15, gamma rtol 1e-7 (the feature gate's).  Every case prints what it measured.
One handle of the longest window (max_track_len = 32, leading dimension 210) takes the states of EVERY window: all but n = 31 leave rows and
columns of padding behind d, which the kernel must not read (the poison case leaves NaN there)."""
import ctypes as C

import numpy as np
import pytest

import aux_update_cases as A
import oracle as O
import scenarios as S

abi, rv = O.abi, O.rv
K = A.K
pytestmark = pytest.mark.gpu
GAMMA_RTOL = 1e-7
CASES = [(n, m) for n in A.WINDOWS for m in ((1, 3, 15, 16) if n == 10 else (1, 16))]


@pytest.fixture(scope="module")
def hL(gpu_required):
    from rvio_amd import hip
    h = hip.RvioHip(A.long_config())
    yield h
    assert h.frame_info()["device_error"] == 0
    h.close()


@pytest.fixture(scope="module")
def hB(gpu_required):
    from rvio_amd import hip
    h = hip.RvioHip(K.config())
    yield h
    assert h.frame_info()["device_error"] == 0
    h.close()


def run(h, x, P, H, v, sigma, mode=abi.RVIO_AUX_RESIDUAL, gate=0):
    h.set_state(x, P)
    h.update_aux(H, v, sigma, mode, gate)
    xd, Pd = h.get_state()
    return xd, Pd, h.aux_diag(), h.pose()


def check(tag, got, want, x_in):
    """device result against (x', P', gamma): the bars, bit symmetry, applied, the pose line of the updated state; returns the worst figures"""
    (xd, Pd, (gam, applied), (pp, pq)), (xw, Pw, gw) = got, want
    dxw, dpw = S.state_delta(xd, xw), float(np.max(np.abs(Pd - Pw)))
    print("%s: state %.3e (bar %.0e)  P %.3e (bar %.3e)  gamma %.6g vs %.6g" % (tag, dxw, A.X_TOL, dpw, A.p_bar(Pw), gam, gw))
    assert applied == 1
    assert dxw <= A.X_TOL and dpw <= A.p_bar(Pw)
    assert np.array_equal(Pd, Pd.T)
    assert abs(gam - gw) <= GAMMA_RTOL * abs(gw)
    wp, wq = abi.pose_line(xd)
    assert np.max(np.abs(pp - wp)) <= 1e-12 and np.max(np.abs(pq - wq)) <= 1e-12
    assert np.max(np.abs(xd - x_in)) > 1e-10
    return dxw, dpw / max(float(np.max(np.abs(Pw))), 1e-300)


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("n,m", CASES)
def test_full_width_H_against_the_model(hL, n, m):
    x, P = A.window_state(n)
    H, v, sigma = A.measurement(P, m, seed=1, kind="full")
    got = run(hL, x, P, H, v, sigma)
    check("full n=%d m=%d" % (n, m), got, abi.aux_update_model(x, P, H, v, sigma), x)


@pytest.mark.parametrize("n,m", [c for c in CASES if c[0] > 0 and c[1] <= 6 * c[0]])
def test_clone_only_H_against_the_oracle_and_the_model(hL, n, m):
    x, P = A.window_state(n)
    H, v, sigma = A.measurement(P, m, seed=2, kind="clone")
    got = run(hL, x, P, H, v, sigma)
    xm, Pm, gm = abi.aux_update_model(x, P, H, v, sigma)
    check("clone/model n=%d m=%d" % (n, m), got, (xm, Pm, gm), x)
    xo, Po = A.oracle_update(A.long_config(), x, P, H, v, sigma)
    check("clone/oracle n=%d m=%d" % (n, m), got, (xo, Po, gm), x)


@pytest.mark.parametrize("name", ["window10", "moved"])
@pytest.mark.parametrize("m", [1, 3, 15, 16])
def test_states_of_the_recorded_sequence(hB, name, m):
    """the two 10-clone states of tests/imu_pose_cases.py on a handle whose leading dimension IS d (no padding); 'moved': qk, pk not identity"""
    x, P = K.state(name)
    H, v, sigma = A.measurement(P, m, seed=4, kind="full")
    check("%s m=%d" % (name, m), run(hB, x, P, H, v, sigma), abi.aux_update_model(x, P, H, v, sigma), x)


@pytest.mark.parametrize("n", [0, 10, 31])
def test_value_mode_zero_velocity_and_velocity(hL, n):
    x, P = A.window_state(n)
    d = P.shape[0]
    for z, sg in (((0.0, 0.0, 0.0), 0.05), (tuple(x[17:20] + np.array([0.02, -0.01, 0.03])), 0.01)):
        H, zz, sigma = A.zupt(d, z, sg)
        got = run(hL, x, P, H, zz, sigma, abi.RVIO_AUX_VALUE)
        check("value n=%d z=%s" % (n, np.round(z, 3)), got, abi.aux_update_model(x, P, H, zz, sigma, abi.RVIO_AUX_VALUE), x)
    # a dense VALUE-mode H over the additive columns (bias, gravity, clone positions)
    rng = np.random.default_rng(n)
    H = rng.standard_normal((5, d))
    rot = [c for c in range(d) if c < 3 or 9 <= c < 12 or (c >= 24 and (c - 24) % 6 < 3)]
    H[:, rot] = 0.0
    sigma = 10.0 ** rng.uniform(-3, -1, 5)
    z = H @ abi.aux_xi(x) + sigma * rng.standard_normal(5)
    assert np.linalg.cond(A.whitened_S(P, H, sigma)) <= A.COND_MAX
    check("value dense n=%d" % n, run(hL, x, P, H, z, sigma, abi.RVIO_AUX_VALUE), abi.aux_update_model(x, P, H, z, sigma, abi.RVIO_AUX_VALUE), x)


# ---------------------------------------------------------------- gate and diag
@pytest.mark.parametrize("n,m", [(10, 1), (10, 3), (10, 16), (31, 16), (0, 3)])
def test_gate_accepts_and_rejects(hL, n, m):
    x, P = A.window_state(n)
    chi = A.chi2_95(m)
    H, v, sigma = A.measurement(P, m, seed=6, kind="full", gamma_target=chi / 4)
    want = abi.aux_update_model(x, P, H, v, sigma)
    assert want[2] <= chi / 2
    check("gate/accept n=%d m=%d" % (n, m), run(hL, x, P, H, v, sigma, gate=1), want, x)
    H, v, sigma = A.measurement(P, m, seed=7, kind="full", gamma_target=4 * chi)
    gw = abi.aux_update_model(x, P, H, v, sigma)[2]
    assert gw >= 2 * chi
    xd, Pd, (gam, applied), _ = run(hL, x, P, H, v, sigma, gate=1)
    print("gate/reject n=%d m=%d: gamma %.6g vs %.6g (table %.6g)" % (n, m, gam, gw, chi))
    assert applied == 0 and np.array_equal(xd, x) and np.array_equal(Pd, P)
    assert abs(gam - gw) <= GAMMA_RTOL * gw
    # the same measurement without the gate is applied
    assert run(hL, x, P, H, v, sigma, gate=0)[2][1] == 1


def test_indefinite_covariance_sets_bit_8_and_leaves_the_state(gpu_required):
    from rvio_amd import hip
    h = hip.RvioHip(K.config())
    x, P = K.state("window10")
    Pbad = -1e3 * P
    H, v, sigma = A.measurement(P, 3, seed=8, kind="full")
    assert np.min(np.linalg.eigvalsh(A.whitened_S(Pbad, H, sigma))) < -1.0
    xd, Pd, (gam, applied), _ = run(h, x, Pbad, H, v, sigma)
    err = h.frame_info()["device_error"]
    h.close()
    assert applied == 0 and np.array_equal(xd, x) and np.array_equal(Pd, Pbad)
    assert err & 8


# ---------------------------------------------------------------- batch handle
def test_batch_handle_strides_and_active_flags(hB, gpu_required):
    import torch
    from rvio_amd import hip
    cfg = K.config()
    states = [K.state("window10"), K.state("moved"), K.state("moved")]
    d, m = 84, 5
    meas = [A.measurement(states[i][1], m, seed=20 + i, kind="full") for i in range(3)]
    plain = [run(hB, states[i][0], states[i][1], *meas[i]) for i in range(3)]
    hb = hip.RvioHip(cfg, batch=3, front_end=False)
    hb.set_state(*states[0])                        # (the window length is handle-wide: set it, then the instances' own states)
    for i in range(3):
        hb.set_state_at(i, *states[i])
    Hs, vs, ss = (np.zeros((3, m * d + 7)), np.zeros((3, m + 3)), np.zeros((3, m + 1)))     # strides longer than the payload
    for i in range(3):
        Hs[i, :m * d], vs[i, :m], ss[i, :m] = meas[i][0].reshape(-1), meas[i][1], meas[i][2]
    dH, dv, ds = (torch.from_numpy(a).cuda() for a in (Hs, vs, ss))
    dact = torch.tensor([1, 0, 1], dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    hb.update_aux_dev(m, abi.RVIO_AUX_RESIDUAL, 0, dH.data_ptr(), Hs.shape[1], dv.data_ptr(), vs.shape[1], ds.data_ptr(), ss.shape[1], dact.data_ptr())
    hb.sync()
    for i in range(3):
        xd, Pd = hb.get_state_at(i)
        gam, applied = hb.aux_diag(i)
        pp, pq = hb.get_pose_at(i)
        if i == 1:
            assert applied == 0 and np.array_equal(xd, states[1][0]) and np.array_equal(Pd, states[1][1])
        else:
            assert applied == 1 and np.array_equal(xd, plain[i][0]) and np.array_equal(Pd, plain[i][1]) and gam == plain[i][2][0]
            assert np.array_equal(pp, plain[i][3][0]) and np.array_equal(pq, plain[i][3][1])
    # the host form on ONE instance: the others stay as they are; -1: every instance the same measurement
    before = [hb.get_state_at(i) for i in range(3)]
    hb.update_aux(*meas[1], instance=1)
    for i in range(3):
        xd, Pd = hb.get_state_at(i)
        if i == 1:
            assert hb.aux_diag(1)[1] == 1 and np.array_equal(xd, plain[1][0]) and np.array_equal(Pd, plain[1][1])
        else:
            assert hb.aux_diag(i)[1] == 0 and np.array_equal(xd, before[i][0]) and np.array_equal(Pd, before[i][1])
    for i in range(3):
        hb.set_state_at(i, *states[1])
    hb.update_aux(*meas[1], instance=-1)
    for i in range(3):
        xd, Pd = hb.get_state_at(i)
        assert np.array_equal(xd, plain[1][0]) and np.array_equal(Pd, plain[1][1])
    assert hb.frame_info()["device_error"] == 0
    hb.close()


# ---------------------------------------------------------------- pipeline
def feed(h, r):
    inp = r["inp"]
    h.frame_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])


def feed_staged(h, r):
    inp = r["inp"]
    h.track_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])
    do_update, do_augment = h.frame_plan()
    h.propagate(inp["imu"])
    if do_update:
        h.update_tracked()
    h.augment_compose(do_augment)


def pipeline(cfg, recs, seq, mode):
    """whole frames with a ZUPT-shaped call behind every second one.  mode 'flat': nothing between the calls; 'sync': rvio_hip_sync behind every
    call; 'staged': the stage entry points, and the state round-trips through the host behind every aux call — which drops whatever factor of
    the clone block the handle kept, so this run cannot use a stale one"""
    from rvio_amd import hip
    h = hip.RvioHip(cfg)
    h.initialize(*seq.init_from_static(38))
    n = 0
    for k, r in enumerate(recs):
        (feed_staged if mode == "staged" else feed)(h, r)
        n = (len(r["x3"]) - 26) // 7
        if mode == "sync":
            h.sync()
        if k % 2 == 1:
            H, z, sigma = A.zupt(24 + 6 * n, sigma=0.5)
            h.update_aux(H, z, sigma, abi.RVIO_AUX_VALUE, 0)
            if mode == "sync":
                h.sync()
            if mode == "staged":
                h.set_state(*h.get_state())
    x, P = h.get_state()
    info = h.frame_info()
    pose = h.pose()
    h.close()
    assert info["device_error"] == 0
    return x, P, pose


def test_pipeline_flat_out_equals_synchronised(gpu_required):
    cfg = K.config()
    seq, recs = K.recorded()
    a, b, c = (pipeline(cfg, recs, seq, mode) for mode in ("flat", "sync", "staged"))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    # the calls did something: the same frames without them end elsewhere
    from rvio_amd import hip
    h = hip.RvioHip(cfg)
    h.initialize(*seq.init_from_static(38))
    for r in recs:
        feed(h, r)
    x0 = h.get_state()[0]
    h.close()
    assert np.max(np.abs(x0 - a[0])) > 1e-6


def test_pipeline_long_window_does_not_use_a_stale_clone_block_factor(gpu_required):
    """6n = 102 > 96: the factor of the clone block for the NEXT visual update starts on the side queue behind augment / compose — the covariance the
    aux call then changes.  The whole-frame run must equal the staged run that cannot have kept one."""
    cfg = abi.config_named("B", enable_equalizer=0, max_track_len=18)
    seq, recs = S.record_sequence(cfg, n_frames=24, duration=6.0)
    assert (len(recs[-1]["x0"]) - 26) // 7 == 17 and sum(1 for r in recs if (len(r["x0"]) - 26) // 7 == 17) >= 5
    a, c = pipeline(cfg, recs, seq, "flat"), pipeline(cfg, recs, seq, "staged")
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    assert np.array_equal(a[2][0], c[2][0]) and np.array_equal(a[2][1], c[2][1])


def test_between_the_stage_entry_points(gpu_required):
    """propagate leaves a factor of the clone block for the update behind it (6n <= 96); an aux call in between must drop it"""
    from rvio_amd import hip
    seq, recs = K.recorded()
    r = recs[11]
    H, v, sigma = A.measurement(r["P1"], 3, seed=9, kind="full")
    out = []
    for roundtrip in (False, True):
        h = hip.RvioHip(K.config())
        h.set_state(r["x0"], r["P0"])
        h.propagate(r["inp"]["imu"])
        h.update_aux(H, v, sigma)
        if roundtrip:
            h.set_state(*h.get_state())
        h.update(r["types"], r["lens"], r["meas"])
        out.append(h.get_state())
        assert h.frame_info()["updated"] == 1
        h.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    xm, Pm, _ = abi.aux_update_model(r["x1"], r["P1"], H, v, sigma)
    x2, P2, _ = O.update(K.config(), xm, Pm, r["types"], r["lens"], r["meas"])
    assert S.state_delta(out[0][0], x2) <= A.X_TOL and float(np.max(np.abs(out[0][1] - P2))) <= A.p_bar(P2)


# ---------------------------------------------------------------- poison
def test_poisoned_leftovers_change_nothing(gpu_required):
    """rvio_hip_debug_poison fills the chip's LDS and the OTHER state / covariance buffer with NaN patterns; the propagate behind it writes its
    d x d result into that buffer and makes it the current one — so the aux call runs on a covariance whose padding up to the leading
    dimension (and whose states behind 26 + 7 n) are NaN, with NaN in every LDS word it does not write itself"""
    from rvio_amd import hip
    h = hip.RvioHip(A.long_config())
    imu = K.batch(10, seed=0)
    res = []
    for poison in (False, True):
        for n in (4, 17):
            x, P = A.window_state(n)
            H, v, sigma = A.measurement(P, 16, seed=11, kind="full")
            h.set_state(x, P)
            if poison:
                h.poison(7)
            h.propagate(imu)
            x1, P1 = h.get_state()
            h.update_aux(H, v, sigma)
            res.append(h.get_state() + (h.aux_diag(), x1, P1))
    h.close()
    for a, b in zip(res[:2], res[2:]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[2][1] == 1
        xm, Pm, gm = abi.aux_update_model(b[3], b[4], *A.measurement(A.window_state((len(b[3]) - 26) // 7)[1], 16, seed=11, kind="full"))
        assert S.state_delta(b[0], xm) <= A.X_TOL and float(np.max(np.abs(b[1] - Pm))) <= A.p_bar(Pm) and np.all(np.isfinite(b[1]))


# ---------------------------------------------------------------- argument errors
def test_argument_errors(gpu_required):
    import torch
    from rvio_amd import hip
    cfg = S.small_image_config()
    h = hip.RvioHip(cfg)
    L = h.L
    H, v, s = np.zeros((3, 24)), np.zeros(3), np.full(3, 0.1)
    H[0, 15] = H[1, 16] = H[2, 17] = 1.0

    def call(Hc, vc, sc, mode=0, gate=0, inst=-1, m=None):
        ms = abi.make_aux_meas(Hc, vc, sc, mode, gate)
        if m is not None:
            ms.m = m
        return L.rvio_hip_update_aux(h.h, inst, C.byref(ms))
    assert call(H, v, s) == -4                                  # no state yet
    seq = rv.synth.SynthSequence(cfg, duration=3.0, seed=0)
    h.initialize(*seq.init_from_static(38))
    assert call(H, v, s, mode=abi.RVIO_AUX_VALUE) == 0          # the empty window, d = 24
    assert h.aux_diag()[1] == 1
    assert call(H, v, s, m=0) == -1 and call(np.zeros((17, 24)), np.zeros(17), np.ones(17)) == -1
    assert call(H, v, np.array([0.1, 0.0, 0.1])) == -1 and call(H, v, np.array([0.1, -1.0, 0.1])) == -1 and call(H, v, np.array([0.1, np.inf, 0.1])) == -1
    Hn = H.copy()
    Hn[1, 7] = np.nan
    assert call(Hn, v, s) == -1 and call(H, np.array([0.0, np.nan, 0.0]), s) == -1
    Hr = H.copy()
    Hr[2, 10] = 1e-3
    assert call(Hr, v, s, mode=abi.RVIO_AUX_VALUE) == -1 and call(Hr, v, s, mode=abi.RVIO_AUX_RESIDUAL) == 0
    assert call(H, v, s, mode=2) == -1 and call(H, v, s, gate=2) == -1 and call(H, v, s, inst=1) == -1 and call(H, v, s, inst=-2) == -1
    assert L.rvio_hip_update_aux(h.h, 0, None) == -1
    g, a = C.c_double(0), C.c_int32(0)
    assert L.rvio_hip_get_aux_diag(h.h, 1, C.byref(g), C.byref(a)) == -1
    dH = torch.from_numpy(H).cuda()
    torch.cuda.synchronize()
    vp = C.c_void_p
    assert L.rvio_hip_update_aux_dev(h.h, 0, 0, 0, vp(dH.data_ptr()), C.c_size_t(0), vp(dH.data_ptr()), C.c_size_t(0), vp(dH.data_ptr()), C.c_size_t(0), None) == -1
    assert L.rvio_hip_update_aux_dev(h.h, 17, 0, 0, vp(dH.data_ptr()), C.c_size_t(0), vp(dH.data_ptr()), C.c_size_t(0), vp(dH.data_ptr()), C.c_size_t(0), None) == -1
    assert L.rvio_hip_update_aux_dev(h.h, 3, 0, 0, None, C.c_size_t(0), vp(dH.data_ptr()), C.c_size_t(0), vp(dH.data_ptr()), C.c_size_t(0), None) == -1
    assert L.rvio_hip_update_aux_dev(h.h, 3, 0, 0, vp(dH.data_ptr()), C.c_size_t(71), vp(dH.data_ptr()), C.c_size_t(0), vp(dH.data_ptr()), C.c_size_t(0), None) == -1
    # inside an open frame
    img, imu = seq.render(39), seq.imu_between(39)
    d_img, d_imu = torch.from_numpy(img).cuda(), torch.from_numpy(imu.view(np.uint8)).cuda()
    torch.cuda.synchronize()
    h.frame_begin_dev(d_img.data_ptr(), img.shape[1], d_imu.data_ptr(), len(imu), 0, 0)
    rc_open = call(H, v, s)
    rc_open_dev = L.rvio_hip_update_aux_dev(h.h, 3, 0, 0, vp(dH.data_ptr()), C.c_size_t(0), vp(dH.data_ptr()), C.c_size_t(0), vp(dH.data_ptr()), C.c_size_t(0), None)
    do_update, do_augment = h.frame_plan()
    if do_update:
        h.update_tracked()
    h.augment_compose(do_augment)
    h.frame_end()
    assert rc_open == -4 and rc_open_dev == -4
    Hw = np.zeros((3, 24 + 6 * h.frame_info()["n_clones"]))
    Hw[0, 15] = Hw[1, 16] = Hw[2, 17] = 1.0
    assert call(Hw, v, s) == 0                                  # behind the frame, on the pipelined handle
    h.sync()
    assert h.frame_info()["device_error"] == 0
    h.close()
