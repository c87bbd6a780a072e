"""GPU: absolute fixes (rvio_hip_update_fix*, csrc/fix_rows.hip in front of csrc/aux_update.hip).  The rows the device forms against
abi.fix_model (bar 1e-12 max(1, max|H|), the columns the header's table lists as 0 exactly 0.0); the applied update against
abi.aux_update_model on the model's rows at the bars of tests/test_gpu_aux_update.py; a twin handle handed the device's own rows through
rvio_hip_update_aux ends with the same bits; the gate; batch handles with strides and flags; frames flat out against synchronised; the long
window; every error.  One handle of the longest window (max_track_len = 32, leading dimension 210) takes the states of every window."""
import ctypes as C

import numpy as np
import pytest

import fix_cases as F
import scenarios as S
from test_gpu_aux_update import GAMMA_RTOL, feed, feed_staged

abi, A, K = F.abi, F.A, F.K
rv = A.rv
pytestmark = pytest.mark.gpu
WINDOWS = (0, 3, 10, 31)          # d = 24, the smallest padded window, the stock window, ld = d (no padding)
KIDS = [F.KIND_NAMES[k] for k in F.KINDS]
# the columns the table of include/rvio_hip.h lists as non-zero, per block of three rows
POS_COLS, ATT_COLS, GRAV_COLS = (0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 14), (0, 1, 2, 9, 10, 11), (6, 7, 8, 9, 10, 11, 21, 22, 23)
TABLE = {abi.RVIO_FIX_POSITION: (POS_COLS,), abi.RVIO_FIX_ATTITUDE: (ATT_COLS,), abi.RVIO_FIX_POSE: (POS_COLS, ATT_COLS), abi.RVIO_FIX_GRAVITY: (GRAV_COLS,)}
K0 = 38


@pytest.fixture(scope="module")
def hL(gpu_required):
    from rvio_amd import hip
    h = hip.RvioHip(A.long_config())
    yield h
    assert h.frame_info()["device_error"] == 0
    h.close()


def diag_of(h, i=0):
    r = h.get_fix(i)
    return dict(r=np.array(r.r[:]), gamma=r.gamma, applied=r.applied, kind=r.kind, m=r.m, img_count=r.img_count)


def place(h, x, P, poison):
    """the state on the handle; poison: through rvio_hip_debug_poison + a propagation, which leaves NaN in the padding of P up to the leading
    dimension and behind the states (tests/test_gpu_aux_update.py test_poisoned_leftovers_change_nothing).  Returns the state the handle holds."""
    h.set_state(x, P)
    if not poison:
        return x, P
    h.poison(7)
    h.propagate(K.batch(10, seed=0))
    return h.get_state()


def run(h, kind, fix, gate=0):
    h.update_fix(kind, fix, gate)
    xd, Pd = h.get_state()
    return dict(x=xd, P=Pd, diag=diag_of(h), pose=h.pose(), rows=h.get_fix_rows())


def cases(n):
    """(tag, x, P, poison): 'moved' (qk, pk off identity; through the poisoned propagation where the window leaves padding) and the all-zero qk"""
    xm, Pm = F.moved_window(n)
    xz, Pz = A.window_state(n)
    return [("moved", xm, Pm, n != 31), ("zero_qk", F.zero_qk(xz), Pz, False)]


def check_rows(tag, cfg, x, kind, fix, out):
    H, r, sigma = abi.fix_model(cfg, x, kind, fix)
    Hd, sd = out["rows"]
    dg = out["diag"]
    m = abi.FIX_ROWS[kind]
    bar = 1e-12 * max(1.0, float(np.max(np.abs(H))))
    eh, er = float(np.max(np.abs(Hd - H))), float(np.max(np.abs(dg["r"][:m] - r)))
    print("%s: max|H - model| %.3e  max|r - model| %.3e (bar %.1e, max|H| %.3g)" % (tag, eh, er, bar, np.max(np.abs(H))))
    assert Hd.shape == H.shape and eh <= bar and er <= bar
    assert np.array_equal(sd, sigma) and not dg["r"][m:].any() and (dg["kind"], dg["m"]) == (kind, m)
    for b, cols in enumerate(TABLE[kind]):
        zero = [c for c in range(H.shape[1]) if c not in cols]
        blk = Hd[3 * b: 3 * b + 3][:, zero]
        assert not blk.any() and not np.signbit(blk).any(), "a column the table lists as 0"
        assert np.abs(Hd[3 * b: 3 * b + 3][:, list(cols)]).sum() > 1.0
    return eh, er


# ---------------------------------------------------------------- 1. the rows
@pytest.mark.parametrize("n", WINDOWS)
@pytest.mark.parametrize("kind", F.KINDS, ids=KIDS)
def test_rows_against_the_model(hL, kind, n):
    cfg = A.long_config()
    for tag, x0, P0, poison in cases(n):
        for li, lever in enumerate(F.LEVERS):
            x, P = place(hL, x0, P0, poison)
            fix = F.fix_near(cfg, x, kind, lever, sigma_p=(0.02, 0.03, 0.04), sigma_q=(0.005, 0.006, 0.007), seed=n + li)
            out = run(hL, kind, fix)
            check_rows("%s %s n=%d lever=%d" % (F.KIND_NAMES[kind], tag, n, 1 - li), cfg, x, kind, fix, out)
            assert out["diag"]["applied"] == 1 and out["rows"][0].shape[1] == 24 + 6 * n


# ---------------------------------------------------------------- 2. the applied update
@pytest.mark.parametrize("n", WINDOWS)
@pytest.mark.parametrize("kind", F.KINDS, ids=KIDS)
def test_applied_update_against_the_model(hL, kind, n):
    cfg = A.long_config()
    for tag, x0, P0, poison in cases(n):
        x, P = place(hL, x0, P0, poison)
        fix = F.fix_near(cfg, x, kind, F.LEVER, sigma_p=0.02, sigma_q=0.005, seed=3 + n)
        out = run(hL, kind, fix)
        xw, Pw, gw = abi.aux_update_model(x, P, *abi.fix_model(cfg, x, kind, fix))
        xd, Pd, dg = out["x"], out["P"], out["diag"]
        dxw, dpw = S.state_delta(xd, xw), float(np.max(np.abs(Pd - Pw)))
        print("%s %s n=%d: state %.3e (bar %.0e)  P %.3e (bar %.3e)  gamma %.6g vs %.6g" % (F.KIND_NAMES[kind], tag, n, dxw, A.X_TOL, dpw, A.p_bar(Pw), dg["gamma"], gw))
        assert dg["applied"] == 1 and np.all(np.isfinite(Pd))
        assert dxw <= A.X_TOL and dpw <= A.p_bar(Pw)
        assert np.array_equal(Pd, Pd.T)
        assert abs(dg["gamma"] - gw) <= GAMMA_RTOL * abs(gw)
        wp, wq = abi.pose_line(xd)
        assert np.max(np.abs(out["pose"][0] - wp)) <= 1e-12 and np.max(np.abs(out["pose"][1] - wq)) <= 1e-12
        assert np.max(np.abs(xd - x)) > 1e-10
        # the state moved onto the fix
        assert np.linalg.norm(abi.fix_model(cfg, xd, kind, fix)[1]) < np.linalg.norm(abi.fix_model(cfg, x, kind, fix)[1])


# ---------------------------------------------------------------- 3. the bits of a twin
@pytest.mark.parametrize("kind", [abi.RVIO_FIX_POSITION, abi.RVIO_FIX_POSE], ids=["m3", "m6"])
def test_a_twin_handed_the_devices_rows_ends_with_the_same_bits(hL, kind):
    from rvio_amd import hip
    cfg = A.long_config()
    twin = hip.RvioHip(cfg)
    for n in (3, 10):
        x, P = F.moved_window(n)
        fix = F.fix_near(cfg, x, kind, F.LEVER, sigma_p=0.02, sigma_q=0.005, seed=n)
        hL.set_state(x, P)
        out = run(hL, kind, fix)
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
        # a later update_aux of the caller's does not overwrite the fix's record
        hL.update_aux(*A.zupt(24 + 6 * n, sigma=0.5), abi.RVIO_AUX_VALUE, 0)
        again = diag_of(hL)
        assert again["gamma"] == out["diag"]["gamma"] and again["applied"] == 1 and np.array_equal(again["r"], out["diag"]["r"])
    assert twin.frame_info()["device_error"] == 0
    twin.close()


# ---------------------------------------------------------------- 4. the gate
def fix_with_gamma(cfg, x, P, kind, target, seed):
    """a fix along a fixed direction, scaled until the model's gamma is `target` (the residual is linear in the offset up to the attitude's sine)"""
    s = 1.0
    for _ in range(8):
        fix = F.fix_near(cfg, x, kind, F.LEVER, dp=0.01 * s, dth=0.002 * s, sigma_p=0.02, sigma_q=0.005, seed=seed)
        g = abi.aux_update_model(x, P, *abi.fix_model(cfg, x, kind, fix))[2]
        s *= np.sqrt(target / g)
    return fix, g


@pytest.mark.parametrize("kind", F.KINDS, ids=KIDS)
def test_gate_accepts_and_rejects(hL, kind):
    cfg = A.long_config()
    n = 10
    x, P = F.moved_window(n)
    chi = A.chi2_95(abi.FIX_ROWS[kind])
    fix, gw = fix_with_gamma(cfg, x, P, kind, chi / 4, seed=5)
    assert gw <= chi / 2
    hL.set_state(x, P)
    out = run(hL, kind, fix, gate=1)
    xw, Pw, _ = abi.aux_update_model(x, P, *abi.fix_model(cfg, x, kind, fix))
    print("gate/accept %s: gamma %.6g vs %.6g (table %.6g)" % (F.KIND_NAMES[kind], out["diag"]["gamma"], gw, chi))
    assert out["diag"]["applied"] == 1 and abs(out["diag"]["gamma"] - gw) <= GAMMA_RTOL * gw
    assert S.state_delta(out["x"], xw) <= A.X_TOL and float(np.max(np.abs(out["P"] - Pw))) <= A.p_bar(Pw)
    fix, gw = fix_with_gamma(cfg, x, P, kind, 4 * chi, seed=6)
    assert gw >= 2 * chi
    hL.set_state(x, P)
    pose0 = hL.pose()
    out = run(hL, kind, fix, gate=1)
    print("gate/reject %s: gamma %.6g vs %.6g (table %.6g)" % (F.KIND_NAMES[kind], out["diag"]["gamma"], gw, chi))
    assert out["diag"]["applied"] == 0 and abs(out["diag"]["gamma"] - gw) <= GAMMA_RTOL * gw
    assert np.array_equal(out["x"], x) and np.array_equal(out["P"], P)
    assert np.array_equal(out["pose"][0], pose0[0]) and np.array_equal(out["pose"][1], pose0[1])
    check_rows("gate/reject rows", cfg, x, kind, fix, out)          # the rows were formed all the same
    # the same fix without the gate is applied
    assert run(hL, kind, fix, gate=0)["diag"]["applied"] == 1


# ---------------------------------------------------------------- 5. batch handles
def test_batch_strides_and_active_flags(hL, gpu_required):
    import torch
    from rvio_amd import hip
    cfg = A.long_config()
    n, kind = 10, abi.RVIO_FIX_POSE
    xw, Pw = A.window_state(n)
    states = [F.moved_window(n), (xw, Pw), (F.zero_qk(xw), Pw)]
    fixes = [F.fix_near(cfg, states[i][0], kind, F.LEVERS[i % 2], sigma_p=0.02, sigma_q=0.005, seed=40 + i) for i in range(3)]
    single = []
    for i in range(3):
        hL.set_state(*states[i])
        single.append(run(hL, kind, fixes[i]))
    hb = hip.RvioHip(cfg, batch=3, front_end=False)
    hb.set_state(*states[0])                        # (the window length is handle-wide: set it, then the instances' own states)
    for i in range(3):
        hb.set_state_at(i, *states[i])
    recs = np.zeros(6, abi.FIX_DTYPE)               # a stride of two records: the odd ones hold NaN, which nobody may read
    recs["z"], recs["sigma"], recs["lever"] = np.nan, np.nan, np.nan
    for i in range(3):
        recs[2 * i] = np.frombuffer(bytes(fixes[i]), abi.FIX_DTYPE)[0]
    d_fix = torch.from_numpy(recs.view(np.uint8)).cuda()
    d_act = torch.tensor([1, 0, 1], dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    hb.update_fix_dev(kind, 0, d_fix.data_ptr(), 2, d_act.data_ptr())
    for i in range(3):
        xd, Pd = hb.get_state_at(i)
        pp, pq = hb.get_pose_at(i)
        dg = diag_of(hb, i)
        if i == 1:
            assert dg["applied"] == 0 and dg["gamma"] == 0.0 and np.array_equal(xd, states[1][0]) and np.array_equal(Pd, states[1][1])
        else:
            s = single[i]
            assert dg["applied"] == 1 and dg["gamma"] == s["diag"]["gamma"] and np.array_equal(dg["r"], s["diag"]["r"])
            assert np.array_equal(xd, s["x"]) and np.array_equal(Pd, s["P"])
            assert np.array_equal(pp, s["pose"][0]) and np.array_equal(pq, s["pose"][1])
            Hd, sd = hb.get_fix_rows(i)
            assert np.array_equal(Hd, s["rows"][0]) and np.array_equal(sd, s["rows"][1])
    # the host form on ONE instance: the others stay as they are
    before = [hb.get_state_at(i) for i in range(3)]
    hb.update_fix(kind, fixes[1], 0, instance=1)
    for i in range(3):
        xd, Pd = hb.get_state_at(i)
        if i == 1:
            assert diag_of(hb, 1)["applied"] == 1 and np.array_equal(xd, single[1]["x"]) and np.array_equal(Pd, single[1]["P"])
        else:
            assert diag_of(hb, i)["applied"] == 0 and np.array_equal(xd, before[i][0]) and np.array_equal(Pd, before[i][1])
    assert hb.frame_info()["device_error"] == 0
    hb.close()


def test_batch_of_128_with_a_shared_fix(gpu_required):
    import torch
    from rvio_amd import hip
    cfg, B, kind = K.config(), 128, abi.RVIO_FIX_POSITION
    x, P = K.state("moved")
    fix = F.fix_near(cfg, x, kind, F.LEVER, sigma_p=0.02, seed=9)
    h1 = hip.RvioHip(cfg)
    h1.set_state(x, P)
    one = run(h1, kind, fix)
    h1.close()
    hb = hip.RvioHip(cfg, batch=B, front_end=False)
    hb.set_state(x, P)
    d_fix = torch.from_numpy(np.frombuffer(bytes(fix), np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    hb.update_fix_dev(kind, 0, d_fix.data_ptr(), 0, None)
    for i in (0, 1, 63, 64, 127):
        xd, Pd = hb.get_state_at(i)
        dg = diag_of(hb, i)
        assert dg["applied"] == 1 and dg["gamma"] == one["diag"]["gamma"] and np.array_equal(xd, one["x"]) and np.array_equal(Pd, one["P"])
        assert np.array_equal(hb.get_fix_rows(i)[0], one["rows"][0])
    # host form, instance -1: every instance the same fix
    hb.set_state(x, P)
    hb.update_fix(kind, fix, 0, instance=-1)
    for i in (0, 77, 127):
        xd, Pd = hb.get_state_at(i)
        assert np.array_equal(xd, one["x"]) and np.array_equal(Pd, one["P"])
    assert hb.frame_info()["device_error"] == 0
    hb.close()


# ---------------------------------------------------------------- 6. between frames, flat out
def frames_run(sync):
    """8 direct-track frames with a POSITION fix behind each; sync: rvio_hip_sync in front of and behind every fix"""
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
        h.update_fix(abi.RVIO_FIX_POSITION, abi.make_fix((0.002 * (k - K0), -0.001 * (k - K0), 0.0), None, 0.05, 0.0, F.LEVER), 0)
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
    assert a["err"] == 0 and b["err"] == 0 and a["ga"][1] == 1 and a["ga"][2] == 8
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------- 7. the long window
def pipeline(cfg, recs, seq, mode):
    """whole frames with a POSITION fix behind every second one.  'flat': nothing between the calls; 'staged': the stage entry points, and the
    state round-trips through the host behind every fix — which drops whatever factor of the clone block the handle kept"""
    from rvio_amd import hip
    h = hip.RvioHip(cfg)
    h.initialize(*seq.init_from_static(38))
    for k, r in enumerate(recs):
        (feed_staged if mode == "staged" else feed)(h, r)
        if k % 2 == 1:
            h.update_fix(abi.RVIO_FIX_POSITION, abi.make_fix((0.001 * k, 0.0, -0.001 * k), None, 0.05, 0.0, F.LEVER), 0)
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
    the fix then changes.  The whole-frame run must equal the staged run that cannot have kept one."""
    cfg = abi.config_named("B", enable_equalizer=0, max_track_len=18)
    seq, recs = S.record_sequence(cfg, n_frames=24, duration=6.0)
    assert (len(recs[-1]["x0"]) - 26) // 7 == 17 and sum(1 for r in recs if (len(r["x0"]) - 26) // 7 == 17) >= 5
    a, c = pipeline(cfg, recs, seq, "flat"), pipeline(cfg, recs, seq, "staged")
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    assert np.array_equal(a[2][0], c[2][0]) and np.array_equal(a[2][1], c[2][1])
    # the fixes did something: the same frames without them end elsewhere
    from rvio_amd import hip
    h = hip.RvioHip(cfg)
    h.initialize(*seq.init_from_static(38))
    for r in recs:
        feed(h, r)
    x0 = h.get_state()[0]
    h.close()
    assert np.max(np.abs(x0 - a[0])) > 1e-6


# ---------------------------------------------------------------- 8. errors
def test_argument_and_state_errors(gpu_required):
    import torch
    from rvio_amd import hip
    cfg = S.small_image_config()
    h = hip.RvioHip(cfg)
    L = h.L
    INVALID, STATE = -1, -4

    def call(kind, fix, gate=0, inst=-1):
        return L.rvio_hip_update_fix(h.h, inst, kind, gate, C.byref(fix))
    def mk(**kw):
        f = abi.make_fix((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0), 0.5, 0.5, (0.1, 0.0, 0.0))
        for name, (i, v) in kw.items():
            getattr(f, name)[i] = v
        return f
    good = mk()
    out, m, d = abi.rvio_fix_diag(), C.c_int32(0), C.c_int32(0)
    # a handle that never called the feature
    assert L.rvio_hip_get_fix(h.h, 0, C.byref(out)) == STATE and L.rvio_hip_get_fix_rows(h.h, 0, C.byref(m), C.byref(d), None, None) == STATE
    d_fix = torch.from_numpy(np.frombuffer(bytes(good), np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    vp = C.c_void_p
    assert call(0, good) == STATE and L.rvio_hip_update_fix_dev(h.h, 0, 0, vp(d_fix.data_ptr()), C.c_size_t(0), None) == STATE      # no state yet
    assert L.rvio_hip_get_fix(h.h, 0, C.byref(out)) == STATE
    seq = rv.synth.SynthSequence(cfg, duration=3.0, seed=0)
    h.initialize(*seq.init_from_static(38))
    for kind in F.KINDS:                                         # the empty window right behind initialisation (qk all zero), d = 24
        assert call(kind, good) == 0 and diag_of(h)["applied"] == 1 and diag_of(h)["kind"] == kind
    assert L.rvio_hip_get_fix_rows(h.h, 0, C.byref(m), C.byref(d), None, None) == 0 and (m.value, d.value) == (3, 24)
    # out of range
    assert call(-1, good) == INVALID and call(4, good) == INVALID and call(0, good, gate=2) == INVALID and call(0, good, gate=-1) == INVALID
    assert call(0, good, inst=1) == INVALID and call(0, good, inst=-2) == INVALID
    assert L.rvio_hip_update_fix(h.h, 0, 0, 0, None) == INVALID and L.rvio_hip_update_fix_dev(h.h, 0, 0, None, C.c_size_t(0), None) == INVALID
    assert L.rvio_hip_update_fix_dev(h.h, 4, 0, vp(d_fix.data_ptr()), C.c_size_t(0), None) == INVALID
    assert L.rvio_hip_update_fix_dev(h.h, 0, 2, vp(d_fix.data_ptr()), C.c_size_t(0), None) == INVALID
    assert L.rvio_hip_get_fix(h.h, 1, C.byref(out)) == INVALID and L.rvio_hip_get_fix(h.h, 0, None) == INVALID
    assert L.rvio_hip_get_fix_rows(h.h, 1, C.byref(m), C.byref(d), None, None) == INVALID and L.rvio_hip_get_fix_rows(h.h, 0, None, C.byref(d), None, None) == INVALID
    # a non-finite entry, a sigma <= 0, a quaternion off unit length — where the kind uses the entry, and only there
    P_, A_, Q_, G_ = abi.RVIO_FIX_POSITION, abi.RVIO_FIX_ATTITUDE, abi.RVIO_FIX_POSE, abi.RVIO_FIX_GRAVITY
    for bad, refused, taken in ((mk(z=(1, np.nan)), (P_, Q_, G_), (A_,)), (mk(z=(4, np.inf)), (A_, Q_), (P_, G_)),
                                (mk(sigma=(2, 0.0)), (P_, Q_, G_), (A_,)), (mk(sigma=(0, -1.0)), (P_, Q_, G_), (A_,)), (mk(sigma=(1, np.nan)), (P_, Q_, G_), (A_,)),
                                (mk(sigma=(4, 0.0)), (A_, Q_), (P_, G_)), (mk(sigma=(5, np.inf)), (A_, Q_), (P_, G_)),
                                (mk(lever=(2, np.nan)), (P_, Q_), (A_, G_)),
                                (mk(z=(6, 1.0 + 1e-5)), (A_, Q_), (P_, G_)), (mk(z=(6, 1.0 - 1e-5)), (A_, Q_), (P_, G_))):
        for kind in refused:
            assert call(kind, bad) == INVALID, kind
        for kind in taken:
            assert call(kind, bad) == 0, kind
    assert call(A_, mk(z=(6, 1.0 + 1e-7))) == 0                  # within 1e-6 of unit length
    # inside an open frame
    img, imu = seq.render(39), seq.imu_between(39)
    d_img, d_imu = torch.from_numpy(img).cuda(), torch.from_numpy(imu.view(np.uint8)).cuda()
    torch.cuda.synchronize()
    h.frame_begin_dev(d_img.data_ptr(), img.shape[1], d_imu.data_ptr(), len(imu), 0, 0)
    rc_open = call(0, good)
    rc_open_dev = L.rvio_hip_update_fix_dev(h.h, 0, 0, vp(d_fix.data_ptr()), C.c_size_t(0), None)
    do_update, do_augment = h.frame_plan()
    if do_update:
        h.update_tracked()
    h.augment_compose(do_augment)
    h.frame_end()
    assert rc_open == STATE and rc_open_dev == STATE
    assert call(Q_, good) == 0                                   # behind the frame, on the pipelined handle
    assert h.get_fix_rows()[0].shape == (6, 24 + 6 * h.frame_info()["n_clones"])
    h.sync()
    assert h.frame_info()["device_error"] == 0
    h.close()
