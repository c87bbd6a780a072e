"""The landmark covariance (rvio_hip_set_landmark_cov / rvio_hip_get_landmark_cov[_at|_dev], csrc/landmark_cov.hip) on the device: cov_r and
cov_w of every record against the np.longdouble twin fed the device's own operands, the bit-level links to the cloud, the status path, empty
and full clouds, every update path, and that a handle which does not enable it is bit-identical to one that does.

Accuracy bar (tests/landmark_cov_cases.py): e = max |C - C_true|_ij / sqrt(C_ii C_jj) <= 1e-11, provided the float64 model's own floor against
the twin on the same case is below 1e-12; a case whose floor is higher is held to 16 x its measured floor.  Measured on the CPU for the cases
below (max_track_len 3 / 10 / 32, both track types, L = 2 .. 32): float64 floor 1.1e-14 / 2.4e-15 / 2.3e-15 at cond(N) <= 2.6e6 / 3.7e3 / 1.0e3 — every
case takes the 1e-11 bar.  Measured on one MI355X: e = 1.1e-14 / 1.9e-15 / 1.8e-15."""
import os

import numpy as np
import pytest

import landmark_cov_cases as K
import oracle as O
import scenarios as S

abi, rv = O.abi, O.rv
pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def links(lm, lc, dg, lens):
    """what ties a record to the cloud and to the update's diagnostics, bit for bit"""
    rec = lc["rec"]
    assert lc["n"] == lm["n"] == len(rec) and lc["frame"] == lm["frame"]
    assert np.array_equal(rec["feat"], lm["feat"])
    assert np.array_equal(rec["p_r"], lm["p_r"])
    assert np.array_equal(rec["n_obs"], np.asarray(lens)[rec["feat"]])
    assert np.array_equal(rec["rho"], dg["pfinv"][rec["feat"], 2]) and not rec["reserved"].any()
    assert np.array_equal(rec["cov_r"], rec["cov_r"].transpose(0, 2, 1), equal_nan=True)
    assert np.array_equal(rec["cov_w"], rec["cov_w"].transpose(0, 2, 1), equal_nan=True)
    ok = rec["status"] == 0
    assert np.isfinite(rec["p_r"]).all() and np.isfinite(rec["p_w"]).all()
    assert np.isfinite(rec["cov_r"][ok]).all() and np.isfinite(rec["cov_w"][ok]).all() and (rec["rho_sigma"][ok] > 0).all()
    assert np.isnan(rec["cov_r"][~ok]).all() and np.isnan(rec["cov_w"][~ok]).all() and np.isnan(rec["rho_sigma"][~ok]).all()


def against_twin(cal, sigma, rec, x1, P1, types, lens, meas, pfinv, pick):
    """(device error, float64 floor, cond(N)) over the records `pick` against the np.longdouble twin at the device's own operands"""
    e_dev, e_f64, cond = 0.0, 0.0, 0.0
    for j in pick:
        r = rec[j]
        f = int(r["feat"])
        args = (cal, x1, P1, chr(types[f]), int(lens[f]), meas[f], pfinv[f])
        t, m = abi.landmark_cov_model_as(*args, sigma=sigma), abi.landmark_cov_model(*args, sigma=sigma)
        assert t["status"] == 0 == r["status"], (j, f)
        e_dev = max(e_dev, K.cov_err(r["cov_r"], t["cov_r"]), K.cov_err(r["cov_w"], t["cov_w"]))
        e_f64 = max(e_f64, K.cov_err(m["cov_r"], t["cov_r"]), K.cov_err(m["cov_w"], t["cov_w"]))
        cond = max(cond, float(np.linalg.cond(m["N"])))
        assert abs(r["rho_sigma"] - float(t["rho_sigma"])) <= 1e-11 * float(t["rho_sigma"]), (j, f)
        assert np.max(np.abs(r["p_w"] - np.asarray(t["p_w"], float))) <= 1e-12 * max(1.0, float(np.linalg.norm(r["p_w"]))), (j, f)
    return e_dev, e_f64, cond


def one_of_each(rec, types, lens, most=10):
    """record indices covering every (type, L) of the cloud, at most `most`"""
    seen, pick = set(), []
    for j, f in enumerate(rec["feat"]):
        key = (int(types[f]), int(lens[f]))
        if key not in seen:
            seen.add(key)
            pick.append(j)
    if len(pick) > most:
        pick = [pick[i] for i in np.unique(np.linspace(0, len(pick) - 1, most).astype(int))]
    return pick


def run_update(cfg, x1, P1, types, lens, meas):
    from rvio_amd import hip
    h = hip.RvioHip(cfg)
    h.set_landmark_cov(True)
    h.set_state(x1, P1)
    h.update(types, lens, meas)
    out = h.landmarks(), h.landmark_cov(), h.update_diag()
    h.close()
    return out


@pytest.mark.parametrize("max_len", K.WINDOWS)
def test_accuracy_and_links(gpu_required, max_len):
    cfg, x1, P1, types, lens, meas = K.window_case(max_len)
    lm, lc, dg = run_update(cfg, x1, P1, types, lens, meas)
    links(lm, lc, dg, lens)
    rec = lc["rec"]
    kinds = {(int(types[f]), int(lens[f])) for f in rec["feat"]}
    assert lc["n"] >= 6 and {k[0] for k in kinds} == {ord("1"), ord("2")}, kinds
    if max_len == 3:
        assert {k[1] for k in kinds} == {2, 3}
    assert max(k[1] for k in kinds) == max_len
    e, floor, cond = against_twin(cfg, None, rec, x1, P1, types, lens, meas, dg["pfinv"], one_of_each(rec, types, lens))
    bar = K.BAR if floor < K.FLOOR_BAR else 16 * floor
    print("landmark cov, max_track_len %d: %d records, device e = %.2e, float64 floor %.2e, cond(N) <= %.1e, bar %.1e" % (max_len, lc["n"], e, floor, cond, bar))
    assert e <= bar, (e, bar)
    # the same call again: the same bits
    lm2, lc2, _ = run_update(cfg, x1, P1, types, lens, meas)
    assert lc2["n"] == lc["n"] and lc2["rec"].tobytes() == rec.tobytes() and np.array_equal(lm2["p_world"], lm["p_world"])


def test_status_path_singular_normal_matrix(gpu_required):
    """a hand-built track whose N is singular: the per-feature stage triangulates on the recorded state, then the state is replaced by one
    whose newest clone is the identity with zero translation before the global stage runs — the L = 2 type-'1' tracks (that clone only) get
    an exactly zero depth column: status 1, NaN covariances, finite points; every other record is the twin's at the replaced state"""
    from rvio_amd import hip
    cfg, x1, P1, types, lens, meas = K.window_case(10)
    n = (len(x1) - 26) // 7
    xs = x1.copy()
    xs[26 + 7 * (n - 1): 26 + 7 * n] = [0, 0, 0, 1, 0, 0, 0]
    h = hip.RvioHip(cfg)
    h.set_landmark_cov(True)
    h.set_state(x1, P1)
    ptr, _ = h.update_local(types, lens, meas, 0, 1)
    h.set_state(xs, P1)
    h.update_global(ptr, 1)
    lm, lc, dg = h.landmarks(), h.landmark_cov(), h.update_diag()
    h.close()
    links(lm, lc, dg, lens)
    rec = lc["rec"]
    short = np.array([types[f] == ord("1") and lens[f] == 2 for f in rec["feat"]])
    assert short.any() and (~short).sum() >= 5
    assert (rec["status"][short] == 1).all() and (rec["status"][~short] == 0).all()
    for f in rec["feat"][short]:
        assert abi.landmark_cov_model(cfg, xs, P1, "1", 2, meas[f], dg["pfinv"][f])["status"] == 1
    pick = [j for j in one_of_each(rec, types, lens) if not short[j]]
    e, floor, _ = against_twin(cfg, None, rec, xs, P1, types, lens, meas, dg["pfinv"], pick)
    print("status path: %d singular of %d records, the others e = %.2e (floor %.2e)" % (short.sum(), len(rec), e, floor))
    assert e <= (K.BAR if floor < K.FLOOR_BAR else 16 * floor)


def test_empty_small_full_and_zero_parallax_clouds(gpu_required):
    from rvio_amd import hip
    cfg = abi.config_named("B", enable_equalizer=0)
    _, recs = S.record_sequence(cfg, n_frames=14)
    r = recs[-1]
    assert r["did_update"]
    x1, P1 = r["x1"], r["P1"]
    h = hip.RvioHip(cfg)
    import ctypes as C
    n, fr = C.c_int32(7), C.c_int32(7)
    assert h.L.rvio_hip_get_landmark_cov(h.h, C.byref(n), C.byref(fr), None) == -4                 # RVIO_ERR_STATE: never enabled
    assert h.L.rvio_hip_get_landmark_cov_dev(h.h, C.c_void_p(64), C.c_size_t(abi.fu(cfg)), None) == -4
    with pytest.raises(hip.RvioHipError):
        h.time_kernel(15, 1)
    h.set_landmark_cov(True)
    assert h.L.rvio_hip_get_landmark_cov_at(h.h, 1, C.byref(n), C.byref(fr), None) == -1           # RVIO_ERR_INVALID: no instance 1
    lc = h.landmark_cov()
    assert lc["n"] == 0 and lc["frame"] == -1
    # three features (the update is skipped, the cloud is published), two, none
    for k in (3, 2, 0):
        h.set_state(x1, P1)
        h.frame_plan()
        h.update(r["types"][:k], r["lens"][:k], r["meas"][:k])
        lm, lc, dg = h.landmarks(), h.landmark_cov(), h.update_diag()
        assert lc["n"] == lm["n"] <= k and lc["frame"] == lm["frame"] >= 0
        links(lm, lc, dg, r["lens"][:k])
    # a full table: ceil(F / 2) features, nearly all of them in the cloud
    types, lens, meas = S.worst_case_tracks(cfg, r, None)
    h.set_state(x1, P1)
    h.update(types, lens, meas)
    lm, lc, dg = h.landmarks(), h.landmark_cov(), h.update_diag()
    links(lm, lc, dg, lens)
    assert len(types) == abi.fu(cfg) and lc["n"] >= abi.fu(cfg) - 10 and (lc["rec"]["status"] == 0).all()
    e, floor, _ = against_twin(cfg, None, lc["rec"], x1, P1, types, lens, meas, dg["pfinv"], [0, lc["n"] // 2, lc["n"] - 1])
    assert e <= (K.BAR if floor < K.FLOOR_BAR else 16 * floor)
    assert h.time_kernel(15, 3) > 0                                                                 # the timing form leaves the records alone
    assert h.landmark_cov()["rec"].tobytes() == lc["rec"].tobytes()
    # the covariance off for one update: that cloud has no records; on again: it has
    h.set_landmark_cov(False)
    h.set_state(x1, P1)
    h.frame_plan()
    h.update(types, lens, meas)
    assert h.landmarks()["frame"] > lc["frame"] and h.landmark_cov()["n"] == 0 and h.landmark_cov()["frame"] == lc["frame"]
    h.set_landmark_cov(True)
    h.set_state(x1, P1)
    h.frame_plan()
    h.update(types, lens, meas)
    assert h.landmark_cov()["n"] == lc["n"] and h.landmark_cov()["frame"] == h.landmarks()["frame"]
    # every clone the identity, every observation its first: accepted features with rho = 0 stay out, as in the cloud
    xz = x1.copy()
    for c in range((len(xz) - 26) // 7):
        xz[26 + 7 * c: 33 + 7 * c] = [0, 0, 0, 1, 0, 0, 0]
    mz = r["meas"].copy()
    for f in range(len(r["types"])):
        mz[f, : r["lens"][f]] = mz[f, 0]
    h.set_state(xz, P1)
    h.update(r["types"], r["lens"], mz)
    lm, lc, dg = h.landmarks(), h.landmark_cov(), h.update_diag()
    zero = [f for f in range(len(dg["accepted"])) if dg["accepted"][f] and dg["pfinv"][f][2] == 0]
    assert zero and lc["n"] == lm["n"] and not set(zero) & set(lc["rec"]["feat"].tolist())
    # initialize clears and keeps the flag
    h.initialize(np.zeros(3), np.array([0.0, 0.0, 9.81]), 10)
    assert h.landmark_cov()["n"] == 0 and h.landmark_cov()["frame"] == -1
    h.close()


# ---------------------------------------------------------------- the update paths
def image_frames(n):
    cfg = abi.config_named("B", enable_equalizer=1)
    seq = rv.synth.SynthSequence(cfg, duration=(38 + n + 4) / 20.0)
    ks = list(range(39, 39 + n))
    return cfg, seq.init_from_static(38), np.stack([seq.render(k) for k in ks]), [seq.imu_between(k) for k in ks]


@pytest.fixture(scope="module")
def frames():
    return image_frames(24)


def run_frames(d, mode, cov="on"):
    """every frame's (cloud, records) and the final (x, P, odometry ring): the pipelined rvio_hip_frame_dev, stage by stage, or the sharded frame
    at world 1; cov: "on", "never", "on-off" (enabled, then disabled before the first frame), "plain" (no cloud either)"""
    import torch
    from rvio_amd import hip
    cfg, init, imgs, imus = d
    d_imgs = torch.from_numpy(imgs).cuda()
    d_imus = [torch.from_numpy(i.view(np.uint8)).cuda() for i in imus]
    torch.cuda.synchronize()
    h = hip.RvioHip(cfg)
    h.set_odometry(64)
    if cov != "plain":
        h.set_landmarks(True)
    if cov in ("on", "on-off"):
        h.set_landmark_cov(True)
    if cov == "on-off":
        h.set_landmark_cov(False)
    h.initialize(*init)
    out = []
    for i in range(len(imgs)):
        if mode == "staged":
            h.track_dev(d_imgs[i].data_ptr(), cfg.width, d_imus[i].data_ptr(), len(imus[i]), 0, 0)
            h.sync()
            do_update, do_augment = h.frame_plan()
            h.propagate_dev(d_imus[i].data_ptr(), len(imus[i]))
            if do_update:
                h.update_tracked()
            h.augment_compose(do_augment)
        elif mode == "sharded1":
            h.frame_sharded_dev(d_imgs[i].data_ptr(), cfg.width, d_imus[i].data_ptr(), len(imus[i]), 0, 0, 0, 1)
        else:
            h.frame_dev(d_imgs[i].data_ptr(), cfg.width, d_imus[i].data_ptr(), len(imus[i]), 0, 0)
        lm = h.landmarks() if cov != "plain" else None
        lc = h.landmark_cov() if cov == "on" else None
        out.append((lm, lc))
    x, P = h.get_state()
    od = h.odometry(0)
    info = h.frame_info()
    h.close()
    assert info["device_error"] == 0, info
    return out, x, P, od


@pytest.fixture(scope="module")
def frames_on(frames):
    return run_frames(frames, "piped", "on")


def same_cloud(a, b):
    return a["n"] == b["n"] and a["frame"] == b["frame"] and all(np.array_equal(a[k], b[k]) for k in ("feat", "p_r", "p_world"))


def test_pipelined_frame_equals_staged_and_its_records_are_the_twins(gpu_required, frames, frames_on):
    out, x, P, _ = frames_on
    got, x2, P2, _ = run_frames(frames, "staged", "on")
    assert np.array_equal(x, x2) and np.array_equal(P, P2)
    pts = 0
    for (lm, lc), (lm2, lc2) in zip(out, got):
        assert same_cloud(lm, lm2) and lc["frame"] == lm["frame"] and lc["n"] == lm["n"] == lc2["n"]
        assert lc["rec"].tobytes() == lc2["rec"].tobytes()
        assert np.array_equal(lc["rec"]["feat"], lm["feat"]) and np.array_equal(lc["rec"]["p_r"], lm["p_r"])
        assert np.array_equal(lc["rec"]["cov_r"], lc["rec"]["cov_r"].transpose(0, 2, 1)) and (lc["rec"]["status"] == 0).all()
        pts += lc["n"]
    assert pts > 30, pts


def test_sharded_frame_world1_equals_pipelined(gpu_required, frames, frames_on):
    got, _, _, _ = run_frames(frames, "sharded1", "on")
    n = 0
    for (lm, lc), (lm2, lc2) in zip(frames_on[0], got):
        assert lc2["frame"] == lc["frame"] and np.array_equal(lc2["rec"]["feat"], lc["rec"]["feat"])
        assert lc2["n"] == lm2["n"] and np.array_equal(lc2["rec"]["p_r"], lm2["p_r"]) and (lc2["rec"]["status"] == 0).all()
        # (the two paths' states agree to rounding, not bit for bit — tests/test_gpu_landmarks.py holds their points to 1e-9 —, and a covariance
        # follows the state with a sensitivity of the order of cond(N) <= 1e3: 1e-6)
        for j in range(lc["n"]):
            assert K.cov_err(lc2["rec"]["cov_r"][j], lc["rec"]["cov_r"][j]) <= 1e-6 and K.cov_err(lc2["rec"]["cov_w"][j], lc["rec"]["cov_w"][j]) <= 1e-6
        n += lc["n"]
    assert n > 30


@pytest.mark.parametrize("cov", ["never", "on-off", "plain"])
def test_off_means_off_and_on_only_reads(gpu_required, frames, frames_on, cov):
    """(x, P), the cloud and the odometry ring of a free run: a handle that never enables the covariance, one that enables and disables it,
    and a plain handle end bit-identical to the handle that runs it on every update — the kernel only reads"""
    out, x, P, od = frames_on
    got, x2, P2, od2 = run_frames(frames, "piped", cov)
    assert np.array_equal(x, x2) and np.array_equal(P, P2) and od.tobytes() == od2.tobytes() and len(od) >= 20
    if cov != "plain":
        assert all(same_cloud(a[0], b[0]) for a, b in zip(out, got))


def test_free_run_fixture_30_frames_off_means_off(gpu_required):
    from rvio_amd import hip
    g = np.load(os.path.join(GOLD, "ref_free_run_30_frames.npz"))
    cfg = abi.config_named("B", enable_equalizer=0)
    res = []
    for cov in ("plain", "never", "on-off", "on"):
        h = hip.RvioHip(cfg)
        if cov != "plain":
            h.set_landmarks(True)
        if cov in ("on", "on-off"):
            h.set_landmark_cov(True)
        if cov == "on-off":
            h.set_landmark_cov(False)
        h.initialize(g["init_w"], g["init_a"], int(g["init_n"]))
        npts = 0
        for i in range(len(g["ref_xlen"])):
            h.frame_points(g["tracked%d" % i], g["status%d" % i], g["imu%d" % i].view(abi.IMU_DTYPE), g["cand%d" % i])
            if cov == "on":
                lm, lc = h.landmarks(), h.landmark_cov()
                assert lc["n"] == lm["n"] and lc["frame"] == lm["frame"] and np.array_equal(lc["rec"]["p_r"], lm["p_r"])
                npts += lc["n"]
        res.append(h.get_state() + ((h.landmarks() if cov != "plain" else None),))
        h.close()
        assert cov != "on" or npts > 100
    for x, P, lm in res[1:]:
        assert np.array_equal(x, res[0][0]) and np.array_equal(P, res[0][1])
    assert same_cloud(res[1][2], res[2][2]) and same_cloud(res[1][2], res[3][2])


def test_batch_of_three_calibrations_across_the_window_fill_and_dev_getter(gpu_required):
    """a batch handle of 3 instances with three calibrations replays recorded hand-over tables from an empty window through its fill:
    landmark_cov_at(i) = a plain handle's with that calibration (to the rounding of the batch forms); the _dev getter = the host getter, bit for bit"""
    import torch
    from rvio_amd import hip
    cfg = abi.config_named("B", enable_equalizer=0, max_track_len=6)
    _, recs = S.record_sequence(cfg, n_frames=10)
    B, Fu, ML = 3, abi.fu(cfg), cfg.max_track_len
    cals = []
    for i in range(B):
        k = abi.calibration_from_config(cfg)
        ang = 0.002 * i
        Rz = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
        T = np.array(list(cfg.T_bc)).reshape(4, 4)
        T[:3, :3] = Rz @ T[:3, :3]
        T[:3, 3] += 0.002 * i
        for j in range(16):
            k.T_bc[j] = T.ravel()[j]
        cals.append(k)
    hb = hip.RvioHip(cfg, batch=B)
    hp = [hip.RvioHip(cfg) for _ in range(B)]
    hb.set_calibrations(cals)
    for i, h in enumerate(hp):
        h.set_calibration_at(0, cals[i])
    for h in [hb] + hp:
        h.set_landmark_cov(True)
        h.set_state(recs[0]["x0"], recs[0]["P0"])
    d_rec = torch.zeros(B * (Fu + 2) * abi.LANDMARK_COV_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    checked, sides = 0, set()
    for r in recs:
        nf = len(r["lens"])
        types, lens, meas = np.zeros((B, Fu), np.uint8), np.zeros((B, Fu), np.int32), np.zeros((B, Fu, ML, 2), np.float32)
        types[:, :nf], lens[:, :nf], meas[:, :nf] = r["types"], r["lens"], r["meas"]
        imu = r["inp"]["imu"]
        d = [torch.from_numpy(a).cuda() for a in (np.ascontiguousarray(imu).view(np.uint8), np.full(B, nf, np.int32), types, lens, meas)]
        torch.cuda.synchronize()
        hb.frame_tracks_dev(d[0].data_ptr(), 0, len(imu), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr())
        hb.landmark_cov_dev(d_rec.data_ptr(), Fu + 2, d_cnt.data_ptr())
        for h in hp:
            do_update, do_augment = h.frame_plan()
            h.propagate(imu)
            if h is hp[2]:
                pre = h.get_state()                    # the operands of instance 2's update: x-, P- read before it
            if do_update:
                h.update(r["types"], r["lens"], r["meas"])
            h.augment_compose(do_augment)
        hb.sync()
        if not r["did_update"]:
            continue
        sides.add((len(r["x1"]) - 26) // 7 == ML - 1)
        dev = d_rec.cpu().numpy().view(abi.LANDMARK_COV_DTYPE).reshape(B, Fu + 2)
        cnt = d_cnt.cpu().numpy()
        for i in range(B):
            a, b = hb.landmark_cov_at(i), hp[i].landmark_cov()
            assert a["n"] == b["n"] == cnt[i] and a["frame"] == b["frame"], (r["k"], i)
            assert a["rec"].tobytes() == dev[i, : cnt[i]].tobytes(), (r["k"], i)                  # the _dev getter: the host getter's bits
            # a batch handle runs the throughput forms of the per-feature stage: its (phi, psi, rho) and states are a plain handle's to
            # rounding, not bit for bit (tests/test_gpu_landmarks.py holds the points to 1e-12); a covariance follows with cond(N)
            ra, rb = a["rec"], b["rec"]
            assert np.array_equal(ra["feat"], rb["feat"]) and np.array_equal(ra["n_obs"], rb["n_obs"]) and np.array_equal(ra["status"], rb["status"])
            assert np.max(np.abs(ra["p_r"] - rb["p_r"])) <= 1e-12 * max(1.0, np.max(np.abs(rb["p_r"]))) if a["n"] else True
            for j in range(a["n"]):
                assert K.cov_err(ra["cov_r"][j], rb["cov_r"][j]) <= 1e-6 and K.cov_err(ra["cov_w"][j], rb["cov_w"][j]) <= 1e-6, (r["k"], i, j)
            checked += a["n"]
        assert hb.landmark_cov_at(1)["n"] == 0 or hb.landmark_cov_at(1)["rec"].tobytes() != hb.landmark_cov_at(0)["rec"].tobytes()
    # the last update of instance 2 against the twin with ITS calibration
    r = recs[-1]
    lc, dg = hp[2].landmark_cov(), hp[2].update_diag()
    e, floor, _ = against_twin(cals[2], abi.landmark_sigma(cfg), lc["rec"], pre[0], pre[1], r["types"], r["lens"], r["meas"], dg["pfinv"],
                               one_of_each(lc["rec"], r["types"], r["lens"], most=4))
    for h in [hb] + hp:
        h.close()
    print("batch of 3 calibrations: %d records compared, instance 2 e = %.2e (floor %.2e)" % (checked, e, floor))
    assert checked > 30 and sides == {False, True} and e <= (K.BAR if floor < K.FLOOR_BAR else 16 * floor)


class _DA:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}


def test_sharded_ranks_world2_merge_equals_the_plain_handle(gpu_required):
    """two ranks on one GPU (update_local -> the blocks in rank order -> update_global): the ranks' records merged by feat are the plain handle's"""
    import torch
    from rvio_amd import hip
    cfg = abi.config_named("B", enable_equalizer=0)
    _, recs = S.record_sequence(cfg, n_frames=14)
    r = recs[-1]
    types, lens, meas = S.worst_case_tracks(cfg, r, None, n_feat=60)
    hp = hip.RvioHip(cfg)
    hp.set_landmark_cov(True)
    hp.set_state(r["x1"], r["P1"])
    hp.update(types, lens, meas)
    plain = hp.landmark_cov()
    hp.close()
    world = 2
    hs = [hip.RvioHip(cfg) for _ in range(world)]
    blocks = []
    for rk, h in enumerate(hs):
        h.set_landmark_cov(True)
        h.set_state(r["x1"], r["P1"])
        ptr, n = h.update_local(types, lens, meas, rk, world)
        h.sync()
        blocks.append(torch.as_tensor(_DA(ptr, n), device="cuda").clone())
    allb = torch.cat(blocks).contiguous()
    torch.cuda.synchronize()
    for h in hs:
        h.update_global(allb.data_ptr(), world)
    parts = [h.landmark_cov() for h in hs]
    clouds = [h.landmarks() for h in hs]
    for h in hs:
        h.close()
    for rk in range(world):
        assert np.array_equal(parts[rk]["rec"]["feat"], clouds[rk]["feat"]) and (parts[rk]["rec"]["feat"] % world == rk).all()
    merged = np.concatenate([p["rec"] for p in parts])
    merged = merged[np.argsort(merged["feat"], kind="stable")]
    assert plain["n"] >= 40 and merged.tobytes() == plain["rec"].tobytes()
