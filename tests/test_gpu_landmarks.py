"""Updater::update's landmark cloud (Updater.cc:78-87,430-448,458) through the C-ABI (rvio_hip_set_landmarks / rvio_hip_get_landmarks[_at]):
who is in it (gate passed AND rho > 0, hand-over order), where the points are ({Rk} as published; the world frame of the pose file), when a
cloud is published (every update call, also a skipped or empty one), and that every update path — stage by stage, the pipelined frame, batch
handles, feature-sharded ranks — delivers the same cloud."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as O
import ref as R
import scenarios as S

abi, rv = O.abi, O.rv
pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_TOL = 2e-10     # p_r against the reference's own points, relative to max(1, |p|): ~10x the measured worst case (1.9e-11, cfg B, 26 updates)
NUM_TOL = 1e-12     # p_r / p_world against a NumPy rebuild from the device's own operands


def rel_err(a, b):
    a, b = np.asarray(a, float).reshape(-1, 3), np.asarray(b, float).reshape(-1, 3)
    if len(a) == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.linalg.norm(b, axis=1))[:, None]))


def chain_tail(x, typ, length):
    """(R_k, t_k) = mRelPosesToFirst.tail(7) (Updater.cc:114-131), as tests/test_ref_pins.py rebuilds it"""
    nph = int(length) - 1
    rel = x[-7 * nph:] if typ == ord("1") else x[26:26 + 7 * nph]
    qI, tI = rel[0:4].copy(), -O.quat_to_rot(rel[0:4]) @ rel[4:7]
    for i in range(1, nph):
        qi, ti = rel[7 * i:7 * i + 4], rel[7 * i + 4:7 * i + 7]
        tI = O.quat_to_rot(qi) @ (tI - ti)
        qI = O.quat_mul(qi, qI)
    return O.quat_to_rot(qI), tI


def rebuild(cfg, x1, types, lens, diag):
    """(feat, p_r) from the device's accept flags and (phi, psi, rho) and the state the update consumed"""
    T = np.array(list(cfg.T_bc)).reshape(4, 4)
    Ric, tic = T[:3, :3], T[:3, 3]
    feat, pts = [], []
    for f in range(len(diag["accepted"])):
        phi, psi, rho = diag["pfinv"][f]
        if not diag["accepted"][f] or not rho > 0:
            continue
        Rk, tk = chain_tail(x1, types[f], lens[f])
        e = np.array([np.cos(phi) * np.sin(psi), np.sin(phi), np.cos(phi) * np.cos(psi)])
        feat.append(f)
        pts.append(Rk @ (Ric @ (e / rho) + tic) + tk)
    return np.array(feat, np.int32), np.array(pts).reshape(-1, 3)


def world_of(x, p_r):
    return (O.quat_to_rot(x[0:4]).T @ (np.asarray(p_r).reshape(-1, 3) - x[4:7]).T).T


def check_update(cfg, h, x1, types, lens, ref_cloud=None):
    """one update just ran on h from x1: the cloud against the rebuild (and the reference's points); returns the worst reference error"""
    lm, dg = h.landmarks(), h.update_diag()
    x2, _ = h.get_state()
    feat, pts = rebuild(cfg, x1, types, lens, dg)
    assert np.array_equal(lm["feat"], feat) and lm["n"] == len(feat), (lm["feat"], feat)
    assert rel_err(lm["p_r"], pts) <= NUM_TOL, rel_err(lm["p_r"], pts)
    assert rel_err(lm["p_world"], world_of(x2, lm["p_r"])) <= NUM_TOL
    worst = 0.0
    if ref_cloud is not None:
        assert lm["n"] == len(ref_cloud)
        worst = rel_err(lm["p_r"], ref_cloud)
        assert worst <= REF_TOL, worst
    return worst


@pytest.fixture(scope="module")
def recs_b():
    cfg = abi.config_named("B", enable_equalizer=0)
    seq, recs = S.record_sequence(cfg, n_frames=30)
    return cfg, seq, recs


def test_stagewise_against_the_reference(gpu_required, recs_b):
    """every update of a cfg B sequence: feat = the accepted indices with rho > 0, n = the reference's n_cloud, p_r = the reference's points"""
    from rvio_amd import hip
    cfg, _, recs = recs_b
    h = hip.RvioHip(cfg)
    h.set_landmarks(True)
    worst, upd, pts = 0.0, 0, 0
    for r in recs:
        if not r["did_update"]:
            continue
        h.set_state(r["x1"], r["P1"])
        h.update(r["types"], r["lens"], r["meas"])
        _, _, d = R.update(cfg, r["x1"], r["P1"], r["types"], r["lens"], r["meas"])
        worst = max(worst, check_update(cfg, h, r["x1"], r["types"], r["lens"], d["cloud"]))
        upd += 1
        pts += d["n_cloud"]
    h.close()
    print("landmarks vs reference: %d updates, %d points, worst |dp| / max(1, |p|) = %.3e" % (upd, pts, worst))
    assert upd >= 15 and pts > 100


def test_reference_written_fixtures(gpu_required):
    import sys
    from rvio_amd import hip
    sys.path.insert(0, GOLD)
    import golden_io as M
    g, r = np.load(os.path.join(GOLD, "cfgB_direct_seed0_frame30.npz")), np.load(os.path.join(GOLD, "ref_cfgB_direct_seed0_frame30.npz"))
    cfg = abi.config_named("B", enable_equalizer=0)
    h = hip.RvioHip(cfg)
    h.set_landmarks(True)
    h.set_state(g["x1"], g["P1"])
    meas = np.zeros((len(g["lens"]), cfg.max_track_len, 2), np.float32)
    meas[:, : g["meas"].shape[1]] = g["meas"]
    h.update(g["types"], g["lens"], meas)
    check_update(cfg, h, g["x1"], g["types"], g["lens"], r["cloud"])
    h.close()
    gi, go = np.load(os.path.join(GOLD, "full_load_inputs.npz")), np.load(os.path.join(GOLD, "ref_full_load_outputs.npz"))
    for name in ("A", "B", "C", "E"):
        cfg, x1, P1, types, lens, meas = M.load_full_load_case(gi, name)
        h = hip.RvioHip(cfg)
        h.set_landmarks(True)
        h.set_state(x1, P1)
        h.update(types, lens, meas)
        check_update(cfg, h, x1, types, lens)
        assert h.landmarks()["n"] == int(go[name + "_n_cloud"]), name
        h.close()


def test_free_run_fixture_publishes_on_every_updating_frame(gpu_required):
    from rvio_amd import hip
    g = np.load(os.path.join(GOLD, "ref_free_run_30_frames.npz"))
    cfg = abi.config_named("B", enable_equalizer=0)
    h = hip.RvioHip(cfg)
    h.set_landmarks(True)
    h.initialize(g["init_w"], g["init_a"], int(g["init_n"]))
    assert h.landmarks()["frame"] == -1
    x_prev, _ = h.get_state()
    last, n_upd = -1, 0
    for i in range(len(g["ref_xlen"])):
        h.frame_points(g["tracked%d" % i], g["status%d" % i], g["imu%d" % i].view(abi.IMU_DTYPE), g["cand%d" % i])
        lm = h.landmarks()
        updating = (len(x_prev) - 26) // 7 > cfg.min_track_len - 1      # System.cc:266
        if updating:
            assert lm["frame"] == i + 1 and lm["frame"] != last, (i, lm["frame"])
            assert lm["n"] == int(g["ref_n_cloud"][i]), (i, lm["n"], int(g["ref_n_cloud"][i]))
            n_upd += 1
        else:
            assert lm["frame"] == last, i
        last = lm["frame"]
        x_prev, _ = h.get_state()
    h.close()
    assert n_upd >= 20


def test_edges_not_enabled_no_update_initialize(gpu_required, recs_b):
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    h = hip.RvioHip(cfg)
    n, fr = C.c_int32(0), C.c_int32(0)
    assert h.L.rvio_hip_get_landmarks(h.h, C.byref(n), C.byref(fr), None, None, None) == -4         # RVIO_ERR_STATE: never enabled
    assert h.L.rvio_hip_get_landmarks_at(h.h, 1, C.byref(n), C.byref(fr), None, None, None) == -1   # RVIO_ERR_INVALID: no instance 1
    with pytest.raises(hip.RvioHipError):
        h.time_kernel(10, 1)
    h.set_landmarks(True)
    lm = h.landmarks()
    assert lm["n"] == 0 and lm["frame"] == -1
    r = next(r for r in recs if r["did_update"] and len(r["types"]) > 8)
    # too few features: a cloud is published (the publish precedes `if (nGoodFeatCount>2)`, Updater.cc:458-460), nothing is applied
    h.set_state(r["x1"], r["P1"])
    h.frame_plan()
    h.update(r["types"][:3], r["lens"][:3], r["meas"][:3])
    lm, info = h.landmarks(), h.frame_info()
    assert info["updated"] == 0 and lm["frame"] == 1
    _, _, d = R.update(cfg, r["x1"], r["P1"], r["types"][:3], r["lens"][:3], r["meas"][:3])
    assert d["updated"] == 0 and lm["n"] == d["n_cloud"]
    check_update(cfg, h, r["x1"], r["types"][:3], r["lens"][:3], d["cloud"])
    h.frame_plan()
    h.update(r["types"][:2], r["lens"][:2], r["meas"][:2])
    assert h.landmarks()["frame"] == 2
    assert h.time_kernel(10, 5) > 0                                                                  # the timing form leaves the cloud alone
    assert h.landmarks()["frame"] == 2
    # initialize clears the cloud and keeps the flag
    w, a, ni = seq.init_from_static(38)
    h.initialize(w, a, ni)
    lm = h.landmarks()
    assert lm["n"] == 0 and lm["frame"] == -1
    h.set_state(r["x1"], r["P1"])
    h.update(r["types"], r["lens"], r["meas"])
    assert h.landmarks()["frame"] == 0 and h.landmarks()["n"] > 0
    # off again: the next update leaves the last cloud where it is
    h.set_landmarks(False)
    h.frame_plan()
    h.update(r["types"], r["lens"], r["meas"])
    assert h.landmarks()["frame"] == 0
    h.close()


def test_zero_parallax_feature_is_accepted_but_not_in_the_cloud(gpu_required, recs_b):
    """every clone the identity, every observation of a track its first one: the LM stays at rho = 0 (Updater.cc:152), the feature can pass
    the gate and is part of the update, but not of the cloud (rho > 0, Updater.cc:430)"""
    from rvio_amd import hip
    cfg, _, recs = recs_b
    r = next(r for r in recs if r["did_update"] and len(r["types"]) > 8)
    x1 = r["x1"].copy()
    n = (len(x1) - 26) // 7
    for c in range(n):
        x1[26 + 7 * c: 26 + 7 * c + 7] = [0, 0, 0, 1, 0, 0, 0]
    meas = r["meas"].copy()
    for f in range(len(r["types"])):
        meas[f, : r["lens"][f]] = meas[f, 0]
    h = hip.RvioHip(cfg)
    h.set_landmarks(True)
    h.set_state(x1, r["P1"])
    h.update(r["types"], r["lens"], meas)
    dg, lm = h.update_diag(), h.landmarks()
    _, _, d = R.update(cfg, x1, r["P1"], r["types"], r["lens"], meas)
    zero = [f for f in range(len(dg["accepted"])) if dg["accepted"][f] and dg["pfinv"][f][2] == 0]
    print("zero parallax: %d accepted with rho == 0 of %d; reference n_cloud %d" % (len(zero), int(np.sum(dg["accepted"])), d["n_cloud"]))
    assert zero, "no accepted feature with rho == 0"
    assert d["updated"] == 1 and d["n_cloud"] == 0          # the reference, too, accepts features at rho = 0 (> 2 of them: it updates) and publishes none
    assert not set(zero) & set(lm["feat"].tolist())
    assert lm["n"] == d["n_cloud"]
    check_update(cfg, h, x1, r["types"], r["lens"])
    h.close()


# ---------------------------------------------------------------- the pipelined frame
def image_frames(cfg_name, n):
    cfg = abi.config_named(cfg_name, enable_equalizer=1)
    seq = rv.synth.SynthSequence(cfg, duration=(38 + n + 4) / 20.0)
    ks = list(range(39, 39 + n))
    return cfg, seq.init_from_static(38), np.stack([seq.render(k) for k in ks]), [seq.imu_between(k) for k in ks]


def run_frames(d, staged=False, stalls=None, poison=0):
    """each frame's cloud (stamp, feat, p_r, p_world) and the final state: rvio_hip_frame_dev (device detector, CLAHE), or stage by stage with
    the host waiting behind each stage"""
    import torch
    from rvio_amd import hip
    cfg, init, imgs, imus = d
    d_imgs = torch.from_numpy(imgs).cuda()
    d_imus = [torch.from_numpy(i.view(np.uint8)).cuda() for i in imus]
    torch.cuda.synchronize()
    h = hip.RvioHip(cfg)
    h.set_landmarks(True)
    h.initialize(*init)
    rng = np.random.default_rng(stalls) if stalls is not None else None
    out = []
    for i in range(len(imgs)):
        if rng is not None:
            for _ in range(int(rng.integers(0, 3))):
                h.stall(int(rng.integers(0, 4)), int(rng.integers(30, 900)))
        if staged:
            h.track_dev(d_imgs[i].data_ptr(), cfg.width, d_imus[i].data_ptr(), len(imus[i]), 0, 0)
            h.sync()
            do_update, do_augment = h.frame_plan()
            h.propagate_dev(d_imus[i].data_ptr(), len(imus[i]))
            if do_update:
                h.update_tracked()
            h.augment_compose(do_augment)
        else:
            h.frame_dev(d_imgs[i].data_ptr(), cfg.width, d_imus[i].data_ptr(), len(imus[i]), 0, 0)
        lm = h.landmarks()
        out.append((lm["frame"], lm["feat"], lm["p_r"], lm["p_world"]))
        if poison:
            h.poison(poison)
    x, _ = h.get_state()
    info = h.frame_info()
    h.close()
    assert info["device_error"] == 0, info
    return out, x


@pytest.fixture(scope="module", params=[("B", 60), ("C", 30)], ids=["cfgB-60", "cfgC-30-long-window"])
def frames(request):
    return image_frames(*request.param)


@pytest.fixture(scope="module")
def frame_ref(frames):
    return run_frames(frames)


def same_clouds(a, b):
    return len(a) == len(b) and all(p[0] == q[0] and all(np.array_equal(u, v) for u, v in zip(p[1:], q[1:])) for p, q in zip(a, b))


def test_pipelined_equals_staged(gpu_required, frames, frame_ref):
    ref, x_ref = frame_ref
    got, x = run_frames(frames, staged=True)
    assert [c[0] for c in got] == [c[0] for c in ref]
    assert sum(len(c[1]) > 0 for c in ref) >= 5
    assert np.array_equal(x, x_ref)
    assert same_clouds(got, ref)


@pytest.mark.parametrize("stalls,poison", [(3, 0), (None, 7), (5, 7)], ids=["stalls", "poison7", "stalls+poison7"])
def test_pipelined_under_stalls_and_poison(gpu_required, frames, frame_ref, stalls, poison):
    got, x = run_frames(frames, stalls=stalls, poison=poison)
    assert same_clouds(got, frame_ref[0]) and np.array_equal(x, frame_ref[1])


# ---------------------------------------------------------------- batch handles
def tables(cfg, r, keep):
    Fu, ML = abi.fu(cfg), cfg.max_track_len
    nf = len(r["lens"]) if keep is None else min(keep, len(r["lens"]))
    types, lens, meas = np.zeros(Fu, np.uint8), np.zeros(Fu, np.int32), np.zeros((Fu, ML, 2), np.float32)
    types[:nf], lens[:nf], meas[:nf] = r["types"][:nf], r["lens"][:nf], r["meas"][:nf]
    return nf, types, lens, meas


@pytest.mark.parametrize("B", [3, 128])
def test_batch_instances_equal_plain_handles(gpu_required, recs_b, B):
    """instance i replays the recorded hand-over tables cut to the first len / (1 + i % 3) features: landmarks_at(i) = a plain handle's"""
    import torch
    from rvio_amd import hip
    cfg, _, recs = recs_b
    hb = hip.RvioHip(cfg, batch=B)
    hp = [hip.RvioHip(cfg) for _ in range(3)]
    for h in [hb] + hp:
        h.set_landmarks(True)
        h.set_state(recs[0]["x0"], recs[0]["P0"])
    worst, checked = 0.0, 0
    for r in recs:
        per = [tables(cfg, r, None if v == 0 else max(3, len(r["lens"]) // (1 + v))) for v in range(3)]
        pick = [per[i % 3] for i in range(B)]
        n_feat = np.array([p[0] for p in pick], np.int32)
        types, lens, meas = (np.stack([p[k] for p in pick]) for k in (1, 2, 3))
        imu = r["inp"]["imu"]
        d = [torch.from_numpy(a).cuda() for a in (np.ascontiguousarray(imu).view(np.uint8), n_feat, types, lens, meas)]
        torch.cuda.synchronize()
        hb.frame_tracks_dev(d[0].data_ptr(), 0, len(imu), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr())
        for v, h in enumerate(hp):
            do_update, do_augment = h.frame_plan()
            h.propagate(imu)
            if do_update:
                nf = per[v][0]
                h.update(per[v][1][:nf], per[v][2][:nf], per[v][3][:nf])
            h.augment_compose(do_augment)
        hb.sync()
        if not r["did_update"]:
            continue
        plain = [h.landmarks() for h in hp]
        for i in range(B):
            lm, pl = hb.landmarks_at(i), plain[i % 3]
            assert lm["frame"] == pl["frame"] and lm["n"] == pl["n"] and np.array_equal(lm["feat"], pl["feat"]), (r["k"], i)
            worst = max(worst, rel_err(lm["p_r"], pl["p_r"]), rel_err(lm["p_world"], pl["p_world"]))
            if i >= 3:
                ref = hb.landmarks_at(i % 3)
                assert all(np.array_equal(lm[k], ref[k]) for k in ("feat", "p_r", "p_world")), (r["k"], i)
        checked += 1
    for h in [hb] + hp:
        h.close()
    print("batch B=%d: %d updates, worst |dp| / max(1, |p|) vs plain handles = %.3e" % (B, checked, worst))   # measured: 4.9e-13 at B = 3 and 128
    assert checked >= 15 and worst <= NUM_TOL


def test_front_end_batch_equals_plain_handle(gpu_required):
    """a batch handle with front end (B = 3, the same image sequence in every instance) = a plain handle on the images"""
    import torch
    from rvio_amd import hip
    cfg, init, imgs, imus = image_frames("B", 40)
    B = 3
    d_imgs = torch.from_numpy(np.ascontiguousarray(np.repeat(imgs[:, None], B, axis=1))).cuda()
    d_imus = [torch.from_numpy(i.view(np.uint8)).cuda() for i in imus]
    torch.cuda.synchronize()
    hb, h1 = hip.RvioHip(cfg, batch=B, front_end=True), hip.RvioHip(cfg)
    for h in (hb, h1):
        h.set_landmarks(True)
        h.initialize(*init)
    npts, worst = 0, 0.0
    for i in range(len(imgs)):
        hb.frame_batch_dev(d_imgs[i].data_ptr(), cfg.width, cfg.width * cfg.height, d_imus[i].data_ptr(), 0, len(imus[i]))
        h1.frame_dev(d_imgs[i, 0].data_ptr(), cfg.width, d_imus[i].data_ptr(), len(imus[i]), 0, 0)
        pl = h1.landmarks()
        for b in range(B):
            lm = hb.landmarks_at(b)
            assert lm["frame"] == pl["frame"] and np.array_equal(lm["feat"], pl["feat"]), (i, b)
            worst = max(worst, rel_err(lm["p_r"], pl["p_r"]), rel_err(lm["p_world"], pl["p_world"]))
        npts += pl["n"]
    hb.close()
    h1.close()
    assert npts > 50 and worst <= NUM_TOL, (npts, worst)


# ---------------------------------------------------------------- feature-sharded ranks
class _DA:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("load", ["above24", "upto24"])
def test_sharded_ranks(gpu_required, recs_b, world, load):
    """one handle per rank (update_local -> the blocks in rank order -> update_global): each rank's cloud is its documented feature set,
    the union by feat is the plain handle's cloud, p_world is the same on every rank"""
    import torch
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    r = recs[-1]
    assert r["did_update"]
    if load == "above24":
        types, lens, meas = S.worst_case_tracks(cfg, r, seq, n_feat=60)
    else:
        types, lens, meas = r["types"][:20], r["lens"][:20], r["meas"][:20]
    nf = len(types)
    assert (nf > 24) == (load == "above24")
    hp = hip.RvioHip(cfg)
    hp.set_landmarks(True)
    hp.set_state(r["x1"], r["P1"])
    hp.update(types, lens, meas)
    plain = hp.landmarks()
    hp.close()
    assert plain["n"] >= 3
    hs = [hip.RvioHip(cfg) for _ in range(world)]
    blocks = []
    for rk, h in enumerate(hs):
        h.set_landmarks(True)
        h.set_state(r["x1"], r["P1"])
        ptr, n = h.update_local(types, lens, meas, rk, world)
        h.sync()
        blocks.append(torch.as_tensor(_DA(ptr, n), device="cuda").clone())
    allb = torch.cat(blocks).contiguous()
    torch.cuda.synchronize()
    for h in hs:
        h.update_global(allb.data_ptr(), world)
    clouds = [h.landmarks() for h in hs]
    for h in hs:
        h.close()
    for rk, c in enumerate(clouds):
        want = plain["feat"] if nf <= 24 else plain["feat"][plain["feat"] % world == rk]
        assert np.array_equal(c["feat"], want), (rk, c["feat"], want)
        sel = np.isin(plain["feat"], c["feat"])
        assert np.array_equal(c["p_r"], plain["p_r"][sel]), rk                    # the same per-feature kernel on the same state: same bits
        assert rel_err(c["p_world"], plain["p_world"][sel]) <= NUM_TOL, rk
    union = np.unique(np.concatenate([c["feat"] for c in clouds]))
    assert np.array_equal(union, plain["feat"])
    for f in plain["feat"]:                                                      # p_world: the replicated state, the same bits on every rank
        got = [c["p_world"][list(c["feat"]).index(f)] for c in clouds if f in c["feat"]]
        assert all(np.array_equal(g, got[0]) for g in got)


def test_sharded_frame_world1(gpu_required):
    """rvio_hip_frame_sharded_dev at world 1 with comm = NULL: the cloud of the pipelined unsharded frame"""
    import torch
    from rvio_amd import hip
    cfg, init, imgs, imus = image_frames("B", 40)
    d_imgs = torch.from_numpy(imgs).cuda()
    d_imus = [torch.from_numpy(i.view(np.uint8)).cuda() for i in imus]
    torch.cuda.synchronize()
    hs, h1 = hip.RvioHip(cfg), hip.RvioHip(cfg)
    for h in (hs, h1):
        h.set_landmarks(True)
        h.initialize(*init)
    npts, worst = 0, 0.0
    for i in range(len(imgs)):
        hs.frame_sharded_dev(d_imgs[i].data_ptr(), cfg.width, d_imus[i].data_ptr(), len(imus[i]), 0, 0, 0, 1)
        h1.frame_dev(d_imgs[i].data_ptr(), cfg.width, d_imus[i].data_ptr(), len(imus[i]), 0, 0)
        a, b = hs.landmarks(), h1.landmarks()
        assert a["frame"] == b["frame"] and np.array_equal(a["feat"], b["feat"]), i
        worst = max(worst, rel_err(a["p_r"], b["p_r"]), rel_err(a["p_world"], b["p_world"]))
        npts += b["n"]
    hs.close()
    h1.close()
    assert npts > 50 and worst <= 1e-9, (npts, worst)
