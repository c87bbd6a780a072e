"""IMU-rate odometry with covariance on the device (csrc/imu_cov.hip; rvio_hip_predict_cov[_dev], rvio_hip_set_imu_odometry_cov /
rvio_hip_get_imu_odometry_cov): the pose_cov / vel_cov an rvio_odom record would carry behind every IMU sample.
  1  rvio_hip_predict_cov / _dev against the oracle's own frame behind every sample (tests/imu_cov_cases.py): max|d| <= 1e-11 max|want| per
     record, exactly symmetric; index / img_count the paired pose record's, seq = 0; the pose records = rvio_hip_predict's bytes.  m = 1, 2, 10:
     inside the kernel's chunk of 32 samples; 63, 64, 65: two chunks, the second one sample short, full, and a third of one sample; 129: four
     chunks and one sample; 193 on the plain handle: the staging grows.
     Batch handles of 1, 3 and 5 instances, shared and per-instance IMU batches, every instance its own state.
  2  record m - 1 against the device's own frame: rvio_odom of propagate + augment_compose(0) on a twin handle.
  3  predict_cov mutates nothing.
  4  the ring on every path that propagates, against a twin's predict_cov_dev in front of every frame; the filter's results, the pose ring and
     the tracker's tables with the covariance ring on = with it off.
  5  ring mechanics: wrap-around, enable mid-run, disable, another capacity, initialize, the timing form.
  6  every error code of the entry points.
The bar is the project's for this quantity (tests/test_gpu_odometry.py); the floor the NumPy model reaches against the same truth is 1.7e-15
(tests/test_imu_cov_abi.py).  Settings: cfg B, equaliser off."""
import ctypes as C

import numpy as np
import pytest

import imu_cov_cases as KC
import imu_pose_cases as K
import oracle as O
import scenarios as S
import test_gpu_imu_odometry as T
from test_gpu_imu_odometry import image_seq, recs_b  # noqa: F401  (fixtures)

abi = O.abi
pytestmark = pytest.mark.gpu
N = T.N
COV_FIELDS = ("index", "pose_cov", "vel_cov")


def cov_buf(n_records, fill=0xAB):
    import torch
    return torch.full((n_records * 376,), fill, dtype=torch.uint8).cuda()


def cov_records(buf):
    return buf.cpu().numpy().view(abi.IMU_COV_DTYPE).copy()


def same_cov_fields(a, b):
    """everything a ring record shares with the predict record of the same sample (seq and img_count differ by design)"""
    return len(a) == len(b) and all(np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes() for f in COV_FIELDS)


def paired(cov, pose):
    return len(cov) == len(pose) and all(np.array_equal(cov[f], pose[f]) for f in ("seq", "img_count", "index"))


_truth = {}


def truth_of(state, bump, m, seed, special):
    """(x, P, imu, (pose_cov, vel_cov) of the oracle) by (state, bump, m, seed, special): computed once, shared by the plain and the batch cases"""
    key = (state, bump, m, seed, special)
    if key not in _truth:
        x, P = K.state(state)
        x = T.bumped(x, bump)
        imu = K.batch(m, seed, special, x)
        _truth[key] = (x, P, imu, KC.oracle_cov_records(x, P, imu))
    return _truth[key]


def check_against_truth(cov, truth, img_count, what):
    m = len(truth[0])
    assert len(cov) == m and np.array_equal(cov["index"], np.arange(m)) and not cov["seq"].any() and np.all(cov["img_count"] == img_count), what
    assert KC.exactly_symmetric(cov), what
    worst = KC.rel_delta(cov, truth)
    print("%s: worst max|d| / max|want| = %.3e" % (what, worst))
    assert worst <= KC.REL_TOL, (what, worst)
    return worst


# ---------------------------------------------------------------- 1. predict_cov against the oracle
@pytest.mark.parametrize("m", KC.MS_GPU + (KC.M_GROW,))
def test_predict_cov_against_oracle_plain_handle(gpu_required, m):
    from rvio_amd import hip
    h = hip.RvioHip(K.config())
    worst = 0.0
    for state in K.STATES:
        for special in ((False, True) if m >= 2 else (False,)):
            x, P, imu, truth = truth_of(state, 0, m, 0, special)
            h.set_state(x, P)
            pose, cov = h.predict_cov(imu)
            worst = max(worst, check_against_truth(cov, truth, 0, (state, m, special)))
            assert T.same_bytes(pose, h.predict(imu))                                 # the pose records are rvio_hip_predict's
            none, cov2 = h.predict_cov(imu, poses=False)                              # covariances only: the same bytes
            assert none is None and T.same_bytes(cov2, cov)
            if special and m > 2:
                # dt = 0 in sample m - 2: Phi = I, Q = 0, the pose stays — its record is the one before it, to rounding
                for f in ("pose_cov", "vel_cov"):
                    assert np.max(np.abs(cov[f][m - 2] - cov[f][m - 3])) <= 1e-13 * np.max(np.abs(cov[f][m - 3])), (state, f)
    h.frame_plan()
    assert np.all(h.predict_cov(imu)[1]["img_count"] == 1)
    h.close()
    print("predict_cov, plain handle, m = %d: worst = %.3e" % (m, worst))


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("m", KC.MS_GPU)
def test_predict_cov_dev_against_oracle_batch_handles(gpu_required, m, B):
    import torch
    from rvio_amd import hip
    cfg = K.config()
    hb = hip.RvioHip(cfg, batch=B)
    names = ["window10", "moved", "window10", "moved", "window10"]     # 10 clones each (one window length per handle); 'moved': qk, pk non-trivial
    hb.set_state(*K.state("window10"))
    for stride in (0, m + 3):
        cases = []
        for i in range(B):
            special = (i == 1 and m >= 2)
            cases.append(truth_of(names[i], i, m, i if stride else 0, special and bool(stride)))
            hb.set_state_at(i, cases[i][0], cases[i][1])
        if stride:
            imus = np.zeros((B, stride), abi.IMU_DTYPE)
            for i in range(B):
                imus[i, :m] = cases[i][2]
            imus[:, m:]["dt"] = np.nan                                   # a kernel that read past m would show
        else:
            imus = cases[0][2]
        d_imu = T.dev(imus)
        os_, cs = m + 2, m + 1
        d_out, d_ref, d_cov, d_cov2 = T.out_buf(B * os_), T.out_buf(B * os_), cov_buf(B * cs), cov_buf(B * cs)
        torch.cuda.synchronize()
        hb.predict_cov_dev(d_imu.data_ptr(), stride, m, d_out.data_ptr(), os_, d_cov.data_ptr(), cs)
        hb.predict_dev(d_imu.data_ptr(), stride, m, d_ref.data_ptr(), os_)
        hb.predict_cov_dev(d_imu.data_ptr(), stride, m, None, 0, d_cov2.data_ptr(), cs)
        hb.sync()
        assert np.array_equal(d_out.cpu().numpy(), d_ref.cpu().numpy())           # every pose record, and the bytes around them
        assert np.array_equal(d_cov.cpu().numpy(), d_cov2.cpu().numpy())
        got = cov_records(d_cov).reshape(B, cs)
        for i in range(B):
            check_against_truth(got[i, :m], cases[i][3], 0, (B, m, stride, i))
            assert np.all(T.raw(got[i, m:]) == 0xAB), (stride, i)                  # nothing beyond record m - 1
            assert T.same_bytes(hb.predict_cov(cases[i][2], instance=i)[1], got[i, :m]), (stride, i)   # the host-buffer entry point: the same bytes
        if B > 1:
            assert not np.array_equal(got[0, :m]["pose_cov"], got[1, :m]["pose_cov"])
    hb.close()


# ---------------------------------------------------------------- 2. the last record against the device's own frame
@pytest.mark.parametrize("m", [1, 10, 17, 65])
def test_last_record_against_the_devices_own_frame(gpu_required, m):
    from rvio_amd import hip
    h, twin = hip.RvioHip(K.config()), hip.RvioHip(K.config())
    twin.set_odometry(4)
    for state in K.STATES:
        x, P = K.state(state)
        imu = K.batch(m, 2, special=(m >= 2), x=x)
        h.set_state(x, P)
        twin.set_state(x, P)
        pose, cov = h.predict_cov(imu)
        twin.propagate(imu)
        twin.augment_compose(False)
        od = twin.odometry()[-1]
        assert np.array_equal(pose[-1]["p"], od["p"]) and np.array_equal(pose[-1]["q"], od["q"]) and np.array_equal(pose[-1]["v"], od["v"])
        for f in ("pose_cov", "vel_cov"):
            d = float(np.max(np.abs(cov[-1][f] - od[f]))) / float(np.max(np.abs(od[f])))
            print("m = %d, %s, %s: max|d| / max|want| against rvio_odom = %.3e" % (m, state, f, d))
            assert d <= KC.REL_TOL, (state, f, d)
    h.close()
    twin.close()


# ---------------------------------------------------------------- 3. no side effect
def snapshot(h):
    s = T.snapshot(h)
    s["imuc"] = h.get_imu_odometry_cov()
    return s


def same_snapshot(a, b):
    return T.same_snapshot(a, b) and T.same_bytes(a["imuc"], b["imuc"])


def test_predict_cov_has_no_side_effect(gpu_required, recs_b):
    import torch
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    hs = [hip.RvioHip(cfg), hip.RvioHip(cfg)]
    for h in hs:
        h.set_odometry(16)
        h.set_imu_odometry(64)
        h.set_imu_odometry_cov(1)
        h.initialize(*seq.init_from_static(38))
        for r in recs[:7]:
            T.feed_points(h, r)
    imu = recs[7]["inp"]["imu"]
    m = len(imu)
    before = snapshot(hs[0])
    assert before["info"]["updated"] == 1 and len(before["imuo"]) == 64 and len(before["imuc"]) == 64 and paired(before["imuc"], before["imuo"])
    pose, cov = hs[0].predict_cov(imu)
    d_imu, d_out, d_cov = T.dev(imu), T.out_buf(m), cov_buf(m)
    torch.cuda.synchronize()
    hs[0].predict_cov_dev(d_imu.data_ptr(), 0, m, d_out.data_ptr(), m, d_cov.data_ptr(), m)
    hs[0].sync()
    assert T.same_bytes(T.records(d_out), pose) and T.same_bytes(cov_records(d_cov), cov) and np.all(cov["img_count"] == 7)
    assert same_snapshot(before, snapshot(hs[0]))
    # a following propagate gives the bits it gives without the predict (the twin never predicted), in the state and in both rings
    for h in hs:
        h.frame_plan()
        h.propagate(imu)
    (xa, Pa), (xb, Pb) = hs[0].get_state(), hs[1].get_state()
    assert np.array_equal(xa, xb) and np.array_equal(Pa, Pb)
    assert T.same_bytes(hs[0].get_imu_odometry(), hs[1].get_imu_odometry()) and T.same_bytes(hs[0].get_imu_odometry_cov(), hs[1].get_imu_odometry_cov())
    assert same_cov_fields(hs[0].get_imu_odometry_cov(first_seq=71), cov)            # what was predicted is what the ring then recorded
    for h in hs:
        h.close()


# ---------------------------------------------------------------- 4. the ring on every path
def check_cov_ring_against_twin(ring, pose_ring, preds, ms, what):
    total = sum(ms)
    assert len(ring) == total and [int(s) for s in ring["seq"]] == list(range(1, total + 1)), what
    assert paired(ring, pose_ring), what
    assert KC.exactly_symmetric(ring), what
    lo = 0
    for k, m in enumerate(ms):
        part = ring[lo:lo + m]
        assert np.all(part["img_count"] == k + 1), (what, k)
        assert same_cov_fields(part, preds[k]), (what, k)
        lo += m


@pytest.mark.parametrize("path", ["staged", "frame_dev", "frame", "frame_points", "frame_begin_end", "frame_sharded"])
def test_cov_ring_on_every_plain_path(gpu_required, recs_b, image_seq, path):
    import torch
    on, off = T.PlainPath(path, True, recs_b, image_seq), T.PlainPath(path, False, recs_b, image_seq)
    on.h.set_imu_odometry_cov(1)
    preds, drained, keep = [], [], []
    for k in range(N):
        # the twin (rings off) predicts in front of its frame k, behind its frame k - 1
        imu = off.imu(k)
        d_imu, d_cov = T.dev(imu), cov_buf(len(imu))
        keep.append(d_imu)
        torch.cuda.synchronize()
        off.h.predict_cov_dev(d_imu.data_ptr(), 0, len(imu), None, 0, d_cov.data_ptr(), len(imu))
        preds.append(d_cov)
        for r in (on, off):
            r.frame(k)
        if k in (5, N - 1):
            drained.append(on.h.get_imu_odometry_cov(first_seq=1 + sum(len(d) for d in drained)))
    ms = [len(on.imu(k)) for k in range(N)]
    odom = on.h.odometry()
    a, b = on.finish(), off.finish()
    assert a["info"]["device_error"] == 0 and b["info"]["device_error"] == 0 and a["info"]["updated"] == 1
    ring = np.concatenate(drained)
    check_cov_ring_against_twin(ring, a["ring"], [cov_records(p) for p in preds], ms, path)
    assert np.array_equal(a["state"][0], b["state"][0]) and np.array_equal(a["state"][1], b["state"][1])
    # frames without an update: the batch's last record carries that frame's rvio_odom covariances, to the bar
    ends = np.cumsum(ms) - 1
    for k in range(4):
        for f in ("pose_cov", "vel_cov"):
            d = float(np.max(np.abs(ring[ends[k]][f] - odom[k][f]))) / float(np.max(np.abs(odom[k][f])))
            assert d <= KC.REL_TOL, (path, k, f, d)


@pytest.mark.parametrize("kind", ["frame_tracks", "frame_batch"])
def test_cov_ring_on_batch_paths(gpu_required, image_seq, kind):
    """B = 3, per-instance IMU batches: rvio_hip_frame_tracks_dev on the recorded hand-over tables of three sequences (the overlapped propagate on
    the second stream from frame 5 on) and rvio_hip_frame_batch_dev on three copies of one camera stream with their own velocities and accelerometers"""
    import torch
    from rvio_amd import hip
    cfg = K.config()
    B = 3
    if kind == "frame_tracks":
        recs = [S.record_sequence(cfg, n_frames=N, seed=s)[1] for s in range(B)]
        hs = [hip.RvioHip(cfg, batch=B) for _ in range(2)]
        for h in hs:
            h.set_state(recs[0][0]["x0"], recs[0][0]["P0"])
            for i in range(B):
                h.set_state_at(i, recs[i][0]["x0"], recs[i][0]["P0"])
        imus_of = lambda k: [recs[i][k]["inp"]["imu"] for i in range(B)]
    else:
        init, imgs, imus_img = image_seq
        hs = [hip.RvioHip(cfg, batch=B, front_end=True) for _ in range(2)]
        for h in hs:
            h.initialize(*init)
            x0, P0 = h.get_state()
            for i in range(B):
                xi = x0.copy()
                xi[17:20] += 1e-3 * i
                h.set_state_at(i, xi, P0)

        def imus_of(k):
            out = [imus_img[k].copy() for _ in range(B)]
            for i in range(B):
                out[i]["a"] += 1e-3 * i
            return out
    hs[0].set_imu_odometry(64)
    hs[0].set_imu_odometry_cov(1)
    keep, preds, ms, drained, drained_p = [], [], [], [[] for _ in range(B)], [[] for _ in range(B)]
    for k in range(N):
        imus = imus_of(k)
        m = len(imus[0])
        ms.append(m)
        d_imu, d_cov = T.dev(np.stack(imus)), cov_buf(B * m)
        if kind == "frame_tracks":
            d = [torch.from_numpy(a).cuda() for a in T.pack_tracks(cfg, [recs[i][k] for i in range(B)])]
        else:
            d = [torch.from_numpy(np.stack([imgs[k]] * B)).cuda()]
        keep += [d_imu, d_cov] + d
        torch.cuda.synchronize()
        hs[1].predict_cov_dev(d_imu.data_ptr(), m, m, None, 0, d_cov.data_ptr(), m)
        preds.append(d_cov)
        for h in hs:
            if kind == "frame_tracks":
                h.frame_tracks_dev(d_imu.data_ptr(), m, m, *[t.data_ptr() for t in d])
            else:
                h.frame_batch_dev(d[0].data_ptr(), cfg.width, cfg.width * cfg.height, d_imu.data_ptr(), m, m)
        if k in (5, N - 1):
            for i in range(B):
                first = 1 + sum(len(d_) for d_ in drained[i])
                drained[i].append(hs[0].get_imu_odometry_cov(instance=i, first_seq=first))
                drained_p[i].append(hs[0].get_imu_odometry(instance=i, first_seq=first))
    for h in hs:
        h.sync()
    for i in range(B):
        ring = np.concatenate(drained[i])
        pred = [cov_records(b).reshape(B, m)[i] for b, m in zip(preds, ms)]
        check_cov_ring_against_twin(ring, np.concatenate(drained_p[i]), pred, ms, (kind, i))
        xa, xb = hs[0].get_state_at(i), hs[1].get_state_at(i)
        assert np.array_equal(xa[0], xb[0]) and np.array_equal(xa[1], xb[1]), i
        if i:
            assert not np.array_equal(ring["pose_cov"], np.concatenate(drained[i - 1])["pose_cov"])
    info = hs[0].frame_info()
    assert info["updated"] == 1 and info["device_error"] == 0, info
    for h in hs:
        h.close()


@pytest.fixture(scope="module")
def full_run(gpu_required, recs_b):
    """the 12 direct-track frames with rings that hold all of them, the covariance ring on and off: records, state, tracker tables"""
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    out = []
    for with_cov in (True, False):
        h = hip.RvioHip(cfg)
        h.set_imu_odometry(256)
        if with_cov:
            h.set_imu_odometry_cov(1)
        h.initialize(*seq.init_from_static(38))
        for r in recs:
            T.feed_points(h, r)
        out.append(dict(pose=h.get_imu_odometry(), cov=h.get_imu_odometry_cov() if with_cov else None, state=h.get_state(), pts=h.get_points(), info=h.frame_info()))
        h.close()
    return out


def test_cov_ring_changes_nothing_else(full_run):
    on, off = full_run
    assert len(on["cov"]) == 120 and paired(on["cov"], on["pose"]) and KC.exactly_symmetric(on["cov"])
    assert np.array_equal(on["state"][0], off["state"][0]) and np.array_equal(on["state"][1], off["state"][1])
    assert T.same_bytes(on["pose"], off["pose"]) and on["info"] == off["info"]
    assert all(np.array_equal(u, v) for u, v in zip(on["pts"], off["pts"]))
    # the covariance grows along a frame's samples and the record behind a frame's last sample is positive definite
    assert np.all(np.linalg.eigvalsh(on["cov"]["pose_cov"]) > 0)


# ---------------------------------------------------------------- 5. ring mechanics
def test_cov_ring_mechanics(full_run, recs_b):
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    ref = full_run[0]["cov"]
    h = hip.RvioHip(cfg)

    def feed(lo, hi):
        for r in recs[lo:hi]:
            T.feed_points(h, r)

    h.set_imu_odometry(25)
    h.initialize(*seq.init_from_static(38))
    feed(0, 2)
    # enabled mid-run: only the records from then on are returned, under the pose ring's seq
    h.set_imu_odometry_cov(1)
    assert len(h.get_imu_odometry_cov()) == 0 and len(h.get_imu_odometry()) == 20
    feed(2, 3)
    got = h.get_imu_odometry_cov()
    assert [int(s) for s in got["seq"]] == list(range(21, 31)) and T.same_bytes(got, ref[20:30])
    assert T.same_bytes(h.get_imu_odometry_cov(first_seq=5, max_n=3), ref[20:23]) and len(h.get_imu_odometry_cov(first_seq=31)) == 0
    # wrap-around: 40 more samples through 25 slots
    feed(3, 7)
    got = h.get_imu_odometry_cov()
    assert [int(s) for s in got["seq"]] == list(range(46, 71)) and T.same_bytes(got, ref[45:70]) and paired(got, h.get_imu_odometry())
    # disable keeps the records while the pose ring goes on; enabling again serves what is recorded from then on
    h.set_imu_odometry_cov(0)
    feed(7, 8)
    assert T.same_bytes(h.get_imu_odometry_cov(), got) and int(h.get_imu_odometry()["seq"][-1]) == 80
    h.set_imu_odometry_cov(1)
    assert len(h.get_imu_odometry_cov()) == 0
    feed(8, 9)
    got2 = h.get_imu_odometry_cov()
    assert [int(s) for s in got2["seq"]] == list(range(81, 91)) and T.same_bytes(got2, ref[80:90])
    # the timing form writes a buffer of its own
    pose2 = h.get_imu_odometry()
    assert h.time_kernel(14, 3) > 0 and T.same_bytes(h.get_imu_odometry_cov(), got2) and T.same_bytes(h.get_imu_odometry(), pose2)
    # set_state and poison leave both rings alone
    h.set_state(*h.get_state())
    h.poison(7)
    assert T.same_bytes(h.get_imu_odometry_cov(), got2)
    # another capacity empties both rings and restarts seq (on a filter that goes on)
    h.set_imu_odometry(40)
    assert len(h.get_imu_odometry_cov()) == 0 and len(h.get_imu_odometry()) == 0
    feed(9, 10)
    got3 = h.get_imu_odometry_cov()
    assert [int(s) for s in got3["seq"]] == list(range(1, 11)) and same_cov_fields(got3, ref[90:100]) and paired(got3, h.get_imu_odometry())
    # initialize empties both rings
    h.initialize(*seq.init_from_static(38))
    assert len(h.get_imu_odometry_cov()) == 0 and len(h.get_imu_odometry()) == 0
    feed(0, 2)
    assert T.same_bytes(h.get_imu_odometry_cov(), ref[:20])
    # the pose ring off stops both
    h.set_imu_odometry(0)
    feed(2, 3)
    assert T.same_bytes(h.get_imu_odometry_cov(), ref[:20])
    h.close()


# ---------------------------------------------------------------- 6. errors
def test_errors(gpu_required, recs_b):
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    INVALID, UNSUPPORTED, STATE = -1, -3, -4
    imu = recs[0]["inp"]["imu"]
    m = len(imu)
    ip = imu.ctypes.data_as(C.POINTER(abi.rvio_imu))
    out, cov = np.zeros(m, abi.IMU_POSE_DTYPE), np.zeros(m, abi.IMU_COV_DTYPE)
    op, cp = out.ctypes.data_as(C.POINTER(abi.ImuPose)), cov.ctypes.data_as(C.POINTER(abi.ImuCov))
    d_imu, d_out, d_cov = T.dev(imu), T.out_buf(m), cov_buf(m)
    vp = C.c_void_p
    n = C.c_int32(-1)
    us = C.c_float(0)
    h = hip.RvioHip(cfg, batch=2)
    L = h.L
    a = (vp(d_imu.data_ptr()), vp(d_out.data_ptr()), vp(d_cov.data_ptr()))
    # before the first state
    assert L.rvio_hip_predict_cov(h.h, 0, ip, m, op, cp) == STATE and b"rvio_hip_set_state" in L.rvio_hip_last_error(h.h)
    assert L.rvio_hip_predict_cov_dev(h.h, a[0], 0, m, a[1], m, a[2], m) == STATE
    # the covariance ring before the IMU-rate ring, the getter before the covariance ring
    assert L.rvio_hip_set_imu_odometry_cov(h.h, 1) == STATE and b"rvio_hip_set_imu_odometry" in L.rvio_hip_last_error(h.h)
    assert L.rvio_hip_set_imu_odometry_cov(h.h, 0) == 0
    assert L.rvio_hip_get_imu_odometry_cov(h.h, 0, C.c_int64(1), 1, cp, C.byref(n)) == STATE
    assert L.rvio_hip_debug_time_kernel(h.h, 14, 1, C.byref(us)) == UNSUPPORTED
    h.set_state(recs[0]["x0"], recs[0]["P0"])
    # predict_cov: cov must not be NULL, out may be
    assert L.rvio_hip_predict_cov(h.h, 2, ip, m, op, cp) == INVALID and L.rvio_hip_predict_cov(h.h, -1, ip, m, op, cp) == INVALID
    assert L.rvio_hip_predict_cov(h.h, 0, ip, -1, op, cp) == INVALID and L.rvio_hip_predict_cov(h.h, 0, None, m, op, cp) == INVALID
    assert L.rvio_hip_predict_cov(h.h, 0, ip, m, op, None) == INVALID and L.rvio_hip_predict_cov(h.h, 0, ip, m, None, cp) == 0
    assert L.rvio_hip_predict_cov(h.h, 1, None, 0, None, None) == 0
    # predict_cov_dev: strides >= m; imu_stride 0 or >= m; m == 0 writes nothing
    assert L.rvio_hip_predict_cov_dev(h.h, a[0], 0, m, a[1], m - 1, a[2], m) == INVALID and L.rvio_hip_predict_cov_dev(h.h, a[0], 0, m, a[1], m, a[2], m - 1) == INVALID
    assert L.rvio_hip_predict_cov_dev(h.h, a[0], m - 1, m, a[1], m, a[2], m) == INVALID and L.rvio_hip_predict_cov_dev(h.h, a[0], -1, m, a[1], m, a[2], m) == INVALID
    assert L.rvio_hip_predict_cov_dev(h.h, a[0], 0, -1, a[1], m, a[2], m) == INVALID
    assert L.rvio_hip_predict_cov_dev(h.h, None, 0, m, a[1], m, a[2], m) == INVALID and L.rvio_hip_predict_cov_dev(h.h, a[0], 0, m, a[1], m, None, m) == INVALID
    assert L.rvio_hip_predict_cov_dev(h.h, None, 0, 0, None, 0, None, 0) == 0
    h.sync()
    assert np.all(d_out.cpu().numpy() == 0xAB) and np.all(d_cov.cpu().numpy() == 0xAB)
    # the ring's setter and getter
    h.set_imu_odometry(4)
    assert L.rvio_hip_set_imu_odometry_cov(h.h, 2) == INVALID and L.rvio_hip_set_imu_odometry_cov(h.h, -1) == INVALID
    assert L.rvio_hip_get_imu_odometry_cov(h.h, 0, C.c_int64(1), 1, cp, C.byref(n)) == STATE            # the pose ring alone does not make one
    assert L.rvio_hip_debug_time_kernel(h.h, 14, 1, C.byref(us)) == UNSUPPORTED                          # the covariance ring is off
    h.set_imu_odometry_cov(1)
    assert L.rvio_hip_get_imu_odometry_cov(h.h, 2, C.c_int64(1), 1, cp, C.byref(n)) == INVALID
    assert L.rvio_hip_get_imu_odometry_cov(h.h, 0, C.c_int64(1), -1, cp, C.byref(n)) == INVALID
    assert L.rvio_hip_get_imu_odometry_cov(h.h, 0, C.c_int64(1), 1, None, C.byref(n)) == INVALID
    assert L.rvio_hip_get_imu_odometry_cov(h.h, 0, C.c_int64(1), 0, None, C.byref(n)) == 0 and n.value == 0
    assert L.rvio_hip_get_imu_odometry_cov(h.h, 1, C.c_int64(1), 4, cp, C.byref(n)) == 0 and n.value == 0   # enabled, nothing recorded yet
    assert L.rvio_hip_debug_time_kernel(h.h, 14, 1, C.byref(us)) == UNSUPPORTED                          # ... and no frame has propagated
    h.set_imu_odometry_cov(0)
    h.propagate(imu)
    assert L.rvio_hip_debug_time_kernel(h.h, 13, 1, C.byref(us)) == 0
    assert L.rvio_hip_debug_time_kernel(h.h, 14, 1, C.byref(us)) == UNSUPPORTED                          # a frame has propagated, the covariance ring is off
    h.close()
    # a covariance ring beyond 1 GiB is refused with the size in the text: 524288 x 11 x 376 bytes (its pose ring, 572 MB, is accepted)
    hb = hip.RvioHip(cfg, batch=11)
    hb.set_imu_odometry(1048576 // 2)
    assert hb.L.rvio_hip_set_imu_odometry_cov(hb.h, 1) == UNSUPPORTED
    msg = hb.L.rvio_hip_last_error(hb.h)
    assert b"1 GiB" in msg and str(524288 * 11 * 376).encode() in msg, msg
    assert hb.L.rvio_hip_get_imu_odometry_cov(hb.h, 0, C.c_int64(1), 1, cp, C.byref(n)) == STATE
    # ... and so is a capacity change that would take an existing covariance ring there: both rings stay as they are
    hb.set_imu_odometry(1024)
    hb.set_imu_odometry_cov(1)
    assert hb.L.rvio_hip_set_imu_odometry(hb.h, 1048576 // 2) == UNSUPPORTED and b"1 GiB" in hb.L.rvio_hip_last_error(hb.h)
    hb.set_state(recs[0]["x0"], recs[0]["P0"])
    hb.propagate(imu)
    assert len(hb.get_imu_odometry_cov(instance=10, max_n=1024)) == m and len(hb.get_imu_odometry(instance=10, max_n=1024)) == m
    hb.close()
