"""The odometry ring (rvio_hip_set_odometry / rvio_hip_get_odometry[_all], csrc/odom.hip): one rvio_odom record per instance behind every
augment/compose stage.  What a record holds (the pose line's bits, vk, the velocity block, the propagated pose covariance), that every path
writes the same ring — stage by stage, rvio_hip_frame, rvio_hip_frame_points, batch handles, the long-window branch with its run-ahead
Cholesky —, how the ring wraps, empties and stops, and that a handle with the ring on computes what one without computes.
Settings: cfg B, equaliser off, the recorded direct-track sequences of scenarios.record_sequence."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import scenarios as S

abi, rv = O.abi, O.rv
pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
N = 12


def raw(recs):
    return np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), -1)


def same_bytes(a, b):
    return len(a) == len(b) and np.array_equal(raw(a), raw(b))


def staged_frame(h, inp):
    """one frame of the direct-track sequence stage by stage, the host waiting behind the tracker"""
    h.track_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])
    h.sync()
    do_update, do_augment = h.frame_plan()
    h.propagate(inp["imu"])
    if do_update:
        h.update_tracked()
    h.augment_compose(do_augment)


def check_record(rec, x, P, pose, seq, img_count):
    """the copied fields bit for bit, the covariance within the rounding bound of its two nested six-term sums"""
    p, q = pose
    assert np.array_equal(rec["p"], p) and np.array_equal(rec["q"], q)
    assert np.array_equal(rec["q"], x[0:4])
    assert np.array_equal(rec["v"], x[17:20])
    assert np.array_equal(rec["vel_cov"], P[15:18, 15:18])
    assert int(rec["seq"]) == seq and int(rec["img_count"]) == img_count and int(rec["n_clones"]) == (len(x) - 26) // 7
    assert np.array_equal(rec["reserved"], [0, 0])
    cov = rec["pose_cov"]
    J = np.abs(abi.odom_pose_jacobian(x[0:4], x[4:7]))
    bound = 64 * EPS * (J @ np.abs(P[:6, :6]) @ J.T)
    err = np.abs(cov - abi.odom_pose_cov(x, P))
    worst = float(np.max(err / bound))
    assert np.all(err <= bound), worst
    assert np.array_equal(cov, cov.T)
    assert np.min(np.linalg.eigvalsh(cov)) >= -64 * EPS * np.linalg.norm(cov, 2)
    return worst


@pytest.fixture(scope="module")
def recs_b():
    cfg = abi.config_named("B", enable_equalizer=0)
    seq, recs = S.record_sequence(cfg, n_frames=N)
    return cfg, seq, recs


@pytest.fixture(scope="module")
def staged(gpu_required, recs_b):
    """the 12 frames stage by stage with capacity 16: every frame's newest record, state and pose line, and the ring read once at the end"""
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    h = hip.RvioHip(cfg)
    h.set_odometry(16)
    h.initialize(*seq.init_from_static(38))
    seqno, none = h.odometry_all()
    assert seqno == 0 and len(h.odometry()) == 0 and not raw(none).any()
    per_frame = []
    for k, r in enumerate(recs):
        staged_frame(h, r["inp"])
        newest = h.odometry(first_seq=k + 1)
        assert len(newest) == 1
        seqno, allrec = h.odometry_all()
        assert seqno == k + 1 and same_bytes(allrec, newest)
        per_frame.append((newest[0], h.get_state(), h.get_pose(), h.get_pose_at(0)))
    ring = h.odometry()
    info = h.frame_info()
    h.close()
    assert info["device_error"] == 0 and info["updated"] == 1, info
    return ring, per_frame


def test_bits_and_covariance(staged):
    ring, per_frame = staged
    assert len(ring) == N and [int(s) for s in ring["seq"]] == list(range(1, N + 1))
    worst = 0.0
    for k, (rec, (x, P), pose, pose_at) in enumerate(per_frame):
        assert raw(ring[k:k + 1]).tobytes() == raw(np.array([rec])).tobytes()
        assert np.array_equal(pose[0], pose_at[0]) and np.array_equal(pose[1], pose_at[1])
        worst = max(worst, check_record(rec, x, P, pose, k + 1, k + 1))
    print("pose_cov vs abi.odom_pose_cov: worst |d| / (64 eps |J| |P6| |J|^T) = %.3f over %d frames" % (worst, N))
    assert int(ring["n_clones"][-1]) == 10 and np.any(ring["v"] != 0)


def test_frame_points_pipelined_writes_the_same_ring(staged, recs_b):
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    h = hip.RvioHip(cfg)
    h.set_odometry(16)
    h.initialize(*seq.init_from_static(38))
    for r in recs:
        inp = r["inp"]
        h.frame_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])
    got = h.odometry()
    h.close()
    assert same_bytes(got, staged[0])


def image_run(cfg, init, imgs, imus, piped, cap=16):
    from rvio_amd import hip
    h = hip.RvioHip(cfg)
    h.set_odometry(cap)
    h.initialize(*init)
    for img, imu in zip(imgs, imus):
        if piped:
            h.frame(img, imu)
        else:
            h.track(img, imu)
            h.sync()
            do_update, do_augment = h.frame_plan()
            h.propagate(imu)
            if do_update:
                h.update_tracked()
            h.augment_compose(do_augment)
    got, x = h.odometry(), h.get_state()[0]
    info = h.frame_info()
    h.close()
    assert info["device_error"] == 0, info
    return got, x


def images(cfg, n):
    seq = rv.synth.SynthSequence(cfg, duration=(38 + n + 4) / 20.0)
    ks = list(range(39, 39 + n))
    return seq.init_from_static(38), [seq.render(k) for k in ks], [seq.imu_between(k) for k in ks]


def test_frame_pipelined_writes_the_same_ring(gpu_required):
    """rvio_hip_frame on 12 images with no synchronisation between them = the same images stage by stage, as raw bytes"""
    cfg = abi.config_named("B", enable_equalizer=0)
    init, imgs, imus = images(cfg, N)
    ref, x_ref = image_run(cfg, init, imgs, imus, piped=False)
    got, x = image_run(cfg, init, imgs, imus, piped=True)
    assert len(ref) == N and np.array_equal(x, x_ref)
    assert same_bytes(got, ref)


def test_long_window_run_ahead_cholesky(gpu_required):
    """max_track_len = 20 (6n = 114 > 96): the record launch shares P_out with the Cholesky factor that starts behind evA on its own queue"""
    cfg = abi.config_named("B", enable_equalizer=0, max_track_len=20)
    init, imgs, imus = images(cfg, 25)
    ref, x_ref = image_run(cfg, init, imgs, imus, piped=False, cap=32)
    got, x = image_run(cfg, init, imgs, imus, piped=True, cap=32)
    assert len(ref) == 25 and int(ref["n_clones"][-1]) == 19 and np.array_equal(x, x_ref)
    assert same_bytes(got, ref)


def test_the_ring(staged, recs_b):
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    ref = staged[0]
    h = hip.RvioHip(cfg)
    n, rec = C.c_int32(-1), abi.rvio_odom()
    assert h.L.rvio_hip_get_odometry(h.h, 0, C.c_int64(1), 1, C.byref(rec), C.byref(n)) == -4           # RVIO_ERR_STATE: never enabled
    assert h.L.rvio_hip_get_odometry_all(h.h, C.byref(rec), None) == -4
    with pytest.raises(hip.RvioHipError):
        h.time_kernel(12, 1)
    assert h.L.rvio_hip_set_odometry(h.h, 65537) == -1 and h.L.rvio_hip_set_odometry(h.h, -1) == -1    # RVIO_ERR_INVALID
    h.set_odometry(4)
    assert h.L.rvio_hip_get_odometry(h.h, 1, C.c_int64(1), 1, C.byref(rec), C.byref(n)) == -1           # no instance 1
    assert h.L.rvio_hip_get_odometry(h.h, 0, C.c_int64(1), -1, C.byref(rec), C.byref(n)) == -1
    assert h.L.rvio_hip_get_odometry(h.h, 0, C.c_int64(1), 1, None, C.byref(n)) == -1
    assert h.L.rvio_hip_get_odometry(h.h, 0, C.c_int64(1), 0, None, C.byref(n)) == 0 and n.value == 0

    def feed(lo, hi):
        for r in recs[lo:hi]:
            inp = r["inp"]
            h.frame_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])

    h.initialize(*seq.init_from_static(38))
    feed(0, 11)
    got = h.odometry(first_seq=1)
    assert [int(s) for s in got["seq"]] == [8, 9, 10, 11] and same_bytes(got, ref[7:11])                 # wrapped: slots 3, 0, 1, 2
    assert same_bytes(h.odometry(first_seq=10), ref[9:11])
    assert same_bytes(h.odometry(first_seq=-5, max_n=2), ref[7:9])
    assert len(h.odometry(first_seq=12)) == 0
    assert h.time_kernel(12, 3) > 0 and same_bytes(h.odometry(), ref[7:11])                             # the timing form leaves the ring alone
    # off: the ring no longer advances, the records stay; on again with the same capacity: it goes on
    h.set_odometry(0)
    feed(11, 12)
    assert same_bytes(h.odometry(), ref[7:11]) and h.odometry_all()[0] == 11
    h.set_odometry(4)
    assert same_bytes(h.odometry(), ref[7:11])
    # another capacity empties it; capacity 1 works
    h.set_odometry(1)
    assert len(h.odometry()) == 0 and h.odometry_all()[0] == 0
    h.initialize(*seq.init_from_static(38))
    feed(0, 3)
    got = h.odometry(first_seq=1, max_n=5)
    assert [int(s) for s in got["seq"]] == [3] and np.array_equal(got["p"], ref["p"][2:3]) and np.array_equal(got["pose_cov"], ref["pose_cov"][2:3])
    # initialize restarts at seq 1 and the old records are gone; set_state leaves the ring alone
    h.set_odometry(4)
    h.initialize(*seq.init_from_static(38))
    assert len(h.odometry()) == 0 and h.odometry_all()[0] == 0
    feed(0, 2)
    assert same_bytes(h.odometry(), ref[0:2])
    h.set_state(*h.get_state())
    assert same_bytes(h.odometry(), ref[0:2])
    h.close()
    # a ring beyond 1 GiB is refused with the size in the text
    hb = hip.RvioHip(cfg, batch=40)
    assert hb.L.rvio_hip_set_odometry(hb.h, 65536) == -3 and b"1 GiB" in hb.L.rvio_hip_last_error(hb.h)
    hb.close()


def test_off_is_off(gpu_required, recs_b):
    """two handles on the same frames, one with the ring on: the same states, covariances and tracker tables"""
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    hs = [hip.RvioHip(cfg), hip.RvioHip(cfg)]
    hs[1].set_odometry(8)
    for h in hs:
        h.initialize(*seq.init_from_static(38))
    for r in recs:
        inp = r["inp"]
        for h in hs:
            h.frame_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])
    (xa, Pa), (xb, Pb) = hs[0].get_state(), hs[1].get_state()
    assert np.array_equal(xa, xb) and np.array_equal(Pa, Pb)
    for a, b in zip(hs[0].get_points() + hs[0].get_tracks(), hs[1].get_points() + hs[1].get_tracks()):
        assert np.array_equal(a, b)
    assert len(hs[1].odometry()) == 8
    for h in hs:
        h.close()


# ---------------------------------------------------------------- batch handles
@pytest.fixture(scope="module")
def recs3():
    cfg = abi.config_named("B", enable_equalizer=0)
    return cfg, [S.record_sequence(cfg, n_frames=8, seed=s)[1] for s in (0, 1, 2)]


def own_state_check(hb, B, frame):
    """every instance's newest record against the batch handle's own state and pose line"""
    seqno, allrec = hb.odometry_all()
    assert seqno == frame
    worst = 0.0
    for i in range(B):
        rec = hb.odometry(instance=i, first_seq=frame)
        assert len(rec) == 1 and same_bytes(rec, allrec[i:i + 1]), i
        x, P = hb.get_state_at(i)
        worst = max(worst, check_record(rec[0], x, P, hb.get_pose_at(i), frame, frame))
    return worst


@pytest.mark.parametrize("B", [1, 3, 4, 5])
def test_filter_batch_instances_equal_plain_handles(gpu_required, recs3, B):
    """1, 3, 4 and 5 instances: the edges of four instances per workgroup, a partial last workgroup at 5.  Every instance starts from its own
    state and integrates its own IMU through rvio_hip_frame_tracks_dev for 6 frames; its records are those of a plain handle fed the same
    inputs, as raw bytes.  The hand-over tables are empty (the updates of frames 5 and 6 pass the state through): a batch handle runs other
    forms of three update kernels than a plain handle (tests/test_gpu_batch.py: the same algorithms, another summation grouping, equal to
    rounding only), and equal bytes out need equal bytes in.  Real updates on a batch handle: test_filter_batch_with_updates_against_its_own_state."""
    import torch
    from rvio_amd import hip
    cfg, recs = recs3
    Fu, ML = abi.fu(cfg), cfg.max_track_len
    hb = hip.RvioHip(cfg, batch=B)
    hs = [hip.RvioHip(cfg) for _ in range(B)]
    for h in [hb] + hs:
        h.set_odometry(8)
    hb.set_state(recs[0][0]["x0"], recs[0][0]["P0"])
    for i in range(B):
        x0, P0 = recs[i % 3][0]["x0"].copy(), recs[i % 3][0]["P0"]
        x0[17:20] += 0.01 * (i + 1)                       # instances replaying the same sequence still differ
        hb.set_state_at(i, x0, P0)
        hs[i].set_state(x0, P0)
    zeros = [torch.zeros(s, dtype=t).cuda() for s, t in (((B,), torch.int32), ((B, Fu), torch.uint8), ((B, Fu), torch.int32), ((B, Fu, ML, 2), torch.float32))]
    keep = []
    for f in range(6):
        imus = [recs[i % 3][f]["inp"]["imu"] for i in range(B)]
        m = len(imus[0])
        assert all(len(u) == m for u in imus)
        d_imu = torch.from_numpy(np.stack(imus).view(np.uint8).reshape(B, -1)).cuda()
        keep.append(d_imu)
        torch.cuda.synchronize()
        hb.frame_tracks_dev(d_imu.data_ptr(), m, m, *[z.data_ptr() for z in zeros])
        for i in range(B):
            hs[i].frame_tracks_dev(d_imu[i].data_ptr(), 0, m, *[z.data_ptr() for z in zeros])
    hb.sync()
    seqno, allrec = hb.odometry_all()
    assert seqno == 6
    for i in range(B):
        got, want = hb.odometry(instance=i), hs[i].odometry()
        assert len(want) == 6 and same_bytes(got, want), i
        assert same_bytes(allrec[i:i + 1], want[5:6]), i
        p, q = hb.get_pose_at(i)
        assert np.array_equal(p, got["p"][-1]) and np.array_equal(q, got["q"][-1]), i
        if i:
            assert not np.array_equal(got["p"][-1], hb.odometry(instance=i - 1)["p"][-1])      # the instances really differ
    own_state_check(hb, B, 6)
    assert hb.L.rvio_hip_get_pose_at(hb.h, B, None, None) == -1
    for h in [hb] + hs:
        assert h.frame_info()["device_error"] == 0
        h.close()


def test_filter_batch_with_updates_against_its_own_state(gpu_required, recs3):
    """5 instances on the recorded hand-over tables (updates from frame 5 on): every record holds the bits of ITS instance's pose line and
    state, and the covariance the mirror gives for that state"""
    import torch
    from test_gpu_batch import pack_inputs
    from rvio_amd import hip
    cfg, recs = recs3
    B = 5
    hb = hip.RvioHip(cfg, batch=B)
    hb.set_odometry(4)
    hb.set_state(recs[0][0]["x0"], recs[0][0]["P0"])
    for i in range(B):
        hb.set_state_at(i, recs[i % 3][0]["x0"], recs[i % 3][0]["P0"])
    worst = 0.0
    for f in range(8):
        n_feat, types, lens, meas, imu, m = pack_inputs(cfg, [recs[i % 3][f] for i in range(B)])
        d = [torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda() for a in (imu, n_feat, types, lens, meas)]
        torch.cuda.synchronize()
        hb.frame_tracks_dev(d[0].data_ptr(), m, m, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr())
        hb.sync()
        worst = max(worst, own_state_check(hb, B, f + 1))
    info = hb.frame_info()
    hb.close()
    assert info["updated"] == 1 and info["device_error"] == 0, info
    print("batch of 5, 8 frames: worst |d pose_cov| / bound = %.3f" % worst)


def test_front_end_batch(gpu_required):
    """rvio_hip_frame_batch_dev, 3 camera streams, 6 frames: every record against its instance's own pose line and state; against a plain handle
    on the same stream as raw bytes while no update has run (frames 1 to 4: from the first update on the two filters agree to rounding only,
    tests/test_gpu_batch.py), and to that rounding afterwards"""
    import torch
    from rvio_amd import hip
    cfg = abi.config_named("B", enable_equalizer=0)
    B, n_frames, k0 = 3, 6, 60
    seqs = [rv.synth.SynthSequence(cfg, duration=4.0, seed=s) for s in range(B)]
    hb = hip.RvioHip(cfg, batch=B, front_end=True)
    hs = [hip.RvioHip(cfg) for _ in range(B)]
    for i, q in enumerate(seqs):
        init = q.init_from_static(38)
        hs[i].initialize(*init)
        if i == 0:
            hb.initialize(*init)
        hb.set_state_at(i, *hs[i].get_state())
    for h in [hb] + hs:
        h.set_odometry(8)
    keep = []
    for f in range(n_frames):
        imus = [q.imu_between(k0 + f) for q in seqs]
        m = len(imus[0])
        assert all(len(u) == m for u in imus)
        d_img = torch.from_numpy(np.stack([q.render(k0 + f) for q in seqs])).cuda()
        d_imu = torch.from_numpy(np.stack(imus).view(np.uint8).reshape(B, -1)).cuda()
        keep += [d_img, d_imu]
        torch.cuda.synchronize()
        hb.frame_batch_dev(d_img.data_ptr(), cfg.width, cfg.width * cfg.height, d_imu.data_ptr(), m, m)
        for i in range(B):
            hs[i].frame_dev(d_img[i].data_ptr(), cfg.width, d_imu[i].data_ptr(), m, 0, 0)
        hb.sync()
        own_state_check(hb, B, f + 1)
    for i in range(B):
        hs[i].sync()
        got, want = hb.odometry(instance=i), hs[i].odometry()
        assert len(got) == n_frames == len(want)
        assert same_bytes(got[:4], want[:4]), i
        assert np.array_equal(got["n_clones"], want["n_clones"]) and np.array_equal(got["img_count"], want["img_count"])
        for k in ("p", "q", "v"):
            assert np.max(np.abs(got[k] - want[k])) <= 1e-11, (i, k)
        assert np.max(np.abs(got["pose_cov"] - want["pose_cov"])) <= 1e-11 * np.max(np.abs(want["pose_cov"])), i
    for h in [hb] + hs:
        h.close()
