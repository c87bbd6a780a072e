"""IMU-rate odometry on the device (csrc/imu_pose.hip; rvio_hip_predict[_dev], rvio_hip_set_imu_odometry / rvio_hip_get_imu_odometry): a pose
behind every IMU sample.
  1  rvio_hip_predict / rvio_hip_predict_dev against oracle prefix propagation (tests/imu_pose_cases.py), |d| <= 1e-9 on p, q, v; t, index,
     img_count exact, seq = 0.  m = 63 / 64 / 65: the wave's chunk boundary; m = 200: the host staging grows.  Batch handles of 1, 3 and 5
     instances (5: a second, partly filled workgroup), shared and per-instance IMU batches, every instance its own state.
  2  predict mutates nothing: state, frame info, tracker points and both rings before = after, and a following propagate gives the same bits.
  3  record m - 1 carries the bits of the device's own propagate (v) and of the pose line behind propagate + augment_compose(0) (p, q).
  4  the ring on every path that propagates: seq without a gap, img_count / index partition the records into the frames' batches, every
     frame's records = a predict_dev issued just before that frame on a twin handle driven in lock-step with the ring off, the last record of a
     frame without an update = that frame's pose line (and rvio_odom record), frames with the fused per-feature + propagate launch among them.
  5  ring mechanics: a batch longer than the ring, wrapping, re-enable, another capacity, initialize, set_state, poison, capacity 0; the
     filter's results with the ring on = with it off, also with poison between the frames and stalls sprinkled over the filter stream.
  6  every error code of the entry points.
Settings: cfg B, equaliser off."""
import ctypes as C

import numpy as np
import pytest

import imu_pose_cases as K
import oracle as O
import scenarios as S

abi, rv = O.abi, O.rv
pytestmark = pytest.mark.gpu
N = 12
FIELDS = ("t", "index", "p", "q", "v")


def raw(recs):
    return np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), -1)


def same_bytes(a, b):
    return len(a) == len(b) and np.array_equal(raw(a), raw(b))


def same_pose_fields(a, b):
    """everything a ring record shares with the predict record of the same sample (seq and img_count differ by design)"""
    return len(a) == len(b) and all(np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes() for f in FIELDS)


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def out_buf(n_records, fill=0xAB):
    import torch
    return torch.full((n_records * 104,), fill, dtype=torch.uint8).cuda()


def records(buf):
    return buf.cpu().numpy().view(abi.IMU_POSE_DTYPE).copy()


def bumped(x, i):
    """instance i's own state: another velocity, other biases"""
    x = x.copy()
    x[17:20] += 0.01 * i
    x[20:23] += 1e-4 * i
    x[23:26] -= 2e-3 * i
    return x


@pytest.fixture(scope="module")
def truth_cache():
    """oracle records by (state, bump, m, seed, special): computed once, shared by the plain and the batch cases"""
    cache = {}

    def get(state, bump, m, seed, special):
        key = (state, bump, m, seed, special)
        if key not in cache:
            x, P = K.state(state)
            x = bumped(x, bump)
            imu = K.batch(m, seed, special, x)
            cache[key] = (x, P, imu, K.oracle_records(x[:26], P[:24, :24], imu))
        return cache[key]
    return get


def check_against_truth(rec, imu, truth, img_count, what):
    m = len(imu)
    assert len(rec) == m
    assert np.array_equal(rec["t"], imu["t"]) and np.array_equal(rec["index"], np.arange(m)), what
    assert not rec["seq"].any() and np.all(rec["img_count"] == img_count), what
    worst = K.worst_delta(rec, truth)
    assert worst <= K.X_TOL, (what, worst)
    return worst


# ---------------------------------------------------------------- 1. predict against the oracle
@pytest.mark.parametrize("m", K.MS_GPU)
def test_predict_against_oracle_plain_handle(gpu_required, truth_cache, m):
    from rvio_amd import hip
    h = hip.RvioHip(K.config())
    worst = 0.0
    for state in K.STATES:
        for special in ((False, True) if m >= 2 else (False,)):
            x, P, imu, truth = truth_cache(state, 0, m, 0, special)
            h.set_state(x, P)
            rec = h.predict(imu)
            worst = max(worst, check_against_truth(rec, imu, truth, 0, (state, special)))
            assert same_bytes(rec, h.predict(imu))                                   # the staging, once grown, gives the same bytes again
    # the handle's current frame count is what a predict record carries
    h.frame_plan()
    h.frame_plan()
    assert np.all(h.predict(imu)["img_count"] == 2)
    h.close()
    print("predict, plain handle, m = %d: worst |d| vs oracle prefix propagation = %.3e" % (m, worst))


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("m", K.MS_GPU)
def test_predict_dev_against_oracle_batch_handles(gpu_required, truth_cache, m, B):
    import torch
    from rvio_amd import hip
    cfg = K.config()
    hb = hip.RvioHip(cfg, batch=B)
    names = ["window10", "moved", "window10", "moved", "window10"]     # 10 clones each (one window length per handle); 'moved': qk, pk non-trivial
    x0, P0 = K.state("window10")
    hb.set_state(x0, P0)
    worst = 0.0
    for stride in (0, m + 3):
        cases = []
        for i in range(B):
            special = (i == 1 and m >= 2)
            cases.append(truth_cache(names[i], i, m, i if stride else 0, special and bool(stride)))
            hb.set_state_at(i, cases[i][0], cases[i][1])
        if stride:
            imus = np.zeros((B, stride), abi.IMU_DTYPE)
            for i in range(B):
                imus[i, :m] = cases[i][2]
            imus[:, m:]["dt"] = np.nan                                   # a kernel that read past m would show
        else:
            imus = cases[0][2]
            assert all(np.array_equal(raw(c[2]), raw(imus)) for c in cases)
        d_imu = dev(imus)
        out_stride = m + 2
        d_out = out_buf(B * out_stride)
        torch.cuda.synchronize()
        hb.predict_dev(d_imu.data_ptr(), stride, m, d_out.data_ptr(), out_stride)
        hb.sync()
        got = records(d_out).reshape(B, out_stride)
        for i in range(B):
            worst = max(worst, check_against_truth(got[i, :m], cases[i][2], cases[i][3], 0, (stride, i)))
            assert np.all(raw(got[i, m:]) == 0xAB), (stride, i)              # nothing beyond record m - 1
            # ... and the host-buffer entry point on that instance gives the same bytes
            assert same_bytes(hb.predict(cases[i][2], instance=i), got[i, :m]), (stride, i)
        if B > 1:
            assert not np.array_equal(got[0, :m]["p"], got[1, :m]["p"])
    hb.close()
    print("predict_dev, B = %d, m = %d: worst |d| vs oracle prefix propagation = %.3e" % (B, m, worst))


# ---------------------------------------------------------------- direct-track frames (the recorded sequence) and image frames
@pytest.fixture(scope="module")
def recs_b():
    seq, recs = K.recorded()
    return K.config(), seq, recs


def feed_points(h, r):
    inp = r["inp"]
    h.frame_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])


def snapshot(h):
    x, P = h.get_state()
    info = h.frame_info()
    pts = h.get_points()
    return dict(x=x, P=P, info=info, pts=pts, odom=h.odometry(), imuo=h.get_imu_odometry())


def same_snapshot(a, b):
    return (np.array_equal(a["x"], b["x"]) and np.array_equal(a["P"], b["P"]) and a["info"] == b["info"]
            and all(np.array_equal(u, v) for u, v in zip(a["pts"], b["pts"])) and same_bytes(a["odom"], b["odom"]) and same_bytes(a["imuo"], b["imuo"]))


# ---------------------------------------------------------------- 2. no side effect
def test_predict_has_no_side_effect(gpu_required, recs_b):
    import torch
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    hs = [hip.RvioHip(cfg), hip.RvioHip(cfg)]
    for h in hs:
        h.set_odometry(16)
        h.set_imu_odometry(64)
        h.initialize(*seq.init_from_static(38))
        for r in recs[:7]:
            feed_points(h, r)
    imu = recs[7]["inp"]["imu"]
    before = snapshot(hs[0])
    assert before["info"]["updated"] == 1 and len(before["imuo"]) == 64 and len(before["odom"]) == 7
    rec = hs[0].predict(imu)
    d_imu, d_out = dev(imu), out_buf(len(imu))
    torch.cuda.synchronize()
    hs[0].predict_dev(d_imu.data_ptr(), 0, len(imu), d_out.data_ptr(), len(imu))
    hs[0].sync()
    assert same_bytes(records(d_out), rec) and np.all(rec["img_count"] == 7)
    assert same_snapshot(before, snapshot(hs[0]))
    # a following propagate gives the bits it gives without the predict (the twin never predicted); and so does a whole frame
    for h in hs:
        h.frame_plan()
        h.propagate(imu)
    (xa, Pa), (xb, Pb) = hs[0].get_state(), hs[1].get_state()
    assert np.array_equal(xa, xb) and np.array_equal(Pa, Pb)
    assert same_bytes(hs[0].get_imu_odometry(), hs[1].get_imu_odometry())
    assert same_pose_fields(hs[0].get_imu_odometry(first_seq=71), rec)               # what was predicted is what the ring then recorded
    for h in hs:
        h.close()


# ---------------------------------------------------------------- 3. bit identity with the device's own propagate
@pytest.mark.parametrize("m", [1, 10, 17, 65])
def test_last_record_has_the_bits_of_propagate(gpu_required, m):
    """Record m - 1 against rvio_hip_propagate(imu, m) from the same state: v = x[17:20] behind it, (p, q) = the pose line behind
    rvio_hip_augment_compose(0).  m = 17 crosses propagate_body's 16-sample chunk, m = 65 this kernel's 64-sample chunk.  Same expressions, same
    device functions, one translation unit, one set of flags: equal bits."""
    from rvio_amd import hip
    h = hip.RvioHip(K.config())
    for state in K.STATES:
        x, P = K.state(state)
        imu = K.batch(m, 2, special=(m >= 2), x=x)
        h.set_state(x, P)
        rec = h.predict(imu)[-1]
        h.propagate(imu)
        x1 = h.get_state()[0]
        h.augment_compose(False)
        p, q = h.get_pose()
        dv, dp, dq = (float(np.max(np.abs(a - b))) for a, b in ((rec["v"], x1[17:20]), (rec["p"], p), (rec["q"], q)))
        print("m = %d, %s: |dv| = %.3e |dp| = %.3e |dq| = %.3e" % (m, state, dv, dp, dq))
        assert np.array_equal(rec["v"], x1[17:20]), (state, dv)
        assert np.array_equal(rec["p"], p) and np.array_equal(rec["q"], q), (state, dp, dq)
    h.close()


# ---------------------------------------------------------------- 4. the ring on every path
@pytest.fixture(scope="module")
def image_seq():
    cfg = K.config()
    seq = rv.synth.SynthSequence(cfg, duration=(38 + N + 4) / 20.0)
    ks = list(range(39, 39 + N))
    return seq.init_from_static(38), [seq.render(k) for k in ks], [seq.imu_between(k) for k in ks]


class PlainPath:
    """one plain handle driven through `path`; the twin (ring off) predicts in front of every frame"""

    def __init__(self, path, ring, recs_b, image_seq):
        import torch
        from rvio_amd import hip
        self.torch, self.path, self.ring = torch, path, ring
        cfg, seq, recs = recs_b
        self.cfg, self.recs = cfg, recs
        self.init_img, self.imgs, self.imus_img = image_seq
        self.points = path in ("staged", "frame_points")
        self.h = hip.RvioHip(cfg)
        if ring:
            self.h.set_imu_odometry(64)
            self.h.set_odometry(16)
        self.h.initialize(*(seq.init_from_static(38) if self.points else self.init_img))
        self.keep, self.pred, self.poses, self.drained = [], [], {}, []

    def imu(self, k):
        return self.recs[k]["inp"]["imu"] if self.points else self.imus_img[k]

    def frame(self, k):
        h, imu, torch = self.h, self.imu(k), self.torch
        m = len(imu)
        d_imu = dev(imu)
        self.keep.append(d_imu)
        torch.cuda.synchronize()
        if not self.ring:
            d_out = out_buf(m)
            torch.cuda.synchronize()
            h.predict_dev(d_imu.data_ptr(), 0, m, d_out.data_ptr(), m)
            self.pred.append(d_out)
        if self.path == "staged":
            inp = self.recs[k]["inp"]
            h.track_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])
            h.sync()
            do_update, do_augment = h.frame_plan()
            h.propagate(imu)
            if do_update:
                h.update_tracked()
            h.augment_compose(do_augment)
        elif self.path == "frame_points":
            feed_points(h, self.recs[k])
        elif self.path == "frame":
            h.frame(self.imgs[k], imu)
        else:
            d_img = torch.from_numpy(self.imgs[k]).cuda()
            self.keep.append(d_img)
            torch.cuda.synchronize()
            args = (d_img.data_ptr(), self.cfg.width, d_imu.data_ptr(), m, 0, 0)
            if self.path == "frame_dev":
                h.frame_dev(*args)
            elif self.path == "frame_begin_end":
                h.frame_begin_dev(*args)
                do_update, do_augment = h.frame_plan()
                if do_update:
                    h.update_tracked()
                h.augment_compose(do_augment)
                h.frame_end()
            else:
                assert self.path == "frame_sharded"
                h.frame_sharded_dev(*args, 0, 1)
        if self.ring and k < 4:
            # the first four frames run no update (n_clones <= min_track_len - 1 in front of them): the host may wait here; the update frames run without a wait
            self.poses[k] = h.get_pose()
            assert h.frame_info()["updated"] == 0
        if self.ring and k in (5, N - 1):
            # 64 slots, 10 samples per frame: the ring is drained in bulk every six frames
            self.drained.append(h.get_imu_odometry(first_seq=1 + sum(len(d) for d in self.drained)))

    def finish(self):
        h = self.h
        out = dict(info=h.frame_info(), state=h.get_state())
        if self.ring:
            out.update(ring=np.concatenate(self.drained), odom=h.odometry(), poses=self.poses)
        else:
            out.update(pred=[records(b) for b in self.pred])
        h.close()
        return out


def check_ring_against_twin(ring, preds, ms, what):
    """seq 1 .. sum(m) without a gap; img_count / index partition the records into the frames' batches; frame k's records = the twin's predict"""
    total = sum(ms)
    assert len(ring) == total and [int(s) for s in ring["seq"]] == list(range(1, total + 1)), what
    lo = 0
    for k, m in enumerate(ms):
        part = ring[lo:lo + m]
        assert np.all(part["img_count"] == k + 1) and np.array_equal(part["index"], np.arange(m)), (what, k)
        assert same_pose_fields(part, preds[k]), (what, k)
        lo += m


@pytest.mark.parametrize("path", ["staged", "frame_dev", "frame", "frame_points", "frame_begin_end", "frame_sharded"])
def test_ring_on_every_plain_path(gpu_required, recs_b, image_seq, path):
    runs = [PlainPath(path, ring, recs_b, image_seq) for ring in (True, False)]
    for k in range(N):
        for r in runs:                    # lock-step: the twin's predict for frame k goes out behind its frame k - 1
            r.frame(k)
    ms = [len(runs[0].imu(k)) for k in range(N)]
    on, off = runs[0].finish(), runs[1].finish()
    assert on["info"]["device_error"] == 0 and off["info"]["device_error"] == 0
    check_ring_against_twin(on["ring"], off["pred"], ms, path)
    # the update frames — on the pipelined paths the fused per-feature + propagate launch — are among the 12, and the ring changes nothing the filter computes
    assert on["info"]["updated"] == 1 and on["info"]["n_clones"] == 10
    assert np.array_equal(on["state"][0], off["state"][0]) and np.array_equal(on["state"][1], off["state"][1])
    # frames without an update: the last record of the frame's batch carries that frame's pose line, and the rvio_odom record's
    ends = np.cumsum(ms) - 1
    assert sorted(on["poses"]) == [0, 1, 2, 3] and len(on["odom"]) == N
    for k, (p, q) in on["poses"].items():
        last = on["ring"][ends[k]]
        assert np.array_equal(last["p"], p) and np.array_equal(last["q"], q), (path, k)
        od = on["odom"][k]
        assert np.array_equal(last["p"], od["p"]) and np.array_equal(last["q"], od["q"]) and np.array_equal(last["v"], od["v"]), (path, k)


def pack_tracks(cfg, recs_f):
    B, Fu, ML = len(recs_f), abi.fu(cfg), cfg.max_track_len
    n_feat, types, lens = np.zeros(B, np.int32), np.zeros((B, Fu), np.uint8), np.zeros((B, Fu), np.int32)
    meas = np.zeros((B, Fu, ML, 2), np.float32)
    for i, r in enumerate(recs_f):
        n = len(r["lens"])
        n_feat[i] = n
        types[i, :n], lens[i, :n], meas[i, :n] = r["types"], r["lens"], r["meas"]
    return n_feat, types, lens, meas


@pytest.mark.parametrize("kind", ["frame_tracks", "frame_batch"])
def test_ring_on_batch_paths(gpu_required, image_seq, kind):
    """B = 3: rvio_hip_frame_tracks_dev on the recorded hand-over tables of three sequences (updates from frame 5 on: the overlapped propagate on the
    second stream) and rvio_hip_frame_batch_dev on three copies of one camera stream whose instances start from their own velocities and read their own
    accelerometers (one rendered sequence keeps the test short; the instances still differ in every record); per-instance IMU batches (imu_stride = m)"""
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
    hs[0].set_odometry(16)
    keep, preds, ms, poses, drained = [], [], [], {}, [[] for _ in range(B)]
    for k in range(N):
        imus = imus_of(k)
        m = len(imus[0])
        assert all(len(u) == m for u in imus)
        ms.append(m)
        d_imu = dev(np.stack(imus))
        d_out = out_buf(B * m)
        keep += [d_imu, d_out]
        if kind == "frame_tracks":
            d = [torch.from_numpy(a).cuda() for a in pack_tracks(cfg, [recs[i][k] for i in range(B)])]
        else:
            d = [torch.from_numpy(np.stack([imgs[k]] * B)).cuda()]
        keep += d
        torch.cuda.synchronize()
        hs[1].predict_dev(d_imu.data_ptr(), m, m, d_out.data_ptr(), m)
        preds.append(d_out)
        for h in hs:
            if kind == "frame_tracks":
                h.frame_tracks_dev(d_imu.data_ptr(), m, m, *[t.data_ptr() for t in d])
            else:
                h.frame_batch_dev(d[0].data_ptr(), cfg.width, cfg.width * cfg.height, d_imu.data_ptr(), m, m)
        if k < 4:
            poses[k] = [hs[0].get_pose_at(i) for i in range(B)]
            assert hs[0].frame_info()["updated"] == 0
        if k in (5, N - 1):
            for i in range(B):
                drained[i].append(hs[0].get_imu_odometry(instance=i, first_seq=1 + sum(len(d_) for d_ in drained[i])))
    for h in hs:
        h.sync()
    ends = np.cumsum(ms) - 1
    for i in range(B):
        ring = np.concatenate(drained[i])
        pred = [records(b).reshape(B, m)[i] for b, m in zip(preds, ms)]
        check_ring_against_twin(ring, pred, ms, (kind, i))
        xa, xb = hs[0].get_state_at(i), hs[1].get_state_at(i)
        assert np.array_equal(xa[0], xb[0]) and np.array_equal(xa[1], xb[1]), i
        odom = hs[0].odometry(instance=i)
        assert len(odom) == N
        for k, ps in poses.items():                     # frames without an update
            last = ring[ends[k]]
            assert np.array_equal(last["p"], ps[i][0]) and np.array_equal(last["q"], ps[i][1]), (kind, i, k)
            assert np.array_equal(last["p"], odom[k]["p"]) and np.array_equal(last["q"], odom[k]["q"]) and np.array_equal(last["v"], odom[k]["v"]), (kind, i, k)
        if i:
            assert not np.array_equal(ring["p"], np.concatenate(drained[i - 1])["p"])
    info = hs[0].frame_info()
    assert info["updated"] == 1 and info["device_error"] == 0, info
    for h in hs:
        h.close()


# ---------------------------------------------------------------- 5. ring mechanics
@pytest.fixture(scope="module")
def full_run(gpu_required, recs_b):
    """the 12 direct-track frames with a ring that holds all of them: every record, and the filter's final state; the same run with the ring off"""
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    out = []
    for cap in (256, 0):
        h = hip.RvioHip(cfg)
        if cap:
            h.set_imu_odometry(cap)
        h.initialize(*seq.init_from_static(38))
        for r in recs:
            feed_points(h, r)
        out.append((h.get_imu_odometry() if cap else None, h.get_state()))
        h.close()
    ms = [len(r["inp"]["imu"]) for r in recs]
    assert all(m == 10 for m in ms)
    return out[0][0], out[0][1], out[1][1]


def test_ring_off_is_off(full_run):
    ring, on, off = full_run
    assert len(ring) == 120 and [int(s) for s in ring["seq"]] == list(range(1, 121))
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])


def test_ring_mechanics(full_run, recs_b):
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    ref = full_run[0]
    h = hip.RvioHip(cfg)

    def feed(lo, hi):
        for r in recs[lo:hi]:
            feed_points(h, r)

    # capacity 7, m = 10: only the last 7 of each batch survive, in order (two records of one launch never share a slot)
    h.set_imu_odometry(7)
    h.initialize(*seq.init_from_static(38))
    for k in range(3):
        feed(k, k + 1)
        got = h.get_imu_odometry()
        assert [int(s) for s in got["seq"]] == list(range(10 * k + 4, 10 * k + 11)) and same_bytes(got, ref[10 * k + 3:10 * k + 10]), k
    assert same_bytes(h.get_imu_odometry(first_seq=28), ref[27:30]) and same_bytes(h.get_imu_odometry(first_seq=-3, max_n=2), ref[23:25])
    assert len(h.get_imu_odometry(first_seq=31)) == 0
    # another capacity restarts seq at 1 (on a filter that goes on: the records are those of a run that enabled its ring at frame 4)
    h.set_imu_odometry(25)
    assert len(h.get_imu_odometry()) == 0
    feed(3, 7)                                        # 40 samples through 25 slots: wrapped
    got = h.get_imu_odometry()
    assert [int(s) for s in got["seq"]] == list(range(16, 41)) and same_pose_fields(got, ref[45:70]) and np.array_equal(got["img_count"], ref["img_count"][45:70])
    # capacity 0 stops the launches and keeps the records; the same capacity again resumes where it stopped
    h.set_imu_odometry(0)
    feed(7, 8)
    assert same_bytes(h.get_imu_odometry(), got)
    h.set_imu_odometry(25)
    assert same_bytes(h.get_imu_odometry(), got)
    feed(8, 9)
    got2 = h.get_imu_odometry()
    assert [int(s) for s in got2["seq"]] == list(range(26, 51)) and same_pose_fields(got2[-10:], ref[80:90]) and same_bytes(got2[:15], got[10:])
    # the timing form writes a buffer of its own
    assert h.time_kernel(13, 3) > 0 and same_bytes(h.get_imu_odometry(), got2)
    # set_state and poison leave the ring alone; initialize empties it
    h.set_state(*h.get_state())
    h.poison(7)
    assert same_bytes(h.get_imu_odometry(), got2)
    h.initialize(*seq.init_from_static(38))
    assert len(h.get_imu_odometry()) == 0
    feed(0, 2)
    assert same_bytes(h.get_imu_odometry(), ref[:20])
    h.close()


def test_ring_with_poison_and_stalls(full_run, recs_b):
    """NaN bytes over the filter's scratch, the chip's LDS and the hand-over tables between the frames, and the filter stream held up in front of
    some of them: the same records, the same final state"""
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    ref, on, _ = full_run
    rng = np.random.default_rng(5)
    h = hip.RvioHip(cfg)
    h.set_imu_odometry(256)
    h.initialize(*seq.init_from_static(38))
    for k, r in enumerate(recs):
        if k % 3 == 1:
            h.poison(1 | 2 | 4)
        if k % 2:
            h.stall(0, int(rng.integers(30, 900)))
        feed_points(h, r)
        if k % 4 == 2:
            h.stall(0, int(rng.integers(30, 900)))
    got, st = h.get_imu_odometry(), h.get_state()
    h.close()
    assert same_bytes(got, ref) and np.array_equal(st[0], on[0]) and np.array_equal(st[1], on[1])


# ---------------------------------------------------------------- 6. errors
def test_errors(gpu_required, recs_b):
    import torch
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    INVALID, UNSUPPORTED, STATE = -1, -3, -4
    imu = recs[0]["inp"]["imu"]
    m = len(imu)
    ip = imu.ctypes.data_as(C.POINTER(abi.rvio_imu))
    out = np.zeros(m, abi.IMU_POSE_DTYPE)
    op = out.ctypes.data_as(C.POINTER(abi.ImuPose))
    d_imu, d_out = dev(imu), out_buf(m)
    vp = C.c_void_p
    n = C.c_int32(-1)
    h = hip.RvioHip(cfg, batch=2)
    L = h.L
    # before the first state
    assert L.rvio_hip_predict(h.h, 0, ip, m, op) == STATE and b"rvio_hip_set_state" in L.rvio_hip_last_error(h.h)
    assert L.rvio_hip_predict_dev(h.h, vp(d_imu.data_ptr()), 0, m, vp(d_out.data_ptr()), m) == STATE
    # the ring before it was enabled
    assert L.rvio_hip_get_imu_odometry(h.h, 0, C.c_int64(1), 1, op, C.byref(n)) == STATE
    with pytest.raises(hip.RvioHipError):
        h.time_kernel(13, 1)
    us = C.c_float(0)
    assert L.rvio_hip_debug_time_kernel(h.h, 13, 1, C.byref(us)) == UNSUPPORTED
    h.set_state(recs[0]["x0"], recs[0]["P0"])
    # predict
    assert L.rvio_hip_predict(h.h, 2, ip, m, op) == INVALID and L.rvio_hip_predict(h.h, -1, ip, m, op) == INVALID
    assert L.rvio_hip_predict(h.h, 0, ip, -1, op) == INVALID and L.rvio_hip_predict(h.h, 0, None, m, op) == INVALID and L.rvio_hip_predict(h.h, 0, ip, m, None) == INVALID
    assert L.rvio_hip_predict(h.h, 1, None, 0, None) == 0
    # predict_dev: out_stride >= m; imu_stride 0 or >= m; m == 0 writes nothing
    a = (vp(d_imu.data_ptr()), vp(d_out.data_ptr()))
    assert L.rvio_hip_predict_dev(h.h, a[0], 0, m, a[1], m - 1) == INVALID
    assert L.rvio_hip_predict_dev(h.h, a[0], m - 1, m, a[1], m) == INVALID and L.rvio_hip_predict_dev(h.h, a[0], -1, m, a[1], m) == INVALID
    assert L.rvio_hip_predict_dev(h.h, a[0], 0, -1, a[1], m) == INVALID
    assert L.rvio_hip_predict_dev(h.h, None, 0, m, a[1], m) == INVALID and L.rvio_hip_predict_dev(h.h, a[0], 0, m, None, m) == INVALID
    assert L.rvio_hip_predict_dev(h.h, None, 0, 0, None, 0) == 0
    h.sync()
    assert np.all(d_out.cpu().numpy() == 0xAB)
    # the ring's setter and getter
    assert L.rvio_hip_set_imu_odometry(h.h, -1) == INVALID and L.rvio_hip_set_imu_odometry(h.h, 1048577) == INVALID
    h.set_imu_odometry(4)
    assert L.rvio_hip_get_imu_odometry(h.h, 2, C.c_int64(1), 1, op, C.byref(n)) == INVALID
    assert L.rvio_hip_get_imu_odometry(h.h, 0, C.c_int64(1), -1, op, C.byref(n)) == INVALID
    assert L.rvio_hip_get_imu_odometry(h.h, 0, C.c_int64(1), 1, None, C.byref(n)) == INVALID
    assert L.rvio_hip_get_imu_odometry(h.h, 0, C.c_int64(1), 0, None, C.byref(n)) == 0 and n.value == 0
    assert L.rvio_hip_get_imu_odometry(h.h, 1, C.c_int64(1), 4, op, C.byref(n)) == 0 and n.value == 0      # enabled, nothing recorded yet
    assert L.rvio_hip_debug_time_kernel(h.h, 13, 1, C.byref(us)) == UNSUPPORTED                              # ... and no frame has propagated
    h.close()
    # a ring beyond 1 GiB is refused with the size in the text: 1048576 x 11 x 104 bytes
    hb = hip.RvioHip(cfg, batch=11)
    assert hb.L.rvio_hip_set_imu_odometry(hb.h, 1048576) == UNSUPPORTED
    msg = hb.L.rvio_hip_last_error(hb.h)
    assert b"1 GiB" in msg and str(1048576 * 11 * 104).encode() in msg, msg
    assert hb.L.rvio_hip_set_imu_odometry(hb.h, 1048576 // 2) == 0                                          # 572 MB: accepted
    hb.close()
