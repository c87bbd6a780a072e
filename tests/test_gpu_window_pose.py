"""The fixed-lag smoothed trajectory (rvio_hip_get_window[_dev], rvio_hip_set_smoothed_odometry, csrc/window_pose.hip): the world pose of every
frame of the clone window as the state holds it NOW, and its 6 x 6 covariance.  What a record holds against the NumPy model and its
extended-precision twin at the shortest, the stock and the longest window; that age 0 is the odometry record; that a record depends on
nothing outside the columns its Jacobian names; the ring (lag, wrap, stop, empty), every path into it, that a handle with the ring on computes
what one without computes, batch handles, and the errors.
Settings: cfg B, equaliser off; states from the 12 recorded direct-track frames of scenarios.record_sequence or built (tests/window_cases.py)
and handed in through set_state — no frames are run at long windows.

Measured on an MI355X (e = max_ij |C - C_true|_ij / sqrt(C_true,ii C_true,jj) against the np.longdouble twin; the float64 model's own e is
the floor; the bar is 1e-11): device e between 1.9e-16 and 6.2e-16 over max_track_len 3 / 11 / 32 and ages 0, 1, n - 1, n, the floor between
1.8e-16 and 4.5e-16 (the table is in DESIGN.md section 3)."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import scenarios as S
import window_cases as W
from test_gpu_odometry import raw, same_bytes, staged_frame

abi, rv = O.abi, O.rv
pytestmark = pytest.mark.gpu
EPS = W.EPS
N = 12
BODY = ("img_count", "age", "n_clones", "reserved", "p", "q", "pose_cov")     # everything but seq


def same_body(a, b):
    """two records (or arrays of them) equal in every member but seq, as raw bytes"""
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    return len(a) == len(b) and all(np.array_equal(raw(np.ascontiguousarray(a[f])), raw(np.ascontiguousarray(b[f]))) for f in BODY)


def bits(rec):
    return tuple(np.ascontiguousarray(rec[f]).tobytes() for f in ("p", "q", "pose_cov"))


@pytest.fixture(scope="module")
def recs_b():
    cfg = abi.config_named("B", enable_equalizer=0)
    seq, recs = S.record_sequence(cfg, n_frames=N)
    return cfg, seq, recs


def built_handle(max_len, seed=0, batch=None):
    from rvio_amd import hip
    cfg = abi.config_named("B", enable_equalizer=0, max_track_len=max_len)
    h = hip.RvioHip(cfg, batch=batch)
    h.set_state(*W.built_state(max_len - 1, seed))
    return h


# ---------------------------------------------------------------- 1  model parity
@pytest.mark.parametrize("max_len", W.WINDOWS)
def test_model_parity(gpu_required, max_len):
    n = max_len - 1
    x, P = W.built_state(n)
    h = built_handle(max_len)
    win = h.get_window()
    assert len(win) == n + 1 and len(h.get_window(max_n=2)) == 2 and same_bytes(h.get_window(max_n=1), win[:1])
    h.close()
    assert [int(a) for a in win["age"]] == list(range(n + 1)) and not win["seq"].any() and not win["reserved"].any()
    assert np.all(win["n_clones"] == n) and np.array_equal(win["img_count"], -np.arange(n + 1))      # a state handed in: reference count 0
    for a in W.ages_of(n):
        rec = win[a]
        p, q, cov = abi.window_pose_model(x, P, a)
        pt, qt, ct = W.truth(n, a)
        assert np.max(np.abs(rec["p"] - p)) <= 1e-12 * max(1.0, np.linalg.norm(p)), a
        assert W.quat_close(rec["q"], q, 1e-12), a
        if a == 0:
            assert np.array_equal(rec["q"], x[0:4])
        else:
            assert rec["q"][3] >= 0 and abs(np.linalg.norm(rec["q"]) - 1) <= 4 * EPS
        C_ = rec["pose_cov"]
        assert np.array_equal(C_, C_.T), a
        assert np.min(np.linalg.eigvalsh(C_)) >= -64 * EPS * np.linalg.norm(C_, 2), a
        e, floor = W.cov_err(C_, ct), W.cov_err(cov, ct)
        print("max_track_len %d, age %d (k = %d): e = %.3e, float64 model (the floor) e = %.3e" % (max_len, a, 6 + 6 * a, e, floor))
        assert e <= 1e-11, (a, e, floor)


# ---------------------------------------------------------------- 2, 4, 5, 6  the ring over the 12 recorded frames
@pytest.fixture(scope="module")
def staged(gpu_required, recs_b):
    """the 12 frames stage by stage on two handles: `h` with the odometry ring and the smoothed ring at lag 3, capacity 16; `t`, its twin,
    with the odometry ring only, asked for its window behind every frame"""
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    h, t = hip.RvioHip(cfg), hip.RvioHip(cfg)
    h.set_odometry(16)
    t.set_odometry(16)
    h.set_smoothed_odometry(16, 3)
    seqno, none = h.smoothed_odometry_all()
    assert seqno == 0 and len(h.smoothed_odometry()) == 0 and not raw(none).any()
    for q in (h, t):
        q.initialize(*seq.init_from_static(38))
    windows, counts = [], []
    for r in recs:
        for q in (h, t):
            staged_frame(q, r["inp"])
        windows.append(t.get_window())
        counts.append(h.smoothed_odometry_all()[0])
    ring, odom, odom_t = h.smoothed_odometry(), h.odometry(), t.odometry()
    info = h.frame_info()
    h.close()
    t.close()
    assert info["device_error"] == 0 and info["updated"] == 1, info
    assert same_bytes(odom, odom_t)
    return ring, odom, windows, counts


def test_ring_lag_3(staged):
    ring, odom, windows, counts = staged
    n_cl = [int(v) for v in odom["n_clones"]]
    assert n_cl[0] < 3 <= n_cl[-1]
    want = [k for k in range(N) if n_cl[k] >= 3]                                  # the frames that write a record
    assert counts == [sum(1 for k in want if k <= f) for f in range(N)]          # nothing until n_clones >= 3, then one per frame
    assert counts[want[0] - 1] == 0 and len(ring) == len(want) and [int(s) for s in ring["seq"]] == list(range(1, len(want) + 1))
    for rec, k in zip(ring, want):
        assert int(rec["img_count"]) == int(odom["img_count"][k]) - 3 and int(rec["age"]) == 3 and int(rec["n_clones"]) == n_cl[k]
        assert len(windows[k]) == n_cl[k] + 1 and same_body(rec, windows[k][3]), k  # = get_window behind the same frame on the twin, bit for bit
    # a smoothed pose is not the filter pose that frame had: later updates have moved it
    assert any(not np.array_equal(ring["p"][j], odom["p"][k - 3]) for j, k in enumerate(want))


def test_age_0_is_the_odometry_record(gpu_required, recs_b, staged):
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    h = hip.RvioHip(cfg)
    h.set_odometry(16)
    h.set_smoothed_odometry(16, 0)
    h.initialize(*seq.init_from_static(38))
    states = []
    for r in recs:
        staged_frame(h, r["inp"])
        states.append(h.get_state())
    smo, odom = h.smoothed_odometry(), h.odometry()
    h.close()
    assert same_bytes(odom, staged[1]) and len(smo) == N == len(odom)
    worst = 0.0
    for k in range(N):
        a, b, (x, P) = smo[k], odom[k], states[k]
        assert int(a["seq"]) == k + 1 == int(b["seq"]) and int(a["img_count"]) == int(b["img_count"]) and int(a["n_clones"]) == int(b["n_clones"])
        assert np.array_equal(a["q"], b["q"]), k
        assert np.max(np.abs(a["p"] - b["p"])) <= 1e-12, k
        J = np.abs(abi.odom_pose_jacobian(x[0:4], x[4:7]))
        bound = 64 * EPS * (J @ np.abs(P[:6, :6]) @ J.T)
        err = np.abs(a["pose_cov"] - b["pose_cov"])
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (k, worst)
        assert np.array_equal(a["pose_cov"], a["pose_cov"].T)
    print("age 0 against rvio_odom.pose_cov: worst |d| / (64 eps |J| |P6| |J|^T) = %.3f over %d frames" % (worst, N))


def test_the_ring(gpu_required, recs_b, staged):
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    ref = staged[0]                                             # lag 3: n_clones = 0, 1, 2, 3, ... behind the frames, 9 records over the 12
    assert len(ref) == 9
    h = hip.RvioHip(cfg)
    h.set_smoothed_odometry(4, 3)

    def feed(lo, hi):
        for r in recs[lo:hi]:
            inp = r["inp"]
            h.frame_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])

    h.initialize(*seq.init_from_static(38))
    feed(0, 3)
    assert len(h.smoothed_odometry()) == 0 and h.smoothed_odometry_all()[0] == 0
    feed(3, 11)
    got = h.smoothed_odometry(first_seq=1)
    assert [int(s) for s in got["seq"]] == [5, 6, 7, 8] and same_bytes(got, ref[4:8])                    # wrapped
    assert same_bytes(h.smoothed_odometry(first_seq=7), ref[6:8])
    assert same_bytes(h.smoothed_odometry(first_seq=-5, max_n=2), ref[4:6])
    assert len(h.smoothed_odometry(first_seq=9)) == 0
    seqno, newest = h.smoothed_odometry_all()
    assert seqno == 8 and same_bytes(newest, ref[7:8])
    # capacity 0: the ring no longer advances, the records stay; on again with the same capacity and lag: it goes on
    h.set_smoothed_odometry(0, 3)
    feed(11, 12)
    assert same_bytes(h.smoothed_odometry(), ref[4:8]) and h.smoothed_odometry_all()[0] == 8
    h.set_smoothed_odometry(4, 3)
    assert same_bytes(h.smoothed_odometry(), ref[4:8])
    # another lag empties it, like another capacity
    h.set_smoothed_odometry(4, 2)
    assert len(h.smoothed_odometry()) == 0 and h.smoothed_odometry_all()[0] == 0
    h.set_smoothed_odometry(4, 3)
    h.set_smoothed_odometry(5, 3)
    assert len(h.smoothed_odometry()) == 0 and h.smoothed_odometry_all()[0] == 0
    # initialize restarts at seq 1; set_state leaves the ring alone
    h.set_smoothed_odometry(4, 3)
    h.initialize(*seq.init_from_static(38))
    feed(0, 4)                                                  # (the frames before the first update: a handle that has run frames draws other RANSAC samples)
    assert same_bytes(h.smoothed_odometry(), ref[0:1])
    h.set_state(*h.get_state())
    assert same_bytes(h.smoothed_odometry(), ref[0:1])
    # the most-smoothed pose still in the window: lag = max_track_len - 1 waits until the window is full
    h.set_smoothed_odometry(4, cfg.max_track_len - 1)
    h.initialize(*seq.init_from_static(38))
    feed(0, 12)
    got = h.smoothed_odometry()
    assert len(got) == int(np.sum(staged[1]["n_clones"] >= cfg.max_track_len - 1)) > 0 and np.all(got["age"] == cfg.max_track_len - 1)
    h.close()


def test_frame_points_pipelined_writes_the_same_ring(gpu_required, recs_b, staged):
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    h = hip.RvioHip(cfg)
    h.set_smoothed_odometry(16, 3)
    h.initialize(*seq.init_from_static(38))
    for r in recs:
        inp = r["inp"]
        h.frame_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])
    got = h.smoothed_odometry()
    h.close()
    assert same_bytes(got, staged[0])


def test_off_is_off(gpu_required, recs_b):
    """two handles on the same frames, one with the ring on: the same states, covariances, pose lines and tracker tables"""
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    hs = [hip.RvioHip(cfg), hip.RvioHip(cfg)]
    hs[1].set_smoothed_odometry(8, 3)
    for h in hs:
        h.initialize(*seq.init_from_static(38))
    for r in recs:
        inp = r["inp"]
        for h in hs:
            h.frame_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])
    (xa, Pa), (xb, Pb) = hs[0].get_state(), hs[1].get_state()
    assert np.array_equal(xa, xb) and np.array_equal(Pa, Pb)
    for a, b in zip(hs[0].get_pose(), hs[1].get_pose()):
        assert np.array_equal(a, b)
    for a, b in zip(hs[0].get_points() + hs[0].get_tracks(), hs[1].get_points() + hs[1].get_tracks()):
        assert np.array_equal(a, b)
    assert len(hs[1].smoothed_odometry()) == 8
    for h in hs:
        h.close()


# ---------------------------------------------------------------- 3  locality
def test_locality(gpu_required):
    """a record of age a reads x[0:7], the newest a clones and the rows / columns {0 - 5, clones n - a .. n - 1} of P: everything else may change"""
    n = 10
    x, P = W.built_state(n)
    h = built_handle(n + 1)
    base = h.get_window()
    rng = np.random.default_rng(5)
    for a in (0, 1, 5, n):
        x2, P2 = np.array(x), np.array(P)
        x2[7:26] = rng.standard_normal(19)
        for i in range(n - a):
            x2[26 + 7 * i: 30 + 7 * i] = W.unit_quat(rng)
            x2[30 + 7 * i: 33 + 7 * i] = rng.standard_normal(3)
        keep = np.zeros(24 + 6 * n, bool)
        keep[0:6] = True
        keep[24 + 6 * (n - a): 24 + 6 * n] = True
        other = rng.standard_normal(P2.shape) * 1e3
        mask = np.outer(keep, keep)
        P2[~mask] = other[~mask]
        assert not np.array_equal(P2, P) and np.array_equal(P2[mask], P[mask])
        h.set_state(x2, P2)
        got = h.get_window()
        assert bits(got[a]) == bits(base[a]), a
        if a < n:
            assert bits(got[n]) != bits(base[n])                # (the changes are seen by a record that does read them)
    h.close()


# ---------------------------------------------------------------- 7  batch handles
def dev_records(h, age_first, n_ages, stride):
    """get_window_dev into a buffer filled with 0xAB bytes: [instance][stride] records"""
    import torch
    buf = torch.full((h.batch * stride * 368,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    h.get_window_dev(age_first, n_ages, buf.data_ptr(), stride)
    h.sync()
    return buf.cpu().numpy().view(abi.WINDOW_POSE_DTYPE).reshape(h.batch, stride)


def test_batch_of_three_equals_three_plain_handles(gpu_required):
    n, B = 10, 3
    hb = built_handle(n + 1, batch=B)
    wins = []
    for i in range(B):
        hb.set_state_at(i, *W.built_state(n, seed=i))
        hi = built_handle(n + 1, seed=i)
        wins.append(hi.get_window())
        assert same_bytes(hb.get_window(instance=i), wins[i])
        hi.close()
    assert not np.array_equal(wins[0]["p"], wins[1]["p"])
    # ages 0 .. n + 1 with a stride of n + 4: the age beyond the window says so, its neighbours and the padding are left alone
    got = dev_records(hb, 0, n + 2, n + 4)
    for i in range(B):
        assert same_bytes(got[i, : n + 1], wins[i]), i
        beyond = got[i, n + 1]
        assert int(beyond["img_count"]) == -1 and int(beyond["n_clones"]) == n
        for f in ("seq", "age", "reserved", "p", "q", "pose_cov"):
            assert not np.any(beyond[f]), f
        assert np.all(raw(got[i, n + 2:]) == 0xAB)
    # a range that starts inside the window
    part = dev_records(hb, 4, 3, 3)
    for i in range(B):
        assert same_bytes(part[i], wins[i][4:7]), i
    hb.close()


def test_batch_of_128_sharing_one_state(gpu_required):
    n = 10
    h1 = built_handle(n + 1)
    want = h1.get_window()
    h1.close()
    hb = built_handle(n + 1, batch=128)
    got = dev_records(hb, 0, n + 1, n + 1)
    hb.close()
    for i in range(128):
        assert same_bytes(got[i], want), i


# ---------------------------------------------------------------- 8  errors
def test_errors(gpu_required, recs_b):
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    h = hip.RvioHip(cfg)
    L = h.L
    n, seqno, rec = C.c_int32(-1), C.c_int64(0), (abi.rvio_window_pose * 16)()

    def err():
        return L.rvio_hip_last_error(h.h)

    # RVIO_ERR_STATE (-4): no state yet; the ring never enabled
    assert L.rvio_hip_get_window(h.h, 0, 4, rec, C.byref(n)) == -4 and b"rvio_hip_get_window before the first" in err()
    assert L.rvio_hip_get_window_dev(h.h, 0, 1, C.c_void_p(8), C.c_size_t(1)) == -4 and b"rvio_hip_get_window_dev before the first" in err()
    assert L.rvio_hip_get_smoothed_odometry(h.h, 0, C.c_int64(1), 1, rec, C.byref(n)) == -4 and b"smoothed-odometry ring was never enabled" in err()
    assert L.rvio_hip_get_smoothed_odometry_all(h.h, rec, C.byref(seqno)) == -4
    # RVIO_ERR_INVALID (-1)
    assert L.rvio_hip_set_smoothed_odometry(h.h, 65537, 0) == -1 and b"capacity" in err()
    assert L.rvio_hip_set_smoothed_odometry(h.h, -1, 0) == -1
    assert L.rvio_hip_set_smoothed_odometry(h.h, 4, -1) == -1 and b"lag outside 0 .. max_track_len - 1" in err()
    assert L.rvio_hip_set_smoothed_odometry(h.h, 4, cfg.max_track_len) == -1
    assert L.rvio_hip_set_smoothed_odometry(h.h, 0, cfg.max_track_len) == -1
    assert L.rvio_hip_get_smoothed_odometry(h.h, 0, C.c_int64(1), 1, rec, C.byref(n)) == -4               # still never enabled
    h.set_smoothed_odometry(4, cfg.max_track_len - 1)
    assert L.rvio_hip_get_smoothed_odometry(h.h, 1, C.c_int64(1), 1, rec, C.byref(n)) == -1               # no instance 1
    assert L.rvio_hip_get_smoothed_odometry(h.h, 0, C.c_int64(1), -1, rec, C.byref(n)) == -1
    assert L.rvio_hip_get_smoothed_odometry(h.h, 0, C.c_int64(1), 1, None, C.byref(n)) == -1
    assert L.rvio_hip_get_smoothed_odometry(h.h, 0, C.c_int64(1), 0, None, C.byref(n)) == 0 and n.value == 0
    assert L.rvio_hip_get_smoothed_odometry_all(h.h, None, C.byref(seqno)) == -1
    h.initialize(*seq.init_from_static(38))
    assert L.rvio_hip_get_window(h.h, 0, 4, None, C.byref(n)) == -1 and b"NULL" in err()
    assert L.rvio_hip_get_window(h.h, 0, 4, rec, None) == -1
    assert L.rvio_hip_get_window(h.h, 1, 4, rec, C.byref(n)) == -1 and b"instance out of range" in err()
    assert L.rvio_hip_get_window(h.h, -1, 4, rec, C.byref(n)) == -1
    assert L.rvio_hip_get_window(h.h, 0, 0, rec, C.byref(n)) == -1 and b"max_n < 1" in err()
    assert L.rvio_hip_get_window_dev(h.h, 0, 1, None, C.c_size_t(1)) == -1 and b"NULL d_out" in err()
    assert L.rvio_hip_get_window_dev(h.h, -1, 1, C.c_void_p(8), C.c_size_t(1)) == -1
    assert L.rvio_hip_get_window_dev(h.h, 0, 0, C.c_void_p(8), C.c_size_t(1)) == -1
    assert L.rvio_hip_get_window_dev(h.h, 0, 3, C.c_void_p(8), C.c_size_t(2)) == -1 and b"out_stride is below n_ages" in err()
    # an empty window has one frame: the reference frame itself
    assert L.rvio_hip_get_window(h.h, 0, 16, rec, C.byref(n)) == 0 and n.value == 1 and rec[0].age == 0 and rec[0].n_clones == 0
    h.close()
    # a ring beyond 1 GiB is refused with the size in the text
    hb = hip.RvioHip(cfg, batch=50)
    assert hb.L.rvio_hip_set_smoothed_odometry(hb.h, 65536, 0) == -3 and b"1 GiB" in hb.L.rvio_hip_last_error(hb.h)
    hb.close()
