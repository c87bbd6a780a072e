"""Pose-graph export (rvio_hip_get_window_edges[_dev], rvio_hip_set_edge_odometry, rvio_hip_get_window_joint[_dev], csrc/window_edge.hip): the
edge between two frames of the clone window — their relative pose with the covariance of that quantity — and the joint covariance of the
window's world poses.  Edges against the NumPy model and its extended-precision twin at the shortest, the stock and the longest window; that an
edge reads nothing outside its span; the joint covariance against get_window() (poses and diagonal blocks byte for byte), its symmetry, its
blocks against the truth, its prefixes; the edge ring (first record, twin handle, wrap, stop, empty, off is off); batch handles; the errors.
Settings: cfg B, equaliser off; states from the 12 recorded direct-track frames of scenarios.record_sequence or built (tests/window_cases.py)
and handed in through set_state — no frames are run at long windows.

Measured on an MI355X (e = max_ij |C - C_true|_ij / sqrt(C_true,ii C_true,jj) against the np.longdouble twin; the float64 model's own e is
the floor; the bar is 1e-11).  Edges, device e (floor): max_track_len 3: (0, 1) 3.5e-16 (3.5e-16), (0, 2) 4.5e-16 (6.3e-16), (1, 2) 3.0e-16
(3.0e-16); 11: (0, 1) 4.9e-16 (4.9e-16), (0, 10) 3.6e-16 (1.3e-15), (9, 10) 3.3e-18 (2.4e-16), (1, 9) 4.0e-16 (1.2e-15); 32: (0, 1) 3.5e-17
(3.5e-17), (0, 31) 1.1e-15 (5.5e-16), (30, 31) 2.0e-17 (5.1e-17), (1, 30) 8.6e-16 (3.1e-16).  Joint covariance, every block normalised by
sqrt(C_aa,ii C_bb,jj): 18 x 18 6.2e-16 (4.2e-16), 66 x 66 4.5e-16 (5.7e-16), 192 x 192 7.0e-16 (1.1e-15).  The table is in DESIGN.md section 3."""
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
BODY = ("img_count_new", "img_count_old", "age_new", "age_old", "n_clones", "reserved", "p", "q", "cov")     # everything but seq


def same_body(a, b):
    """two records (or arrays of them) equal in every member but seq, as raw bytes"""
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    return len(a) == len(b) and all(np.array_equal(raw(np.ascontiguousarray(a[f])), raw(np.ascontiguousarray(b[f]))) for f in BODY)


def pairs_of(n):
    """(0, 1), (0, n), (n - 1, n), (1, n - 1) where valid"""
    out = []
    for a, b in ((0, 1), (0, n), (n - 1, n), (1, n - 1)):
        if 0 <= a < b <= n and (a, b) not in out:
            out.append((a, b))
    return out


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


# ---------------------------------------------------------------- 1  edges against the model and its longdouble twin
@pytest.mark.parametrize("max_len", W.WINDOWS)
def test_edges_model_parity(gpu_required, max_len):
    n = max_len - 1
    x, P = W.built_state(n)
    h = built_handle(max_len)
    pairs = pairs_of(n)
    got = h.get_window_edges(pairs)
    h.close()
    assert len(got) == len(pairs) and not got["seq"].any() and not got["reserved"].any() and np.all(got["n_clones"] == n)
    for rec, (a, b) in zip(got, pairs):
        assert (int(rec["age_new"]), int(rec["age_old"]), int(rec["img_count_new"]), int(rec["img_count_old"])) == (a, b, -a, -b)
        p, q, cov = abi.window_edge_model(x, P, a, b)
        pt, qt, ct = abi.window_edge_model_as(x, P, a, b, np.longdouble)
        for ref_p, ref_q in ((p, q), (pt, qt)):
            assert np.max(np.abs(rec["p"] - np.asarray(ref_p, float))) <= 1e-12 * max(1.0, float(np.linalg.norm(np.asarray(ref_p, float)))), (a, b)
            assert W.quat_close(rec["q"], np.asarray(ref_q, float), 1e-12), (a, b)
        assert rec["q"][3] >= 0 and abs(np.linalg.norm(rec["q"]) - 1) <= 4 * EPS
        C_ = rec["cov"]
        assert np.array_equal(C_, C_.T), (a, b)
        assert np.min(np.linalg.eigvalsh(C_)) >= -64 * EPS * np.linalg.norm(C_, 2), (a, b)
        e, floor = W.cov_err(C_, ct), W.cov_err(cov, ct)
        print("max_track_len %d, edge (%d, %d) (6k = %d): e = %.3e, float64 model (the floor) e = %.3e" % (max_len, a, b, 6 * (b - a), e, floor))
        assert e <= 1e-11, (a, b, e, floor)


def test_every_pair_of_the_longest_window_in_one_call(gpu_required):
    """528 pairs is the limit; the longest window has 496: all of them in one launch equal the calls pair by pair"""
    n = 31
    h = built_handle(n + 1)
    pairs = [(a, b) for a in range(n + 1) for b in range(a + 1, n + 1)]
    assert len(pairs) == 496 <= abi.WINDOW_EDGE_MAX_PAIRS
    got = h.get_window_edges(pairs)
    for i in (0, 30, 31, 250, 495):
        assert same_bytes(got[i: i + 1], h.get_window_edges([pairs[i]])), pairs[i]
    assert same_bytes(h.get_window_edges(pairs + pairs[:32]), np.concatenate([got, got[:32]]))       # 528 records
    h.close()


# ---------------------------------------------------------------- 2  locality
def test_an_edge_reads_nothing_outside_its_span(gpu_required):
    """the edge (a, b) reads the clones n - b .. n - a - 1 and their square of P: x[0:26], every other clone and every other row and column
    of P may change"""
    n = 10
    x, P = W.built_state(n)
    h = built_handle(n + 1)
    rng = np.random.default_rng(7)
    wide = (0, n)
    base_wide = h.get_window_edges([wide])
    for a, b in ((0, 1), (3, 7), (n - 1, n), (1, n - 1)):
        h.set_state(x, P)
        base = h.get_window_edges([(a, b)])
        x2, P2 = np.array(x), np.array(P)
        x2[0:4] = W.unit_quat(rng)
        x2[4:10] = rng.standard_normal(6)
        x2[10:14] = W.unit_quat(rng)
        x2[14:26] = rng.standard_normal(12)
        for i in list(range(0, n - b)) + list(range(n - a, n)):
            x2[26 + 7 * i: 30 + 7 * i] = W.unit_quat(rng)
            x2[30 + 7 * i: 33 + 7 * i] = rng.standard_normal(3)
        keep = np.zeros(24 + 6 * n, bool)
        keep[24 + 6 * (n - b): 24 + 6 * (n - a)] = True
        other = rng.standard_normal(P2.shape) * 1e3
        mask = np.outer(keep, keep)
        P2[~mask] = other[~mask]
        assert not np.array_equal(P2, P) and np.array_equal(P2[mask], P[mask])
        h.set_state(x2, P2)
        got = h.get_window_edges([(a, b)])
        assert same_bytes(got, base), (a, b)
        assert not same_bytes(h.get_window_edges([wide]), base_wide)       # (the changes are seen by a record that does read them)
    h.close()


# ---------------------------------------------------------------- 3  the joint covariance
@pytest.mark.parametrize("max_len", W.WINDOWS)
def test_joint(gpu_required, max_len):
    n = max_len - 1
    m = n + 1
    x, P = W.built_state(n)
    h = built_handle(max_len)
    win = h.get_window()
    poses, X = h.get_window_joint()
    p1, X1 = h.get_window_joint(max_n=1)
    p2, X2 = h.get_window_joint(max_n=2)
    h.close()
    assert len(poses) == m and X.shape == (6 * m, 6 * m)
    assert same_bytes(poses, win)                                                   # the records of get_window(), byte for byte
    for a in range(m):
        assert np.array_equal(raw(np.ascontiguousarray(X[6 * a: 6 * a + 6, 6 * a: 6 * a + 6])), raw(np.ascontiguousarray(win["pose_cov"][a]))), a
    assert np.array_equal(raw(np.ascontiguousarray(X)), raw(np.ascontiguousarray(X.T)))
    assert np.min(np.linalg.eigvalsh(X)) >= -64 * EPS * np.linalg.norm(X, 2)
    # prefixes
    assert same_bytes(p1, win[:1]) and same_bytes(p2, win[:2])
    assert np.array_equal(raw(np.ascontiguousarray(X1)), raw(np.ascontiguousarray(X[:6, :6])))
    assert np.array_equal(raw(np.ascontiguousarray(X2)), raw(np.ascontiguousarray(X[:12, :12])))
    # every block against the longdouble J_a P J_b^T, normalised by sqrt(C_aa,ii C_bb,jj)
    Xt = abi.window_joint_model_as(x, P, m, np.longdouble)
    Xm = abi.window_joint_model(x, P, m)
    dg = np.sqrt(np.diag(Xt))
    e = float(np.max(np.abs(np.asarray(X, np.longdouble) - Xt) / np.outer(dg, dg)))
    floor = float(np.max(np.abs(np.asarray(Xm, np.longdouble) - Xt) / np.outer(dg, dg)))
    print("max_track_len %d, joint %d x %d: e = %.3e, float64 model (the floor) e = %.3e" % (max_len, 6 * m, 6 * m, e, floor))
    assert e <= 1e-11, (e, floor)


# ---------------------------------------------------------------- 4  the ring over the 12 recorded frames
@pytest.fixture(scope="module")
def staged(gpu_required, recs_b):
    """the 12 frames stage by stage on three handles: `h` with the edge ring at (2, 3), `g` at (0, 3), capacity 16; `t`, their twin, with no
    edge ring, asked for both edges behind every frame once its window reaches"""
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    h, g, t = hip.RvioHip(cfg), hip.RvioHip(cfg), hip.RvioHip(cfg)
    for q in (h, g, t):
        q.set_odometry(16)
    h.set_edge_odometry(16, 2, 3)
    g.set_edge_odometry(16, 0, 3)
    seqno, none = h.edge_odometry_all()
    assert seqno == 0 and len(h.edge_odometry()) == 0 and not raw(none).any()
    for q in (h, g, t):
        q.initialize(*seq.init_from_static(38))
    twin, counts = [], []
    for r in recs:
        for q in (h, g, t):
            staged_frame(q, r["inp"])
        ncl = int(t.odometry_all()[1]["n_clones"][0])
        twin.append(t.get_window_edges([(2, 3), (0, 3)]) if ncl >= 3 else None)
        counts.append((h.edge_odometry_all()[0], g.edge_odometry_all()[0]))
    rings = (h.edge_odometry(), g.edge_odometry())
    odom = t.odometry()
    states = [q.get_state() for q in (h, g, t)]
    info = h.frame_info()
    for q in (h, g, t):
        q.close()
    assert info["device_error"] == 0 and info["updated"] == 1, info
    return rings, odom, twin, counts, states


def test_ring_records_equal_the_twin_handle(staged):
    rings, odom, twin, counts, states = staged
    n_cl = [int(v) for v in odom["n_clones"]]
    assert n_cl[0] < 3 <= n_cl[-1]
    want = [k for k in range(N) if n_cl[k] >= 3]
    expect = [sum(1 for k in want if k <= f) for f in range(N)]                   # nothing until n_clones >= age_old, then one per frame
    assert [c[0] for c in counts] == expect and [c[1] for c in counts] == expect and expect[want[0] - 1] == 0
    for which, (ring, (a, b)) in enumerate(zip(rings, ((2, 3), (0, 3)))):
        assert len(ring) == len(want) and [int(s) for s in ring["seq"]] == list(range(1, len(want) + 1))
        for rec, k in zip(ring, want):
            assert (int(rec["age_new"]), int(rec["age_old"]), int(rec["n_clones"])) == (a, b, n_cl[k])
            assert int(rec["img_count_new"]) == int(odom["img_count"][k]) - a and int(rec["img_count_old"]) == int(odom["img_count"][k]) - b
            assert same_body(rec, twin[k][which]), (a, b, k)                        # = get_window_edges behind the same frame on the twin
    # the handles with the ring on end in the twin's state bytes
    for x, P in states[:2]:
        assert np.array_equal(raw(x), raw(states[2][0])) and np.array_equal(raw(P), raw(states[2][1]))


def test_the_ring(gpu_required, recs_b, staged):
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    ref = staged[0][0]                                          # (2, 3): 9 records over the 12 frames
    assert len(ref) == 9
    h = hip.RvioHip(cfg)
    h.set_edge_odometry(4, 2, 3)

    def feed(lo, hi):
        for r in recs[lo:hi]:
            inp = r["inp"]
            h.frame_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])

    h.initialize(*seq.init_from_static(38))
    feed(0, 3)
    assert len(h.edge_odometry()) == 0 and h.edge_odometry_all()[0] == 0
    feed(3, 11)
    got = h.edge_odometry(first_seq=1)
    assert [int(s) for s in got["seq"]] == [5, 6, 7, 8] and same_bytes(got, ref[4:8])                    # wrapped
    assert same_bytes(h.edge_odometry(first_seq=7), ref[6:8])
    assert same_bytes(h.edge_odometry(first_seq=-5, max_n=2), ref[4:6])
    assert len(h.edge_odometry(first_seq=9)) == 0
    seqno, newest = h.edge_odometry_all()
    assert seqno == 8 and same_bytes(newest, ref[7:8])
    # capacity 0: the ring no longer advances, the records stay; on again with the same capacity and ages: it goes on
    h.set_edge_odometry(0, 2, 3)
    feed(11, 12)
    assert same_bytes(h.edge_odometry(), ref[4:8]) and h.edge_odometry_all()[0] == 8
    h.set_edge_odometry(4, 2, 3)
    assert same_bytes(h.edge_odometry(), ref[4:8])
    # other ages empty it, like another capacity
    h.set_edge_odometry(4, 1, 3)
    assert len(h.edge_odometry()) == 0 and h.edge_odometry_all()[0] == 0
    h.set_edge_odometry(4, 2, 3)
    h.set_edge_odometry(5, 2, 3)
    assert len(h.edge_odometry()) == 0 and h.edge_odometry_all()[0] == 0
    # initialize restarts at seq 1; set_state leaves the ring alone
    h.set_edge_odometry(4, 2, 3)
    h.initialize(*seq.init_from_static(38))
    feed(0, 4)                                                  # (the frames before the first update: a handle that has run frames draws other RANSAC samples)
    assert same_bytes(h.edge_odometry(), ref[0:1])
    h.set_state(*h.get_state())
    assert same_bytes(h.edge_odometry(), ref[0:1])
    # a back end's odometry chain: the oldest clone behind every frame waits until the window is full
    ml = cfg.max_track_len
    h.set_edge_odometry(4, ml - 2, ml - 1)
    h.initialize(*seq.init_from_static(38))
    feed(0, 12)
    got = h.edge_odometry()
    assert len(got) == int(np.sum(staged[1]["n_clones"] >= ml - 1)) > 0 and np.all(got["age_old"] == ml - 1) and np.all(got["age_new"] == ml - 2)
    h.close()


# ---------------------------------------------------------------- 5  batch handles
def test_batch_of_three_equals_three_plain_handles(gpu_required):
    import torch
    n, B = 10, 3
    hb = built_handle(n + 1, batch=B)
    pairs = pairs_of(n) + [(3, 7)]
    edges, joints = [], []
    for i in range(B):
        hb.set_state_at(i, *W.built_state(n, seed=i))
        hi = built_handle(n + 1, seed=i)
        edges.append(hi.get_window_edges(pairs))
        joints.append(hi.get_window_joint())
        hi.close()
        assert same_bytes(hb.get_window_edges(pairs, instance=i), edges[i])
        pj, Xj = hb.get_window_joint(instance=i)
        assert same_bytes(pj, joints[i][0]) and np.array_equal(raw(Xj), raw(joints[i][1]))
    assert not np.array_equal(edges[0]["p"], edges[1]["p"])
    # _dev, edges: the pairs and one beyond the window, a stride with padding
    dev_pairs = pairs + [(2, n + 1), (4, 4), (-1, 3)]
    npairs, stride = len(dev_pairs), len(dev_pairs) + 2
    d_new = torch.tensor([p[0] for p in dev_pairs], dtype=torch.int32).cuda()
    d_old = torch.tensor([p[1] for p in dev_pairs], dtype=torch.int32).cuda()
    buf = torch.full((B * stride * 376,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    hb.get_window_edges_dev(npairs, d_new.data_ptr(), d_old.data_ptr(), buf.data_ptr(), stride)
    hb.sync()
    got = buf.cpu().numpy().view(abi.WINDOW_EDGE_DTYPE).reshape(B, stride)
    for i in range(B):
        assert same_bytes(got[i, : len(pairs)], edges[i]), i
        for beyond in got[i, len(pairs): npairs]:
            assert int(beyond["img_count_new"]) == -1 and int(beyond["n_clones"]) == n
            for f in ("seq", "img_count_old", "age_new", "age_old", "reserved", "p", "q", "cov"):
                assert not np.any(beyond[f]), f
        assert np.all(raw(got[i, npairs:]) == 0xAB)
    # _dev, joint: ages 0 .. n + 1, one beyond the window
    m = n + 2
    pbuf = torch.full((B * (m + 1) * 368,), 0xAB, dtype=torch.uint8, device="cuda")
    cbuf = torch.full((B * (36 * m * m + 5),), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    hb.get_window_joint_dev(m, pbuf.data_ptr(), m + 1, cbuf.data_ptr(), 36 * m * m + 5)
    hb.sync()
    gp = pbuf.cpu().numpy().view(abi.WINDOW_POSE_DTYPE).reshape(B, m + 1)
    gc = cbuf.cpu().numpy().reshape(B, 36 * m * m + 5)
    for i in range(B):
        X = gc[i, : 36 * m * m].reshape(6 * m, 6 * m)
        assert same_bytes(gp[i, : n + 1], joints[i][0]) and np.array_equal(raw(np.ascontiguousarray(X[: 6 * (n + 1), : 6 * (n + 1)])), raw(joints[i][1]))
        assert int(gp[i, n + 1]["img_count"]) == -1 and int(gp[i, n + 1]["n_clones"]) == n and not np.any(gp[i, n + 1]["pose_cov"])
        assert not X[6 * (n + 1):, :].any() and not X[:, 6 * (n + 1):].any()
        assert np.all(raw(gp[i, m:]) == 0xAB) and np.all(gc[i, 36 * m * m:] == 7.0)
    hb.close()


# ---------------------------------------------------------------- 6  errors
def test_errors(gpu_required, recs_b):
    from rvio_amd import hip
    cfg, seq, recs = recs_b
    h = hip.RvioHip(cfg)
    L = h.L
    n, seqno, rec, prec = C.c_int32(-1), C.c_int64(0), (abi.rvio_window_edge * 16)(), (abi.rvio_window_pose * 16)()
    cov = (C.c_double * (96 * 96))()
    a1, b1 = (C.c_int32 * 2)(0, 0), (C.c_int32 * 2)(1, 1)
    ml = cfg.max_track_len

    def err():
        return L.rvio_hip_last_error(h.h)

    # RVIO_ERR_STATE (-4): no state yet; the ring never enabled
    assert L.rvio_hip_get_window_edges(h.h, 0, 1, a1, b1, rec) == -4 and b"rvio_hip_get_window_edges before the first" in err()
    assert L.rvio_hip_get_window_edges_dev(h.h, 1, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), C.c_size_t(1)) == -4
    assert L.rvio_hip_get_window_joint(h.h, 0, 4, prec, cov, C.c_size_t(24), C.byref(n)) == -4 and b"rvio_hip_get_window_joint before the first" in err()
    assert L.rvio_hip_get_window_joint_dev(h.h, 1, C.c_void_p(8), C.c_size_t(1), C.c_void_p(8), C.c_size_t(36)) == -4
    assert L.rvio_hip_get_edge_odometry(h.h, 0, C.c_int64(1), 1, rec, C.byref(n)) == -4 and b"edge-odometry ring was never enabled" in err()
    assert L.rvio_hip_get_edge_odometry_all(h.h, rec, C.byref(seqno)) == -4
    # RVIO_ERR_INVALID (-1): the ring
    assert L.rvio_hip_set_edge_odometry(h.h, 65537, 0, 1) == -1 and b"capacity" in err()
    assert L.rvio_hip_set_edge_odometry(h.h, -1, 0, 1) == -1
    assert L.rvio_hip_set_edge_odometry(h.h, 4, -1, 1) == -1 and b"0 <= age_new < age_old <= max_track_len - 1" in err()
    assert L.rvio_hip_set_edge_odometry(h.h, 4, 2, 2) == -1
    assert L.rvio_hip_set_edge_odometry(h.h, 4, 3, 2) == -1
    assert L.rvio_hip_set_edge_odometry(h.h, 4, 0, ml) == -1
    assert L.rvio_hip_set_edge_odometry(h.h, 0, 0, ml) == -1
    assert L.rvio_hip_get_edge_odometry(h.h, 0, C.c_int64(1), 1, rec, C.byref(n)) == -4                   # still never enabled
    h.set_edge_odometry(4, ml - 2, ml - 1)
    assert L.rvio_hip_get_edge_odometry(h.h, 1, C.c_int64(1), 1, rec, C.byref(n)) == -1                   # no instance 1
    assert L.rvio_hip_get_edge_odometry(h.h, 0, C.c_int64(1), -1, rec, C.byref(n)) == -1
    assert L.rvio_hip_get_edge_odometry(h.h, 0, C.c_int64(1), 1, None, C.byref(n)) == -1
    assert L.rvio_hip_get_edge_odometry(h.h, 0, C.c_int64(1), 0, None, C.byref(n)) == 0 and n.value == 0
    assert L.rvio_hip_get_edge_odometry_all(h.h, None, C.byref(seqno)) == -1
    h.set_state(*W.built_state(ml - 1))
    # RVIO_ERR_INVALID: the edges
    assert L.rvio_hip_get_window_edges(h.h, 0, 1, None, b1, rec) == -1 and b"NULL" in err()
    assert L.rvio_hip_get_window_edges(h.h, 0, 1, a1, None, rec) == -1
    assert L.rvio_hip_get_window_edges(h.h, 0, 1, a1, b1, None) == -1
    assert L.rvio_hip_get_window_edges(h.h, 1, 1, a1, b1, rec) == -1 and b"instance out of range" in err()
    assert L.rvio_hip_get_window_edges(h.h, 0, 0, a1, b1, rec) == -1 and b"n_pairs outside 1 .. 528" in err()
    assert L.rvio_hip_get_window_edges(h.h, 0, 529, a1, b1, rec) == -1
    for bad in ((1, 1), (2, 1), (-1, 1), (0, ml)):
        a2, b2 = (C.c_int32 * 2)(0, bad[0]), (C.c_int32 * 2)(1, bad[1])
        assert L.rvio_hip_get_window_edges(h.h, 0, 2, a2, b2, rec) == -1 and b"pair 1" in err(), bad
    assert L.rvio_hip_get_window_edges(h.h, 0, 2, a1, b1, rec) == 0 and rec[1].age_old == 1
    assert L.rvio_hip_get_window_edges_dev(h.h, 1, None, C.c_void_p(8), C.c_void_p(8), C.c_size_t(1)) == -1 and b"NULL" in err()
    assert L.rvio_hip_get_window_edges_dev(h.h, 1, C.c_void_p(8), None, C.c_void_p(8), C.c_size_t(1)) == -1
    assert L.rvio_hip_get_window_edges_dev(h.h, 1, C.c_void_p(8), C.c_void_p(8), None, C.c_size_t(1)) == -1
    assert L.rvio_hip_get_window_edges_dev(h.h, 0, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), C.c_size_t(1)) == -1
    assert L.rvio_hip_get_window_edges_dev(h.h, 65536, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), C.c_size_t(65536)) == -1
    assert L.rvio_hip_get_window_edges_dev(h.h, 3, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), C.c_size_t(2)) == -1 and b"out_stride is below n_pairs" in err()
    # RVIO_ERR_INVALID: the joint covariance
    assert L.rvio_hip_get_window_joint(h.h, 0, 4, None, cov, C.c_size_t(24), C.byref(n)) == -1 and b"NULL" in err()
    assert L.rvio_hip_get_window_joint(h.h, 0, 4, prec, None, C.c_size_t(24), C.byref(n)) == -1
    assert L.rvio_hip_get_window_joint(h.h, 0, 4, prec, cov, C.c_size_t(24), None) == -1
    assert L.rvio_hip_get_window_joint(h.h, 1, 4, prec, cov, C.c_size_t(24), C.byref(n)) == -1 and b"instance out of range" in err()
    assert L.rvio_hip_get_window_joint(h.h, 0, 0, prec, cov, C.c_size_t(24), C.byref(n)) == -1 and b"max_n < 1" in err()
    assert L.rvio_hip_get_window_joint(h.h, 0, 4, prec, cov, C.c_size_t(23), C.byref(n)) == -1 and b"ld is below 6 max_n" in err()
    assert L.rvio_hip_get_window_joint(h.h, 0, 4, prec, cov, C.c_size_t(24), C.byref(n)) == 0 and n.value == 4
    assert L.rvio_hip_get_window_joint_dev(h.h, 1, None, C.c_size_t(1), C.c_void_p(8), C.c_size_t(36)) == -1 and b"NULL" in err()
    assert L.rvio_hip_get_window_joint_dev(h.h, 1, C.c_void_p(8), C.c_size_t(1), None, C.c_size_t(36)) == -1
    assert L.rvio_hip_get_window_joint_dev(h.h, 0, C.c_void_p(8), C.c_size_t(1), C.c_void_p(8), C.c_size_t(36)) == -1
    assert L.rvio_hip_get_window_joint_dev(h.h, 33, C.c_void_p(8), C.c_size_t(33), C.c_void_p(8), C.c_size_t(36 * 33 * 33)) == -1
    assert L.rvio_hip_get_window_joint_dev(h.h, 2, C.c_void_p(8), C.c_size_t(1), C.c_void_p(8), C.c_size_t(144)) == -1 and b"pose_stride is below n_ages" in err()
    assert L.rvio_hip_get_window_joint_dev(h.h, 2, C.c_void_p(8), C.c_size_t(2), C.c_void_p(8), C.c_size_t(143)) == -1 and b"cov_stride is below" in err()
    h.close()
    # a ring beyond 1 GiB is refused with the size in the text
    hb = hip.RvioHip(cfg, batch=50)
    assert hb.L.rvio_hip_set_edge_odometry(hb.h, 65536, 0, 1) == -3 and b"1 GiB" in hb.L.rvio_hip_last_error(hb.h)
    hb.close()
