"""CPU-side checks of the pose-graph export's C-ABI surface (added within ABI 6): the seven entry points are exported and declared,
rvio_window_edge has the layout a C++ compiler gives the header's struct (tests/hostemu/window_edge_layout.cpp), NULL handles are refused, and
the NumPy statements of csrc/window_edge.hip hold their conventions: abi.window_edge_model is abi.rel_h and the RVIO_REL_POSE rows of
abi.rel_model at lever 0, a consecutive edge is the clone's block of P with its 3-blocks swapped, abi.window_joint_model's diagonal is
abi.window_pose_model, and the identity G Joint[{a, b}] G^T = edge cov pins the two conventions to each other.  No compute is launched here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
import window_cases as W

abi = O.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rvio_hip_get_window_edges", "rvio_hip_get_window_edges_dev", "rvio_hip_set_edge_odometry", "rvio_hip_get_edge_odometry",
       "rvio_hip_get_edge_odometry_all", "rvio_hip_get_window_joint", "rvio_hip_get_window_joint_dev")
FIELDS = ("seq", "img_count_new", "img_count_old", "age_new", "age_old", "n_clones", "reserved", "p", "q", "cov")
CASES = [(n, a, b) for n in (2, 10, 31) for a, b in ((0, 1), (0, n), (n - 1, n), (1, n - 1)) if 0 <= a < b <= n]


@pytest.fixture(scope="module")
def lib():
    from rvio_amd import build, hip
    build.build()
    return hip.load()


def test_symbols_exported_and_declared_within_abi_6(lib):
    from rvio_amd import hip
    assert abi.ABI_VERSION == 6 and lib.rvio_hip_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "rvio_hip.h")).read()
    declared = set(re.findall(r"\b(rvio_(?:hip_)?[a-z_]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in hip.SYMBOLS and hasattr(lib, s), s
    # what is not done is said in the header
    for phrase in ("correlation between successive ring edges", "already left the window", "(qk, pk) as an endpoint", "information-matrix / g2o",
                   "interpolation between frames"):
        assert phrase in hdr, phrase


def test_record_layout_matches_a_cxx_compiler(tmp_path):
    assert C.sizeof(abi.rvio_window_edge) == 376 and abi.WINDOW_EDGE_DTYPE.itemsize == 376
    exe = str(tmp_path / "layout")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "hostemu", "window_edge_layout.cpp"), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got[0] == 376
    assert got[1:] == [getattr(abi.rvio_window_edge, f).offset for f in FIELDS]
    assert got[1:] == [abi.WINDOW_EDGE_DTYPE.fields[f][1] for f in FIELDS]
    assert got[1:] == [0, 8, 12, 16, 20, 24, 28, 32, 56, 88]          # no padding: 8 + 6 * 4 + 8 * (3 + 4 + 36) = 376


def test_null_handle_is_invalid(lib):
    n, seq = C.c_int32(0), C.c_int64(0)
    rec, pose, a, b, cov = abi.rvio_window_edge(), abi.rvio_window_pose(), C.c_int32(0), C.c_int32(1), (C.c_double * 36)()
    assert lib.rvio_hip_get_window_edges(None, 0, 1, C.byref(a), C.byref(b), C.byref(rec)) == -1
    assert lib.rvio_hip_get_window_edges_dev(None, 1, C.byref(a), C.byref(b), C.byref(rec), C.c_size_t(1)) == -1
    assert lib.rvio_hip_set_edge_odometry(None, 16, 0, 1) == -1
    assert lib.rvio_hip_get_edge_odometry(None, 0, C.c_int64(1), 1, C.byref(rec), C.byref(n)) == -1
    assert lib.rvio_hip_get_edge_odometry_all(None, C.byref(rec), C.byref(seq)) == -1
    assert lib.rvio_hip_get_window_joint(None, 0, 1, C.byref(pose), cov, C.c_size_t(6), C.byref(n)) == -1
    assert lib.rvio_hip_get_window_joint_dev(None, 1, C.byref(pose), C.c_size_t(1), cov, C.c_size_t(36)) == -1


# ---------------------------------------------------------------- the model's conventions
@pytest.mark.parametrize("n,a,b", CASES)
def test_edge_model_is_rel_h_and_the_rel_pose_rows(n, a, b):
    x, P = W.built_state(n)
    p, q, cov = abi.window_edge_model(x, P, a, b)
    z = abi.rel_h(x, a, b)
    assert np.array_equal(p, z[0:3]) and np.array_equal(q, z[3:7]) and q[3] >= 0
    fix = abi.make_fix(p=z[0:3], q=z[3:7])                      # lever 0
    H, r, _ = abi.rel_model(x, abi.RVIO_REL_POSE, fix, a, b)
    assert np.array_equal(abi.window_edge_jacobian(x, a, b), H)
    assert np.max(np.abs(r)) <= 8 * W.EPS                        # the edge handed back as a measurement has no residual
    Cm = H @ P @ H.T
    assert np.array_equal(cov, 0.5 * (Cm + Cm.T)) and np.array_equal(cov, cov.T)
    # columns outside the span are zero
    keep = np.zeros(H.shape[1], bool)
    keep[24 + 6 * (n - b): 24 + 6 * (n - a)] = True
    assert not H[:, ~keep].any() and H[:, keep].any()
    # the twin
    pt, qt, ct = abi.window_edge_model_as(x, P, a, b, np.longdouble)
    assert pt.dtype == qt.dtype == ct.dtype == np.longdouble
    assert np.max(np.abs(p - pt)) <= 1e-14 and W.quat_close(q, np.asarray(qt, float), 1e-14) and W.cov_err(cov, ct) <= 1e-13


@pytest.mark.parametrize("n", (2, 10, 31))
def test_a_consecutive_edge_is_the_clone(n):
    """b = a + 1: p, q are clone n - b as the state holds it and cov is its block of P with the two 3-blocks swapped (P: rotation, position)"""
    x, P = W.built_state(n)
    for a in sorted({0, 1, n - 1}):
        if a + 1 > n:
            continue
        i = n - a - 1
        p, q, cov = abi.window_edge_model(x, P, a, a + 1)
        assert np.max(np.abs(p - x[30 + 7 * i: 33 + 7 * i])) <= 4 * W.EPS and W.quat_close(q, x[26 + 7 * i: 30 + 7 * i], 4 * W.EPS)
        c = 24 + 6 * i
        idx = np.r_[c + 3: c + 6, c: c + 3]
        blk = P[np.ix_(idx, idx)]
        assert W.cov_err(cov, blk) <= 64 * W.EPS, (a, W.cov_err(cov, blk))


@pytest.mark.parametrize("n", (2, 10, 31))
def test_joint_model_diagonal_is_the_window_pose_model(n):
    x, P = W.built_state(n)
    m = n + 1
    X = abi.window_joint_model(x, P, m)
    assert X.shape == (6 * m, 6 * m) and np.array_equal(X, X.T)
    for a in range(m):
        assert np.array_equal(X[6 * a: 6 * a + 6, 6 * a: 6 * a + 6], abi.window_pose_model(x, P, a)[2]), a
    assert np.array_equal(abi.window_joint_model(x, P, 2), X[:12, :12])
    Xt = abi.window_joint_model_as(x, P, m, np.longdouble)
    assert Xt.dtype == np.longdouble and W.cov_err(X, Xt) <= 1e-13
    for a in W.ages_of(n):
        assert W.cov_err(Xt[6 * a: 6 * a + 6, 6 * a: 6 * a + 6], W.truth(n, a)[2]) <= 1e-17


@pytest.mark.parametrize("n,a,b", CASES)
def test_the_identity_that_pins_both_conventions(n, a, b):
    """G maps the world-pose errors of the frames a, b (pose_cov's convention) to the edge's error: H = G [J_a; J_b] by the chain rule, so
    G Joint[{a, b}] G^T = the edge's cov.  Both sides in np.longdouble, held to 1e-11 in cov_err's metric; what float64 gives for the same
    product is printed: the cancellation the direct kernel avoids."""
    x, P = W.built_state(n)
    ld = np.longdouble
    G = abi.window_edge_from_poses(x, a, b, ld)
    Ja, Jb = abi.window_pose_jacobian_as(x, a, ld), abi.window_pose_jacobian_as(x, b, ld)
    J = np.vstack([Ja, Jb])
    Pl = np.asarray(P, ld)
    joint = J @ Pl @ J.T
    lhs = G @ joint @ G.T
    _, _, ct = abi.window_edge_model_as(x, P, a, b, ld)
    e = W.cov_err(0.5 * (lhs + lhs.T), ct)
    # the same product in float64: from the joint covariance the device publishes
    G64 = abi.window_edge_from_poses(x, a, b, float)
    J64 = np.vstack([abi.window_pose_jacobian(x, a), abi.window_pose_jacobian(x, b)])
    via64 = G64 @ (J64 @ P @ J64.T) @ G64.T
    e64 = W.cov_err(0.5 * (via64 + via64.T), ct)
    direct = W.cov_err(abi.window_edge_model(x, P, a, b)[2], ct)
    print("n = %d, edge (%d, %d): identity in longdouble e = %.3e; through the float64 joint covariance e = %.3e; the direct float64 form e = %.3e"
          % (n, a, b, e, e64, direct))
    assert e <= 1e-11, e
    # and the chain rule itself
    Ht = G @ J
    assert float(np.max(np.abs(Ht - np.asarray(abi.window_edge_jacobian(x, a, b), ld)))) <= 1e-14
