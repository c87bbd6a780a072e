"""PreIntegrator::propagate on the device at the IMU batch shapes of tests/propagate_cases.py, through every launch form of propagate_body
(csrc/filter_kernels2.hip), against the oracle's sample-by-sample recursion.

Which entry point reaches which form (propagate_dev and frame_dev_impl in csrc/rvio_hip.hip):
  * rvio_hip_propagate[_dev] on a plain handle: propagate_chol_kernel<2> at 6n_max <= 64 and <3> at 65..96 — once the window holds a clone: the
    Cholesky role needs n >= 1, so the EMPTY window of such a handle launches propagate_kernel3 —, propagate_kernel3 above 96;
  * rvio_hip_frame_tracks_dev on a batch handle of 2..8 instances with per-instance IMU batches: propagate_kernel3 with the slab stride; of more
    than 8: propagate_kernel3b (chunks of 8; at 6n > 144 its clone cross-columns take two staging tiles).  A batch handle has no propagate-only
    entry with per-instance batches: the frame runs with empty hand-over tables (n_feat = 0) and is compared with the oracle's propagate followed
    by its augment / compose;
  * rvio_hip_frame / rvio_hip_frame_dev (the pipelined image path) with an update in the frame: the last workgroup of feat_prop_kernel.
    rvio_hip_frame_points does NOT: it propagates through the staged forms of the first item.

Bars: states 1e-9 (1e-8 for batch instances at the long window, as tests/test_gpu_batch.py and test_gpu_windows.py have it), P by p_close of
tests/test_gpu_filter.py on the whole matrix, and max |dP_ij| / sqrt(P_ii P_jj) <= propagate_cases.P_NORM_BAR over the head and the head-by-clone
cross block (measured figures: profiles/propagate_edges.md).  Every case prints its figures before it asserts."""
import functools

import numpy as np
import pytest

import propagate_cases as PC

O, S = PC.O, PC.S
abi, rv = O.abi, O.rv
pytestmark = pytest.mark.gpu

PLAIN_FORM = {"empty": "propagate_kernel3 (n = 0)", "window10": "propagate_chol_kernel<2>", "mid": "propagate_chol_kernel<3>", "long": "propagate_kernel3"}
PLAIN_CASES = [("irregular", m) for m in PC.M_EDGES] + [("branch", 10), ("branch", 17)]
BATCH_CASES = [("irregular", m) for m in (1, 7, 8, 9, 16, 17, 33)] + [("branch", 9)]
FUSED_MS = (1, 16, 17, 33)
# the fused frame ends behind the update and the Joseph form, whose rounding the normalised figure then carries: measured worst 2.17e-12 (mid window,
# m = 33; profiles/propagate_edges.md), the bar by the same rule as propagate_cases.P_NORM_BAR — 10 x the worst, rounded up to a power of ten
FUSED_P_NORM_BAR = 1e-10
assert FUSED_P_NORM_BAR <= 1e-8


def figures(form, tag, x, P, xo, Po):
    d = S.state_delta(x, xo), PC.p_proj(P, Po), PC.p_norm(P, Po)
    print("PROPEDGE | %s | %s | state %.3e | P project %.3e | P normalised %.3e" % ((form, tag) + d))
    return d


def held(form, tag, x, P, xo, Po, x_tol=PC.X_TOL):
    assert x.shape == xo.shape and np.all(np.isfinite(x)) and np.all(np.isfinite(P)), tag
    d = figures(form, tag, x, P, xo, Po)
    assert d[0] <= x_tol, (tag, d)
    assert PC.p_close(P, Po), (tag, d)
    assert d[2] <= PC.P_NORM_BAR, (tag, d)


@pytest.fixture(scope="module")
def handles(gpu_required):
    """one plain handle per (state, kind): the cfg of a branch case differs in small_angle"""
    from rvio_amd import hip
    hs = {}

    def get(state, kind):
        if (state, kind) not in hs:
            hs[state, kind] = hip.RvioHip(PC.case_cfg(state, kind))
        return hs[state, kind]
    yield get
    for h in hs.values():
        h.close()


def to_dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8) if a.dtype.fields else np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


# ------------------------------------------------------------------------------------------------ plain staged forms
@pytest.mark.parametrize("kind,m", PLAIN_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("state", PC.STATES)
def test_plain_staged_forms(handles, state, kind, m):
    cfg, x, P, imu, (xo, Po) = PC.case(state, kind, m)
    PC.conditions(state, kind, m)                         # the case can fail (CPU, from the oracle alone)
    h = handles(state, kind)
    h.set_state(x, P)
    h.propagate(imu)
    xa, Pa = h.get_state()
    d_imu = to_dev(imu)
    h.set_state(x, P)
    h.propagate_dev(d_imu.data_ptr(), len(imu))
    xb, Pb = h.get_state()
    assert h.frame_info()["device_error"] == 0
    assert np.array_equal(xa, xb) and np.array_equal(Pa, Pb)                      # host and device batches end on the same bits
    held(PLAIN_FORM[state], "%s %s(%d)" % (state, kind, m), xa, Pa, xo, Po)
    # what propagation does not touch keeps its bits: the clone block, and the state outside qk, pk, vk
    assert np.array_equal(Pa[24:, 24:], P[24:, 24:])
    keep = np.r_[0:10, 20:len(x)]
    assert np.array_equal(xa[keep], x[keep])
    assert np.array_equal(Pa, Pa.T)


# ------------------------------------------------------------------------------------------------ batch forms
@pytest.mark.parametrize("kind,m", BATCH_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("B", [3, 9])                 # 3: propagate_kernel3 with the slab stride; 9: the smallest batch that launches propagate_kernel3b
@pytest.mark.parametrize("state", ["window10", "long"])
def test_batch_forms(gpu_required, state, B, kind, m):
    """every instance its own batch of the same m (seed = instance: other dt, other positions of the slow and zero-dt samples)"""
    from rvio_amd import hip
    cfg = PC.case_cfg(state, kind)
    x, P = PC.state(state)
    cases = [PC.case(state, kind, m, seed) for seed in range(B)]
    if m > 8:
        for seed in range(B):
            PC.conditions(state, kind, m, seed)
    imu = np.stack([c[3] for c in cases])
    assert imu.shape == (B, m) and not np.array_equal(imu[0], imu[1])
    Fu, ML = abi.fu(cfg), cfg.max_track_len
    tables = [to_dev(a) for a in (np.zeros(B, np.int32), np.zeros((B, Fu), np.uint8), np.zeros((B, Fu), np.int32), np.zeros((B, Fu, ML, 2), np.float32))]
    d_imu = to_dev(imu)
    form = "propagate_kernel3 (batch %d)" % B if B <= 8 else "propagate_kernel3b"
    x_tol, tol_plain = (PC.X_TOL, 1e-11) if state == "window10" else (1e-8, 1e-10)
    hb, hp = hip.RvioHip(cfg, batch=B), hip.RvioHip(cfg)
    try:
        hb.set_state(x, P)
        for i in range(B):
            hb.set_state_at(i, x, P)
        hb.L.rvio_hip_frame_plan(hb.h, None, None)        # (img_count > 1 behind the call below: the frame augments, as every frame but the first does)
        hb.frame_tracks_dev(d_imu.data_ptr(), m, m, *[t.data_ptr() for t in tables])
        hb.sync()
        info = hb.frame_info()
        assert info["device_error"] == 0 and info["updated"] == 0, info
        for i in range(B):
            xo, Po = cases[i][4]
            xo, Po, _, _ = O.augment_compose(cfg, xo, Po, True)
            xa, Pa = hb.get_state_at(i)
            held(form, "%s %s(%d) instance %d" % (state, kind, m, i), xa, Pa, xo, Po, x_tol)
            if i in (0, B - 1):
                hp.set_state(x, P)
                hp.propagate(imu[i])
                hp.augment_compose(True)
                xb, Pb = hp.get_state()
                assert S.state_delta(xa, xb) <= tol_plain and float(np.max(np.abs(Pa - Pb))) <= tol_plain * float(np.max(np.abs(Pb))), (state, B, kind, m, i)
        assert hp.frame_info()["device_error"] == 0
    finally:
        hb.close()
        hp.close()


# ------------------------------------------------------------------------------------------------ fused form
@functools.lru_cache(maxsize=None)
def rendered(k):
    """image k of the sequence both windows were recorded on (the cfgs differ in max_track_len only)"""
    return PC.recorded("window10")[0].render(k)


def corners(seq, k):
    xy, vis = seq.project(k, noise=False)
    return seq.candidates(k, xy, vis)[0]


@pytest.mark.parametrize("m", FUSED_MS)
@pytest.mark.parametrize("state", ["window10", "mid"])
def test_fused_form(gpu_required, state, m):
    """The recorded frame that starts on the full window, through rvio_hip_frame: its update rides behind feat_prop_kernel, whose last workgroup
    propagates.  The tracker gets its history from the images of the frames before (front end only: rvio_hip_track), the filter starts from
    set_state, and the frame's IMU batch is irregular(m) — RANSAC's gyro prior sees it too, so the tracks are the ones this frame hands over.
    Against the oracle's propagate, update and augment on those tracks, and against the staged sequence on a second handle (the bar of
    tests/test_gpu_solve9.py between two routes to the same update: 1e-12).  (On the CPU the oracle's tracker hands over 100 tracks at every m
    and the update is applied.)"""
    from rvio_amd import hip
    cfg = PC.config(state)
    seq, _ = PC.recorded(state)
    r = PC.frame_record(state)
    k, x, P = r["k"], r["x0"], r["P0"]
    assert (cfg.width, cfg.height, seq.seed) == (PC.config("window10").width, PC.config("window10").height, PC.recorded("window10")[0].seed)
    imu = PC.irregular(m, x)[0]
    if m > 8:
        PC.conditions(state, "irregular", m)
    h, hs = hip.RvioHip(cfg), hip.RvioHip(cfg)
    try:
        for kk in range(39, k):
            h.track(rendered(kk), seq.imu_between(kk), corners(seq, kk))
        h.sync()
        assert len(h.get_points()[0]) > 100
        h.set_state(x, P)
        h.L.rvio_hip_frame_plan(h.h, None, None)          # (img_count > 1 in the frame below: it augments)
        h.frame(rendered(k), imu, corners(seq, k))
        h.sync()
        info = h.frame_info()
        xa, Pa = h.get_state()
        types, lens, meas = h.get_tracks()
        dg = h.update_diag()
        assert info["device_error"] == 0 and info["updated"] == 1 and len(types) > 50, info          # the frame did update
        x1, P1 = O.propagate(cfg, x, P, imu)
        x2, P2, od = O.update(cfg, x1, P1, types, lens, meas)
        assert od["updated"] and np.array_equal(dg["accepted"], od["accepted"])
        xo, Po, _, _ = O.augment_compose(cfg, x2, P2, True)
        d = figures("feat_prop_kernel", "%s irregular(%d)" % (state, m), xa, Pa, xo, Po)
        assert np.all(np.isfinite(xa)) and np.all(np.isfinite(Pa))
        assert d[0] <= PC.X_TOL and PC.p_close(Pa, Po) and d[2] <= FUSED_P_NORM_BAR, d
        hs.set_state(x, P)
        hs.propagate(imu)
        hs.update(types, lens, meas)
        hs.augment_compose(True)
        xb, Pb = hs.get_state()
        assert hs.frame_info()["device_error"] == 0
        assert S.state_delta(xa, xb) <= 1e-12 and np.max(np.abs(Pa - Pb)) <= 1e-12 * np.max(np.abs(Pb)), (state, m)
    finally:
        h.close()
        hs.close()
