"""The device at EVERY accepted window length and at the edges of the feature count.

rvio_hip_create accepts max_track_len 3..32 and n_features 2..4096; between the five configurations of BASELINE.json the host picks other
kernels, templates and LDS layouts by threshold (r-vio_amd/csrc/launch_plan.h; pinned on the CPU by tests/test_launch_plan.py): the solve's
tile count at 6n <= 64 / 96 / 128, the Cholesky role in the per-feature launch at 6n <= 96, one image chain at 6n > 96, 128- or 256-thread
feature workgroups at 6n <= 127, T in global memory from max_track_len 25 on, the literal sweep's state in global memory at long windows,
book-keeping's wave count by n_features — and every kernel works on 16-column tiles, so a window with 6n not a multiple of 16 runs the
tile edges.  This file runs each of those on the device against the oracle, at the bars of tests/test_gpu_configs.py:

  * every window 3..32 (+ two with min_track_len = max_track_len - 1): stage parity, a full-load update, the sharded updater at world 2 and 3,
    and a free run from the empty window (every partial window 0..n is launched);
  * the literal compression (csrc/literal.h) on random small stacks at eight windows, against the reference's own Updater::update;
  * n_features 2 .. 2048 (and 2851 / 4096: the two-launch form of book-keeping) through the tracker tables, a free run and a full-load update;
    4097 and 4098 are refused with a message;
  * batch handles of 3 and 128 instances on both sides of 6n = 64, 96, 126 and at the last window.

The literal path at max_track_len 3..5: reachable or not is printed by test_literal_path_at_the_shortest_windows, not asserted.  On the CPU
mirror, 150 stacks of two- and three-observation type-'1' tracks reach it 0 times at max_track_len 3 and 4 (every track ends at the newest
clone and spans at most two clone columns: no column gap behind an over-determined group can form) and 13 times at max_track_len 5 — so the
path IS reachable from the 4-clone window on, and not below it.
"""
import functools

import numpy as np
import pytest

import oracle as O
import scenarios as S
import test_truncation as TT

abi, rv = O.abi, O.rv
pytestmark = pytest.mark.gpu

# (max_track_len, min_track_len, seed of the sequence): min 3 — at max_track_len = 3 the two-clone window would never update with it.
# Two cases with min_track_len = max_track_len - 1.  At 23 / 22 the direct-track sequence hands over three or more tracks of >= 22 observations
# in ONE of its 37 frames at best (on the CPU, seeds 0..7: an applied update at seed 4 and 6 only, in frame 23 — the frame in which the tracks
# seeded by the first image reach the maximum length together; never in the last frame): that case runs seed 4, checks the stages on frame
# 23 as well, and its free run must reproduce that one applied update instead of ending on one.
WINDOWS = [(3, 2, 0)] + [(ml, 3, 0) for ml in range(4, 33)] + [(6, 5, 0), (23, 22, 4)]
RARE_UPDATES = [(23, 22)]
LITERAL_WINDOWS = [8, 12, 17, 21, 22, 26, 31, 32]
FEATURES = [2, 3, 7, 65, 801, 1001, 1002, 1024, 1037, 1038, 1765, 1828, 2048, 2851, 4096]
BATCH_WINDOWS = [11, 12, 17, 18, 22, 23, 32]     # 6n = 60 | 66, 96 | 102, 126 | 132, 186


def window_cfg(ml, min_len=None, **kw):
    return abi.config_named("B", enable_equalizer=0, max_track_len=ml, min_track_len=(2 if ml == 3 else 3) if min_len is None else min_len, **kw)


@functools.lru_cache(maxsize=4)
def recorded(ml, min_len, seed=0):
    cfg = window_cfg(ml, min_len)
    seq, recs = S.record_sequence(cfg, n_frames=ml + 14, duration=6.0, seed=seed)
    return cfg, seq, recs


def p_close(Pa, Pb):
    return float(np.max(np.abs(Pa - Pb))) <= 1e-9 * np.max(np.abs(Pb)) + 1e-15


class DA:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}


# ------------------------------------------------------------------------------------------------ every window
@pytest.fixture(scope="module", params=WINDOWS, ids=lambda w: "ml%d-min%d" % w[:2])
def window(request, gpu_required):
    from rvio_amd import hip
    ml, min_len, seed = request.param
    cfg, seq, recs = recorded(ml, min_len, seed)
    h = hip.RvioHip(cfg)
    yield ml, cfg, seq, recs, h
    assert h.frame_info()["device_error"] == 0
    h.close()


def test_window_stage_parity(window):
    ml, cfg, seq, recs, h = window
    applied = [r for r in recs if r["did_update"] and r["diag"]["updated"]]
    rare = (ml, cfg.min_track_len) in RARE_UPDATES
    assert sum(int(r["did_update"]) for r in recs) >= 14 and len(applied) >= (1 if rare else 14), ml     # (the window is full in the last 14 frames)
    assert rare or recs[-1]["diag"]["updated"]
    for r in (applied[:1] if rare else []) + recs[-2:]:
        assert (len(r["x1"]) - 26) // 7 == ml - 1          # window full
        h.set_state(r["x0"], r["P0"])
        h.propagate(r["inp"]["imu"])
        x, P = h.get_state()
        assert S.state_delta(x, r["x1"]) <= 1e-9 and p_close(P, r["P1"])
        assert r["did_update"]
        h.set_state(r["x1"], r["P1"])
        h.update(r["types"], r["lens"], r["meas"])
        x, P = h.get_state()
        dg = h.update_diag()
        assert np.array_equal(dg["accepted"], r["diag"]["accepted"])
        assert np.allclose(dg["gamma"], r["diag"]["gamma"], rtol=1e-7, atol=1e-9)
        assert S.state_delta(x, r["x2"]) <= 1e-9 and p_close(P, r["P2"])
        h.set_state(r["x2"], r["P2"])
        h.augment_compose(r["do_augment"])
        x, P = h.get_state()
        assert S.state_delta(x, r["x3"]) <= 1e-12 and p_close(P, r["P3"])


def test_window_full_load_update(window):
    """ceil(F/2) = 100 features, half of them at the maximum track length"""
    ml, cfg, seq, recs, h = window
    r = recs[-1]
    types, lens, meas = S.worst_case_tracks(cfg, r, seq)
    xo, Po, od = O.update(cfg, r["x1"], r["P1"], types, lens, meas)
    assert od["n_good"] > len(types) // 2
    h.set_state(r["x1"], r["P1"])
    h.update(types, lens, meas)
    x, P = h.get_state()
    dg = h.update_diag()
    assert np.array_equal(dg["accepted"], od["accepted"])
    assert S.state_delta(x, xo) <= 1e-9 and p_close(P, Po)


def test_window_sharded_update(window):
    """the same full load through rvio_hip_update_local on the shards f mod world, the blocks laid out as the all-gather delivers them, and
    rvio_hip_update_global on the whole: the packed wire format (16 x 16 tiles) at every 6n"""
    import torch
    ml, cfg, seq, recs, h = window
    r = recs[-1]
    types, lens, meas = S.worst_case_tracks(cfg, r, seq)
    xo, Po, od = O.update(cfg, r["x1"], r["P1"], types, lens, meas)
    for world in (2, 3):
        h.set_state(r["x1"], r["P1"])
        blocks = []
        for rk in range(world):
            ptr, n = h.update_local(types, lens, meas, rk, world)
            h.sync()
            blocks.append(torch.as_tensor(DA(ptr, n), device="cuda").clone())
        allb = torch.cat(blocks).contiguous()
        torch.cuda.synchronize()
        h.update_global(allb.data_ptr(), world)
        x, P = h.get_state()
        info = h.frame_info()
        assert info["n_feat_accepted"] == od["n_good"] and info["n_rows"] == od["n_rows"] and info["updated"] == 1, (ml, world)
        assert S.state_delta(x, xo) <= 1e-9 and p_close(P, Po), (ml, world)


def test_window_free_run(window):
    """from rvio_hip_initialize through rvio_hip_frame_points: the window fills from empty, so every partial window is launched"""
    from rvio_amd import hip
    ml, cfg, seq, recs, h0 = window
    h = hip.RvioHip(cfg)
    w, a, n = seq.init_from_static(38)
    h.initialize(w, a, n)
    n_applied = 0
    try:
        for i, r in enumerate(recs):
            inp = r["inp"]
            h.frame_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])
            x, P = h.get_state()
            assert S.state_delta(x, r["x3"]) <= 1e-6, (ml, i)
            pts, hl = h.get_points()
            assert np.array_equal(pts, r["pts"]) and np.array_equal(hl, r["hist_len"]), (ml, i)
            info = h.frame_info()
            want = int(bool(r["did_update"] and r["diag"]["updated"]))
            assert info["updated"] == want, (ml, i, info)
            n_applied += want
        assert info["device_error"] == 0 and info["n_clones"] == ml - 1, (ml, info)
        if (ml, cfg.min_track_len) in RARE_UPDATES:
            assert n_applied >= 1, ml
        else:
            assert info["updated"] == 1 and n_applied >= 14, (ml, info, n_applied)
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------ the literal compression per window
def literal_sweep(ml, trials=150, short_only=False):
    return TT.sweep_few(trials, cfg=window_cfg(ml), short_only=short_only)


@pytest.mark.parametrize("ml", LITERAL_WINDOWS)
def test_literal_path_per_window(gpu_required, ml):
    """150 stacks in the style of test_truncation.sweep_few (3..15 features, random mix, half of the type-'1' tracks shortened) at this window,
    against the reference's own Updater::update where oracle/_ref is built: the rules of tests/test_gpu_literal.py.  (On the CPU mirror 6 / 3 / 4 /
    14 / 9 / 9 / 7 / 8 of the 150 take the literal path at max_track_len 8 / 12 / 17 / 21 / 22 / 26 / 31 / 32.)"""
    import test_gpu_literal as GL
    o = GL._replay(literal_sweep(ml))
    print("literal sweep at max_track_len %d:" % ml, o)
    assert o["updates"] > 100 and o["literal"] >= 3, o
    assert o["exceptions"] == [] and len(o["noise_decided"]) <= 6 and len(o["rounding_level"]) <= 3, o
    assert all(q[2] in q[4] for q in o["rank_mismatch"]), o     # nRank differs only where the reference's own does


@pytest.mark.parametrize("ml", [3, 4, 5])
def test_literal_path_at_the_shortest_windows(gpu_required, ml):
    """stacks made only of two- and three-observation type-'1' tracks: whether the literal path is reachable here is printed, not asserted
    (see the module docstring); parity is asserted either way"""
    import test_gpu_literal as GL
    o = GL._replay(literal_sweep(ml, short_only=True))
    print("short-track stacks at max_track_len %d:" % ml, o)
    assert o["exceptions"] == [] and len(o["noise_decided"]) <= 6 and len(o["rounding_level"]) <= 3, o


# ------------------------------------------------------------------------------------------------ feature-count edges
def feature_cfg(F, **kw):
    return abi.config_named("B", enable_equalizer=0, n_features=F, min_dist=3, **kw)


def tracker_script(cfg):
    """three rvio_hip_track_points calls that fill the feature list through the ChessGrid refill: F // 2 random points seed it; then nine of
    them survive (too few for RANSAC) and F random candidates refill; then nine survive again and the same candidates come in reverse order"""
    F = cfg.n_features
    rng = np.random.default_rng(1000 + F)

    def pts(n):
        return np.stack([rng.uniform(4, cfg.width - 4, n), rng.uniform(4, cfg.height - 4, n)], 1).astype(np.float32)
    return pts(max(1, F // 2)), pts(F)


def run_tracker_script(tr, cfg, seed, cand):
    imu = np.zeros(0, abi.IMU_DTYPE)
    tr.track_points(np.zeros((0, 2), np.float32), np.zeros(0, np.uint8), imu, seed)
    for c in (cand, cand[::-1].copy()):
        cur = tr.get_points()[0]
        st = np.zeros(len(cur), np.uint8)
        st[:9] = 1
        tr.track_points(cur, st, imu, c)


@pytest.mark.parametrize("F", FEATURES)
def test_feature_count_tracker_tables(gpu_required, F):
    """book-keeping's refill with the list really full: points, history lengths and hand-over tables bit-identical to the oracle"""
    from rvio_amd import hip
    from test_gpu_edges import _same_tracker
    cfg = feature_cfg(F)
    seed, cand = tracker_script(cfg)
    h, t = hip.RvioHip(cfg), O.Tracker(cfg)
    try:
        run_tracker_script(t, cfg, seed, cand)
        run_tracker_script(h, cfg, seed, cand)
        n_pts, _ = _same_tracker(h, t, F)
        print("n_features %d: %d points in the list" % (F, n_pts))
        if F >= 65:
            assert n_pts >= 0.7 * F, (F, n_pts)     # (0.74 .. 0.75 F on the CPU at F >= 801: the per-wave cell lists are really filled)
        assert h.frame_info()["device_error"] == 0
    finally:
        h.close()


@pytest.mark.parametrize("F", FEATURES)
def test_feature_count_free_run(gpu_required, F):
    """24 frames of the direct-track sequence; a full-load update at 7, 65, 1024 and 2048 features"""
    from rvio_amd import hip
    cfg = feature_cfg(F)
    seq, recs = S.record_sequence(cfg, n_frames=24)
    h = hip.RvioHip(cfg)
    try:
        w, a, n = seq.init_from_static(38)
        h.initialize(w, a, n)
        n_upd = 0
        for i, r in enumerate(recs):
            inp = r["inp"]
            h.frame_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])
            x, P = h.get_state()
            pts, hl = h.get_points()
            assert np.array_equal(pts, r["pts"]) and np.array_equal(hl, r["hist_len"]), (F, i)
            assert np.all(np.isfinite(x)) and np.all(np.isfinite(P)), (F, i)
            assert S.state_delta(x, r["x3"]) <= 1e-6, (F, i)
            n_upd += int(bool(r["did_update"] and r["diag"]["updated"]))
            assert h.frame_info()["updated"] == int(bool(r["did_update"] and r["diag"]["updated"])), (F, i)
        print("n_features %d: %d applied updates in 24 frames" % (F, n_upd))
        if F >= 7:
            assert n_upd >= 3, (F, n_upd)           # (F = 2, 3: no update on the CPU either — equal tables and finite states only)
        if F in (7, 65, 1024, 2048):
            r = recs[-1]
            types, lens, meas = S.worst_case_tracks(cfg, r, seq)
            assert len(types) == abi.fu(cfg)
            xo, Po, od = O.update(cfg, r["x1"], r["P1"], types, lens, meas)
            h.set_state(r["x1"], r["P1"])
            h.update(types, lens, meas)
            x, P = h.get_state()
            dg = h.update_diag()
            assert np.array_equal(dg["accepted"], od["accepted"]), F
            assert S.state_delta(x, xo) <= 1e-9 and p_close(P, Po), F
        assert h.frame_info()["device_error"] == 0
    finally:
        h.close()


@pytest.mark.parametrize("F", [4097, 4098])
def test_feature_counts_beyond_the_limit_are_refused(gpu_required, F):
    from rvio_amd import hip
    import re
    with pytest.raises(hip.RvioHipError) as e:
        hip.RvioHip(feature_cfg(F))
    m = re.search(r"rc=(-?\d+) (.*)", str(e.value))
    assert m and int(m.group(1)) == -3 and "4096" in m.group(2), str(e.value)       # RVIO_ERR_UNSUPPORTED, and the text names the limit
    with pytest.raises(hip.RvioHipError) as e:
        hip.RvioHip(feature_cfg(F), batch=2, front_end=True)
    assert "rc=-3" in str(e.value) and "4096" in str(e.value)


@pytest.mark.parametrize("F,frames", [(1024, 6), (3000, 3)])
def test_feature_count_on_images(gpu_required, F, frames):
    """cfg B with CLAHE through rvio_hip_track in the default pipelined path: RANSAC and book-keeping in ONE launch (ransac_book_kernel) at a
    feature count whose LDS the budget of rounds 1-6 got wrong (1024: 8 waves), and as the two-launch form where the one launch no longer fits
    a CU (3000).  Points equal to the oracle's in every frame (258 -> 224 points over frames 60..65 on the CPU at 1024)."""
    from rvio_amd import hip
    cfg = abi.config_named("B", enable_equalizer=1, n_features=F)
    seq = rv.synth.SynthSequence(cfg, duration=4.0)
    h, t = hip.RvioHip(cfg), O.Tracker(cfg)
    try:
        for k in range(60, 60 + frames):
            img, imu = seq.render(k), seq.imu_between(k)
            t.track(img, imu, None)
            h.track(img, imu, None)
            pa, ha = h.get_points()
            pb, hb = t.get_points()
            assert len(pb) > 100 and np.array_equal(pa, pb) and np.array_equal(ha, hb), (F, k, len(pa), len(pb))
        assert h.frame_info()["device_error"] == 0
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------ batch handles across the solve's thresholds
@pytest.mark.parametrize("B", [3, 128])
@pytest.mark.parametrize("ml", BATCH_WINDOWS)
def test_batch_handles_across_the_window_thresholds(gpu_required, ml, B):
    """rvio_hip_frame_tracks_dev on the recorded hand-over tables of two differently seeded sequences, instances 0 and B - 1 against plain handles
    and the recorded oracle states.  Bars of tests/test_gpu_batch.py: at the 10-clone window (cfg B) 1e-11 against the plain handle and 1e-9
    against the oracle, at the longer windows 1e-10 and 1e-8 (test_batch_handles_cover_the_long_windows)."""
    from rvio_amd import hip
    import torch
    from test_gpu_batch import pack_inputs, same_filter_state, spread
    n_seq = 2
    cfg = window_cfg(ml)
    two = [S.record_sequence(cfg, n_frames=ml + 14, duration=6.0, seed=s)[1] for s in range(n_seq)]
    recs = spread(two, B)
    tol_plain, tol_oracle = (1e-11, 1e-9) if ml <= 11 else (1e-10, 1e-8)
    hb = hip.RvioHip(cfg, batch=B)
    hs = [hip.RvioHip(cfg) for _ in range(n_seq)]
    try:
        hb.set_state(recs[0][0]["x0"], recs[0][0]["P0"])
        for i in range(B):
            hb.set_state_at(i, recs[i][0]["x0"], recs[i][0]["P0"])
        for i in range(n_seq):
            hs[i].set_state(recs[i][0]["x0"], recs[i][0]["P0"])
        n_upd = 0
        for f in range(len(two[0])):
            rf = [recs[i][f] for i in range(B)]
            n_feat, types, lens, meas, imu, m = pack_inputs(cfg, rf)
            d = [torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda() for a in (imu, n_feat, types, lens, meas)]
            torch.cuda.synchronize()
            hb.frame_tracks_dev(d[0].data_ptr(), m, m, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr())
            for i in range(n_seq):
                do_update, do_augment = hs[i].frame_plan()
                hs[i].propagate(imu[i])
                if do_update:
                    hs[i].update(rf[i]["types"], rf[i]["lens"], rf[i]["meas"])
                    n_upd += 1
                hs[i].augment_compose(do_augment)
            hb.sync()
            for i in (0, B - 1):
                xa, Pa = hb.get_state_at(i)
                xb, Pb = hs[i % n_seq].get_state()
                assert same_filter_state(xa, Pa, xb, Pb, tol_plain), (ml, B, f, i)
                assert S.state_delta(xa, rf[i]["x3"]) <= tol_oracle, (ml, B, f, i)
        assert n_upd > ml and (len(xa) - 26) // 7 == ml - 1
        assert hb.frame_info()["device_error"] == 0
    finally:
        hb.close()
        for h in hs:
            h.close()
