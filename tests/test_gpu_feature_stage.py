"""The per-feature stage of the update (U1 .. U5 of Updater::update and the feature's share of the information block: feat_build_kernel<16> on a
plain handle, geom4_kernel + feat_build_kernel<4> on batch handles) on the device, feature by feature, against the np.longdouble twin
abi.feature_update_model_as evaluated at the device's OWN triple — which sidesteps the discrete decisions of the LM loop and is indifferent to
Householder against Givens — at every (type, L) of the windows 3, 10, 16, 17, 22 and 32, on the N = 2 branch, and on hand-built tracks for every
branch of the LM loop (the cases and their conditions: tests/feature_cases.py; asserted on the CPU by tests/test_feature_update_model.py).

Bars (tests/feature_cases.py, tabulated on the CPU at the oracle's triple: floors_of; nothing of them is read from the device).  gamma:
|gamma - twin| / twin; the share: max |dA_ij| / sqrt(A_ii A_jj) and max |db_i| / (sqrt(A_ii) |rn|) over the feature's column range, exact zeros
outside it.  The float64 model's floor against the twin (one evaluation per case), worst per window 3 / 10 / 16 / 17 / 22 / 32: gamma 3.6e-15 /
4.6e-15 / 7.5e-15 / 1.5e-14 / 1.1e-14 / 3.3e-14, share 1.7e-11 / 3.9e-14 / 4.0e-13 / 3.4e-14 / 3.9e-14 / 6.6e-13.  The floors do not follow cond(S)
(<= 111, below 8 on all but a few cases) but cond(Hf) of the columns the projection takes out (up to 2.4e3: a type-'2' track of three
observations): worst floor / (2^-52 cond(Hf)) = 22.9 (gamma) and 71.0 (share), both on window 32.  So the bars are K 2^-52 cond(Hf) with
K = 16 x these ratios, rounded up: 400 and 1200 — 8.9e-14 cond(Hf) and 2.7e-13 cond(Hf), never looser than what the suite held before (gamma rtol
1e-7, block 1e-9).  The triple against the oracle's: rtol 1e-8 / atol 1e-10 as before; one device form against another: PF_FORM_BAR = 8e-3
(16 x the 3.9e-4 by which the oracle's own triple moves under one ulp on the state and one float32 ulp on the observations; the oracle bar
binds long before).
Measured on one MI355X, worst per window 3 / 10 / 16 / 17 / 22 / 32 on the plain handle: gamma 1.2e-14 / 1.2e-14 / 3.4e-14 / 2.7e-14 / 2.3e-14 /
4.5e-13, share 7.1e-11 / 3.8e-13 / 2.3e-12 / 1.9e-14 / 6.9e-14 / 2.3e-13 (the large ones at cond(Hf) ~ 2e3); batch handles and feat_prop_kernel at
windows 10 / 16 / 17: gamma 1.9e-14 / 3.4e-14 / 2.7e-14, the triple within 1.3e-13 of the plain handle's.

What the C-ABI lets a test see.  A plain handle: rvio_hip_update_local hands out the block (one feature per call at world 1: the block IS that
feature's share) and rvio_hip_get_update_diag the gate.  A batch handle: rvio_hip_get_update_diag reads instance 0 and takes its count from the
handle's own hand-over table, which rvio_hip_update_local fills (and runs the batch form of the stage on); rvio_hip_frame_tracks_dev then runs
every instance.  feat_prop_kernel rides only in the image-path frames, whose table the tracker owns; rvio_hip_debug_time_kernel(8) launches it
on a hand-built table.  The batch and fused forms expose no block: their share is seen through the state behind the frame only."""
import ctypes as C
import functools

import numpy as np
import pytest

import feature_cases as F
import oracle as O
import scenarios as S

abi, rv = O.abi, O.rv
pytestmark = pytest.mark.gpu


class _DA:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}


@functools.lru_cache(maxsize=None)
def plain_results(max_len):
    """every case of F.all_cases(max_len) through rvio_hip_update_local as a one-feature table at world 1 on a plain handle: per case
    dict(accepted, ndof, gamma, pf, parts [2, 6n, 6n + 1], counters [8]).  Computed once per window and shared by the tests below."""
    import torch
    from rvio_amd import hip
    cases = F.all_cases(max_len)
    cfg = cases[0][1]
    c6 = 6 * (max_len - 1)
    h = hip.RvioHip(cfg)
    out, cur = [], None
    for _, _, x, P, ty, L, meas in cases:
        if cur is not x:
            h.set_state(x, P)
            cur = x
        ptr, nd = h.update_local(np.array([ty], np.uint8), np.array([L], np.int32), meas[None], 0, 1)
        h.sync()
        assert nd == abi.shard_payload_doubles(c6, max_len)
        pay = torch.as_tensor(_DA(ptr, nd), device="cuda").cpu().numpy().copy()
        dg = h.update_diag()
        assert len(dg["accepted"]) == 1
        parts, cnt = abi.shard_unpack(pay, c6, max_len, c6 + 1)
        out.append(dict(accepted=int(dg["accepted"][0]), ndof=int(dg["ndof"][0]), gamma=float(dg["gamma"][0]), pf=dg["pfinv"][0].copy(),
                        parts=parts[:, :c6, :], counters=cnt))
    assert h.frame_info()["device_error"] == 0
    h.close()
    return tuple(out)


def hold_to_twin(case, orc, dev, floor):
    """one feature of the plain handle against the oracle (valid or not, the triple) and the twin at the device's own triple (ndof, the gate,
    gamma, the share); returns (gamma error, share error, gamma bar, share bar) — zeros for a feature without a triple"""
    label, cfg, x, P, ty, L, meas = case
    share = "parts" in dev          # (the forms that expose no block are held to the gate alone)
    if not orc["valid"]:
        assert (dev["accepted"], dev["ndof"], dev["gamma"]) == (0, 0, 0.0), label
        assert not share or (not dev["parts"].any() and not dev["counters"][:3].any()), label
        return 0.0, 0.0, 0.0, 0.0
    assert np.allclose(dev["pf"], orc["pf"], rtol=F.PF_RTOL, atol=F.PF_ATOL), (label, dev["pf"], orc["pf"])
    a = (cfg, x, P, chr(ty), L, meas, dev["pf"])
    t = abi.feature_update_model_as(*a)
    bar_g, bar_s = floor["bar_g"], floor["bar_s"]
    assert dev["ndof"] == t["ndof"] == orc["ndof"], label
    accept = bool(t["gamma"] < O.chi2_95(t["ndof"]))
    assert bool(dev["accepted"]) == accept == bool(orc["accepted"]), label
    eg = F.gamma_err(dev["gamma"], t)
    print("   %-28s ndof %2d accepted %d gamma %.6g: e %.1e (bar %.1e)" % (label, dev["ndof"], dev["accepted"], dev["gamma"], eg, bar_g), end="")
    assert eg <= bar_g, (label, eg, bar_g)
    if not share:
        print()
        return eg, 0.0, bar_g, bar_s
    own, other = (0, 1) if ty == ord("2") else (1, 0)
    assert not dev["parts"][other].any(), label
    if not accept:          # a refused feature writes nothing into the block
        print()
        assert not dev["parts"].any() and not dev["counters"][:3].any(), label
        return eg, 0.0, bar_g, bar_s
    assert dev["counters"][0] == 1 and dev["counters"][1] == t["ndof"], (label, dev["counters"])
    c6 = dev["parts"].shape[1]
    eA, eb, outside = F.share_err(dev["parts"][own][:, :c6], dev["parts"][own][:, c6], t)
    print("  share A %.1e b %.1e (bar %.1e)" % (eA, eb, bar_s))
    assert outside == 0.0, (label, outside)
    assert max(eA, eb) <= bar_s, (label, eA, eb, bar_s)
    return eg, max(eA, eb), bar_g, bar_s


def hold_all(max_len, pick):
    cases, orc, dev, floors = F.all_cases(max_len), F.oracle_of(max_len), plain_results(max_len), F.floors_of(max_len)
    worst, n = [0.0, 0.0], 0
    for c, o, d, fl in zip(cases, orc, dev, floors):
        if pick(c[0]):
            eg, es, _, _ = hold_to_twin(c, o, d, fl)
            worst, n = [max(worst[0], eg), max(worst[1], es)], n + 1
    print("max_track_len %d: %d features, device gamma error <= %.2e, share error <= %.2e" % (max_len, n, worst[0], worst[1]))
    return n


# ---------------------------------------------------------------- (a) gate and share, every (type, L)
@pytest.mark.parametrize("max_len", F.WINDOWS)
def test_gate_and_share_of_every_kind(gpu_required, max_len):
    """one track of every type and every length the window accepts: ndof of every valid feature, the gate, gamma and the feature's share of the
    information block read on its own, against the twin at the device's own triple"""
    assert hold_all(max_len, lambda s: s.startswith("kind")) == len(F.kinds(max_len))


# ---------------------------------------------------------------- (c) N = 2 and the edges of the LDL^T templates
@pytest.mark.parametrize("max_len", sorted(F.STILL_LENS))
def test_zero_depth_column_takes_two_columns_out(gpu_required, max_len):
    """a window at rest (every clone the identity, zero translation): the depth column is exactly zero, N = 2, rho stays 0; type-'1' tracks of
    L = 7 and 11 give rr = 12 and 20, the last sizes of the two register-resident LDL^T templates, L = 12 gives rr = 22, the first even size of
    the LDS form"""
    cases, dev = F.all_cases(max_len), plain_results(max_len)
    n = 0
    for c, d in zip(cases, dev):
        if c[0].startswith("zero-depth"):
            assert d["ndof"] == 2 * c[5] - 2 and d["pf"][2] == 0.0 and d["accepted"] == 1, (c[0], d["ndof"], d["pf"])
            n += 1
    assert n == len(F.STILL_LENS[max_len]) == hold_all(max_len, lambda s: s.startswith("zero-depth"))


# ---------------------------------------------------------------- (d) the LM branches
@pytest.mark.parametrize("max_len", F.LM_WINDOWS)
def test_lm_branches_on_the_plain_handle(gpu_required, max_len):
    """the hand-built tracks of the eight LM classes (the oracle's trace proves on the CPU that each is reached): valid or not as the oracle; a
    feature without a triple reports accepted = 0, ndof = 0, gamma = 0 and writes nothing into the block; the triple of the others within the
    bar, then the twin's checks at the device's triple"""
    assert hold_all(max_len, lambda s: not s.startswith("kind")) == len(F.LM_HAND) + len(F.STILL_LENS[max_len])


# ---------------------------------------------------------------- (b), (d) the same features through the batch forms
def p_close(Pa, Pb):
    return float(np.max(np.abs(Pa - Pb))) <= 1e-9 * float(np.max(np.abs(Pb))) + 1e-15


def chunks_of(max_len):
    """the cases of the window as hand-over tables of at most Fu features that share a state: [(x, P, [case index ...])]"""
    cases = F.all_cases(max_len)
    fu = abi.fu(cases[0][1])
    out = []
    for i, c in enumerate(cases):
        if out and out[-1][0] is c[2] and len(out[-1][2]) < fu:
            out[-1][2].append(i)
        else:
            out.append((c[2], c[3], [i]))
    return out


def diag_of(dg, j):
    return dict(accepted=int(dg["accepted"][j]), ndof=int(dg["ndof"][j]), gamma=float(dg["gamma"][j]), pf=dg["pfinv"][j].copy())


@pytest.mark.parametrize("B", [3, 128])
@pytest.mark.parametrize("max_len", [10, 16, 17])
def test_the_same_features_through_a_batch_handle(gpu_required, max_len, B):
    """geom4_kernel + feat_build_kernel<4> (windows 10 and 16; geom4_kernel carries the second LM loop) and feat_build_kernel<4> with its own chain
    (window 17), B = 3 and 128 instances.  rvio_hip_get_update_diag reads instance 0 (csrc/rvio_hip.hip: h->acc, h->gamma, h->ndof, h->pfinv at
    offset 0 of the slab) and takes its count from the handle's own hand-over table, so per table: rvio_hip_update_local uploads it into that
    table (instance 0; the other instances' tables are empty: the slab is zeroed at creation) and runs the batch form of the stage on it — diag
    read —, then rvio_hip_frame_tracks_dev runs the same table in every instance with an empty IMU batch — diag read again: the same bits.
    Every feature: ndof / accepted / gamma against the twin at the device's triple, 0 / 0 / 0 without a triple, the whole triple within PF_RTOL of
    the oracle's and within PF_FORM_BAR of the plain handle's; the cloud records of instance 0 are exactly the features the gate let pass with
    rho > 0; the state behind the frame against O.update + O.augment_compose at the suite's 1e-9; the last instance bit for bit the first."""
    import torch
    from rvio_amd import hip
    cases, orc, plain, floors = F.all_cases(max_len), F.oracle_of(max_len), plain_results(max_len), F.floors_of(max_len)
    cfg = cases[0][1]
    fu, ML = abi.fu(cfg), cfg.max_track_len
    hb = hip.RvioHip(cfg, batch=B)
    hb.set_landmark_cov(True)
    worst_form, worst_g, seen = 0.0, 0.0, 0
    for k, (x, P, idx) in enumerate(chunks_of(max_len)):
        nf = len(idx)
        types, lens, meas = np.zeros((B, fu), np.uint8), np.zeros((B, fu), np.int32), np.zeros((B, fu, ML, 2), np.float32)
        for j, i in enumerate(idx):
            types[:, j], lens[:, j], meas[:, j] = cases[i][4], cases[i][5], cases[i][6]
        d = [torch.from_numpy(a).cuda() for a in (np.full(B, nf, np.int32), types, lens, meas)]
        torch.cuda.synchronize()
        hb.set_state(x, P)
        hb.update_local(types[0, :nf], lens[0, :nf], meas[0, :nf], 0, 1)
        dg_local = hb.update_diag()
        hb.frame_tracks_dev(0, 0, 0, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr())
        hb.sync()
        assert hb.frame_info()["device_error"] == 0
        dg = hb.update_diag()
        assert len(dg["accepted"]) == nf
        for key in ("accepted", "ndof", "gamma", "pfinv"):
            assert np.array_equal(dg[key], dg_local[key]), (k, key)
        for j, i in enumerate(idx):
            dev = diag_of(dg, j)
            eg, _, _, _ = hold_to_twin(cases[i], orc[i], dev, floors[i])
            worst_g = max(worst_g, eg)
            if orc[i]["valid"]:
                form = F.pf_move(dev["pf"], plain[i]["pf"])
                worst_form, seen = max(worst_form, form), seen + 1
                assert form <= F.PF_FORM_BAR, (cases[i][0], form)
        x0, P0 = hb.get_state_at(0)
        xl, Pl = hb.get_state_at(B - 1)
        assert np.array_equal(x0, xl) and np.array_equal(P0, Pl)
        xo, Po, od = O.update(cfg, x, P, types[0, :nf], lens[0, :nf], meas[0, :nf])
        x3, P3, _, _ = O.augment_compose(cfg, xo, Po, k > 0)          # (System.cc:280: no augmentation behind the handle's first frame)
        assert S.state_delta(x0, x3) <= 1e-9, (k, S.state_delta(x0, x3))
        assert p_close(P0, P3), k
        rec = hb.landmark_cov_at(0)["rec"]
        want = [j for j, i in enumerate(idx) if orc[i]["accepted"] and orc[i]["pf"][2] > 0]
        assert [int(f) for f in rec["feat"]] == want, (k, rec["feat"], want)
        assert np.array_equal(rec["rho"], dg["pfinv"][rec["feat"], 2]) and np.array_equal(rec["n_obs"], lens[0][rec["feat"]])
    hb.close()
    print("max_track_len %d, %d instances: %d features with a triple, gamma error <= %.2e, triple against the plain handle's <= %.2e (scale-free)"
          % (max_len, B, seen, worst_g, worst_form))
    assert seen >= 0.8 * len(cases)


# ---------------------------------------------------------------- (b) the fused form
FUSED_WINDOWS = (10, 16, 17)


@pytest.mark.parametrize("max_len", FUSED_WINDOWS)
def test_the_same_features_through_the_fused_kernel(gpu_required, max_len):
    """feat_prop_kernel (the per-feature stage fused with propagate) rides only in the image-path frames, whose hand-over table the tracker owns;
    rvio_hip_frame_tracks_dev on a plain handle launches feat_build_kernel<16> like rvio_hip_update_local (csrc/rvio_hip.hip: fuse_m < 0 there).
    The fused kernel is reached with a hand-built table through rvio_hip_debug_time_kernel(8, 1), which launches it exactly as the pipelined
    frame does on the handle's last hand-over table and the IMU batch of the last propagate, and restores the state behind it.  So: one
    propagate (the IMU batch), the table uploaded by rvio_hip_update_local on the window AT REST (a different state, so that what is read
    afterwards cannot be that call's), then the recorded state and the hook — rvio_hip_get_update_diag is what the fused kernel left.  Every
    feature: the triple against the plain handle's and the oracle's, ndof / accepted / gamma against the twin."""
    from rvio_amd import hip
    cases, orc, plain, floors = F.all_cases(max_len), F.oracle_of(max_len), plain_results(max_len), F.floors_of(max_len)
    cfg = cases[0][1]
    h = hip.RvioHip(cfg)
    m = 4
    imu = abi.as_imu_array(np.tile([0.01, -0.02, 0.015], (m, 1)), np.tile([0.1, 0.2, 9.7], (m, 1)), 0.005 * np.arange(1, m + 1), np.full(m, 0.005))
    worst_g, seen = 0.0, 0
    for x, P, idx in chunks_of(max_len):
        if x is not cases[0][2]:
            continue                    # (the tracks on the window at rest have no other state to be uploaded on)
        types, lens = np.array([cases[i][4] for i in idx], np.uint8), np.array([cases[i][5] for i in idx], np.int32)
        meas = np.stack([cases[i][6] for i in idx])
        h.set_state(x, P)
        h.propagate(imu)
        h.set_state(F.still_state(x), P)
        h.update_local(types, lens, meas, 0, 1)
        other = h.update_diag()
        h.set_state(x, P)
        assert h.time_kernel(8, 1) > 0
        dg = h.update_diag()
        xa, Pa = h.get_state()
        assert np.array_equal(xa, x) and np.array_equal(Pa, P)          # the hook restores what the fused propagate moved
        assert len(dg["accepted"]) == len(idx) and not np.array_equal(dg["pfinv"], other["pfinv"])
        for j, i in enumerate(idx):
            dev = diag_of(dg, j)
            eg, _, _, _ = hold_to_twin(cases[i], orc[i], dev, floors[i])
            worst_g = max(worst_g, eg)
            if orc[i]["valid"]:
                assert F.pf_move(dev["pf"], plain[i]["pf"]) <= F.PF_FORM_BAR, cases[i][0]
                seen += 1
    assert h.frame_info()["device_error"] == 0
    h.close()
    print("max_track_len %d, feat_prop_kernel: %d features with a triple, gamma error <= %.2e" % (max_len, seen, worst_g))
    assert seen >= len(F.kinds(max_len))
