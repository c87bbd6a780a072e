"""The cases of tests/golden/imu_bits_parent.npz (test infrastructure).  Shared by tools/record_imu_bits.py, which writes the fixture, and
tests/test_gpu_imu_bits.py, which replays it: both run every case through the SAME run_case, so the bits recorded and the bits compared come
from identical calls.

The cases send stored inputs through every kernel that runs PreIntegrator::propagate's sample loop (csrc/imu_preint.h, propagate_body), at the smallest shapes at which they can go wrong:
    plain    rvio_hip_propagate on a plain handle: propagate_kernel3 at n = 0 ('empty') and at the long window ('long'), propagate_chol_kernel<2>
             ('window10') and <3> ('mid'); chunks of 16
    batch    rvio_hip_frame_tracks_dev with empty hand-over tables and per-instance IMU batches on a batch handle of 3 (propagate_kernel3 with the
             slab stride) and of 9 (propagate_kernel3b, chunks of 8); the frame propagates and augments
    fused    rvio_hip_frame on stored images (tests/golden/imu_bits_images.npz): the last workgroup of feat_prop_kernel propagates
    predict  rvio_hip_predict, rvio_hip_predict_cov and rvio_hip_predict_cov with out == NULL on a plain handle (imu_pose_kernel: chunks of 64,
             imu_cov_kernel: chunks of 32)
    pdev     rvio_hip_predict_dev and rvio_hip_predict_cov_dev on a batch of 3 with a per-instance IMU stride
    ring     one staged propagate of 17 samples with both IMU-rate rings on at capacity 8: the wrap, and only the last 8 records stored
What the fixture holds:
    parent                           the commit whose build left the recorded outputs
    st_<state>_x0, st_<state>_P0u    start states (tests/propagate_cases.py: empty, window10, mid, long; tests/imu_pose_cases.py: ip_empty,
                                     ip_window10, ip_moved), the covariance as its upper triangle
    <case>_imu                       the IMU batch as raw bytes ([B, m] records for a batch handle)
    <case>_<output>                  what the build left.  An output of more than FULL_BYTES bytes is stored as its SHA-256 digest (pack()): the
                                     comparison is of every bit either way; of a propagated covariance of a plain handle the 24 x 24 head is stored in full as well
The generators (tools/record_imu_bits.py --inputs) need the CPU oracle; run_case needs the stored inputs and a device only."""
import hashlib
import os

import numpy as np

from pkgload import load_pkg

abi = load_pkg().abi
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLD, "imu_bits_parent.npz")
IMAGES = os.path.join(GOLD, "imu_bits_images.npz")
FULL_BYTES = 4096

PROP_MS = (1, 8, 9, 16, 17, 33)          # propagate_body's chunk edges: 16 (plain), 8 (propagate_kernel3b)
PRED_MS = (1, 2, 32, 33, 64, 65)         # imu_cov_kernel's (32) and imu_pose_kernel's (64)
FUSED_MS = (1, 17)
STATE_ML = {"mid": 14, "long": 32}       # max_track_len of the states that do not have configuration B's own (propagate_cases.MID_ML, long_ml())
BRANCH_SMALL_ANGLE = 0.5                 # propagate_cases.BRANCH_SMALL_ANGLE: the settings at which the two nSmallAngle branches differ
PROP_STATES = ("empty", "window10", "mid", "long")
PRED_STATES = ("ip_empty", "ip_window10", "ip_moved")
RING_M, RING_CAP = 17, 8
FUSED_FIRST = 39                         # the first image the tracker sees ahead of the fused frame

# a branch batch needs a sample on either side of small_angle, so it starts at m = 8; m = 1 is the irregular batch's alone
KINDS = {m: (("irregular",) if m < 2 else ("irregular", "branch")) for m in PROP_MS}
CASES = [dict(name="p_%s_%s%d" % (s, k[:3], m), op="plain", state=s, kind=k, m=m) for s in PROP_STATES for m in PROP_MS for k in KINDS[m]]
CASES += [dict(name="b%d_%s%d" % (B, k[:3], m), op="batch", state="window10", B=B, kind=k, m=m) for B in (3, 9) for m in PROP_MS for k in KINDS[m]]
CASES += [dict(name="f%d" % m, op="fused", state="window10", kind="irregular", m=m) for m in FUSED_MS]
CASES += [dict(name="d_%s_%d" % (s[3:], m), op="predict", state=s, kind="special", m=m) for s in PRED_STATES for m in PRED_MS]
CASES += [dict(name="dd_%d" % m, op="pdev", state="ip_moved", B=3, kind="special", m=m) for m in PRED_MS]
CASES += [dict(name="ring", op="ring", state="window10", kind="irregular", m=RING_M)]


def triu(P):
    return np.ascontiguousarray(P[np.triu_indices(P.shape[0])])


def from_triu(u):
    d = int(round((np.sqrt(8 * len(u) + 1) - 1) / 2))
    P = np.zeros((d, d))
    P[np.triu_indices(d)] = u
    return P + np.triu(P, 1).T


def is_input(k):
    return k.startswith("st_") or k.endswith("_imu")


def pack(out):
    """what is stored and compared of a case's outputs: small arrays as they are, large ones as the SHA-256 of their bytes"""
    r = {}
    for k, v in out.items():
        v = np.ascontiguousarray(v)
        r[k] = v.view(np.uint8).reshape(-1) if v.dtype.fields else v
        if v.nbytes > FULL_BYTES:
            r[k] = np.array(hashlib.sha256(v.tobytes()).hexdigest())
    return r


def cfg_of(case):
    kw = {}
    if case["state"] in STATE_ML:
        kw.update(max_track_len=STATE_ML[case["state"]], min_track_len=3)
    if case["kind"] == "branch":
        kw.update(small_angle=BRANCH_SMALL_ANGLE)
    return abi.config_named("B", enable_equalizer=0, **kw)


def state_of(g, case):
    s = case["state"]
    return g["st_%s_x0" % s].copy(), from_triu(g["st_%s_P0u" % s])


def imu_of(g, case):
    imu = np.ascontiguousarray(g[case["name"] + "_imu"]).view(abi.IMU_DTYPE)
    return imu.reshape(case["B"], case["m"]) if "B" in case else imu


def to_dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8) if a.dtype.fields else np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _handle(handles, case, **kw):
    """one handle per configuration and kind of handle, made on first use; the caller closes them"""
    from rvio_amd import hip
    key = (case["state"] in STATE_ML and STATE_ML[case["state"]], case["kind"] == "branch", tuple(sorted(kw.items())))
    if key not in handles:
        handles[key] = hip.RvioHip(cfg_of(case), **kw)
    return handles[key]


def _propagated(tag, x, P, head=True):
    assert np.array_equal(P, P.T), tag
    return {tag + "x": x, tag + "P": P, **({tag + "Ph": triu(P[:24, :24])} if head else {})}


def run_case(g, case, handles):
    """-> {key: array} of everything the case leaves, device_error included"""
    import torch
    name, op, m = case["name"], case["op"], case["m"]
    x, P = state_of(g, case)
    imu = imu_of(g, case)
    out = {}
    if op == "plain":
        h = _handle(handles, case)
        h.set_state(x, P)
        h.propagate(imu)
        out.update(_propagated("", *h.get_state()))
    elif op == "batch":
        B, cfg = case["B"], cfg_of(case)
        Fu, ML = abi.fu(cfg), cfg.max_track_len
        h = _handle(handles, case, batch=B)
        tables = [to_dev(a) for a in (np.zeros(B, np.int32), np.zeros((B, Fu), np.uint8), np.zeros((B, Fu), np.int32), np.zeros((B, Fu, ML, 2), np.float32))]
        d_imu = to_dev(imu)
        h.set_state(x, P)
        for i in range(B):
            h.set_state_at(i, x, P)
        h.L.rvio_hip_frame_plan(h.h, None, None)          # (img_count > 1 behind the call below: the frame augments, as every frame but the first does)
        h.frame_tracks_dev(d_imu.data_ptr(), m, m, *[t.data_ptr() for t in tables])
        h.sync()
        assert h.frame_info()["updated"] == 0
        for i in range(B):
            out.update(_propagated("i%d_" % i, *h.get_state_at(i), head=False))
    elif op == "fused":
        from rvio_amd import hip
        im = np.load(IMAGES)
        imgs = im["imgs"]
        h = hip.RvioHip(cfg_of(case))                     # (a handle of its own: the tracker's history starts with it)
        try:
            for k in range(len(imgs) - 1):
                h.track(imgs[k], np.ascontiguousarray(im["imu%d" % k]).view(abi.IMU_DTYPE), im["cand%d" % k])
            h.sync()
            h.set_state(x, P)
            h.L.rvio_hip_frame_plan(h.h, None, None)      # (img_count > 1 in the frame below: it augments)
            h.frame(imgs[-1], imu, im["cand%d" % (len(imgs) - 1)])
            h.sync()
            info = h.frame_info()
            assert info["updated"] == 1, info             # the update rode behind feat_prop_kernel
            out.update(_propagated("", *h.get_state()))
            types, lens, meas = h.get_tracks()
            out.update(types=types, lens=lens, meas=meas, err=np.array(info["device_error"]))
        finally:
            h.close()
        return {name + "_" + k: v for k, v in out.items()}
    elif op == "predict":
        h = _handle(handles, case)
        h.set_state(x, P)
        out["pose"] = h.predict(imu)
        pose2, out["cov"] = h.predict_cov(imu)
        none, cov_only = h.predict_cov(imu, poses=False)
        # (the pose records do not depend on the covariance leg, nor the covariance records on the pose leg)
        assert none is None and np.array_equal(pose2, out["pose"]) and np.array_equal(cov_only, out["cov"])
    elif op == "pdev":
        B = case["B"]
        h = _handle(handles, case, batch=B)
        h.set_state(x, P)
        for i in range(B):
            h.set_state_at(i, x, P)
        d_imu = to_dev(imu)
        d_pose, d_pose2 = (torch.zeros(B * (m + 1) * abi.IMU_POSE_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for _ in range(2))
        d_cov, d_cov2 = (torch.zeros(B * (m + 2) * abi.IMU_COV_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        h.predict_dev(d_imu.data_ptr(), m, m, d_pose.data_ptr(), m + 1)
        h.predict_cov_dev(d_imu.data_ptr(), m, m, d_pose2.data_ptr(), m + 1, d_cov.data_ptr(), m + 2)
        h.predict_cov_dev(d_imu.data_ptr(), m, m, None, 0, d_cov2.data_ptr(), m + 2)
        h.sync()
        out.update(pose=d_pose.cpu().numpy(), cov=d_cov.cpu().numpy())
        assert np.array_equal(d_pose2.cpu().numpy(), out["pose"]) and np.array_equal(d_cov2.cpu().numpy(), out["cov"])
    else:
        assert op == "ring"
        from rvio_amd import hip
        h = hip.RvioHip(cfg_of(case))                     # (a handle of its own: the rings count from its first sample)
        try:
            h.set_state(x, P)
            h.set_imu_odometry(RING_CAP)
            h.set_imu_odometry_cov(1)
            h.propagate(imu)
            out["pose"], out["cov"] = h.get_imu_odometry(), h.get_imu_odometry_cov()
            out.update(_propagated("", *h.get_state()))
            out["err"] = np.array(h.frame_info()["device_error"])
        finally:
            h.close()
        return {name + "_" + k: v for k, v in out.items()}
    out["err"] = np.array(h.frame_info()["device_error"])
    return {name + "_" + k: v for k, v in out.items()}
