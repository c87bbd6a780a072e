"""What the IMU-rate odometry ring costs (rvio_hip_set_imu_odometry: imu_pose_kernel in front of every propagate), measured on warmed handles,
the legs of a comparison alternating window by window inside one process (other people's work shares the host); every window ends in
rvio_hip_sync; medians with their spread:

  a  cfg B single stream, rvio_hip_frame_dev on resident frames: ring off / ring on (capacity 4096), us per frame and frames per second.  Every
     timed pass runs the SAME frames (the handle is re-initialised, warmed over the same lead-in, then timed over the same window): the load of
     a frame depends on its content, and windows over different stretches of the sequence differ by more than the ring costs.  Passes alternate
     off / on; the paired differences on - off are reported with the medians
  b  imu_pose_kernel and imu_cov_kernel alone (rvio_hip_debug_time_kernel(13) and (14), HIP events) on the IMU batch of the last frame (m = 10 at
     200 Hz / 20 Hz): one instance — there also the fused launch, feat_prop_kernel with propagate as its last workgroup (8) —, and a filter-only
     batch handle of 128 instances
  c  rvio_hip_predict and rvio_hip_predict_cov of 10 samples from host buffers (host clock around the call: staging copy, launches, read-backs,
     one synchronise)
  d  rvio_hip_propagate_dev of 10 samples on a filter-only batch handle of 2048 instances at n = 10 (HIP events, tools/_timing.py): propagate_kernel3b
     where it is issue bound

  python tools/imu_odometry_cost.py [--repeats 6] [--window 600] [--batch 128] [--out FILE]      one JSON line (also appended to FILE)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _timing import timed  # noqa: E402


def spread(v, nd=2):
    v = np.asarray(v, float)
    return dict(median=round(float(np.median(v)), nd), min=round(float(v.min()), nd), max=round(float(v.max()), nd), runs=[round(float(x), nd) for x in v])


def leg_a(repeats, K, warm=40):
    import torch
    import bench
    from rvio_amd import abi, hip
    cfg = abi.config_named("B")
    W, H = cfg.width, cfg.height
    legs = ("ring_off", "ring_on_4096")
    n_steps = warm + K + 8
    n_res = bench.resident_frames(n_steps + 1)
    assert n_res > n_steps, "the resident sequence must cover a pass (no seam inside a window)"
    seq, imgs, imu_arr, imu_cnt, _, _ = bench.build_inputs(cfg, n_res, workers=bench.render_workers(n_res))
    d_img = torch.from_numpy(imgs).cuda()
    d_imu = torch.from_numpy(imu_arr.view(np.uint8).reshape(n_res, -1)).cuda()
    torch.cuda.synchronize()
    msb = int(d_imu.shape[1])
    h = hip.RvioHip(cfg)
    h.set_imu_odometry(4096)
    h.set_imu_odometry(0)
    init = seq.init_from_static(bench.K0)
    step = 0

    def frame():
        nonlocal step
        i, m = step, int(imu_cnt[step])
        step += 1
        h.frame_dev(d_img.data_ptr() + i * W * H, W, d_imu.data_ptr() + i * msb, m, 0, 0)

    def one_pass(leg):
        nonlocal step
        h.set_imu_odometry(4096 if leg == "ring_on_4096" else 0)
        h.initialize(*init)
        step = 0
        for _ in range(warm):
            frame()
        h.sync()
        t0 = time.perf_counter()
        for _ in range(K):
            frame()
        h.sync()
        return 1e6 * (time.perf_counter() - t0) / K

    for leg in legs:          # untimed: code objects, the detector's buffers, the ring
        one_pass(leg)
    us = {leg: [] for leg in legs}
    for rep in range(repeats):
        for leg in (legs if rep % 2 == 0 else legs[::-1]):
            us[leg].append(one_pass(leg))
    h.set_imu_odometry(4096)
    frame()
    h.set_imu_odometry_cov(1)
    frame()
    kern = {name: spread([h.time_kernel(w, 200) for _ in range(5)]) for name, w in (("imu_pose_kernel", 13), ("imu_cov_kernel", 14), ("feat_prop_kernel", 8))}
    m_last = int(imu_cnt[step - 1])
    n_ring = len(h.get_imu_odometry())
    imu_host = np.ascontiguousarray(imu_arr[step - 1][:m_last])
    pred = {}
    for name, call in (("predict", h.predict), ("predict_cov", h.predict_cov)):
        call(imu_host)
        us_call = []
        for _ in range(20):
            t0 = time.perf_counter()
            call(imu_host)
            us_call.append(1e6 * (time.perf_counter() - t0))
        pred[name] = spread(us_call)
    info = h.frame_info()
    h.close()
    out = dict(cfg="B", window_frames=K, repeats=repeats, device_error=info["device_error"], records_in_ring=n_ring, imu_samples_per_frame=m_last,
               us_per_frame={leg: spread(v) for leg, v in us.items()},
               us_per_frame_on_minus_off=spread([b - a for a, b in zip(us["ring_off"], us["ring_on_4096"])]),
               frames_per_s={leg: spread([1e6 / x for x in v], 1) for leg, v in us.items()})
    return out, kern, dict(samples=m_last, us_per_call=pred)


def leg_b(B, m=10):
    import torch
    from rvio_amd import abi, hip
    rv = sys.modules["rvio_amd"]
    cfg = abi.config_named("B", enable_equalizer=0)
    seq = rv.synth.SynthSequence(cfg, duration=4.0)
    imu = seq.imu_all()[600:600 + m].copy()
    Fu, ML = abi.fu(cfg), cfg.max_track_len
    h = hip.RvioHip(cfg, batch=B)
    h.initialize(*seq.init_from_static(38))
    h.set_imu_odometry(64)
    h.set_imu_odometry_cov(1)
    d_imu = torch.from_numpy(imu.view(np.uint8).reshape(-1).copy()).cuda()
    zeros = [torch.zeros(s, dtype=t).cuda() for s, t in (((B,), torch.int32), ((B, Fu), torch.uint8), ((B, Fu), torch.int32), ((B, Fu, ML, 2), torch.float32))]
    torch.cuda.synchronize()
    for _ in range(3):
        h.frame_tracks_dev(d_imu.data_ptr(), 0, m, *[z.data_ptr() for z in zeros])
    h.sync()
    kern = {name: spread([h.time_kernel(w, 200) for _ in range(5)]) for name, w in (("imu_pose_kernel", 13), ("imu_cov_kernel", 14))}
    h.close()
    return kern


def leg_d(B=2048, m=10, repeats=2):
    import torch
    import aux_update_cases as A
    from rvio_amd import abi, hip
    rv = sys.modules["rvio_amd"]
    cfg = abi.config_named("B", enable_equalizer=0)
    x, P = A.window_state(10)
    imu = rv.synth.SynthSequence(cfg, duration=4.0).imu_all()[600:600 + m].copy()
    h = hip.RvioHip(cfg, batch=B, front_end=False)
    h.set_state(x, P)          # (the window length of the handle; then every instance's own copy)
    for i in range(B):
        h.set_state_at(i, x, P)
    st = torch.cuda.ExternalStream(h.stream())
    d_imu = torch.from_numpy(imu.view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    us = [timed(h, st, x, P, lambda: h.propagate_dev(d_imu.data_ptr(), m), 20, 200) for _ in range(repeats)]
    err = h.frame_info()["device_error"]
    h.close()
    return dict(instances=B, clones=10, samples=m, device_error=err, us_per_call=spread(us))


def run(repeats, K, B):
    import bench  # noqa: F401  (loads the package the way bench.py does: rvio_amd becomes importable)
    a, kern1, pred = leg_a(repeats, K)
    print("leg a done", file=sys.stderr, flush=True)
    kernB = leg_b(B)
    return dict(a_single_stream=a, b_kernel_us={"one_instance": kern1, "batch_%d" % B: kernB}, c_predict_host=pred, d_propagate_dev_batch=leg_d())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--window", type=int, default=600)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    line = json.dumps(run(a.repeats, a.window, a.batch))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
