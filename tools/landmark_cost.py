"""What the landmark cloud costs the pipelined frame (rvio_hip_set_landmarks): frames resident in HBM as in bench.py's timed loop
(device detector, rvio_hip_frame_dev back to back, one drain at the end of a window), the cloud switched off and on in alternation in ONE
process — windows of 20 and 200 steps, three repeats each — and landmark_kernel alone (rvio_hip_debug_time_kernel(10), HIP events).

  python tools/landmark_cost.py [--cfg B E] [--out FILE] [--cov]    one JSON line per configuration (also appended to FILE)

--cov: the same alternation one level up — the cloud stays on, the landmark covariance (rvio_hip_set_landmark_cov, csrc/landmark_cov.hip) is
switched off and on: "off" is then cloud only, "on" cloud + covariance; the kernel timed alone is landmark_cov_kernel (hook 15).

With the cloud on, a getter per frame would synchronise the pipeline: the timed windows read nothing back (the kernel runs behind every
update all the same); the cloud of the last frame is read once at the end of a window as a check that it is there."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(name, windows=(20, 200), repeats=3, warm=40, cov=False):
    import torch
    import bench
    from rvio_amd import abi, hip
    cfg = abi.config_named(name)
    n_steps = warm + repeats * 2 * sum(windows)
    n_res = bench.resident_frames(n_steps + 1)
    seq, imgs, imu_arr, imu_cnt, _, _ = bench.build_inputs(cfg, n_res, workers=bench.render_workers(n_res))
    fs = bench.FrameSet(torch, cfg, imgs, imu_arr, imu_cnt)
    torch.cuda.synchronize()
    h = hip.RvioHip(cfg)
    h.initialize(*seq.init_from_static(bench.K0))
    step = 0

    def frames(k):
        nonlocal step
        for _ in range(k):
            h.frame_dev(*fs.args(bench.loop_frame(step)))
            step += 1

    frames(warm)
    h.set_landmarks(True)   # (first enable: allocation, outside every timed window)
    if cov:
        h.set_landmark_cov(True)
    switch = h.set_landmark_cov if cov else h.set_landmarks
    frames(4)
    h.sync()
    rates = {}
    for K in windows:
        for rep in range(repeats):
            for on in (False, True):
                switch(on)
                h.sync()
                t0 = time.perf_counter()
                frames(K)
                h.sync()
                rates.setdefault("%d_%s" % (K, "on" if on else "off"), []).append(K / (time.perf_counter() - t0))
                if on:
                    lm = h.landmarks()
                    assert lm["frame"] > 0 and lm["n"] > 0, lm
                    assert not cov or h.landmark_cov()["n"] == lm["n"]
    switch(True)
    frames(2)
    h.sync()
    us = h.time_kernel(15 if cov else 10, 200)
    info = h.frame_info()
    h.close()
    out = dict(cfg=name, features=cfg.n_features, window=cfg.max_track_len - 1, device_error=info["device_error"])
    out["landmark_cov_kernel_us" if cov else "landmark_kernel_us"] = round(us, 3)
    if cov:
        out["off"], out["on"] = "cloud only", "cloud + covariance"
    for K in windows:
        off, on = np.array(rates["%d_off" % K]), np.array(rates["%d_on" % K])
        out["w%d" % K] = dict(off_fps=[round(v, 1) for v in off], on_fps=[round(v, 1) for v in on],
                              median_change_pct=round(100.0 * (np.median(on) / np.median(off) - 1.0), 2))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", nargs="+", default=["B", "E"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--cov", action="store_true", help="the cloud stays on; alternate the landmark covariance instead")
    a = ap.parse_args()
    for name in a.cfg:
        res = run(name, cov=a.cov)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
