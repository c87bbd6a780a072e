#!/usr/bin/env python3
"""Device time of the landmark covariance (csrc/landmark_cov.hip): 200 back-to-back launches of landmark_cov_kernel between two HIP events on the
handle's filter stream (rvio_hip_debug_time_kernel(15): the kernel as the update launches it, on the cloud and operands of the last update,
into records of its own), at 6n = 12, 60 and 186 (max_track_len 3, 11, 32) with full clouds (ceil(F / 2) = 100 hand-over slots, tracks of
both types consistent with the state: tests/landmark_cov_cases.py), for one instance and for a batch of 128.  Beside each figure:
landmark_kernel alone (hook 10) on the same handle, and the same hook 15 on an EMPTY cloud of the same grid — every workgroup returns at
once, so that figure is the interval at which launches of this grid follow one another on the stream.  Where us_per_launch is not clearly
above launch_interval_us it is that interval — an upper bound of the kernel's time, not the kernel's time.  host_us_per_launch is the wall
clock of the whole hook call (drain, 200 enqueues, the wait for the second event) per launch: where it agrees with us_per_launch the host's
enqueue rate, not the device, sets the figure.  Prints one JSON line per case.

    python tools/landmark_cov_cost.py [--batch 128]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def hook(h, which, iters):
    t0 = time.perf_counter()
    us = h.time_kernel(which, iters)
    return us, 1e6 * (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    import landmark_cov_cases as K
    import window_cases as W
    from rvio_amd import hip
    abi = K.abi
    for max_len in (3, 11, 32):
        n = max_len - 1
        cfg = abi.config_named("B", enable_equalizer=0, max_track_len=max_len, min_track_len=min(3, max_len - 1))   # (a frame updates once n > min_track_len - 1)
        Fu = abi.fu(cfg)
        x, P = W.built_state(n)
        types, lens, meas = K.make_tracks(cfg, x, K.spec_for(max_len, Fu), seed=max_len)
        imu = np.zeros(4, abi.IMU_DTYPE)
        imu["a"], imu["dt"], imu["t"] = cfg.gravity * x[7:10], 0.005, 0.005 * np.arange(1, 5)
        for B in (1, a.batch):
            h = hip.RvioHip(cfg) if B == 1 else hip.RvioHip(cfg, batch=B, front_end=False)
            h.set_landmark_cov(True)

            def frame(nf):
                if B == 1:          # a plain handle: the update stage alone
                    h.set_state(x, P)
                    h.update(types[:nf], lens[:nf], meas[:nf])
                    h.sync()
                    return None
                d = [torch.from_numpy(v).cuda() for v in (imu.view(np.uint8), np.full(B, nf, np.int32), np.tile(types, (B, 1)), np.tile(lens, (B, 1)),
                                                          np.tile(meas, (B, 1, 1, 1)))]
                torch.cuda.synchronize()
                h.set_state(x, P)          # (every instance)
                h.frame_tracks_dev(d[0].data_ptr(), 0, len(imu), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr())
                h.sync()
                return d

            keep = frame(Fu)
            cnt = [h.landmark_cov_at(i)["n"] for i in (0, B - 1)]
            for rep in range(2):          # (twice: the spread)
                us, host_us = hook(h, 15, a.launches)
                cloud_us, _ = hook(h, 10, a.launches)
                print(json.dumps(dict(case="full_cloud", rep=rep, batch=B, clones=n, c6=6 * n, slots=Fu, cloud_points=cnt, us_per_launch=round(us, 2),
                                      host_us_per_launch=round(host_us, 2), landmark_kernel_us=round(cloud_us, 2), us_per_instance=round(us / B, 3))), flush=True)
            keep = frame(0)
            assert h.landmark_cov_at(0)["n"] == 0
            for rep in range(2):
                us, host_us = hook(h, 15, a.launches)
                print(json.dumps(dict(case="empty_cloud_same_grid", rep=rep, batch=B, clones=n, c6=6 * n, slots=Fu, launch_interval_us=round(us, 2),
                                      host_us_per_launch=round(host_us, 2))), flush=True)
            del keep
            h.close()


if __name__ == "__main__":
    main()
