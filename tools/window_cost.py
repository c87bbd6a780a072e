#!/usr/bin/env python3
"""Device time of the fixed-lag smoothed trajectory (csrc/window_pose.hip): HIP events on the handle's filter stream around 200 calls behind 20
warm-up calls, at 6n = 12, 60 and 186 (max_track_len 3, 11, 32), one instance and a batch of 128.  Two cases: the launch the smoothed-odometry
ring makes behind every frame — one age, the oldest (lag = n: the longest chain and the most columns, k = 6 + 6 n), issued here as
rvio_hip_get_window_dev(n, 1), the same grid and arguments — and rvio_hip_get_window_dev over all n + 1 ages.  Built states (tests/window_cases.py),
filter-only handles.  Prints one JSON line per case.

The events span 200 back-to-back calls, so us_per_call is the larger of the kernel's time and the rate at which the launches issue; beside
it every line carries host_us_per_call, the wall clock of the enqueue loop alone (the calls return without waiting).  Where the two agree
the figure is the launch rate — an upper bound of the kernel's time, not the kernel's time.

    python tools/window_cost.py [--batch 128]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(h, st, x, P, call, warmup, launches):
    """(device microseconds per call between two events on the filter stream, host microseconds per call of the enqueue loop)"""
    import time
    import torch
    h.set_state(x, P)
    for _ in range(warmup):
        call()
    h.set_state(x, P)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    t0 = time.perf_counter()
    for _ in range(launches):
        call()
    t1 = time.perf_counter()
    e1.record(st)
    h.sync()
    return 1e3 * e0.elapsed_time(e1) / launches, 1e6 * (t1 - t0) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import window_cases as W
    from rvio_amd import hip
    abi = W.abi
    for max_len in W.WINDOWS:
        n = max_len - 1
        x, P = W.built_state(n)
        cfg = abi.config_named("B", enable_equalizer=0, max_track_len=max_len)
        for B in (1, a.batch):
            h = hip.RvioHip(cfg) if B == 1 else hip.RvioHip(cfg, batch=B, front_end=False)
            st = torch.cuda.ExternalStream(h.stream())
            buf = torch.zeros(B * (n + 1) * 368, dtype=torch.uint8).cuda()
            torch.cuda.synchronize()
            cases = (("ring_launch_oldest_age", lambda: h.get_window_dev(n, 1, buf.data_ptr(), 1)),
                     ("all_ages", lambda: h.get_window_dev(0, n + 1, buf.data_ptr(), n + 1)))
            for rep in range(2):          # (twice, alternating: the spread)
                for case, call in cases:
                    us, host_us = timed(h, st, x, P, call, a.warmup, a.launches)
                    print(json.dumps(dict(case=case, rep=rep, batch=B, clones=n, c6=6 * n, us_per_call=round(us, 2), host_us_per_call=round(host_us, 2),
                                          us_per_instance=round(us / B, 3))), flush=True)
            h.close()


if __name__ == "__main__":
    main()
