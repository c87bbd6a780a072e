#!/usr/bin/env python3
"""Device time of the pose-graph export (csrc/window_edge.hip): HIP events on the handle's filter stream around 200 calls behind 20 warm-up
calls, at 6n = 12, 60 and 186 (max_track_len 3, 11, 32), one instance and a batch of 128.  Four cases: one edge at the longest span (0, n) —
the most columns, 6 n; the launch the edge-odometry ring makes behind every frame at its stock setting, the oldest clone (n - 1, n), issued
here as rvio_hip_get_window_edges_dev with that one pair, the same grid and kernel; the full joint call, rvio_hip_get_window_joint_dev over all
n + 1 ages; and, beside them, window_pose_kernel's ring launch at the oldest age (tools/window_cost.py's first case) on the same handle.  Built
states (tests/window_cases.py), filter-only handles.  Prints one JSON line per case.

The events span 200 back-to-back calls, so us_per_call is the larger of the kernel's time and the rate at which the launches issue; beside
it every line carries host_us_per_call, the wall clock of the enqueue loop alone (the calls return without waiting).  Where the two agree
the figure is the launch rate — an upper bound of the kernel's time, not the kernel's time.

    python tools/edge_cost.py [--batch 128]
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
        m = n + 1
        x, P = W.built_state(n)
        cfg = abi.config_named("B", enable_equalizer=0, max_track_len=max_len)
        for B in (1, a.batch):
            h = hip.RvioHip(cfg) if B == 1 else hip.RvioHip(cfg, batch=B, front_end=False)
            st = torch.cuda.ExternalStream(h.stream())
            ages = torch.tensor([0, n, n - 1, n], dtype=torch.int32).cuda()        # (0, n) at [0], [1]; (n - 1, n) at [2], [3]
            ebuf = torch.zeros(B * 376, dtype=torch.uint8).cuda()
            wbuf = torch.zeros(B * 368, dtype=torch.uint8).cuda()
            pbuf = torch.zeros(B * m * 368, dtype=torch.uint8).cuda()
            cbuf = torch.zeros(B * 36 * m * m, dtype=torch.float64).cuda()
            torch.cuda.synchronize()
            p0 = ages.data_ptr()
            cases = (("edge_longest_span", lambda: h.get_window_edges_dev(1, p0, p0 + 4, ebuf.data_ptr(), 1)),
                     ("edge_ring_launch_oldest_clone", lambda: h.get_window_edges_dev(1, p0 + 8, p0 + 12, ebuf.data_ptr(), 1)),
                     ("joint_all_ages", lambda: h.get_window_joint_dev(m, pbuf.data_ptr(), m, cbuf.data_ptr(), 36 * m * m)),
                     ("window_pose_ring_launch_oldest_age", lambda: h.get_window_dev(n, 1, wbuf.data_ptr(), 1)))
            for rep in range(2):          # (twice, alternating: the spread)
                for case, call in cases:
                    us, host_us = timed(h, st, x, P, call, a.warmup, a.launches)
                    print(json.dumps(dict(case=case, rep=rep, batch=B, clones=n, c6=6 * n, us_per_call=round(us, 2), host_us_per_call=round(host_us, 2),
                                          us_per_instance=round(us / B, 3))), flush=True)
            h.close()


if __name__ == "__main__":
    main()
