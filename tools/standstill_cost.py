#!/usr/bin/env python3
"""Device time of one standstill call (rvio_hip_standstill_dev, csrc/standstill.hip in front of csrc/aux_update.hip): HIP events on the handle's
filter stream around 200 calls behind 20 warm-up calls, at the stock window (6n = 60), m = 10 IMU samples, one instance and a batch of 128,
detect only (apply = 0) and with the update (apply = 1, every instance static, no gate), beside rvio_hip_update_aux_dev alone at m = 3 rows on
the same build.  Filter-only handles: the detector runs on the filter stream (no cross-stream events in the timed window).  Prints one JSON line
per case.

    python tools/standstill_cost.py [--batch 128]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _timing import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import aux_update_cases as A
    import standstill_cases as Z
    from rvio_amd import hip
    abi = A.abi
    n, m = 10, 10
    cfg = abi.config_named("B", enable_equalizer=0)
    x, P = A.window_state(n)
    d = 24 + 6 * n
    imu = Z.imu_batch(x, m, seed=0)
    c = Z.ss_config(gate=0)
    for B in (1, a.batch):
        h = hip.RvioHip(cfg) if B == 1 else hip.RvioHip(cfg, batch=B, front_end=False)
        h.set_standstill(c)
        st = torch.cuda.ExternalStream(h.stream())
        d_imu = torch.from_numpy(imu.view(np.uint8)).cuda()
        H, z, sigma = abi.standstill_measurement(d, np.zeros(3), c)
        dH, dv, ds = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (H, z, sigma))
        torch.cuda.synchronize()
        cases = (("aux_update_m3", lambda: h.update_aux_dev(3, abi.RVIO_AUX_VALUE, 0, dH.data_ptr(), 0, dv.data_ptr(), 0, ds.data_ptr(), 0)),
                 ("standstill_detect_only", lambda: h.standstill_dev(d_imu.data_ptr(), 0, m, 0)),
                 ("standstill_apply", lambda: h.standstill_dev(d_imu.data_ptr(), 0, m, 1)))
        for rep in range(2):          # (twice, alternating: the spread)
            for name, call in cases:
                us = timed(h, st, x, P, call, a.warmup, a.launches)
                flags = int(h.get_standstill(B - 1).flags) if name.startswith("standstill") else None
                print(json.dumps(dict(case=name, rep=rep, batch=B, clones=n, imu_samples=m, us_per_call=round(us, 2), us_per_instance=round(us / B, 3),
                                      flags=flags)), flush=True)
        h.close()


if __name__ == "__main__":
    main()
