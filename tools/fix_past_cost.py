#!/usr/bin/env python3
"""Device time of one past-frame fix (rvio_hip_update_fix_past_dev: csrc/fix_past.hip in front of csrc/aux_update.hip) beside a fix of now
(rvio_hip_update_fix_dev: csrc/fix_rows.hip in front of the same update) on the same handle: HIP events on the handle's filter stream around 200
calls behind 20 warm-up calls, at 6n = 60 and 6n = 180, one instance and a batch of 128, a POSITION fix (m = 3), ages 1 and n (the shortest and the
longest chain), gate off.  Filter-only handles.  Prints one JSON line per case.

    python tools/fix_past_cost.py [--batch 128]
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
    import fix_cases as F
    import fix_past_cases as FP
    from rvio_amd import hip
    abi = A.abi
    cfg = A.long_config()
    kind = abi.RVIO_FIX_POSITION
    for n in (10, 30):
        x, P = A.window_state(n)
        for B in (1, a.batch):
            h = hip.RvioHip(cfg) if B == 1 else hip.RvioHip(cfg, batch=B, front_end=False)
            st = torch.cuda.ExternalStream(h.stream())
            # (a wide sigma: 220 updates in a row must leave a covariance the next one can still factor)
            now = F.fix_near(cfg, x, kind, F.LEVER, sigma_p=1.0)
            d_now = torch.from_numpy(np.frombuffer(bytes(now), np.uint8).copy()).cuda()
            cases = [("update_fix_dev", None, lambda: h.update_fix_dev(kind, 0, d_now.data_ptr(), 0, None))]
            keep = [d_now]
            for age in (1, n):
                fix = FP.fix_near(x, kind, age, 0.0, FP.LEVER, sigma_p=1.0)
                d_fix = torch.from_numpy(np.frombuffer(bytes(fix), np.uint8).copy()).cuda()
                d_age = torch.full((B,), age, dtype=torch.int32).cuda()
                keep += [d_fix, d_age]
                cases.append(("update_fix_past_dev", age, lambda d_fix=d_fix, d_age=d_age: h.update_fix_past_dev(kind, 0, d_fix.data_ptr(), 0, d_age.data_ptr(), None, None)))
            torch.cuda.synchronize()
            for rep in range(2):          # (twice, alternating: the spread)
                for case, age, call in cases:
                    us = timed(h, st, x, P, call, a.warmup, a.launches)
                    print(json.dumps(dict(case=case, age=age, rep=rep, batch=B, clones=n, us_per_call=round(us, 2), us_per_instance=round(us / B, 3),
                                          applied=int(h.get_fix(B - 1).applied))), flush=True)
            assert h.frame_info()["device_error"] == 0
            h.close()


if __name__ == "__main__":
    main()
