#!/usr/bin/env python3
"""Device time of one relative-pose measurement (rvio_hip_update_rel_dev: csrc/rel_rows.hip in front of csrc/aux_update.hip) beside a past-frame
fix of the same row count at age = age_old (rvio_hip_update_fix_past_dev: csrc/fix_past.hip in front of the same update — the same chain length)
on the same handle: HIP events on the handle's filter stream around 200 calls behind 20 warm-up calls, at 6n = 60 and 6n = 180, m = 3 (POSITION)
and m = 6 (POSE), one instance and a batch of 128, spans (0, 1) and (0, n) (the shortest and the longest chain), gate off, two alternating
repetitions.  Filter-only handles.  Prints one JSON line per case.

    python tools/rel_cost.py [--batch 128]
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
    import fix_past_cases as FP
    import rel_cases as R
    from rvio_amd import hip
    abi = A.abi
    cfg = A.long_config()
    for n in (10, 30):
        x, P = A.window_state(n)
        for B in (1, a.batch):
            h = hip.RvioHip(cfg) if B == 1 else hip.RvioHip(cfg, batch=B, front_end=False)
            st = torch.cuda.ExternalStream(h.stream())
            cases, keep = [], []
            for m, rel_kind, fix_kind in ((3, abi.RVIO_REL_POSITION, abi.RVIO_FIX_POSITION), (6, abi.RVIO_REL_POSE, abi.RVIO_FIX_POSE)):
                for b in (1, n):
                    # (wide sigmas: 220 updates in a row must leave a covariance the next one can still factor)
                    meas = R.meas_near(x, rel_kind, 0, b, R.LEVER, sigma_p=1.0, sigma_q=1.0)
                    fix = FP.fix_near(x, fix_kind, b, 0.0, FP.LEVER, sigma_p=1.0, sigma_q=1.0)
                    d_meas = torch.from_numpy(np.frombuffer(bytes(meas), np.uint8).copy()).cuda()
                    d_fix = torch.from_numpy(np.frombuffer(bytes(fix), np.uint8).copy()).cuda()
                    d_new = torch.zeros(B, dtype=torch.int32).cuda()
                    d_old = torch.full((B,), b, dtype=torch.int32).cuda()
                    keep += [d_meas, d_fix, d_new, d_old]
                    cases.append(("update_rel_dev", m, b, lambda k=rel_kind, d_meas=d_meas, d_new=d_new, d_old=d_old: h.update_rel_dev(k, 0, d_meas.data_ptr(), 0, d_new.data_ptr(), d_old.data_ptr(), None)))
                    cases.append(("update_fix_past_dev", m, b, lambda k=fix_kind, d_fix=d_fix, d_old=d_old: h.update_fix_past_dev(k, 0, d_fix.data_ptr(), 0, d_old.data_ptr(), None, None)))
            torch.cuda.synchronize()
            for rep in range(2):          # (twice, alternating: the spread)
                for case, m, b, call in cases:
                    us = timed(h, st, x, P, call, a.warmup, a.launches)
                    print(json.dumps(dict(case=case, m=m, k=b, rep=rep, batch=B, clones=n, us_per_call=round(us, 2), us_per_instance=round(us / B, 3),
                                          applied=int(h.get_fix(B - 1).applied))), flush=True)
            assert h.frame_info()["device_error"] == 0
            h.close()


if __name__ == "__main__":
    main()
