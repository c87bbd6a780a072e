#!/usr/bin/env python3
"""Device time of one map-landmark call (rvio_hip_update_map_dev: csrc/map_rows.hip in front of csrc/aux_update.hip) for 1 / 4 / 8 observed points
at ages 0, 10 and n, with and without the per-point gate, beside a past-frame RVIO_FIX_POSE of the same age (rvio_hip_update_fix_past_dev:
csrc/fix_past.hip in front of the same update — what a caller who ran PnP on the host would send) in the same process and on the same handle:
HIP events on the handle's filter stream around 200 calls behind 20 warm-up calls at 6n = 180, one instance and a batch of 128, stack gate off,
two alternating repetitions.  Filter-only handles.  Prints one JSON line per case.

    python tools/map_cost.py [--batch 128]
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
    import fix_past_cases as FP
    import map_cases as M
    from rvio_amd import hip
    abi, A = M.abi, M.A
    cfg = A.long_config()
    n = 30
    x, P = A.window_state(n)
    for B in (1, a.batch):
        h = hip.RvioHip(cfg) if B == 1 else hip.RvioHip(cfg, batch=B, front_end=False)
        st = torch.cuda.ExternalStream(h.stream())
        cases, keep = [], []
        for age in (0, 10, n):
            d_age = torch.full((B,), age, dtype=torch.int32).cuda()
            # (wide sigmas: 220 updates in a row must leave a covariance the next one can still factor)
            fix = FP.fix_near(x, abi.RVIO_FIX_POSE, age, 0.0, FP.LEVER, sigma_p=1.0, sigma_q=1.0)
            d_fix = torch.from_numpy(np.frombuffer(bytes(fix), np.uint8).copy()).cuda()
            keep += [d_age, d_fix]
            cases.append(("update_fix_past_dev", 0, age, 0, lambda d_fix=d_fix, d_age=d_age: h.update_fix_past_dev(abi.RVIO_FIX_POSE, 0, d_fix.data_ptr(), 0, d_age.data_ptr(), None, None)))
            for k in (1, 4, 8):
                obs = abi.make_map_obs(M.observations(cfg, x, age, [M.GOOD] * k, seed=age + k, sigma=1.0))
                d_obs = torch.from_numpy(np.frombuffer(bytes(obs), np.uint8).copy()).cuda()
                keep.append(d_obs)
                for ge in (0, 1):
                    cases.append(("update_map_dev", k, age, ge, lambda k=k, ge=ge, d_obs=d_obs, d_age=d_age: h.update_map_dev(abi.RVIO_MAP_NORMALISED, 0, ge, k, d_obs.data_ptr(), 0, None, d_age.data_ptr(), None)))
        torch.cuda.synchronize()
        for rep in range(2):          # (twice, alternating: the spread)
            for case, k, age, ge, call in cases:
                us = timed(h, st, x, P, call, a.warmup, a.launches)
                if k:
                    rec = h.get_map(B - 1)[0]
                    applied, used = int(rec.applied), int(rec.n_used)
                else:
                    applied, used = int(h.get_fix(B - 1).applied), 0
                print(json.dumps(dict(case=case, points=k, age=age, gate_each=ge, rep=rep, batch=B, clones=n, us_per_call=round(us, 2), us_per_instance=round(us / B, 3),
                                      applied=applied, n_used=used)), flush=True)
        assert h.frame_info()["device_error"] == 0
        h.close()


if __name__ == "__main__":
    main()
