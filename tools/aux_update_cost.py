#!/usr/bin/env python3
"""Device time of one auxiliary measurement update (rvio_hip_update_aux_dev, csrc/aux_update.hip): HIP events on the handle's filter stream
around 200 launches behind 20 warm-up launches, at 6n = 60 and 6n = 180 (and the empty window), m = 3 and 16 rows, one instance and a batch
of 128.  The state is the recorded sequence's at that window; H is dense N(0, 1), sigma 1 (no gate: every launch applies and writes the whole
covariance — repeated updates shrink P, the work per launch does not change).  Prints one JSON line per case.

    python tools/aux_update_cost.py [--batch 128]
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
    from rvio_amd import hip
    abi = A.abi
    for n in (0, 10, 30):
        ml = max(n + 1, 11)
        cfg = abi.config_named("B", enable_equalizer=0, max_track_len=ml)
        x, P = A.window_state(n)
        d = 24 + 6 * n
        for B in (1, a.batch):
            if B > 1 and ml > 22:
                continue      # (batch handles take windows up to 6n = 126 here: launch_plan.h)
            h = hip.RvioHip(cfg) if B == 1 else hip.RvioHip(cfg, batch=B, front_end=False)
            st = torch.cuda.ExternalStream(h.stream())
            for m in (3, 16):
                rng = np.random.default_rng(m)
                dH = torch.from_numpy(rng.standard_normal((m, d))).cuda()
                dv = torch.from_numpy(1e-3 * rng.standard_normal(m)).cuda()
                ds = torch.ones(m, dtype=torch.float64).cuda()
                torch.cuda.synchronize()
                us = timed(h, st, x, P, lambda: h.update_aux_dev(m, abi.RVIO_AUX_RESIDUAL, 0, dH.data_ptr(), 0, dv.data_ptr(), 0, ds.data_ptr(), 0), a.warmup, a.launches)
                gam, applied = h.aux_diag(B - 1)
                Pn = h.get_state_at(B - 1)[1]
                print(json.dumps(dict(clones=n, d=d, m=m, batch=B, us_per_launch=round(us, 2), us_per_instance=round(us / B, 3), applied=applied,
                                      finite=bool(np.all(np.isfinite(Pn))), symmetric=bool(np.array_equal(Pn, Pn.T)))), flush=True)
            h.close()


if __name__ == "__main__":
    main()
