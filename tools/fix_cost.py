#!/usr/bin/env python3
"""Device time of one absolute fix (rvio_hip_update_fix_dev: csrc/fix_rows.hip in front of csrc/aux_update.hip): HIP events on the handle's filter
stream around 200 calls behind 20 warm-up calls, at 6n = 60 and 6n = 180, one instance and a batch of 128, a POSITION fix (m = 3, the <4> form of
the update) and a POSE fix (m = 6, the <16> form), gate off.  fix_rows_kernel alone is the same call with every instance flagged inactive — the
kernel then returns at once, so that case bounds the launch, not the arithmetic — and, for the arithmetic, the difference between the whole call
and rvio_hip_update_aux_dev alone on the rows the device formed.  Filter-only handles.  Prints one JSON line per case.

    python tools/fix_cost.py [--batch 128]
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
    from rvio_amd import hip
    abi = A.abi
    cfg = A.long_config()
    for n in (10, 30):
        x, P = F.moved_window(n)
        for B in (1, a.batch):
            h = hip.RvioHip(cfg) if B == 1 else hip.RvioHip(cfg, batch=B, front_end=False)
            st = torch.cuda.ExternalStream(h.stream())
            d_off = torch.zeros(B, dtype=torch.int32).cuda()
            torch.cuda.synchronize()
            for kind, name in ((abi.RVIO_FIX_POSITION, "position_m3"), (abi.RVIO_FIX_POSE, "pose_m6")):
                # (a wide sigma: 220 updates in a row must leave a covariance the next one can still factor)
                fix = F.fix_near(cfg, x, kind, F.LEVER, sigma_p=1.0, sigma_q=0.5)
                d_fix = torch.from_numpy(np.frombuffer(bytes(fix), np.uint8).copy()).cuda()
                h.set_state(x, P)
                h.update_fix_dev(kind, 0, d_fix.data_ptr(), 0, None)
                Hd, sd = h.get_fix_rows(0)
                rd = np.array(h.get_fix(0).r[:len(sd)])
                dH, dr, ds = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (Hd, rd, sd))
                torch.cuda.synchronize()
                cases = (("aux_update_alone", lambda: h.update_aux_dev(len(sd), abi.RVIO_AUX_RESIDUAL, 0, dH.data_ptr(), 0, dr.data_ptr(), 0, ds.data_ptr(), 0)),
                         ("fix_all_inactive", lambda: h.update_fix_dev(kind, 0, d_fix.data_ptr(), 0, d_off.data_ptr())),
                         ("fix_with_update", lambda: h.update_fix_dev(kind, 0, d_fix.data_ptr(), 0, None)))
                for rep in range(2):          # (twice, alternating: the spread)
                    for case, call in cases:
                        us = timed(h, st, x, P, call, a.warmup, a.launches)
                        applied = int(h.get_fix(B - 1).applied) if case.startswith("fix") else None
                        print(json.dumps(dict(case=case, fix=name, rep=rep, batch=B, clones=n, us_per_call=round(us, 2), us_per_instance=round(us / B, 3),
                                              applied=applied)), flush=True)
            assert h.frame_info()["device_error"] == 0
            h.close()


if __name__ == "__main__":
    main()
