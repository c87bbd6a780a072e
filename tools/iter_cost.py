#!/usr/bin/env python3
"""Device time of an iterated measurement call (rvio_hip_set_meas_iterations: the rows kernel and csrc/aux_update.hip aux_iter_kernel, max_iters
times on the filter stream) against the same call at max_iters = 1 — the plain kernels — on the same build, handle and state: a POSITION fix
(m = 3: the MB 4 form) and a map call of 8 points at age n (m = 16: the MB 16 form) at 6n = 60 and 186, one instance, tol = 0 so that every
pass runs to the end of the kernel's decision (the last one alone writes P).  HIP events on the handle's filter stream around 200 calls behind
20 warm-up calls, two alternating repetitions.  Prints one JSON line per case; us_per_extra_pass = (t_K - t_1) / (K - 1).

    python tools/iter_cost.py
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
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import map_cases as M
    from rvio_amd import hip
    abi, A = M.abi, M.A
    cfg = A.long_config()
    h = hip.RvioHip(cfg)
    st = torch.cuda.ExternalStream(h.stream())
    keep = []
    for n in (10, 31):
        x, P = A.window_state(n)
        # (wide sigmas: 220 updates in a row must leave a covariance the next one can still factor)
        fix = abi.make_fix(abi.fix_h(cfg, x, abi.RVIO_FIX_POSITION)[0:3] + 0.01, None, 1.0, 0.0)
        d_fix = torch.from_numpy(np.frombuffer(bytes(fix), np.uint8).copy()).cuda()
        obs = abi.make_map_obs(M.observations(cfg, x, n, [M.GOOD] * 8, seed=n, sigma=1.0))
        d_obs = torch.from_numpy(np.frombuffer(bytes(obs), np.uint8).copy()).cuda()
        d_age = torch.full((1,), n, dtype=torch.int32).cuda()
        keep += [d_fix, d_obs, d_age]
        torch.cuda.synchronize()
        calls = (("update_fix_dev", 3, lambda d_fix=d_fix: h.update_fix_dev(abi.RVIO_FIX_POSITION, 0, d_fix.data_ptr(), 0, None)),
                 ("update_map_dev", 16, lambda d_obs=d_obs, d_age=d_age: h.update_map_dev(abi.RVIO_MAP_NORMALISED, 0, 0, 8, d_obs.data_ptr(), 0, None, d_age.data_ptr(), None)))
        for rep in range(2):          # (twice, alternating: the spread)
            for case, m, call in calls:
                base = None
                for iters in (1, 2, 4, 8):
                    h.set_meas_iterations(iters, 0.0)
                    us = timed(h, st, x, P, call, a.warmup, a.launches)
                    it = h.get_meas_iter()
                    base = us if iters == 1 else base
                    print(json.dumps(dict(case=case, rows=m, clones=n, max_iters=iters, rep=rep, us_per_call=round(us, 2),
                                          us_per_extra_pass=None if iters == 1 else round((us - base) / (iters - 1), 2), passes=int(it.iterations))), flush=True)
    h.set_meas_iterations(1, 0.0)
    assert h.frame_info()["device_error"] == 0
    h.close()


if __name__ == "__main__":
    main()
