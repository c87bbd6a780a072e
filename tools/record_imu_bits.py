#!/usr/bin/env python3
"""Records tests/golden/imu_bits_parent.npz (and the images of its fused case, tests/golden/imu_bits_images.npz): the inputs of every case of
tests/imu_bits_cases.py and what a build of the library leaves for them — propagate in every launch form, the IMU-rate pose and covariance
records in their host and _dev forms, and both rings.

    python tools/record_imu_bits.py --inputs                                       # CPU: start states, IMU batches and images, checked through the oracle
    RVIO_HIP_LIB=<parent build>.so python tools/record_imu_bits.py <parent hash>   # GPU: the outputs of THAT build beside the stored inputs

The fixture pins a change to the sample loop of csrc/imu_preint.h and propagate_body to the bits of the build it was recorded from: run the second
step with RVIO_HIP_LIB pointing at the library of the commit BEFORE the change, and name that commit.  tests/test_gpu_imu_bits.py replays the
stored inputs through the same run_case."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import imu_bits_cases as IB  # noqa: E402


def record_inputs():
    import ctypes
    import imu_pose_cases as IC
    import propagate_cases as PC
    assert IB.STATE_ML == {"mid": PC.MID_ML, "long": PC.long_ml()} and IB.BRANCH_SMALL_ANGLE == PC.BRANCH_SMALL_ANGLE
    g = {}
    for s in IB.PROP_STATES:
        x, P = PC.state(s)
        g["st_%s_x0" % s], g["st_%s_P0u" % s] = x, IB.triu(P)
    for s in IC.STATES:
        x, P = IC.state(s)
        g["st_ip_%s_x0" % s], g["st_ip_%s_P0u" % s] = x, IB.triu(P)

    def raw(cfg):
        return ctypes.string_at(ctypes.addressof(cfg), ctypes.sizeof(cfg))

    def irregular(state, m, n=1):
        """n batches: those of the first n seeds at which a batch of m >= 2 samples has a zero dt"""
        x = g["st_%s_x0" % state]
        seeds = [s for s in range(18) if m < 2 or np.any(PC.irregular(m, x, s)[0]["dt"] == 0.0)][:n]
        assert len(seeds) == n, (state, m, n)
        for s in seeds:
            PC.conditions(state, "irregular", m, s)           # the oracle's result is finite and reacts to a dt swapped across every chunk boundary
        return [PC.irregular(m, x, s)[0] for s in seeds]

    def branch(state, m, n=1):
        x = g["st_%s_x0" % state]
        out = [PC.branch(m, x, i) for i in range(n)]
        for i, imu in enumerate(out):
            w1 = np.linalg.norm(imu["w"] - x[20:23], axis=1)
            assert np.any(w1 < IB.BRANCH_SMALL_ANGLE) and np.any(w1 > IB.BRANCH_SMALL_ANGLE), (state, m, i)
            PC.conditions(state, "branch", m, i)              # forcing the other branch moves the oracle's state by >= 1000 bars
        return out

    def special(state, m, n=1):
        """imu_pose_cases' batches: from m = 2 on the last sample in the small-angle branch, the one before it with dt = 0"""
        x = g["st_%s_x0" % state]
        out = [IC.batch(m, i, m >= 2, x) for i in range(n)]
        for imu in out:
            if m >= 2:
                assert imu["dt"][m - 2] == 0.0 and np.linalg.norm(imu["w"][m - 1] - x[20:23]) < IC.config().small_angle
                assert np.linalg.norm(imu["w"][0] - x[20:23]) > IC.config().small_angle or m == 2
            p, q, v = IC.oracle_records(x[:26], IB.from_triu(g["st_%s_P0u" % state])[:24, :24], imu)
            assert np.all(np.isfinite(p)) and np.all(np.isfinite(q)) and np.all(np.isfinite(v))
        return out

    make = {"irregular": irregular, "branch": branch, "special": special}
    for c in IB.CASES:
        if c["state"] in IB.PROP_STATES:
            assert raw(IB.cfg_of(c)) == raw(PC.case_cfg(c["state"], c["kind"])), c["name"]
        else:
            assert raw(IB.cfg_of(c)) == raw(IC.config()), c["name"]
        imu = make[c["kind"]](c["state"], c["m"], c.get("B", 1))
        g[c["name"] + "_imu"] = np.ascontiguousarray(np.stack(imu) if "B" in c else imu[0]).view(np.uint8)
        print("%-22s %-8s m = %2d  zero dt %d" % (c["name"], c["kind"], c["m"], int(np.count_nonzero(np.concatenate(imu)["dt"] == 0.0))), flush=True)
    assert all(IB.is_input(k) for k in g)
    np.savez_compressed(IB.FIXTURE, **g)
    # the fused case's front end: the images, corner lists and IMU batches of the frames ahead of the recorded frame that starts on the full window
    seq, r = PC.recorded("window10")[0], PC.frame_record("window10")
    assert np.array_equal(r["x0"], g["st_window10_x0"])
    im = {"imgs": np.stack([seq.render(k) for k in range(IB.FUSED_FIRST, r["k"] + 1)])}
    for i, k in enumerate(range(IB.FUSED_FIRST, r["k"] + 1)):
        xy, vis = seq.project(k, noise=False)
        im["cand%d" % i] = np.ascontiguousarray(seq.candidates(k, xy, vis)[0], np.float32)
        im["imu%d" % i] = np.ascontiguousarray(seq.imu_between(k)).view(np.uint8)
    np.savez_compressed(IB.IMAGES, **im)
    print("inputs of %d cases written: %d + %d bytes" % (len(IB.CASES), os.path.getsize(IB.FIXTURE), os.path.getsize(IB.IMAGES)))


def record_outputs(parent):
    import torch                 # before the library: torch brings its own HIP runtime
    assert torch.cuda.is_available()
    torch.cuda.init()
    from rvio_amd import hip
    g = {k: v for k, v in np.load(IB.FIXTURE).items() if IB.is_input(k)}
    out, handles = {"parent": np.array(parent)}, {}
    t0 = time.time()
    try:
        for c in IB.CASES:
            o = IB.pack(IB.run_case(g, c, handles))
            assert int(o[c["name"] + "_err"]) == 0, c["name"]
            out.update(o)
            print("%-22s recorded from %s: %d arrays" % (c["name"], hip.LIB_PATH, len(o)), flush=True)
    finally:
        for h in handles.values():
            h.close()
    g.update(out)
    np.savez_compressed(IB.FIXTURE, **g)
    print("fixture written: %d bytes, parent %s, %.1f s for %d cases" % (os.path.getsize(IB.FIXTURE), parent, time.time() - t0, len(IB.CASES)))


if __name__ == "__main__":
    if "--inputs" in sys.argv[1:]:
        record_inputs()
    elif len(sys.argv) == 2 and os.environ.get("RVIO_HIP_LIB"):
        record_outputs(sys.argv[1])
    else:
        sys.exit(__doc__)
