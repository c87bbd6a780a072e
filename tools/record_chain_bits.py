#!/usr/bin/env python3
"""Records tests/golden/chain_bits_parent.npz: the inputs of every case of tests/chain_bits_cases.py and what a build of the library
leaves for them after set_state -> propagate -> update (state in full; covariance as its upper triangle, or as a SHA-256 digest).

    python tools/record_chain_bits.py --inputs              # CPU: the case inputs, from the oracle's recorded sequences (no device)
    RVIO_HIP_LIB=<parent build>.so python tools/record_chain_bits.py     # GPU: the outputs of THAT build beside the stored inputs

The fixture pins a re-scheduling of the solve / Joseph kernels to the bits of the build it was recorded from: run the second step with
RVIO_HIP_LIB pointing at the library of the commit BEFORE the change.  The comparison never involves the host's oracle build: the test
replays the stored inputs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import chain_bits_cases as CB  # noqa: E402


def record_inputs():
    import oracle as O
    import scenarios as S
    abi = O.abi
    out = {}

    def put(s, x0, P0, imu, types, lens, meas):
        out[s + "_x0"], out[s + "_P0u"] = np.asarray(x0, float), CB.triu(np.asarray(P0, float))
        out[s + "_imu"] = np.ascontiguousarray(imu).view(np.uint8)
        out[s + "_types"], out[s + "_lens"], out[s + "_meas"] = np.asarray(types), np.asarray(lens), np.asarray(meas)

    cfg = abi.config_named("B", enable_equalizer=0)
    seq, recs = S.record_sequence(cfg, n_frames=30)
    by_n = {}
    for r in recs:
        if r["did_update"]:
            by_n[(len(r["x0"]) - 26) // 7] = r      # the last record of every window length
    for n in (3, 5, 8, 10):
        r = by_n[n]
        put("fill%d" % n if n < 10 else "n10", r["x0"], r["P0"], r["inp"]["imu"], r["types"], r["lens"], r["meas"])
    # the full loads (cfg B: the headline load; cfg A, cfg C: the longer windows) are those of full_load_inputs.npz; only the IMU samples of the
    # propagation in front of them are stored here
    for s in CB.FULL_LOAD_SETS:
        out[s + "_imu"] = np.ascontiguousarray(by_n[10]["inp"]["imu"]).view(np.uint8)
    # what the oracle makes of every case: the loaded cases must update, the pass-through must not
    g = out
    for case in CB.CASES_B + CB.CASES_WINDOWS:
        cfg, x0, P0, imu, types, lens, meas = CB.case_inputs(g, abi, case)
        x1, P1 = O.propagate(cfg, x0, P0, imu)
        x2, P2, dg = O.update(cfg, x1, P1, types, lens, meas)
        print("%-6s n = %2d  features %3d  accepted %3d  updated %d" % (case[0], (len(x0) - 26) // 7, len(types), int(np.count_nonzero(dg["accepted"])), int(dg["updated"])), flush=True)
        assert bool(dg["updated"]) == (case[0] != "pass"), case
    np.savez_compressed(CB.FIXTURE, **out)
    print("inputs written:", os.path.getsize(CB.FIXTURE), "bytes")


def record_outputs():
    import torch                 # before the library: torch brings its own HIP runtime
    assert torch.cuda.is_available()
    torch.cuda.init()
    from pkgload import load_pkg
    abi = load_pkg().abi
    from rvio_amd import hip
    g = dict(np.load(CB.FIXTURE))
    for k in [k for k in g if k.endswith(("_x", "_Pu", "_Psha"))]:
        del g[k]
    handles = {}
    for case in CB.CASES_B + CB.CASES_WINDOWS:
        cfg, x0, P0, imu, types, lens, meas = CB.case_inputs(g, abi, case)
        if case[1] not in handles:
            handles[case[1]] = hip.RvioHip(cfg)
        x, P, err = CB.run_case(handles[case[1]], x0, P0, imu, types, lens, meas)
        assert err == 0 and np.array_equal(P, P.T), case
        g[case[0] + "_x"] = x
        if case[0] in CB.DIGEST_ONLY:
            g[case[0] + "_Psha"] = np.array(CB.sha(P))
        else:
            g[case[0] + "_Pu"] = CB.triu(P)
        print("%-6s recorded from %s: P %s" % (case[0], hip.LIB_PATH, CB.sha(P)[:16]), flush=True)
    for h in handles.values():
        h.close()
    np.savez_compressed(CB.FIXTURE, **g)
    print("fixture written:", os.path.getsize(CB.FIXTURE), "bytes")


if __name__ == "__main__":
    if "--inputs" in sys.argv[1:]:
        record_inputs()
    else:
        record_outputs()
