#!/usr/bin/env python3
"""Records tests/golden/meas_bits_parent.npz: the inputs of every case of tests/meas_bits_cases.py and what a build of the library leaves
for them — the measurement updates (auxiliary, standstill, absolute fix, past-frame fix) in their host and _dev forms.

    python tools/record_meas_bits.py --inputs                                       # CPU: start states and step inputs, from the feature tests' generators
    RVIO_HIP_LIB=<parent build>.so python tools/record_meas_bits.py <parent hash>   # GPU: the outputs of THAT build beside the stored inputs

The fixture pins a change of the host-side layer in front of aux_update_kernel to the bits of the build it was recorded from: run the second
step with RVIO_HIP_LIB pointing at the library of the commit BEFORE the change, and name that commit.  tests/test_gpu_meas_bits.py replays
the stored inputs through the same run_case."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import meas_bits_cases as MB  # noqa: E402


def record_inputs():
    g = MB.make_states()
    for c in MB.CASES:
        g.update(MB.make_inputs(g, c))
    assert all(MB.is_input(k) for k in g), [k for k in g if not MB.is_input(k)]
    np.savez_compressed(MB.FIXTURE, **g)
    print("inputs of %d cases written: %d bytes" % (len(MB.CASES), os.path.getsize(MB.FIXTURE)))


def record_outputs(parent):
    import torch                 # before the library: torch brings its own HIP runtime
    assert torch.cuda.is_available()
    torch.cuda.init()
    from rvio_amd import hip
    g = {k: v for k, v in np.load(MB.FIXTURE).items() if MB.is_input(k)}
    out = {"parent": np.array(parent)}
    for c in MB.CASES:
        o = MB.run_case(g, c)
        assert int(o[c["name"] + "_err"]) == 0, c["name"]
        for k in [k for k in o if "_P" in k]:
            P = o.pop(k)
            assert np.array_equal(P, P.T), k
            o[k.replace("_P", "_Pu")] = MB.triu(P)
        out.update(o)
        print("%-16s recorded from %s: %d arrays" % (c["name"], hip.LIB_PATH, len(o)), flush=True)
    g.update(out)
    np.savez_compressed(MB.FIXTURE, **g)
    print("fixture written: %d bytes, parent %s" % (os.path.getsize(MB.FIXTURE), parent))


if __name__ == "__main__":
    if "--inputs" in sys.argv[1:]:
        record_inputs()
    elif len(sys.argv) == 2 and os.environ.get("RVIO_HIP_LIB"):
        record_outputs(sys.argv[1])
    else:
        sys.exit(__doc__)
