"""The measurement updates keep their bits: auxiliary update, standstill, absolute fix and past-frame fix, in their host and _dev forms,
against what the build of commit a75ebdd45ed7949ec43b43aa5cfe2da6dc2c34a2 — the parent of the change that gave them one staging, guard and
read-back path — left for the same inputs (tests/golden/meas_bits_parent.npz, recorded by tools/record_meas_bits.py from THAT build's library,
not from the code under test).

No kernel and no launch argument changed, so every result is the SAME BITS: the state in full, the covariance (symmetric; compared as its
upper triangle), the feature's read-back behind every step, and no device error.  The cases (tests/meas_bits_cases.py) are the smallest that
reach every path of the host-side layer: both forms of aux_update_kernel in both modes at windows of 0, 3 and 10 clones; the host forms on
every instance and on one of three (the staged flags); the _dev forms with strides and device flags; an age outside the window; and two host
calls back to back on one handle, where the second takes the staging's reuse path."""
import numpy as np
import pytest

import meas_bits_cases as MB

pytestmark = pytest.mark.gpu
PARENT = "a75ebdd45ed7949ec43b43aa5cfe2da6dc2c34a2"


@pytest.fixture(scope="module")
def fixture():
    g = dict(np.load(MB.FIXTURE))
    assert str(g["parent"]) == PARENT
    return g


@pytest.mark.parametrize("case", MB.CASES, ids=[c["name"] for c in MB.CASES])
def test_measurement_update_keeps_the_parents_bits(case, fixture, gpu_required):
    g, name = fixture, case["name"]
    out = MB.run_case(g, case)
    assert int(out[name + "_err"]) == 0, name
    want = {k: v for k, v in g.items() if k.startswith(name + "_") and not MB.is_input(k)}
    seen = set()
    for k, v in out.items():
        if "_P" in k:                                    # symmetric, then its upper triangle
            assert np.array_equal(v, v.T), k
            k, v = k.replace("_P", "_Pu"), MB.triu(v)
        assert k in want, k
        assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), k
        seen.add(k)
    assert seen == set(want), sorted(set(want) - seen)
    # what the cases are there for, read off the replay itself
    states = MB.states_of(g, case)
    last = case["steps"][-1]
    untouched = [i for i in range(len(states)) if (last["form"] == "host" and last.get("instance", -1) not in (-1, i)) or
                 (last.get("active") is not None and not last["active"][i]) or (last["op"] == "past" and last["form"] == "dev" and last["age"][i] > case["n"])]
    for i in untouched:
        assert np.array_equal(out["%s_x%d" % (name, i)], states[i][0]) and np.array_equal(out["%s_P%d" % (name, i)], states[i][1]), (name, i)
    if last["op"] == "ss":                               # rvio_standstill.flags (byte 28): at rest, so is_static (4) and applied (8)
        flags = out["%s_s0_rec" % name][:, 28:32].copy().view(np.int32)
        assert np.all(flags & 4) and np.all(flags & 8), flags
    if last["op"] == "past" and last["form"] == "dev" and untouched:     # rvio_fix_diag (applied, kind, m, img_count from byte 56) outside the window
        applied, _, m, img_count = out["%s_s0_rec" % name][untouched[-1]][56:72].copy().view(np.int32)
        assert (applied, m, img_count) == (0, 0, -1)
