"""The kernels that run PreIntegrator::propagate's sample loop keep their bits: propagate in every launch form (propagate_chol_kernel<2> and <3>, propagate_kernel3
at n = 0, at the long window and with the slab stride, propagate_kernel3b, feat_prop_kernel), imu_pose_kernel and imu_cov_kernel through
rvio_hip_predict / rvio_hip_predict_cov in their host and _dev forms, and both IMU-rate rings — against what the build of commit
00b55d4 — the parent of the change that folded the record kernels' copies of the sample loop into csrc/imu_preint.h — left for the
same inputs (tests/golden/imu_bits_parent.npz, recorded by tools/record_imu_bits.py from THAT build's library, not from the code under test).

The machine code of the two record kernels changed (instruction order, register numbers), their arithmetic may not; the propagate forms are in
the fixture for the day propagate_body calls the header too: every output is the SAME BITS —
the state in full, the covariance (as the SHA-256 of its bytes, and its 24 x 24 head in full), every record, and no device error.  The cases
(tests/imu_bits_cases.py) are the chunk edges of each kernel with zero dt, samples at rest and both nSmallAngle branches in the batches."""
import numpy as np
import pytest

import imu_bits_cases as IB

pytestmark = pytest.mark.gpu
PARENT = "00b55d4"


@pytest.fixture(scope="module")
def fixture():
    g = dict(np.load(IB.FIXTURE))
    assert str(g["parent"]).startswith(PARENT)
    return g


@pytest.fixture(scope="module")
def handles(gpu_required):
    hs = {}
    yield hs
    for h in hs.values():
        h.close()


@pytest.mark.parametrize("case", IB.CASES, ids=[c["name"] for c in IB.CASES])
def test_imu_preintegration_keeps_the_parents_bits(case, fixture, handles):
    g, name = fixture, case["name"]
    raw = IB.run_case(g, case, handles)
    assert int(raw[name + "_err"]) == 0, name
    out = IB.pack(raw)
    want = {k: v for k, v in g.items() if k.startswith(name + "_") and not IB.is_input(k)}
    assert set(out) == set(want), sorted(set(out) ^ set(want))
    for k, v in out.items():
        assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), k
    # what the cases are there for, read off the replay itself
    if case["op"] == "ring":                         # of 17 samples a ring of 8 keeps the last 8, under the same seq in both rings
        pose, cov = raw[name + "_pose"], raw[name + "_cov"]
        last = np.arange(IB.RING_M - IB.RING_CAP + 1, IB.RING_M + 1)
        assert np.array_equal(pose["seq"], last) and np.array_equal(cov["seq"], last) and np.array_equal(pose["index"], last - 1)
        assert np.array_equal(pose["v"][-1], raw[name + "_x"][17:20])      # the last record is what propagate leaves
