"""The cases of tests/propagate_cases.py on the CPU: every case that goes to the device can fail there (the oracle reacts to a dt swapped across
a chunk boundary, or to the other nSmallAngle branch, by >= 1000 bars), the oracle stays finite on all of them, and the oracle agrees with a
fresh np.longdouble restatement of the recursion on the 24 x 24 head — the printed figures are the rounding floor of the reference itself, the
floor under the normalised P bar of tests/test_gpu_propagate_edges.py."""
import numpy as np
import pytest

import propagate_cases as PC

O, S = PC.O, PC.S


def test_start_states():
    for name in PC.STATES:
        x, P = PC.state(name)
        n = (len(x) - 26) // 7
        assert n == PC.n_clones(name) and P.shape[0] == 24 + 6 * n and np.all(np.isfinite(x)) and np.all(np.isfinite(P))
        assert np.array_equal(P, P.T)
    assert PC.n_clones("empty") == 0 and PC.n_clones("window10") == 10
    assert 65 <= 6 * PC.n_clones("mid") <= 96 and 6 * PC.n_clones("long") > 144
    assert PC.config("long").max_track_len == 32          # the longest window rvio_hip_create accepts
    for name in ("window10", "mid"):
        assert PC.frame_record(name)["diag"]["updated"]   # the fused form's frame applies an update


@pytest.mark.parametrize("seed", [0, 1, 5])
def test_irregular_batches_have_what_they_promise(seed):
    x, _ = PC.state("window10")
    small = PC.config("window10").small_angle
    for m in PC.M_EDGES:
        imu, slow, zero = PC.irregular(m, x, seed)
        assert len(imu) == m and imu["dt"].sum() > 0
        assert set(np.round(imu["dt"] / PC.DT0, 6)) <= set(PC.DT_MULT)
        wn = np.linalg.norm(imu["w"] - x[20:23], axis=1)
        assert all(wn[p] < small for p in slow) and len(slow) == (m + 2) // 5
        if zero >= 0:
            assert wn[zero] == 0.0
        assert m == 1 or zero >= 0
        for b in PC.BOUNDARIES:
            if b < m:
                assert imu["dt"][b - 1] != imu["dt"][b]
    # over the sizes, every kind of edge position is hit by a slow sample, zero-dt duplicates and dropped samples occur
    hit, dts = set(), set()
    for m in PC.M_EDGES:
        for s in range(9):
            imu, slow, zero = PC.irregular(m, x, s)
            hit |= set(slow)
            dts |= set(np.round(imu["dt"] / PC.DT0, 6))
    assert {0, 7, 8, 15, 16, 31, 32} <= hit and dts == set(PC.DT_MULT)


def test_branch_batches_alternate_around_small_angle():
    x, _ = PC.state("window10")
    for m in (9, 10, 17):
        imu = PC.branch(m, x)
        wn = np.linalg.norm(imu["w"] - x[20:23], axis=1)
        assert np.allclose(wn[0::2], 0.4, atol=1e-12) and np.allclose(wn[1::2], 0.6, atol=1e-12) and np.all(imu["dt"] == PC.BRANCH_DT)
        assert PC.case_cfg("window10", "branch").small_angle == 0.5


@pytest.mark.parametrize("state", PC.STATES)
def test_every_plain_case_can_fail(state):
    """chunk boundaries 7|8, 15|16, 31|32 and the branch: the oracle's reaction, in bars"""
    for m in PC.M_EDGES:
        c = PC.conditions(state, "irregular", m)
        assert (m > 8) == bool(c)
        for what, d in c.items():
            print("%-8s irregular(%2d) %-9s state %.2e   normalised P %.2e" % (state, m, what, d[0], d[1]))
    for m in (10, 17):
        d = PC.conditions(state, "branch", m)["branch"]
        print("%-8s branch(%2d)    other branch: state %.2e   normalised P %.2e" % (state, m, d[0], d[1]))


def test_every_batch_case_can_fail():
    """the per-instance seeds of the batch forms (tests/test_gpu_propagate_edges.py: seeds 0 .. 8)"""
    for state in ("window10", "long"):
        for seed in range(9):
            for m in (9, 16, 17, 33):
                PC.conditions(state, "irregular", m, seed)
            PC.conditions(state, "branch", 9, seed)
        # different instances really get different batches
        a, b = PC.case(state, "irregular", 17, 0)[3], PC.case(state, "irregular", 17, 1)[3]
        assert not np.array_equal(a["dt"], b["dt"]) and not np.array_equal(a["w"], b["w"])


def test_oracle_against_the_longdouble_model():
    """the oracle (double, the reference's order of operations) against the recursion in np.longdouble on the head: the reference's own floor"""
    assert np.finfo(np.longdouble).eps < 1e-18
    worst = [0.0, 0.0, 0.0]
    for state in ("empty", "window10"):
        for kind, ms in (("irregular", PC.M_EDGES), ("branch", (9, 10, 17))):
            for m in ms:
                d = PC.oracle_vs_longdouble(state, kind, m)
                print("%-8s %-9s m %2d   state %.2e   P project norm %.2e   P normalised %.2e" % ((state, kind, m) + d))
                worst = [max(a, b) for a, b in zip(worst, d)]
    print("oracle against longdouble, worst: state %.2e   P project norm %.2e   P normalised %.2e" % tuple(worst))
    # double rounding over at most 65 samples of 24 x 24 products: m * 24 * eps = 3.5e-13, with a factor for the cancellation in Phi P Phi^T
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12 and worst[2] <= 1e-11, worst
    assert worst[2] * 10 <= 1e-8            # the floor leaves room for a device bar under the 1e-8 cap
