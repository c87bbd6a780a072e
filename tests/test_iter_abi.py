"""CPU: the iterated measurement update's ABI mirror and its NumPy model (abi.iter_update_model) on the cases of tests/iter_cases.py.  The model
with one pass is abi.aux_update_model; every far case is one a single linearisation fails at (its whitened residuals at the posterior are at
least 10 x the iterated update's); the step sequence converges; the same loop in extended precision gives the rounding floor the device is
held against (tests/test_gpu_iter.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import iter_cases as I

abi, A = I.abi, I.A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = I.cases()
FAR = [c for c in CASES if "-far-" in c.name]
STEP_FLOOR = 1e-12      # below it a step is the rounding of a correction of size <= 1 (2^-53 x a few hundred operations), not the iteration's progress


def test_struct_setting_and_symbols():
    assert C.sizeof(abi.rvio_meas_iter) == 24 and abi.RVIO_MEAS_MAX_ITERS == 8 and abi.ABI_VERSION == 6
    assert [f[0] for f in abi.rvio_meas_iter._fields_] == ["step", "gamma0", "iterations", "converged"]
    hdr = open(os.path.join(ROOT, "include", "rvio_hip.h")).read()
    assert "#define RVIO_MEAS_MAX_ITERS 8" in hdr and "#define RVIO_HIP_ABI_VERSION 6" in hdr
    assert re.search(r"typedef struct rvio_meas_iter \{ double step; double gamma0; int32_t iterations, converged; \} rvio_meas_iter;", hdr)
    from rvio_amd import hip
    for s in ("rvio_hip_set_meas_iterations", "rvio_hip_get_meas_iterations", "rvio_hip_get_meas_iter"):
        assert s in hip.SYMBOLS and re.search(r"\bint %s\(rvio_hip\* h" % s, hdr), s


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_one_pass_is_the_one_shot_update(c):
    x1, P1, g1 = c.one_shot()
    xm, Pm, info = c.model(1, 0.0)
    ex, eP = float(np.max(np.abs(xm - x1))), float(np.max(np.abs(Pm - P1)))
    print("%s: |x - one shot| %.1e  |P - one shot| %.1e  gamma0 %.6g vs %.6g" % (c.name, ex, eP, info["gamma0"], g1))
    assert ex <= 1e-14 and eP <= 1e-14 and info["iterations"] == 1 and len(info["steps"]) == 1
    assert abs(info["gamma0"] - g1) <= 1e-9 * g1


@pytest.mark.parametrize("c", FAR, ids=lambda c: c.name)
def test_one_linearisation_fails_every_far_case(c):
    x1 = c.one_shot()[0]
    x8 = c.model(8, 0.0)[0]
    s1, s8 = c.whitened_ss(x1), c.whitened_ss(x8)
    e0, e1, e8 = (float(np.linalg.norm(abi.pose_line(x)[0] - abi.pose_line(c.x_true)[0])) for x in (c.x0, x1, x8))
    print("%s: whitened residual sum one shot %.4g, 8 passes %.4g (x %.1f); pose line error prior %.3g m, one shot %.3g m, 8 passes %.3g m"
          % (c.name, s1, s8, s1 / s8, e0, e1, e8))
    assert s1 >= 10 * s8


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_the_steps_converge(c):
    steps = c.model(8, 0.0)[2]["steps"]
    print("%s: steps %s" % (c.name, " ".join("%.1e" % s for s in steps)))
    assert len(steps) == 8 and min(steps) < 1e-6
    for i in range(1, 7):
        assert steps[i + 1] < steps[i] or steps[i] <= STEP_FLOOR, i
    early = c.model(8, 1e-6)[2]
    assert early["converged"] and early["iterations"] == 1 + next(i for i, s in enumerate(steps) if s < 1e-6) and early["steps"] == steps[:early["iterations"]]


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_float_floor_against_extended_precision(c):
    """the float64 loop against the same loop with its linear algebra in np.longdouble: the floor of any float64 implementation of it"""
    assert np.finfo(np.longdouble).eps < np.finfo(float).eps, "np.longdouble is no wider than float64 here: this check needs x87 extended precision"
    for iters in (2, 5, 8):
        x, P, _ = c.model(iters, 0.0)
        xl, Pl, _ = c.model(iters, 0.0, np.longdouble)
        fx, fP = float(np.max(np.abs(x - xl))), float(np.max(np.abs(P - np.asarray(Pl, float))))
        print("%s K=%d: floor state %.1e (device bar %.0e), P %.1e (device bar %.1e)" % (c.name, iters, fx, A.X_TOL, fP, A.p_bar(P)))
        assert 10 * fx <= A.X_TOL and 10 * fP <= A.p_bar(P)      # the project's bars leave the floor its 10 x
