"""CPU-side checks of the auxiliary measurement update (added within ABI 6): the three entry points are exported, declared and named on the
ABI-version line; rvio_aux_meas has the layout a C++ compiler gives the header's struct; NULL handles are refused; and abi.aux_update_model —
the NumPy model the device is held to — is pinned to the CPU oracle on the sub-class the oracle covers (an H whose first 24 columns are zero:
tests/aux_update_cases.py oracle_update).  No compute is launched here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import aux_update_cases as A
import oracle as O

abi = O.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rvio_hip_update_aux", "rvio_hip_update_aux_dev", "rvio_hip_get_aux_diag")
FIELDS = ("m", "mode", "gate", "reserved", "H", "v", "sigma")


@pytest.fixture(scope="module")
def lib():
    from rvio_amd import build, hip
    build.build()
    return hip.load()


def test_symbols_exported_and_declared_within_abi_6(lib):
    from rvio_amd import hip
    assert abi.ABI_VERSION == 6 and lib.rvio_hip_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "rvio_hip.h")).read()
    declared = set(re.findall(r"\b(rvio_(?:hip_)?[a-z_]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in hip.SYMBOLS and hasattr(lib, s), s
    version_line = [l for l in hdr.splitlines() if l.startswith("#define RVIO_HIP_ABI_VERSION")][0]
    assert "#define RVIO_HIP_ABI_VERSION 6" in version_line and "within 6" in version_line.lower()
    assert all(s in version_line for s in NEW + ("rvio_aux_meas",))
    assert "#define RVIO_AUX_MAX_ROWS 16" in hdr and abi.RVIO_AUX_MAX_ROWS == 16
    assert re.search(r"RVIO_AUX_RESIDUAL\s*=\s*0\s*,\s*RVIO_AUX_VALUE\s*=\s*1", hdr) and (abi.RVIO_AUX_RESIDUAL, abi.RVIO_AUX_VALUE) == (0, 1)


def test_struct_layout_matches_a_cxx_compiler(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "rvio_hip.h"\nint main() {\n  std::printf("%zu", sizeof(rvio_aux_meas));\n'
                   + "".join('  std::printf(" %%zu", offsetof(rvio_aux_meas, %s));\n' % f for f in FIELDS) + '  std::printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == C.sizeof(abi.rvio_aux_meas) == 40
    assert got[1:] == [getattr(abi.rvio_aux_meas, f).offset for f in FIELDS] == [0, 4, 8, 12, 16, 24, 32]


def test_null_handle_is_invalid(lib):
    H, v, s = np.zeros((1, 24)), np.zeros(1), np.ones(1)
    ms = abi.make_aux_meas(H, v, s)
    g, a = C.c_double(0), C.c_int32(0)
    dp = C.POINTER(C.c_double)
    assert lib.rvio_hip_update_aux(None, 0, C.byref(ms)) == -1
    assert lib.rvio_hip_update_aux_dev(None, 1, 0, 0, H.ctypes.data_as(dp), C.c_size_t(0), v.ctypes.data_as(dp), C.c_size_t(0), s.ctypes.data_as(dp), C.c_size_t(0), None) == -1
    assert lib.rvio_hip_get_aux_diag(None, 0, C.byref(g), C.byref(a)) == -1


# ---------------------------------------------------------------- the NumPy model against the oracle
# n = 3, 4: states of the max_track_len = 32 sequence while its window fills; n = 10: the two 10-clone states of tests/imu_pose_cases.py
def _states(n):
    if n == 10:
        return [("window10",) + A.K.state("window10"), ("moved",) + A.K.state("moved")]
    return [("fill%d" % n,) + A.window_state(n)]


@pytest.mark.parametrize("m", [1, 3, 16])
@pytest.mark.parametrize("n", [3, 4, 10])
def test_model_against_the_oracle_on_clone_only_stacks(n, m):
    cfg = A.K.config() if n == 10 else A.long_config()
    for name, x, P in _states(n):
        H, v, sigma = A.measurement(P, m, seed=3, kind="clone")
        xo, Po = A.oracle_update(cfg, x, P, H, v, sigma)
        xm, Pm, gamma = abi.aux_update_model(x, P, H, v, sigma)
        dxw, dpw = A.S.state_delta(xm, xo), float(np.max(np.abs(Pm - Po)))
        print("%s n = %d m = %d: model vs oracle  state %.3e  P %.3e (max|P| %.3e)  gamma %.4g" % (name, n, m, dxw, dpw, np.max(np.abs(Po)), gamma))
        assert dxw <= A.X_TOL and dpw <= A.p_bar(Po)
        assert np.array_equal(Pm, Pm.T)
        assert np.max(np.abs(xm - x)) > 1e-9        # the update moved the state: the comparison is not between two copies of the input


@pytest.mark.parametrize("name", ["window10", "moved"])
def test_value_mode_is_residual_mode_on_z_minus_H_xi(name):
    x, P = A.K.state(name)
    d = P.shape[0]
    rng = np.random.default_rng(5)
    H = rng.standard_normal((6, d))
    H[:, [0, 1, 2, 9, 10, 11]] = 0.0
    for p in range((d - 24) // 6):
        H[:, 24 + 6 * p: 27 + 6 * p] = 0.0
    z, sigma = rng.standard_normal(6), 10.0 ** rng.uniform(-3, -1, 6)
    xi = abi.aux_xi(x)
    assert np.array_equal(xi[15:18], x[17:20]) and np.array_equal(xi[3:9], x[4:10]) and np.array_equal(xi[27:30], x[30:33]) and not xi[24:27].any()
    a = abi.aux_update_model(x, P, H, z, sigma, abi.RVIO_AUX_VALUE)
    b = abi.aux_update_model(x, P, H, z - H @ xi, sigma, abi.RVIO_AUX_RESIDUAL)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    # zero velocity: the residual is minus the velocity, and the update pulls the velocity towards zero
    Hz, zz, sz = A.zupt(d, sigma=1e-3)
    xz = abi.aux_update_model(x, P, Hz, zz, sz, abi.RVIO_AUX_VALUE)[0]
    assert np.linalg.norm(xz[17:20]) < np.linalg.norm(x[17:20])


def test_replay_usage_lists_velocity():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host")], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(ROOT, "host", "rvio_replay")], capture_output=True, text=True)
    assert r.returncode == 2 and "--velocity FILE" in r.stderr and "--velocity-sigma S" in r.stderr and "--velocity-gate" in r.stderr, r.stderr
