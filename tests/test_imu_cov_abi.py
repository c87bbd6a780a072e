"""CPU-side checks of IMU-rate odometry with covariance (added within ABI 6): rvio_imu_cov has the layout a C++ compiler gives the header's
struct, the four entry points are exported, declared and refuse a NULL handle, abi.imu_pose_cov_jacobian is the Jacobian central differences of
the reference's injection give through composition and the pose line, and abi.imu_cov_model — the NumPy model of csrc/imu_cov.hip — gives the
covariances of the oracle's own frame behind every sample (tests/imu_cov_cases.py), exactly symmetric.  No compute is launched here.

The bar is the project's for this quantity, max|got - want| <= 1e-11 max|want| per record.  Measured floor of the model against the oracle (two
double-precision evaluations in different operation orders): 1.3e-15 at m = 129 and 1.7e-15 at m = 193 over the three start states."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import imu_cov_cases as KC
import imu_pose_cases as K
import oracle as O

abi = O.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rvio_hip_predict_cov", "rvio_hip_predict_cov_dev", "rvio_hip_set_imu_odometry_cov", "rvio_hip_get_imu_odometry_cov")
FIELDS = ("seq", "img_count", "index", "pose_cov", "vel_cov")


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
    version_line = [l for l in hdr.splitlines() if l.startswith("#define RVIO_HIP_ABI_VERSION 6")][0]
    assert all(s in version_line for s in NEW + ("rvio_imu_cov",))
    # the prototypes, argument for argument
    flat = re.sub(r"\s+", " ", hdr)
    for proto in ("int rvio_hip_predict_cov(rvio_hip* h, int instance, const rvio_imu* imu, int m, rvio_imu_pose* out, rvio_imu_cov* cov);",
                  "int rvio_hip_predict_cov_dev(rvio_hip* h, const rvio_imu* d_imu, int imu_stride, int m, rvio_imu_pose* d_out, int out_stride, rvio_imu_cov* d_cov, int cov_stride);",
                  "int rvio_hip_set_imu_odometry_cov(rvio_hip* h, int enable);",
                  "int rvio_hip_get_imu_odometry_cov(rvio_hip* h, int instance, int64_t first_seq, int max_n, rvio_imu_cov* out, int32_t* n);"):
        assert proto in flat, proto
    # the definition stands in the header
    for phrase in ("IN FRONT of step s", "Vk_j[0..5]", "pjG = Rk_j (pG - pk_j)", "sym(P11_j)[15..17][15..17]", "14 = the IMU-covariance kernel"):
        assert phrase in hdr, phrase


def test_record_layout_matches_a_cxx_compiler(tmp_path):
    assert C.sizeof(abi.ImuCov) == 376 and abi.IMU_COV_DTYPE.itemsize == 376
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "rvio_hip.h"\nint main() {\n  std::printf("%zu", sizeof(rvio_imu_cov));\n'
                   + "".join('  std::printf(" %%zu", offsetof(rvio_imu_cov, %s));\n' % f for f in FIELDS) + '  std::printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == 376
    assert got[1:] == [getattr(abi.ImuCov, f).offset for f in FIELDS]
    assert got[1:] == [abi.IMU_COV_DTYPE.fields[f][1] for f in FIELDS]
    assert got[1:] == [0, 8, 12, 16, 304]                    # no padding: 8 + 4 + 4 + 8 * (36 + 9) = 376
    # the head is the paired pose record's
    assert [abi.IMU_POSE_DTYPE.fields[f][1] for f in FIELDS[:3]] == got[1:4]


def test_null_handle_is_invalid(lib):
    n = C.c_int32(0)
    rec, cov, imu = abi.ImuPose(), abi.ImuCov(), abi.rvio_imu()
    assert lib.rvio_hip_predict_cov(None, 0, C.byref(imu), 1, C.byref(rec), C.byref(cov)) == -1
    assert lib.rvio_hip_predict_cov_dev(None, C.byref(imu), 0, 1, C.byref(rec), 1, C.byref(cov), 1) == -1
    assert lib.rvio_hip_set_imu_odometry_cov(None, 1) == -1
    assert lib.rvio_hip_get_imu_odometry_cov(None, 0, C.c_int64(1), 1, C.byref(cov), C.byref(n)) == -1


# ---------------------------------------------------------------- the 6 x 12 map behind pose_cov
def inject(q, p, dth, dp):
    """the reference's injection (Updater.cc:549-566): dq = [dth / 2; sqrt(1 - |dth|^2 / 4)], q <- dq (x) q, p <- p + dp"""
    dq = np.concatenate([0.5 * dth, [np.sqrt(1.0 - 0.25 * float(dth @ dth))]])
    return O.quat_mul(dq, q), p + dp


def published(qG, pG, qk, pk):
    """composition (System.cc:339-340) and what the pose line carries of it: pGk = -R(qkG)^T pkG and the attitude R_wb = R(qkG)^T"""
    qkG = O.quat_mul(qk, qG)
    pkG = O.quat_to_rot(qk) @ (pG - pk)
    R = O.quat_to_rot(qkG)
    return -R.T @ pkG, R.T


def numeric_jacobian(qG, pG, qk, pk, step=1e-6):
    p0, Rwb0 = published(qG, pG, qk, pk)
    J = np.zeros((6, 12))
    for k in range(12):
        d = np.zeros(12)
        d[k] = step
        col = []
        for s in (+1.0, -1.0):
            qGs, pGs = inject(qG, pG, s * d[0:3], s * d[3:6])
            qks, pks = inject(qk, pk, s * d[6:9], s * d[9:12])
            p, Rwb = published(qGs, pGs, qks, pks)
            E = Rwb @ Rwb0.T                                    # ~ I + [phi x]
            phi = 0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
            col.append(np.concatenate([p - p0, phi]))
        J[:, k] = (col[0] - col[1]) / (2 * step)
    return J


def test_pose_cov_jacobian_against_central_differences_of_the_injection():
    rng = np.random.default_rng(17)
    worst = 0.0

    def unit_q():
        q = rng.standard_normal(4)
        q /= np.linalg.norm(q)
        return -q if q[3] < 0 else q
    for t in range(20):
        qG, qk = unit_q(), unit_q()
        pG, pk = rng.standard_normal(3), rng.standard_normal(3)
        pG *= (0.5 * (t + 1)) / np.linalg.norm(pG)              # |pG| = 0.5, 1, ..., 10
        pk *= 0.05 * (t + 1) / np.linalg.norm(pk)
        scale = max(1.0, np.linalg.norm(pG) + np.linalg.norm(pk))
        M, Mn = abi.imu_pose_cov_jacobian(qG, pG, qk, pk), numeric_jacobian(qG, pG, qk, pk)
        err = float(np.max(np.abs(M - Mn)))
        worst = max(worst, err / scale)
        assert M.shape == (6, 12) and err <= 1e-7 * scale, (t, err)
    # at the composed state (qk = identity, pk = 0) the map is the odometry record's J on the first six columns
    M = abi.imu_pose_cov_jacobian(qG, pG, [0, 0, 0, 1], [0, 0, 0])
    assert np.max(np.abs(M[:, :6] - abi.odom_pose_jacobian(qG, pG))) <= 1e-15 * scale
    print("imu_pose_cov_jacobian vs central differences: worst |dM| / max(1, |pG| + |pk|) = %.2e" % worst)


# ---------------------------------------------------------------- the NumPy model against the oracle's own frame behind every sample
CASES = [(s, m, sp) for s in K.STATES for m in KC.MS_CPU for sp in ((False, True) if m >= 2 else (False,))]


@pytest.mark.parametrize("state,m,special", CASES)
def test_model_against_oracle_prefix_propagation(state, m, special):
    cfg = K.config()
    x, P, imu, truth = KC.case(state, m, 0, special)
    rec = abi.imu_cov_model(cfg, x, P[:24, :24], imu)
    assert len(rec) == m and np.array_equal(rec["index"], np.arange(m)) and not rec["seq"].any() and not rec["img_count"].any()
    assert KC.exactly_symmetric(rec)
    assert np.all(np.linalg.eigvalsh(rec["pose_cov"]) > 0) and np.all(np.linalg.eigvalsh(rec["vel_cov"]) >= 0)
    worst = KC.rel_delta(rec, truth)
    print("%s m = %d special = %d: worst max|d| / max|want| vs the oracle = %.3e" % (state, m, special, worst))
    assert worst <= KC.REL_TOL
    if special:
        assert imu["dt"][m - 2] == 0.0
        if m > 2:
            # dt = 0: Phi = I, Q = 0 and the pose does not move — record m - 2 is record m - 3 up to rounding
            for f in ("pose_cov", "vel_cov"):
                assert np.max(np.abs(rec[f][m - 2] - rec[f][m - 3])) <= 1e-14 * np.max(np.abs(rec[f][m - 3])), f
            assert not np.array_equal(rec["pose_cov"][m - 1], rec["pose_cov"][m - 2])
    if state == "moved":
        # the start state's own qk / pk (a rotation of 0.5 degrees, 5 cm) matter to F, Vk and J: five orders of magnitude above the bar
        x0 = x.copy()
        x0[10:17] = [0, 0, 0, 1, 0, 0, 0]
        assert np.max(np.abs(abi.imu_cov_model(cfg, x0, P[:24, :24], imu)["pose_cov"] - rec["pose_cov"])) > 1e-6 * np.max(np.abs(rec["pose_cov"]))


@pytest.mark.parametrize("m", [129, 193])
def test_floor_of_the_model_against_the_oracle_at_long_batches(m):
    """what the device can be expected to reach: two double-precision evaluations in different operation orders.  Under 2.5e-12, so the device
    tests keep the project's 1e-11"""
    cfg = K.config()
    worst = 0.0
    for state in K.STATES:
        x, P, imu, truth = KC.case(state, m)
        worst = max(worst, KC.rel_delta(abi.imu_cov_model(cfg, x, P[:24, :24], imu), truth))
    print("m = %d: floor of imu_cov_model against the oracle = %.3e" % (m, worst))
    assert worst <= 2.5e-12


def test_the_covariance_does_not_depend_on_the_clones():
    """the oracle on the whole state (10 clones) gives the head the 24 x 24 truth has"""
    cfg = K.config()
    x, P, imu, truth = KC.case("window10", 10)
    xj, Pj = O.propagate(cfg, x, P, imu)
    xc, Pc = O.augment_compose(cfg, xj, Pj, False)[:2]
    assert np.max(np.abs(abi.odom_pose_cov(xc, Pc) - truth[0][-1])) <= 1e-13 * np.max(np.abs(truth[0][-1]))
    assert np.max(np.abs(Pc[15:18, 15:18] - truth[1][-1])) <= 1e-13 * np.max(np.abs(truth[1][-1]))


def test_host_formatter_appends_the_upper_triangles(tmp_path, lib):
    """host/rvio_host.cpp format_imu_odometry_cov, compiled into a stand-alone program and fed known records: the 11 columns of format_imu_odometry,
    then pose_cov's upper triangle row by row (21) and vel_cov's (6); every column parses back to the record's double bit for bit"""
    rng = np.random.default_rng(12)
    n = 32
    rec, cov = np.zeros(n, abi.IMU_POSE_DTYPE), np.zeros(n, abi.IMU_COV_DTYPE)
    rec["seq"] = cov["seq"] = np.arange(1, n + 1)
    rec["t"] = 1403636579.0 + 0.005 * np.arange(n)
    for f, w in (("p", 3), ("q", 4), ("v", 3)):
        rec[f] = rng.standard_normal((n, w)) * 10.0 ** rng.integers(-12, 6, (n, w))
    cov["pose_cov"] = rng.standard_normal((n, 6, 6)) * 10.0 ** rng.integers(-12, 3, (n, 6, 6))
    cov["vel_cov"] = rng.standard_normal((n, 3, 3)) * 10.0 ** rng.integers(-12, 3, (n, 3, 3))
    cov["pose_cov"][0] = np.arange(36).reshape(6, 6)           # a column marker per entry
    cov["vel_cov"][0] = 100 + np.arange(9).reshape(3, 3)
    cov["pose_cov"][1][0, :3] = [0.0, -0.0, 5e-324]
    (tmp_path / "poses.bin").write_bytes(rec.tobytes())
    (tmp_path / "covs.bin").write_bytes(cov.tobytes())
    exe = tmp_path / "format_imu_odometry_cov"
    host, libdir = os.path.join(ROOT, "host"), os.path.join(ROOT, "r-vio_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", host, os.path.join(ROOT, "tests", "hostemu", "format_imu_odometry_cov_main.cpp"),
                           os.path.join(host, "rvio_host.cpp"), "-o", str(exe), "-L", libdir, "-lrvio_hip", "-lz", "-ldl",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    lines = subprocess.check_output([str(exe), str(tmp_path / "poses.bin"), str(tmp_path / "covs.bin")], text=True).splitlines()
    assert len(lines) == n
    got = np.array([[float(v) for v in l.split(" ")] for l in lines])
    assert got.shape == (n, 11 + 21 + 6)
    iu6, iu3 = np.triu_indices(6), np.triu_indices(3)
    want = np.concatenate([rec["t"][:, None], rec["p"], rec["q"], rec["v"], cov["pose_cov"][:, iu6[0], iu6[1]], cov["vel_cov"][:, iu3[0], iu3[1]]], axis=1)
    assert got.tobytes() == want.tobytes()
    assert lines[0].split(" ")[11:] == [str(6 * i + j) for i in range(6) for j in range(i, 6)] + [str(100 + 3 * i + j) for i in range(3) for j in range(i, 3)]


def test_replay_usage_lists_the_flag():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host")], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(ROOT, "host", "rvio_replay")], capture_output=True, text=True)
    assert r.returncode == 2 and "--imu-odometry-cov" in r.stderr, r.stderr
