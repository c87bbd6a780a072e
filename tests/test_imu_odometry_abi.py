"""CPU-side checks of IMU-rate odometry (added within ABI 6): rvio_imu_pose has the layout a C++ compiler gives the header's struct, the four
entry points are exported and declared, NULL handles are refused, and abi.imu_pose_model — the NumPy model of csrc/imu_pose.hip — gives the
records of oracle prefix propagation: for every j, x_j = oracle.propagate(cfg, x, P, imu[:j + 1]), q = QuatMul(x_j[10:14], x[0:4]),
p = R(x[0:4])^T (x_j[14:17] - x[4:7]), v = x_j[17:20].  No compute is launched here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import imu_pose_cases as K
import oracle as O

abi = O.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rvio_hip_predict", "rvio_hip_predict_dev", "rvio_hip_set_imu_odometry", "rvio_hip_get_imu_odometry")
FIELDS = ("seq", "img_count", "index", "t", "p", "q", "v")


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
    assert "#define RVIO_HIP_ABI_VERSION 6" in hdr and "IMU-rate odometry" in hdr
    version_line = [l for l in hdr.splitlines() if l.startswith("#define RVIO_HIP_ABI_VERSION")][0]
    assert "within 6" in version_line.lower() and all(s in version_line for s in NEW + ("rvio_imu_pose",))


def test_record_layout_matches_a_cxx_compiler(tmp_path):
    assert C.sizeof(abi.ImuPose) == 104 and abi.IMU_POSE_DTYPE.itemsize == 104
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "rvio_hip.h"\nint main() {\n  std::printf("%zu", sizeof(rvio_imu_pose));\n'
                   + "".join('  std::printf(" %%zu", offsetof(rvio_imu_pose, %s));\n' % f for f in FIELDS) + '  std::printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == 104
    assert got[1:] == [getattr(abi.ImuPose, f).offset for f in FIELDS]
    assert got[1:] == [abi.IMU_POSE_DTYPE.fields[f][1] for f in FIELDS]
    assert got[1:] == [0, 8, 12, 16, 24, 48, 80]          # no padding: 8 + 4 + 4 + 8 + 8 * (3 + 4 + 3) = 104


def test_null_handle_is_invalid(lib):
    n = C.c_int32(0)
    rec, imu = abi.ImuPose(), abi.rvio_imu()
    assert lib.rvio_hip_predict(None, 0, C.byref(imu), 1, C.byref(rec)) == -1
    assert lib.rvio_hip_predict_dev(None, C.byref(imu), 0, 1, C.byref(rec), 1) == -1
    assert lib.rvio_hip_set_imu_odometry(None, 16) == -1
    assert lib.rvio_hip_get_imu_odometry(None, 0, C.c_int64(1), 1, C.byref(rec), C.byref(n)) == -1


# ---------------------------------------------------------------- the NumPy model against oracle prefix propagation
# Quaternions are compared directly, not up to sign: the oracle's QuatMul, like the reference's, returns a unit quaternion with w >= 0, and so does
# the model; no case here has w near 0.
CASES = [(s, m, sd, sp) for s, sd in (("empty", 0), ("moved", 1)) for m in K.MS_CPU for sp in ((False, True) if m >= 2 else (False,))]


@pytest.mark.parametrize("state,m,seed,special", CASES)
def test_model_against_oracle_prefix_propagation(state, m, seed, special):
    cfg = K.config()
    x, P, imu, truth = K.case(state, m, seed, special)
    rec = abi.imu_pose_model(cfg, x, imu)
    assert len(rec) == m and np.array_equal(rec["index"], np.arange(m)) and np.array_equal(rec["t"], imu["t"]) and not rec["seq"].any()
    assert np.all(truth[1][:, 3] > 0.1)
    if special:
        # both special samples are really in the batch and really take their branch
        assert imu["dt"][m - 2] == 0.0 and np.linalg.norm(imu["w"][m - 1] - x[20:23]) < cfg.small_angle
        if m > 2:
            assert np.array_equal(rec["p"][m - 2], rec["p"][m - 3]) and np.array_equal(rec["v"][m - 2], rec["v"][m - 3])   # dt = 0: nothing moves
    worst = K.worst_delta(rec, truth)
    print("%s m = %d special = %d: worst |d| vs oracle prefix propagation = %.3e" % (state, m, special, worst))
    assert worst <= K.X_TOL
    if state == "moved":
        # the start state's own qk / pk matter: the same batch from the composed state (qk = identity, pk = 0) gives other records
        x0 = x.copy()
        x0[10:17] = [0, 0, 0, 1, 0, 0, 0]
        assert np.max(np.abs(abi.imu_pose_model(cfg, x0, imu)["q"] - rec["q"])) > 1e-6


def test_model_is_the_last_state_of_a_whole_propagate():
    """record m - 1 holds what PreIntegrator::propagate leaves in xk1k, composed by System.cc:339-341"""
    cfg = K.config()
    x, P, imu, _ = K.case("moved", 10, 1)
    x1 = O.propagate(cfg, x, P, imu)[0]
    x3, _, pp, pq = O.augment_compose(cfg, x1, O.propagate(cfg, x, P, imu)[1], False)
    rec = abi.imu_pose_model(cfg, x, imu)[-1]
    assert np.max(np.abs(rec["p"] - pp)) <= K.X_TOL and np.max(np.abs(rec["q"] - pq)) <= K.X_TOL and np.max(np.abs(rec["v"] - x1[17:20])) <= K.X_TOL


def test_host_formatter_round_trips_every_column(tmp_path, lib):
    """host/rvio_host.cpp format_imu_odometry, compiled into a stand-alone program and fed known records: each line is
    `t px py pz qx qy qz qw vx vy vz`, and its 19 digits parse back to the record's doubles bit for bit — every column, in this order"""
    rng = np.random.default_rng(11)
    n = 64
    rec = np.zeros(n, abi.IMU_POSE_DTYPE)
    rec["seq"], rec["img_count"], rec["index"] = np.arange(1, n + 1), np.arange(n) // 10 + 1, np.arange(n) % 10
    rec["t"] = 1403636579.0 + 0.005 * np.arange(n) + rng.random(n) * 1e-6
    for f, w in (("p", 3), ("q", 4), ("v", 3)):
        rec[f] = rng.standard_normal((n, w)) * 10.0 ** rng.integers(-12, 6, (n, w))
    # values a formatter can get wrong: zero, minus zero, the smallest normal, a denormal, the largest double, 1 +- one ulp, a column marker per field
    rec["p"][0], rec["q"][0], rec["v"][0] = [0.0, -0.0, np.finfo(float).tiny], [5e-324, np.finfo(float).max, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53], [-1.0 / 3.0, 2.0 / 3.0, 1e-300]
    rec["p"][1], rec["q"][1], rec["v"][1] = [1.0, 2.0, 3.0], [4.0, 5.0, 6.0, 7.0], [8.0, 9.0, 10.0]
    raw_file = tmp_path / "records.bin"
    raw_file.write_bytes(rec.tobytes())
    exe = tmp_path / "format_imu_odometry"
    host, libdir = os.path.join(ROOT, "host"), os.path.join(ROOT, "r-vio_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", host, os.path.join(ROOT, "tests", "hostemu", "format_imu_odometry_main.cpp"),
                           os.path.join(host, "rvio_host.cpp"), "-o", str(exe), "-L", libdir, "-lrvio_hip", "-lz", "-ldl",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    lines = subprocess.check_output([str(exe), str(raw_file)], text=True).splitlines()
    assert len(lines) == n
    got = np.array([[float(v) for v in l.split(" ")] for l in lines])             # (single blanks, no leading or trailing one)
    assert got.shape == (n, 11)
    want = np.concatenate([rec["t"][:, None], rec["p"], rec["q"], rec["v"]], axis=1)
    assert got.tobytes() == want.tobytes()                                        # bit for bit, the sign of zero included
    assert lines[1].split(" ")[1:] == ["1", "2", "3", "4", "5", "6", "7", "8", "9", "10"]


def test_replay_usage_lists_imu_odometry():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host")], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(ROOT, "host", "rvio_replay")], capture_output=True, text=True)
    assert r.returncode == 2 and "--imu-odometry FILE" in r.stderr and "--imu-odometry-ring N" in r.stderr, r.stderr
