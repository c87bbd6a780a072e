"""(Collected with the host tests at the end.)  rvio_replay on a synthetic ASL folder whose platform never moves, with Standstill.Enable: 1 in
the settings and --standstill FILE: System::MonoVIO calls rvio_hip_standstill(the frame's IMU samples, apply = 1) behind every rvio_hip_frame,
the record of every frame is kept on the host and written once at the end.  Every line must say `static` and `applied`, the velocity at the end
of the replay must be smaller than without the key, and Standstill.Enable: 0 must leave the pose file what it is without any Standstill.* key.
The thresholds are the test's own (Standstill.ImuThr 40 against T ~ 6-10 at rest; the images are identical, so the disparity is 0), not the
library's defaults; the start-up gate's thresholds are 0 so that a platform that never moves is initialised at its first image."""
import math
import os
import subprocess

import numpy as np
import pytest

import oracle as O
from test_host import EUROC_YAML, ensure_bin, write_pgm

abi, rv = O.abi, O.rv
pytestmark = pytest.mark.gpu
T0_NS = 1403636579_000000000
N_FRAMES = 14


def write_stationary_asl(root, seq, frames):
    """mav0/{cam0,imu0} as tests/test_host.py write_asl lays them out; the platform stands still, so ONE rendered image serves every frame"""
    cam = os.path.join(root, "mav0", "cam0", "data")
    os.makedirs(cam, exist_ok=True)
    os.makedirs(os.path.join(root, "mav0", "imu0"), exist_ok=True)
    img = seq.render(frames[0])
    with open(os.path.join(root, "mav0", "cam0", "data.csv"), "w") as f:
        f.write("#timestamp [ns],filename\n")
        for k in frames:
            ns = T0_NS + int(round(seq.frame_time(k) * 1e9))
            f.write("%d,%d.pgm\n" % (ns, ns))
            write_pgm(os.path.join(cam, "%d.pgm" % ns), img)
    with open(os.path.join(root, "mav0", "imu0", "data.csv"), "w") as f:
        f.write("#timestamp [ns],w_RS_S_x [rad s^-1],w_RS_S_y [rad s^-1],w_RS_S_z [rad s^-1],a_RS_S_x [m s^-2],a_RS_S_y [m s^-2],a_RS_S_z [m s^-2]\n")
        for s in seq.imu_all():
            ns = T0_NS + int(round(float(s["t"]) * 1e9))
            f.write("%d,%s\n" % (ns, ",".join(repr(float(v)) for v in list(s["w"]) + list(s["a"]))))


def settings(extra=""):
    y = EUROC_YAML.replace("INI.nThresholdAngle: 0.005", "INI.nThresholdAngle: 0").replace("INI.nThresholdDispl: 0.01", "INI.nThresholdDispl: 0")
    assert "INI.nThresholdAngle: 0 " in y and "INI.nThresholdDispl: 0\n" in y
    return y + extra


def standstill_keys(enable):
    cfg = abi.config_named("A", enable_equalizer=1)
    sa, sw = cfg.sigma_a * math.sqrt(cfg.imu_rate), cfg.sigma_g * math.sqrt(cfg.imu_rate)
    return ("Standstill.Enable: %d\nStandstill.SigmaA: %r\nStandstill.SigmaW: %r\nStandstill.ImuThr: 40\nStandstill.DispThrPx: 0.5\n"
            "Standstill.MinPairs: 5\nStandstill.SigmaV: 0.05\nStandstill.SigmaBg: %r\nStandstill.BiasRows: 0\nStandstill.Gate: 0\n" % (enable, sa, sw, sw))


def replay(tmp_path, name, yaml_text, root, extra=()):
    y = tmp_path / (name + ".yaml")
    y.write_text(yaml_text)
    poses, odom = tmp_path / (name + "_poses.dat"), tmp_path / (name + "_odom.dat")
    r = subprocess.run([ensure_bin(), str(y), root, str(poses), "--odometry", str(odom)] + list(extra), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "DEVICE-SIDE FLAGS" not in r.stderr, r.stderr[-1000:]
    return poses.read_bytes(), np.loadtxt(str(odom), ndmin=2), r.stderr


def test_replay_detects_standstill_and_fuses_zero_velocity(gpu_required, tmp_path):
    cfg = abi.config_named("A", enable_equalizer=1)          # the stock settings file
    seq = rv.synth.SynthSequence(cfg, duration=4.0, motion="stationary")
    root = str(tmp_path / "asl")
    write_stationary_asl(root, seq, list(range(30, 30 + N_FRAMES)))
    ssfile = tmp_path / "standstill.dat"
    p_none, od_none, _ = replay(tmp_path, "none", settings(), root)
    p_off, od_off, _ = replay(tmp_path, "off", settings(standstill_keys(0)), root)
    p_on, od_on, _ = replay(tmp_path, "on", settings(standstill_keys(1)), root, ["--standstill", str(ssfile)])
    # Enable: 0 is no key at all
    assert p_off == p_none and len(p_none) > 0 and np.array_equal(od_off, od_none)
    # one line per filtered frame: t T disparity n_pairs flags gamma — static and applied throughout
    rows = np.loadtxt(str(ssfile), ndmin=2)
    n = len(p_on.splitlines())
    print(rows)
    assert rows.shape == (n, 6) and n == len(od_on) >= N_FRAMES - 2
    assert np.array_equal(rows[:, 0], od_on[:, 0])
    flags = rows[:, 4].astype(int)
    assert np.all(flags & 4) and np.all(flags & 8), flags
    assert np.all(rows[:, 1] < 40 / 1.5) and np.all(rows[:, 2] < 0.5 / 1.5)
    assert rows[0, 3] == 0 and np.all(rows[2:, 3] >= 5)       # the first frame has no pairs: the image test has no opinion there
    # the velocity at the end of the replay (odometry line: t seq p(3) q(4) v(3) ...): smaller with the updates than without
    v_on, v_none = np.linalg.norm(od_on[-1, 9:12]), np.linalg.norm(od_none[-1, 9:12])
    print("final |v|: %.3e with the standstill update, %.3e without" % (v_on, v_none))
    assert v_on < v_none and p_on != p_none
    # --standstill without the key is refused before anything runs
    y = tmp_path / "none.yaml"
    r = subprocess.run([ensure_bin(), str(y), root, "--standstill", str(tmp_path / "x.dat")], capture_output=True, text=True)
    assert r.returncode == 1 and "Standstill.Enable" in r.stderr
