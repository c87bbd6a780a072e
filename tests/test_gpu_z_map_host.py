"""(Collected with the host tests at the end.)  rvio_replay --map FILE on the synthetic ASL folder of test_gpu_z_host.py, in a child process: the
map file holds pixel observations of the synthetic scene's TRUE landmarks, expressed in the filter's world frame through the TRUE pose and the
TRUE gravity direction at the instant of initialisation (the stock settings align that frame with gravity), twelve per group (two calls: 8 + 4), each group stamped with its image and delivered two frames late.  Every group the
window holds is fused at the frame of its stamp; one stamped before the first filtered frame is reported and skipped; and the end position is no
further from the synthetic truth than that of the same run without --map.  The replay runs without --map-gate: the short run starts while the
platform already moves, the filter's velocity starts at zero and its covariance does not admit the drift that follows (tens of centimetres
against millimetres), so the per-point gate would refuse every TRUE match — the case of a relocalisation, which the caller trusts."""
import subprocess

import numpy as np
import pytest

import map_cases as M
from test_gpu_z_host import _asl
from test_host import ensure_bin

abi, rv = M.abi, M.A.rv
pytestmark = pytest.mark.gpu
PER_GROUP = 12
T0 = 1403636579.0            # tests/test_host.py write_asl: the stamp of the sequence's t = 0


def test_replay_fuses_delayed_map_observations_and_ends_nearer_the_truth(gpu_required, tmp_path):
    yaml, root = _asl(tmp_path, n=40)
    cfg = abi.config_named("A", enable_equalizer=1)          # the stock settings file _asl writes
    seq = rv.synth.SynthSequence(cfg, duration=4.0)          # ... and the sequence it renders
    pa, pb = tmp_path / "poses_plain.dat", tmp_path / "poses_map.dat"
    ra = subprocess.run([ensure_bin(), yaml, root, str(pa)], capture_output=True, text=True)
    assert ra.returncode == 0, ra.stderr[-2000:]
    Pa = np.loadtxt(str(pa), ndmin=2)
    assert len(Pa) >= 16
    # the filter's world frame is anchored at the IMU frame of the instant of initialisation — one image period in front of the first filtered
    # frame: System::MonoVIO initialises in front of the first IMU sample of that frame's batch — and, with Initialization.EnableAlignment: 1
    # (the stock settings), turned so that its z axis is the direction of the accelerometer at rest and its x axis the IMU's x axis made
    # horizontal (System.cc:115-170).  Here from the truth alone: the synthetic pose and the synthetic world's up axis
    dt = 1.0 / seq.cam_hz
    R_i, p_i = seq.pose(float(Pa[0, 0]) - T0 - dt)
    g = R_i.T @ np.array([0.0, 0.0, 1.0])
    xv = np.array([1.0, 0.0, 0.0]) - g * g[0]
    xv /= np.linalg.norm(xv)
    R_wG = R_i @ np.stack([xv, np.cross(g, xv), g], 1)          # the axes of the filter's world frame in the synthetic world

    def to_G(p):
        return R_wG.T @ (np.asarray(p, float) - p_i)

    def truth(t):
        return to_G(seq.pose(float(t) - T0)[1])
    lines, groups = ["# t x y z u v sigma"], 0
    for i in range(4, len(Pa) - 2, 2):
        k = int(round((float(Pa[i, 0]) - T0) * seq.cam_hz))
        assert abs(seq.frame_time(k) - (float(Pa[i, 0]) - T0)) < 1e-6
        xy, vis = seq.project(k, noise=True)
        ids = np.flatnonzero(vis)
        np.random.default_rng(900 + k).shuffle(ids)
        assert len(ids) >= PER_GROUP
        for j in ids[:PER_GROUP]:
            f = to_G(seq.landmarks[j])
            lines.append("%r %r %r %r %r %r 1.5" % (float(Pa[i, 0]), float(f[0]), float(f[1]), float(f[2]), float(xy[j, 0]), float(xy[j, 1])))
        groups += 1
    lines.append("%r 1.0 2.0 3.0 100.0 100.0 1.5" % (float(Pa[0, 0]) - 20 * dt))          # from before the first filtered frame: no window ever holds it
    mfile = tmp_path / "map.txt"
    mfile.write_text("\n".join(lines) + "\n")
    rb = subprocess.run([ensure_bin(), yaml, root, str(pb), "--map", str(mfile), "--map-units", "px", "--map-latency", repr(1.98 * dt)], capture_output=True, text=True)
    assert rb.returncode == 0, rb.stderr[-2000:]
    print(rb.stderr[-600:])
    assert "map: %d rows, %d groups, %d applied, 1 outside the window and skipped" % (groups * PER_GROUP + 1, groups + 1, groups) in rb.stderr, rb.stderr[-1500:]
    assert "is older than the clone window: skipped" in rb.stderr and "DEVICE-SIDE FLAGS" not in rb.stderr
    Pb = np.loadtxt(str(pb), ndmin=2)
    assert Pa.shape == Pb.shape
    # the plain run's file up to the frame the first group was delivered behind (two frames behind its stamp), another from there on
    assert np.array_equal(Pa[:6].view(np.uint64), Pb[:6].view(np.uint64)) and not np.array_equal(Pa[6], Pb[6])
    ea, eb = (float(np.linalg.norm(P[-1, 1:4] - truth(P[-1, 0]))) for P in (Pa, Pb))
    print("end position error against the synthetic truth: %.4f m without --map, %.4f m with it (%d groups of %d points)" % (ea, eb, groups, PER_GROUP))
    assert eb <= ea
