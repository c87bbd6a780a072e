"""(Collected with the host tests at the end.)  rvio_replay --map FILE --meas-iters 4 on the synthetic ASL folder and the map file of
test_gpu_z_map_host.py (pixel observations of the scene's TRUE landmarks in the filter's world frame, twelve per group, delivered two frames
late), in child processes: the run ends, every map call took its four passes and the record says so, and the end position is finite and no
further from the synthetic truth than the run without --map.  The error is printed beside the one-shot run's; no claim is made that
iteration beats one shot here — this short run's covariance is overconfident (map landmarks)."""
import re
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


def test_replay_iterates_the_map_updates(gpu_required, tmp_path):
    yaml, root = _asl(tmp_path, n=40)
    cfg = abi.config_named("A", enable_equalizer=1)
    seq = rv.synth.SynthSequence(cfg, duration=4.0)
    pa, pb, pc = (tmp_path / nm for nm in ("poses_plain.dat", "poses_map.dat", "poses_iter.dat"))
    ra = subprocess.run([ensure_bin(), yaml, root, str(pa)], capture_output=True, text=True)
    assert ra.returncode == 0, ra.stderr[-2000:]
    Pa = np.loadtxt(str(pa), ndmin=2)
    assert len(Pa) >= 16
    # the filter's world frame from the truth alone, as test_gpu_z_map_host.py forms it
    dt = 1.0 / seq.cam_hz
    R_i, p_i = seq.pose(float(Pa[0, 0]) - T0 - dt)
    g = R_i.T @ np.array([0.0, 0.0, 1.0])
    xv = np.array([1.0, 0.0, 0.0]) - g * g[0]
    xv /= np.linalg.norm(xv)
    R_wG = R_i @ np.stack([xv, np.cross(g, xv), g], 1)

    def to_G(p):
        return R_wG.T @ (np.asarray(p, float) - p_i)
    lines, groups = ["# t x y z u v sigma"], 0
    for i in range(4, len(Pa) - 2, 2):
        k = int(round((float(Pa[i, 0]) - T0) * seq.cam_hz))
        xy, vis = seq.project(k, noise=True)
        ids = np.flatnonzero(vis)
        np.random.default_rng(900 + k).shuffle(ids)
        assert len(ids) >= PER_GROUP
        for j in ids[:PER_GROUP]:
            f = to_G(seq.landmarks[j])
            lines.append("%r %r %r %r %r %r 1.5" % (float(Pa[i, 0]), float(f[0]), float(f[1]), float(f[2]), float(xy[j, 0]), float(xy[j, 1])))
        groups += 1
    mfile = tmp_path / "map.txt"
    mfile.write_text("\n".join(lines) + "\n")
    common = [ensure_bin(), yaml, root]
    tail = ["--map", str(mfile), "--map-units", "px", "--map-latency", repr(1.98 * dt)]
    rb = subprocess.run(common + [str(pb)] + tail, capture_output=True, text=True)
    rc = subprocess.run(common + [str(pc)] + tail + ["--meas-iters", "4"], capture_output=True, text=True)
    assert rb.returncode == 0 and rc.returncode == 0, (rb.stderr[-1500:], rc.stderr[-1500:])
    print(rc.stderr[-700:])
    assert "meas-iters" not in rb.stderr and "DEVICE-SIDE FLAGS" not in rc.stderr
    assert "map: %d rows, %d groups, %d applied, 0 outside the window and skipped" % (groups * PER_GROUP, groups, groups) in rc.stderr, rc.stderr[-1500:]
    m = re.search(r"meas-iters: at most 4 passes, tolerance 0; the last measurement took (\d+), last step (\S+), converged (\d), gamma of pass 0 (\S+)", rc.stderr)
    assert m, rc.stderr[-1500:]
    passes, step, conv, gamma0 = int(m.group(1)), float(m.group(2)), int(m.group(3)), float(m.group(4))
    assert passes == 4 and conv == 0 and np.isfinite(step) and step > 0.0 and np.isfinite(gamma0) and gamma0 > 0.0
    Pb, Pc = np.loadtxt(str(pb), ndmin=2), np.loadtxt(str(pc), ndmin=2)
    assert Pa.shape == Pb.shape == Pc.shape and np.all(np.isfinite(Pc))
    assert np.array_equal(Pb[:6].view(np.uint64), Pc[:6].view(np.uint64)) and not np.array_equal(Pb[6], Pc[6])     # other from the first map call on
    ea, eb, ec = (float(np.linalg.norm(P[-1, 1:4] - to_G(seq.pose(float(P[-1, 0]) - T0)[1]))) for P in (Pa, Pb, Pc))
    print("end position error against the synthetic truth: %.4f m without --map, %.4f m one shot, %.4f m with --meas-iters 4 (%d groups of %d points; last step %.3e)"
          % (ea, eb, ec, groups, PER_GROUP, step))
    assert np.isfinite(ec) and ec < ea
    # a value the library refuses is refused at the command line
    bad = subprocess.run(common + [str(pc)] + tail + ["--meas-iters", "9"], capture_output=True, text=True)
    assert bad.returncode != 0 and "--meas-iters takes an integer in 1 .. 8" in bad.stderr
