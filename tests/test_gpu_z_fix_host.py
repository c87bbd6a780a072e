"""(Collected with the host tests at the end.)  rvio_replay --fix on the synthetic ASL folder of test_gpu_z_host.py: a text file of absolute
fixes — positions and one pose, a little off the poses the plain replay wrote — each fused behind the first frame whose stamp is >= its t, ahead
of that frame's pose line (System::fix_position / fix_pose -> rvio_hip_update_fix).  The pose file is what the plain replay wrote up to the first
fixed frame and differs from it on every line from there on; with the flag it is held, line for line and bit for bit, to a Python handle walked
over the same folder by the same host logic and issued the same update_fix calls."""
import subprocess

import numpy as np
import pytest

import fix_cases as F
from test_gpu_z_host import _asl, load_asl
from test_gpu_z_imu_odometry_host import read_pgm
from test_host import ensure_bin

abi = F.abi
pytestmark = pytest.mark.gpu


def handle_walk(cfg, root, rows):
    """MonoVIO's host logic (rvio_replay + System::MonoVIO) in Python with a device handle as the engine: rvio_hip_frame per image, then — rows:
    (t, kind, rvio_fix) sorted by t — every fix whose stamp the frame has reached, then the pose line.  Returns the pose lines and the call count."""
    from rvio_amd import hip
    imu, imgs = load_asl(root)
    h = hip.RvioHip(cfg)
    fifo, ii = [], 0
    moving = ready = False
    wm, am, n_imu = np.zeros(3), np.zeros(3), 0
    out, nxt = [], 0
    for t_img, path in imgs:
        while ii < len(imu) and (imu[ii][0] <= t_img or (ii > 0 and imu[ii - 1][0] <= t_img)):
            fifo.append(imu[ii])
            ii += 1
        if not fifo or fifo[-1][0] < t_img:
            continue
        cur = [d for d in fifo if d[0] <= t_img]
        fifo = [d for d in fifo if d[0] > t_img]
        if len(cur) < 2:
            continue
        first = 0
        if not ready:
            if not moving:
                ang, vel, displ = np.zeros(3), np.zeros(3), np.zeros(3)
                for (_, dt, w, a) in cur:
                    a = np.array(a)
                    a = a - cfg.gravity * a / np.linalg.norm(a)
                    ang += dt * np.array(w)
                    vel += dt * a
                    displ += dt * vel + .5 * dt * dt * a
                if np.linalg.norm(ang) > cfg.ini_thr_angle or np.linalg.norm(displ) > cfg.ini_thr_displ:
                    moving = True
            while first < len(cur):
                if not moving:
                    wm += cur[first][2]
                    am += cur[first][3]
                    first += 1
                    n_imu += 1
                else:
                    if n_imu == 0:
                        wm, am, n_imu = np.array(cur[first][2]), np.array(cur[first][3]), 1
                    else:
                        wm, am = wm / n_imu, am / n_imu
                    h.initialize(wm, am, n_imu)
                    ready = True
                    break
            if not ready:
                continue
        arr = np.zeros(len(cur) - first, abi.IMU_DTYPE)
        for i, (t, dt, w, a) in enumerate(cur[first:]):
            arr["w"][i], arr["a"][i], arr["t"][i], arr["dt"][i] = w, a, t, dt
        h.frame(read_pgm(path, cfg.width, cfg.height), arr)
        while nxt < len(rows) and rows[nxt][0] <= t_img:
            h.update_fix(rows[nxt][1], rows[nxt][2], 0)
            nxt += 1
        p, q = h.pose()
        out.append(np.r_[t_img, p, q])
    info = h.frame_info()
    h.close()
    assert info["device_error"] == 0, info
    return np.array(out), nxt


def test_replay_fuses_a_fix_file(gpu_required, tmp_path):
    yaml, root = _asl(tmp_path, n=34)
    cfg = abi.config_named("A", enable_equalizer=1)          # the stock settings file _asl writes
    pa, pb = tmp_path / "poses_plain.dat", tmp_path / "poses_fix.dat"
    ra = subprocess.run([ensure_bin(), yaml, root, str(pa)], capture_output=True, text=True)
    assert ra.returncode == 0, ra.stderr[-2000:]
    assert "fix:" not in ra.stderr
    Pa = np.loadtxt(str(pa), ndmin=2)
    assert len(Pa) >= 14
    # fixes a little off the plain run's own poses: a position 3 ms in front of line 4's stamp (line 4 is the first frame at or past it), a
    # pose exactly on line 8's stamp, a position with a lever 3 ms in front of line 12's
    lever = F.LEVER
    rows, lines = [], ["# t kind values sigmas [lever]"]
    f = abi.make_fix(Pa[4, 1:4] + np.array([0.01, -0.01, 0.005]), None, 0.002)
    rows.append((float(Pa[4, 0]) - 0.003, abi.RVIO_FIX_POSITION, f))
    lines.append("%r position %r %r %r 0.002 0.002 0.002" % ((rows[-1][0],) + tuple(f.z[0:3])))
    q = abi.quat_mul(F.rot_quat([0.004, -0.003, 0.002]), Pa[8, 4:8])
    f = abi.make_fix(Pa[8, 1:4] + np.array([-0.01, 0.0, 0.01]), q, 0.01, 0.002)
    rows.append((float(Pa[8, 0]), abi.RVIO_FIX_POSE, f))
    lines.append("%r, pose, %s, 0.01, 0.01, 0.01, 0.002, 0.002, 0.002" % (rows[-1][0], ", ".join(repr(v) for v in f.z[0:7])))
    f = abi.make_fix(Pa[12, 1:4] + np.array([0.0, 0.02, 0.0]), None, 0.02, 0.0, lever)
    rows.append((float(Pa[12, 0]) - 0.003, abi.RVIO_FIX_POSITION, f))
    lines.append("%r 0 %r %r %r 0.02 0.02 0.02 %r %r %r" % ((rows[-1][0],) + tuple(f.z[0:3]) + lever))
    ffile = tmp_path / "fixes.txt"
    ffile.write_text("\n".join(lines) + "\n")
    rb = subprocess.run([ensure_bin(), yaml, root, str(pb), "--fix", str(ffile)], capture_output=True, text=True)
    assert rb.returncode == 0, rb.stderr[-2000:]
    assert "fix: 3 rows, 3 applied" in rb.stderr, rb.stderr[-1500:]
    Pb = np.loadtxt(str(pb), ndmin=2)
    assert Pa.shape == Pb.shape
    # the same file up to the first fixed frame, another on every line from there on
    assert np.array_equal(Pa[:4].view(np.uint64), Pb[:4].view(np.uint64))
    differs = [not np.array_equal(Pa[i], Pb[i]) for i in range(len(Pa))]
    assert differs[4:] == [True] * (len(Pa) - 4), differs
    # ... towards the fix: the fixed frame's position lies nearer to it than the plain run's 1.5 cm
    da, db = (float(np.linalg.norm(Pp[4, 1:4] - np.array(rows[0][2].z[0:3]))) for Pp in (Pa, Pb))
    print("line 4: |p - fix| %.4g m without, %.4g m with --fix" % (da, db))
    assert db < da
    # every line the bits of the handle that was issued the same calls
    want, n_fix = handle_walk(cfg, root, rows)
    assert want.shape == Pb.shape and n_fix == 3
    bad = np.argwhere(Pb.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), float(np.max(np.abs(Pb - want))))
    # a malformed line is refused before anything runs, by file and line
    ffile.write_text(lines[0] + "\n" + lines[1] + "\n1.0 position 1 2 3 0.1 0.1\n")
    r = subprocess.run([ensure_bin(), yaml, root, "--fix", str(ffile)], capture_output=True, text=True)
    assert r.returncode == 1 and (str(ffile) + ":3: ") in r.stderr
