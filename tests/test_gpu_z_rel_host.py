"""(Collected with the host tests at the end.)  rvio_replay --rel FILE on the synthetic ASL folder of test_gpu_z_host.py: every row of the file — a
delta pose between two instants — is fused behind the first frame stamped >= its t_new, between the two frames of the clone window nearest to
its stamps (System::update_rel_at -> rvio_hip_update_rel); a row whose older stamp the window never held, and one whose stamps fall onto one
frame, are dropped and counted.  The pose file is held, line for line and bit for bit, to a Python handle walked over the same folder by the
same host logic and issued the same calls."""
import subprocess

import numpy as np
import pytest

import rel_cases as R
from test_gpu_z_fix_past_host import resolve
from test_gpu_z_host import _asl, load_asl
from test_gpu_z_imu_odometry_host import read_pgm
from test_host import ensure_bin

abi, F = R.abi, R.F
pytestmark = pytest.mark.gpu


def resolve_span(stamps, t_new, t_old):
    """host/rvio_host.cpp resolve_rel_span; stamps newest first.  (age_new, age_old) or None"""
    if not stamps:
        return None
    a, b = resolve(stamps, t_new, False), resolve(stamps, t_old, False)
    if a[0] == "old" or b[0] == "old":
        return None
    an, ao = (0 if a[0] == "now" else a[1]), (0 if b[0] == "now" else b[1])
    return (an, ao) if an < ao else None


def handle_walk(cfg, root, rows):
    """MonoVIO's host logic (rvio_replay + System::MonoVIO) in Python with a device handle as the engine: rvio_hip_frame per image, then — rows:
    (t_new, t_old, kind, rvio_fix) sorted by t_new — every row whose t_new the frame has reached, then the pose line.  Returns the pose lines
    and the calls made: (line index, span or None)."""
    from rvio_amd import hip
    imu, imgs = load_asl(root)
    h = hip.RvioHip(cfg)
    fifo, ii = [], 0
    moving = ready = False
    wm, am, n_imu = np.zeros(3), np.zeros(3), 0
    out, nxt, calls, stamps, n_img = [], 0, [], [], 0
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
        n_img += 1
        stamps = ([t_img] + stamps)[: min(n_img, cfg.max_track_len)]
        while nxt < len(rows) and rows[nxt][0] <= t_img:
            t_new, t_old, kind, meas = rows[nxt]
            sp = resolve_span(stamps, t_new, t_old)
            if sp is not None:
                h.update_rel(kind, meas, sp[0], sp[1], 0)
            calls.append((len(out), sp))
            nxt += 1
        p, q = h.pose()
        out.append(np.r_[t_img, p, q])
    info = h.frame_info()
    h.close()
    assert info["device_error"] == 0, info
    return np.array(out), calls


def delta(Pa, i_new, i_old):
    """(d, q) between two pose lines: the newer origin in the older IMU frame, the quaternion rotating the older frame into the newer"""
    Rn, Ro = abi.quat_to_rot(Pa[i_new, 4:8]), abi.quat_to_rot(Pa[i_old, 4:8])
    return Ro @ (Pa[i_new, 1:4] - Pa[i_old, 1:4]), abi.rot_to_quat(Rn @ Ro.T)


def test_replay_fuses_relative_poses_between_the_frames_of_their_stamps(gpu_required, tmp_path):
    yaml, root = _asl(tmp_path, n=40)
    cfg = abi.config_named("A", enable_equalizer=1)          # the stock settings file _asl writes
    pa, pb = tmp_path / "poses_plain.dat", tmp_path / "poses_rel.dat"
    ra = subprocess.run([ensure_bin(), yaml, root, str(pa)], capture_output=True, text=True)
    assert ra.returncode == 0, ra.stderr[-2000:]
    Pa = np.loadtxt(str(pa), ndmin=2)
    assert len(Pa) >= 16
    dt = float(Pa[5, 0] - Pa[4, 0])
    rows, lines = [], ["# t_new t_old kind values sigmas [lever]"]
    # a pose between lines 6 and 3, on their stamps, a little off the plain run's own delta
    d, q = delta(Pa, 6, 3)
    f = abi.make_fix(d + np.array([0.01, -0.01, 0.005]), abi.quat_mul(F.rot_quat([0.004, -0.003, 0.002]), q), 0.01, 0.002)
    rows.append((float(Pa[6, 0]), float(Pa[3, 0]), abi.RVIO_REL_POSE, f))
    lines.append("%r, %r, pose, %s, 0.01, 0.01, 0.01, 0.002, 0.002, 0.002" % (rows[-1][0], rows[-1][1], ", ".join(repr(v) for v in f.z[0:7])))
    # a displacement with a lever, 0.3 frames behind line 9 (available at line 10, nearest: line 9) back to 0.2 frames in front of line 7
    d, q = delta(Pa, 9, 7)
    f = abi.make_fix(d + np.array([0.0, 0.01, -0.01]), None, 0.01, 0.0, R.LEVER)
    rows.append((float(Pa[9, 0]) + 0.3 * dt, float(Pa[7, 0]) - 0.2 * dt, abi.RVIO_REL_POSITION, f))
    lines.append("%r %r 16 %r %r %r 0.01 0.01 0.01 %r %r %r" % ((rows[-1][0], rows[-1][1]) + tuple(f.z[0:3]) + R.LEVER))
    # a one-step rotation between lines 11 and 10
    d, q = delta(Pa, 11, 10)
    f = abi.make_fix(None, abi.quat_mul(F.rot_quat([-0.002, 0.003, 0.001]), q), 0.0, 0.002)
    rows.append((float(Pa[11, 0]), float(Pa[10, 0]), abi.RVIO_REL_ATTITUDE, f))
    lines.append("%r %r attitude %s 0.002 0.002 0.002" % (rows[-1][0], rows[-1][1], " ".join(repr(v) for v in f.z[3:7])))
    # an older stamp from before the first filtered frame, which no window ever holds; two stamps that fall onto one frame
    f = abi.make_fix((0.0, 0.0, 0.0), None, 0.02)
    rows.append((float(Pa[12, 0]), float(Pa[0, 0]) - 5 * dt, abi.RVIO_REL_POSITION, f))
    lines.append("%r %r position 0 0 0 0.02 0.02 0.02" % (rows[-1][0], rows[-1][1]))
    rows.append((float(Pa[13, 0]) + 0.1 * dt, float(Pa[13, 0]) - 0.1 * dt, abi.RVIO_REL_POSITION, f))
    lines.append("%r %r position 0 0 0 0.02 0.02 0.02" % (rows[-1][0], rows[-1][1]))
    ffile = tmp_path / "rels.txt"
    ffile.write_text("\n".join(lines) + "\n")
    rb = subprocess.run([ensure_bin(), yaml, root, str(pb), "--rel", str(ffile)], capture_output=True, text=True)
    assert rb.returncode == 0, rb.stderr[-2000:]
    assert "rel: 5 rows, 3 fused, 2 outside the window or on one frame and dropped" in rb.stderr, rb.stderr[-1500:]
    Pb = np.loadtxt(str(pb), ndmin=2)
    assert Pa.shape == Pb.shape
    # every line the bits of the handle that was issued the same calls
    want, calls = handle_walk(cfg, root, rows)
    print("calls (line, span):", calls)
    assert calls == [(6, (0, 3)), (10, (1, 3)), (11, (0, 1)), (12, None), (14, None)]
    assert want.shape == Pb.shape
    bad = np.argwhere(Pb.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), float(np.max(np.abs(Pb - want))))
    # the plain run's file up to the frame the first measurement was fused behind, another from there on
    assert np.array_equal(Pa[:6].view(np.uint64), Pb[:6].view(np.uint64)) and not np.array_equal(Pa[6], Pb[6])
