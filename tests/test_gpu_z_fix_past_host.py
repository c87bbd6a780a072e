"""(Collected with the host tests at the end.)  rvio_replay --fix FILE --fix-latency S on the synthetic ASL folder of test_gpu_z_host.py: the fixes
of the file arrive S seconds late — a row becomes available behind the first frame stamped >= t + S — and each is fused AT ITS OWN t against the
pose the clone window still holds for it (System::fix_*_at -> rvio_hip_update_fix_past): a position interpolated between the two frames around t,
a pose at the nearest frame.  The pose file is held, line for line and bit for bit, to a Python handle walked over the same folder by the same host
logic and issued the same calls; without --fix-latency the tool writes what it wrote before the flag existed (tests/test_gpu_z_fix_host.py holds
that form to its own handle walk; here: the bits of a run that fuses the same rows at the frames)."""
import subprocess

import numpy as np
import pytest

import fix_cases as F
from test_gpu_z_host import _asl, load_asl
from test_gpu_z_imu_odometry_host import read_pgm
from test_host import ensure_bin

abi = F.abi
pytestmark = pytest.mark.gpu
SNAP = 1e-6


def resolve(stamps, t, interpolate):
    """host/rvio_host.cpp resolve_fix_age; stamps newest first.  ('now' | 'old' | 'past', age, frac)"""
    if not stamps or not t < stamps[0]:
        return "now", 0, 0.0
    if t < stamps[-1]:
        return "old", 0, 0.0
    a = 0
    while a + 1 < len(stamps) and not stamps[a + 1] < t:
        a += 1
    lam = (stamps[a] - t) / (stamps[a] - stamps[a + 1]) if a + 1 < len(stamps) and stamps[a] > stamps[a + 1] else 0.0
    if interpolate:
        if lam < SNAP:
            lam = 0.0
        elif lam > 1.0 - SNAP:
            a, lam = a + 1, 0.0
        return "past", a, lam
    return "past", (a if lam < 0.5 else a + 1), 0.0


def handle_walk(cfg, root, rows, latency):
    """MonoVIO's host logic (rvio_replay + System::MonoVIO) in Python with a device handle as the engine: rvio_hip_frame per image, then — rows:
    (t, kind, rvio_fix) sorted by t — every fix whose t + latency the frame has reached, fused at its own t, then the pose line.  Returns the
    pose lines and the calls made: (line index, 'now' | 'past' | 'old', age, frac)."""
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
        assert len(stamps) == h.frame_info()["n_clones"] + 1
        while nxt < len(rows) and rows[nxt][0] + latency <= t_img:
            t, kind, fix = rows[nxt]
            where, age, frac = resolve(stamps, t, kind == abi.RVIO_FIX_POSITION)
            if where == "now":
                h.update_fix(kind, fix, 0)
            elif where == "past":
                h.update_fix_past(kind, fix, age, frac, 0)
            calls.append((len(out), where, age, frac))
            nxt += 1
        p, q = h.pose()
        out.append(np.r_[t_img, p, q])
    info = h.frame_info()
    h.close()
    assert info["device_error"] == 0, info
    return np.array(out), calls


def test_replay_fuses_late_fixes_at_their_own_stamps(gpu_required, tmp_path):
    yaml, root = _asl(tmp_path, n=40)
    cfg = abi.config_named("A", enable_equalizer=1)          # the stock settings file _asl writes
    pa, pb, pc = tmp_path / "poses_plain.dat", tmp_path / "poses_late.dat", tmp_path / "poses_frame.dat"
    ra = subprocess.run([ensure_bin(), yaml, root, str(pa)], capture_output=True, text=True)
    assert ra.returncode == 0, ra.stderr[-2000:]
    Pa = np.loadtxt(str(pa), ndmin=2)
    assert len(Pa) >= 16
    dt = float(Pa[5, 0] - Pa[4, 0])
    latency = 2.6 * dt
    # a position 0.4 frames in front of line 4's stamp, a pose 0.3 frames behind line 8's (nearest: line 8), a position with a lever on line 11's
    # stamp — each a little off the plain run's own poses — and a position from before the first filtered frame, which no window ever holds
    rows, lines = [], ["# t kind values sigmas [lever]"]
    f = abi.make_fix(0.6 * Pa[4, 1:4] + 0.4 * Pa[3, 1:4] + np.array([0.01, -0.01, 0.005]), None, 0.002)
    rows.append((float(Pa[4, 0]) - 0.4 * dt, abi.RVIO_FIX_POSITION, f))
    lines.append("%r position %r %r %r 0.002 0.002 0.002" % ((rows[-1][0],) + tuple(f.z[0:3])))
    q = abi.quat_mul(F.rot_quat([0.004, -0.003, 0.002]), Pa[8, 4:8])
    f = abi.make_fix(Pa[8, 1:4] + np.array([-0.01, 0.0, 0.01]), q, 0.01, 0.002)
    rows.append((float(Pa[8, 0]) + 0.3 * dt, abi.RVIO_FIX_POSE, f))
    lines.append("%r, pose, %s, 0.01, 0.01, 0.01, 0.002, 0.002, 0.002" % (rows[-1][0], ", ".join(repr(v) for v in f.z[0:7])))
    f = abi.make_fix(Pa[11, 1:4] + np.array([0.0, 0.02, 0.0]), None, 0.02, 0.0, F.LEVER)
    rows.append((float(Pa[11, 0]), abi.RVIO_FIX_POSITION, f))
    lines.append("%r 0 %r %r %r 0.02 0.02 0.02 %r %r %r" % ((rows[-1][0],) + tuple(f.z[0:3]) + F.LEVER))
    f = abi.make_fix(Pa[0, 1:4], None, 0.02)
    rows.insert(0, (float(Pa[0, 0]) - 5 * dt, abi.RVIO_FIX_POSITION, f))
    lines.insert(1, "%r position %r %r %r 0.02 0.02 0.02" % ((rows[0][0],) + tuple(f.z[0:3])))
    ffile = tmp_path / "fixes.txt"
    ffile.write_text("\n".join(lines) + "\n")
    rb = subprocess.run([ensure_bin(), yaml, root, str(pb), "--fix", str(ffile), "--fix-latency", repr(latency)], capture_output=True, text=True)
    assert rb.returncode == 0, rb.stderr[-2000:]
    assert "fix: 4 rows, 3 fused, 1 older than the window and dropped" in rb.stderr, rb.stderr[-1500:]
    Pb = np.loadtxt(str(pb), ndmin=2)
    assert Pa.shape == Pb.shape
    # every line the bits of the handle that was issued the same calls
    want, calls = handle_walk(cfg, root, rows, latency)
    print("calls (line, where, age, frac):", calls)
    assert [c[1] for c in calls] == ["old", "past", "past", "past"]
    assert calls[1][2] == 3 and abs(calls[1][3] - 0.4) < 1e-6          # line 4 - 0.4 frames, available at line 7: age 3, 0.4 towards age 4
    assert calls[2][2:] == (3, 0.0) and calls[3][2:] == (3, 0.0)      # line 8 + 0.3 -> nearest line 8, available at line 11; line 11 at line 14
    assert want.shape == Pb.shape
    bad = np.argwhere(Pb.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), float(np.max(np.abs(Pb - want))))
    # the plain run's file up to the frame the first fix arrived at, another from there on
    k = calls[1][0]
    assert np.array_equal(Pa[:k].view(np.uint64), Pb[:k].view(np.uint64)) and not np.array_equal(Pa[k], Pb[k])
    # without --fix-latency: the rows fused at the first frame at or past their t, as before the flag existed — a handle issued rvio_hip_update_fix
    rc = subprocess.run([ensure_bin(), yaml, root, str(pc), "--fix", str(ffile)], capture_output=True, text=True)
    assert rc.returncode == 0 and "fix: 4 rows, 4 applied" in rc.stderr and "latency" not in rc.stderr, rc.stderr[-1500:]
    from test_gpu_z_fix_host import handle_walk as walk_at_the_frame
    want_c, n_fix = walk_at_the_frame(cfg, root, rows)
    Pc = np.loadtxt(str(pc), ndmin=2)
    assert n_fix == 4 and np.array_equal(Pc.view(np.uint64), want_c.view(np.uint64))
    assert not np.array_equal(Pc, Pb)
