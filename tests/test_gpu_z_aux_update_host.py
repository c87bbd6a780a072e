"""(Collected with the host tests at the end.)  rvio_replay --velocity on the synthetic ASL folder of test_gpu_z_host.py: a CSV of
`t_ns, vx, vy, vz` — the synthetic truth's velocity in the IMU frame at the image stamps — is fused right behind the frame whose stamp is
nearest (System::velocity -> rvio_hip_update_aux, VALUE mode).  The pose file is held, line for line and bit for bit, to a Python handle
walked over the same folder by the same host logic and issued the same update_aux calls; without the flag the pose file is what the parent
wrote (the same walk with no aux call); rows far from every image stamp are counted and the count is printed."""
import subprocess

import numpy as np
import pytest

import aux_update_cases as A
import oracle as O
from test_gpu_z_host import _asl, load_asl
from test_gpu_z_imu_odometry_host import read_pgm
from test_host import ensure_bin

abi, rv = O.abi, O.rv
pytestmark = pytest.mark.gpu
T0_NS = 1403636579_000000000
SIGMA = 0.05


def body_velocity(seq, t, h=1e-4):
    """R_wb^T dp/dt of the synthetic trajectory: the state's v (velocity in the IMU frame)"""
    R, _ = seq.pose(t)
    return R.T @ ((seq.pose(t + h)[1] - seq.pose(t - h)[1]) / (2 * h))


def handle_walk(cfg, root, rows):
    """MonoVIO's host logic (rvio_replay + System::MonoVIO) in Python with a device handle as the engine: rvio_hip_frame per image, the pose
    line read behind it, then — rows: {image time: velocity} — the aux call rvio_replay --velocity issues.  Returns the pose lines."""
    from rvio_amd import hip
    imu, imgs = load_asl(root)
    h = hip.RvioHip(cfg)
    fifo, ii = [], 0
    moving = ready = False
    wm, am, n_imu = np.zeros(3), np.zeros(3), 0
    out, n_img, n_aux = [], 0, 0
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
        p, q = h.pose()
        out.append(np.r_[t_img, p, q])
        if t_img in rows:
            d = 24 + 6 * min(n_img - 1, cfg.max_track_len - 1)
            H, z, sigma = A.zupt(d, rows[t_img], SIGMA)
            h.update_aux(H, z, sigma, abi.RVIO_AUX_VALUE, 0)
            n_aux += 1
    info = h.frame_info()
    h.close()
    assert info["device_error"] == 0, info
    return np.array(out), n_aux


def test_replay_fuses_a_velocity_file(gpu_required, tmp_path):
    yaml, root = _asl(tmp_path, n=34)
    cfg = abi.config_named("A", enable_equalizer=1)          # the stock settings file _asl writes
    seq = rv.synth.SynthSequence(cfg, duration=4.0)
    imu, imgs = load_asl(root)
    frames = list(range(30, 30 + 34))
    # one row per image stamp, 3 ms late (inside half a period of 25 ms); the row of image 30 twice (the later one, which wins, carries the truth);
    # two rows nowhere near an image: one long before the first, one 20 ms behind the last stamp + a period
    rows, lines = {}, ["#t_ns,vx,vy,vz"]
    for i, k in enumerate(frames):
        ns = T0_NS + int(round(seq.frame_time(k) * 1e9))
        v = body_velocity(seq, seq.frame_time(k))
        if i == 30:
            lines.append("%d,%r,%r,%r" % (ns - 2000000, 9.0, 9.0, 9.0))
        lines.append("%d, %r, %r, %r" % (ns + 3000000, float(v[0]), float(v[1]), float(v[2])))
        rows[imgs[i][0]] = v
    lines.append("%d,1.0,1.0,1.0" % (T0_NS - 5_000_000_000))
    lines.append("%d,1.0,1.0,1.0" % (T0_NS + int(round(seq.frame_time(frames[-1]) * 1e9)) + 70_000_000))
    vfile = tmp_path / "velocity.csv"
    vfile.write_text("\n".join(lines) + "\n")
    pa, pb = tmp_path / "poses_plain.dat", tmp_path / "poses_velocity.dat"
    ra = subprocess.run([ensure_bin(), yaml, root, str(pa)], capture_output=True, text=True)
    rb = subprocess.run([ensure_bin(), yaml, root, str(pb), "--velocity", str(vfile), "--velocity-sigma", repr(SIGMA)], capture_output=True, text=True)
    assert ra.returncode == 0 and rb.returncode == 0, (ra.stderr[-2000:], rb.stderr[-2000:])
    assert "velocity" not in ra.stderr
    Pa, Pb = np.loadtxt(str(pa), ndmin=2), np.loadtxt(str(pb), ndmin=2)
    assert Pa.shape == Pb.shape and len(Pa) >= 8
    # with the flag: every line the bits of the handle that was issued the same calls
    want, n_aux = handle_walk(cfg, root, rows)
    assert want.shape == Pb.shape and n_aux == len(Pb)
    bad = np.argwhere(Pb.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), float(np.max(np.abs(Pb - want))))
    assert "velocity: %d rows, %d applied, 2 matched no frame" % (len(frames) + 3, n_aux) in rb.stderr, rb.stderr[-1500:]
    # without it: what the same walk gives with no aux call at all
    plain, n0 = handle_walk(cfg, root, {})
    assert n0 == 0 and np.array_equal(Pa.view(np.uint64), plain.view(np.uint64))
    # the measurements did something (from the second filtered frame on: the first pose line is read in front of the first call), and towards the truth
    assert np.array_equal(Pa[0], Pb[0]) and np.max(np.abs(Pa[2:, 1:4] - Pb[2:, 1:4])) > 1e-6
    # a sigma that is not positive is refused before anything runs
    r = subprocess.run([ensure_bin(), yaml, root, "--velocity", str(vfile), "--velocity-sigma", "0"], capture_output=True, text=True)
    assert r.returncode == 1 and "--velocity-sigma" in r.stderr
