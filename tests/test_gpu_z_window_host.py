"""(Collected with the host tests at the end.)  rvio_replay --smoothed on the synthetic ASL folder of test_gpu_z_host.py, lag 3, a ring of 8
records over 40 images (read several times, wraps): one line per record of the smoothed ring, seq 1 .. N, stamped with the image the record
describes — the one 3 images before the frame it was written behind —, in the layout of the odometry file (the velocity columns 0), and the
values of a Python handle issued the same calls through a transcription of the host loop.
Line format (System::record_smoothed_to): t seq px py pz qx qy qz qw 0 0 0 c00 .. c55."""
import subprocess

import numpy as np
import pytest

import oracle as O
from test_gpu_z_host import _asl, load_asl
from test_host import ensure_bin

abi, rv = O.abi, O.rv
pytestmark = pytest.mark.gpu
LAG = 3


def hip_replay(cfg, root, lag, ring):
    """the host loop of test_gpu_z_host.oracle_replay (InputBuffer.cc:53-81, the start-up gate of System.cc:185-250) with a device handle as
    the engine: (stamps of the filtered frames, the smoothed records)"""
    from rvio_amd import hip
    imu, imgs = load_asl(root)
    h = hip.RvioHip(cfg)
    h.set_smoothed_odometry(ring, lag)
    fifo, ii = [], 0
    moving = ready = False
    wm, am, n_imu = np.zeros(3), np.zeros(3), 0
    stamps = []
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
        img = np.fromfile(path, np.uint8)[-cfg.width * cfg.height:].reshape(cfg.height, cfg.width)   # binary PGM: the pixels end the file
        h.frame(img, arr)
        stamps.append(t_img)
    recs = h.smoothed_odometry()
    h.close()
    return np.array(stamps), recs


def test_replay_writes_the_smoothed_file(gpu_required, tmp_path):
    yaml, root = _asl(tmp_path, n=40)
    cfg = abi.config_named("A", enable_equalizer=1)          # the stock settings file = cfg A
    poses, smo = tmp_path / "poses.dat", tmp_path / "smoothed.dat"
    r = subprocess.run([ensure_bin(), yaml, root, str(poses), "--max-frames", "40"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([ensure_bin(), yaml, root, "--max-frames", "40", "--smoothed", str(smo), "--smoothed-lag", str(LAG), "--smoothed-ring", "8"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    P, D = np.loadtxt(str(poses), ndmin=2), np.loadtxt(str(smo), ndmin=2)
    # n_clones behind frame k (1-based) is min(k - 1, max_track_len - 1): the first record is written behind frame LAG + 1 and describes frame 1
    n_rec = len(P) - LAG
    assert n_rec > 16 and D.shape == (n_rec, 2 + 3 + 4 + 3 + 36) and np.all(np.isfinite(D))        # more than two rings of 8: the ring wraps twice
    assert np.array_equal(D[:, 1], np.arange(1, n_rec + 1))
    assert np.array_equal(D[:, 0], P[:n_rec, 0])                                                   # the stamps, shifted by LAG images
    assert not D[:, 9:12].any()
    cov = D[:, 12:].reshape(-1, 6, 6)
    assert np.array_equal(cov, cov.transpose(0, 2, 1)) and np.all(np.einsum("kii->ki", cov) > 0)
    # smoothed, not filtered: the same frames as the pose file, close to it and not it
    dp = np.abs(D[:, 2:5] - P[:n_rec, 1:4]).max()
    assert 0 < dp < 0.5, dp
    # a Python handle issued the same calls
    stamps, recs = hip_replay(cfg, root, LAG, 64)
    assert np.array_equal(stamps, P[:, 0]) and len(recs) == n_rec
    assert np.array_equal(recs["seq"], D[:, 1].astype(np.int64)) and np.array_equal(recs["img_count"], np.arange(1, n_rec + 1))
    # ... as bits: %.19g carries a double exactly
    for name, got in (("p", D[:, 2:5]), ("q", D[:, 5:9]), ("pose_cov", cov)):
        want = np.ascontiguousarray(recs[name])
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint64), want.view(np.uint64)), (name, float(np.abs(got - want).max()))
