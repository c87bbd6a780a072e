"""(Collected with the host tests at the end.)  rvio_replay --landmark-cov on the synthetic ASL folder of test_gpu_z_host.py: one line per cloud
point behind every updating frame, the records of a Python handle issued the same calls through a transcription of the host loop, bit for bit,
and the --landmarks file of the same run unchanged against a run without the new flag.
Line format (System::record_landmark_cov_to): t feat n_obs status p_w[3] cov_w (6 upper) p_r[3] cov_r (6 upper) rho rho_sigma."""
import subprocess

import numpy as np
import pytest

import oracle as O
from test_gpu_z_host import _asl, load_asl
from test_host import ensure_bin

abi, rv = O.abi, O.rv
pytestmark = pytest.mark.gpu
UP = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def hip_replay(cfg, root):
    """the host loop of test_gpu_z_host.oracle_replay (InputBuffer.cc:53-81, the start-up gate of System.cc:185-250) with a device handle as
    the engine, the covariance on: (stamps of the filtered frames, [(stamp, records)] of every frame whose cloud stamp is new)"""
    from rvio_amd import hip
    imu, imgs = load_asl(root)
    h = hip.RvioHip(cfg)
    h.set_landmark_cov(True)
    blocks, last = [], -1
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
        lc = h.landmark_cov()
        if lc["frame"] >= 0 and lc["frame"] != last:
            last = lc["frame"]
            blocks.append((t_img, lc["rec"]))
    h.close()
    return np.array(stamps), blocks


def test_replay_writes_the_landmark_covariance_file(gpu_required, tmp_path):
    yaml, root = _asl(tmp_path, n=40)
    cfg = abi.config_named("A", enable_equalizer=1)          # the stock settings file = cfg A
    poses, lm0, lm1, lcf = tmp_path / "poses.dat", tmp_path / "lm0.dat", tmp_path / "lm1.dat", tmp_path / "lmc.dat"
    r = subprocess.run([ensure_bin(), yaml, root, str(poses), "--max-frames", "40", "--landmarks", str(lm0)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([ensure_bin(), yaml, root, "--max-frames", "40", "--landmarks", str(lm1), "--landmark-cov", str(lcf)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert open(str(lm0)).read() == open(str(lm1)).read() and len(open(str(lm0)).read()) > 0      # the cloud file: unchanged by the new flag
    P, Lm, D = np.loadtxt(str(poses), ndmin=2), np.loadtxt(str(lm1), ndmin=2), np.loadtxt(str(lcf), ndmin=2)
    assert D.shape == (len(Lm), 4 + 3 + 6 + 3 + 6 + 2) and len(D) > 20
    # line by line the cloud's: stamp, feat, p_r
    assert np.array_equal(D[:, 0], Lm[:, 0]) and np.array_equal(D[:, 1], Lm[:, 2]) and np.array_equal(D[:, 13:16], Lm[:, 6:9])
    ok = D[:, 3] == 0
    assert ok.sum() > 20 and np.all(np.isfinite(D[ok])) and np.all(D[ok][:, [7, 10, 12, 16, 19, 21, 23]] > 0)
    # a Python handle issued the same calls: the same records, as bits (%.19g carries a double exactly)
    stamps, blocks = hip_replay(cfg, root)
    assert np.array_equal(stamps, P[:, 0])
    rec = np.concatenate([b[1] for b in blocks])
    t = np.concatenate([np.full(len(b[1]), b[0]) for b in blocks])
    assert len(rec) == len(D) and np.array_equal(t, D[:, 0])
    assert np.array_equal(rec["feat"], D[:, 1].astype(np.int32)) and np.array_equal(rec["n_obs"], D[:, 2].astype(np.int32)) and np.array_equal(rec["status"], D[:, 3].astype(np.int32))
    want = np.column_stack([rec["p_w"]] + [rec["cov_w"][:, a, b] for a, b in UP] + [rec["p_r"]] + [rec["cov_r"][:, a, b] for a, b in UP] + [rec["rho"], rec["rho_sigma"]])
    got = np.ascontiguousarray(D[:, 4:])
    assert np.array_equal(got.view(np.uint64)[ok], np.ascontiguousarray(want).view(np.uint64)[ok]), float(np.nanmax(np.abs(got - want)))
    assert np.array_equal(np.isnan(got), np.isnan(want))
