"""(Collected with the host tests at the end.)  rvio_replay --edges on the synthetic ASL folder of test_gpu_z_host.py: the default — the oldest
clone behind every frame, span 1 — and span 2, a ring of 4 records over 48 images (read several times, wraps): one line per record of the
edge ring, stamped with the two images it connects, and the values of a Python handle issued the same calls through a transcription of the
host loop.
Line format (System::record_edges_to, format_edge): t_new t_old px py pz qx qy qz qw c00 .. c55."""
import subprocess

import numpy as np
import pytest

import oracle as O
from test_gpu_z_host import _asl, load_asl
from test_host import ensure_bin

abi, rv = O.abi, O.rv
pytestmark = pytest.mark.gpu


def hip_replay(cfg, root, age_new, age_old, ring):
    """the host loop of test_gpu_z_host.oracle_replay (InputBuffer.cc:53-81, the start-up gate of System.cc:185-250) with a device handle as
    the engine: (stamps of the filtered frames, the edge records)"""
    from rvio_amd import hip
    imu, imgs = load_asl(root)
    h = hip.RvioHip(cfg)
    h.set_edge_odometry(ring, age_new, age_old)
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
    recs = h.edge_odometry()
    h.close()
    return np.array(stamps), recs


@pytest.mark.parametrize("span", [1, 2])
def test_replay_writes_the_edge_file(gpu_required, tmp_path, span):
    yaml, root = _asl(tmp_path, n=48)
    cfg = abi.config_named("A", enable_equalizer=1)          # the stock settings file = cfg A
    ml = cfg.max_track_len
    poses = tmp_path / "poses.dat"
    r = subprocess.run([ensure_bin(), yaml, root, str(poses), "--max-frames", "48"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    P = np.loadtxt(str(poses), ndmin=2)
    for extra in ([] if span == 1 else ["--edges-span", str(span)],):      # (span 1 is the default)
        out = tmp_path / ("edges%d.dat" % span)
        r = subprocess.run([ensure_bin(), yaml, root, "--max-frames", "48", "--edges", str(out), "--edges-ring", "4"] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        D = np.loadtxt(str(out), ndmin=2)
        a, b = ml - 1 - span, ml - 1
        # n_clones behind frame k (1-based) is min(k - 1, max_track_len - 1): the first record is written behind frame b + 1 and connects the
        # frames 1 and 1 + span
        n_rec = len(P) - b
        assert n_rec > 8 and D.shape == (n_rec, 2 + 3 + 4 + 36) and np.all(np.isfinite(D))            # more than two rings of 4: the ring wraps twice
        assert np.array_equal(D[:, 1], P[:n_rec, 0]) and np.array_equal(D[:, 0], P[span: n_rec + span, 0])   # the stamps of the older and the newer image
        cov = D[:, 9:].reshape(-1, 6, 6)
        assert np.array_equal(cov, cov.transpose(0, 2, 1)) and np.all(np.einsum("kii->ki", cov) > 0)
        assert np.all(np.abs(np.linalg.norm(D[:, 5:9], axis=1) - 1) <= 1e-14) and np.all(D[:, 8] >= 0)
        # a Python handle issued the same calls
        stamps, recs = hip_replay(cfg, root, a, b, 64)
        assert np.array_equal(stamps, P[:, 0]) and len(recs) == n_rec
        assert np.array_equal(recs["seq"], np.arange(1, n_rec + 1)) and np.array_equal(recs["img_count_old"], np.arange(1, n_rec + 1))
        assert np.all(recs["img_count_new"] == recs["img_count_old"] + span) and np.all(recs["age_new"] == a) and np.all(recs["age_old"] == b)
        # ... as bits: %.19g carries a double exactly
        for name, got in (("p", D[:, 2:5]), ("q", D[:, 5:9]), ("cov", cov)):
            want = np.ascontiguousarray(recs[name])
            assert np.array_equal(np.ascontiguousarray(got).view(np.uint64), want.view(np.uint64)), (span, name, float(np.abs(got - want).max()))
