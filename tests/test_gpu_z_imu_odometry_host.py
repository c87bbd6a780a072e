"""(Collected with the host tests at the end.)  rvio_replay --imu-odometry on the synthetic ASL folder of test_gpu_z_host.py: one line per IMU
sample the filter consumed after initialisation — t px py pz qx qy qz qw vx vy vz at 19 digits (System::record_imu_odometry_to).  EVERY line
is held, all 11 columns bit for bit, to the record a Python handle with its ring on gives for the same sample when it is walked over the same
folder by the same host logic (InputBuffer + the start-up gate, as oracle_replay of test_gpu_z_host.py transcribes them): the pipelined
replay (default ring, one read at the end) against rvio_hip_frame, the recording replay (a ring of 32 samples that wraps several times,
read every 16) against the stages one by one.  stamped_pose_ests.dat is the same file, byte for byte, with and without the flag; a ring too
small to be drained in time ends the replay with an error, not with a short file.  (tests/test_imu_odometry_abi.py holds the line
formatter itself to known records.)"""
import subprocess

import numpy as np
import pytest

import oracle as O
from test_gpu_z_host import _asl, load_asl
from test_host import ensure_bin

abi = O.abi
pytestmark = pytest.mark.gpu


def read_pgm(path, w, h):
    data = open(path, "rb").read()
    assert data.startswith(b"P5")
    return np.frombuffer(data[-w * h:], np.uint8).reshape(h, w)


def handle_walk(cfg, root, staged):
    """MonoVIO's host logic (rvio_replay + System::MonoVIO) in Python with a device handle as the engine, its IMU-rate ring holding the whole
    run: (image times of the filtered frames, every record).  staged: the stages one by one with the host waiting behind the tracker, as
    INI.RecordOutputs runs them; else rvio_hip_frame, nothing waited for."""
    from rvio_amd import hip
    imu, imgs = load_asl(root)
    h = hip.RvioHip(cfg)
    h.set_imu_odometry(4096)
    fifo, ii = [], 0
    moving = ready = False
    wm, am, n_imu = np.zeros(3), np.zeros(3), 0
    t_frames = []
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
        img = read_pgm(path, cfg.width, cfg.height)
        if staged:
            h.track(img, arr)
            h.sync()
            do_update, do_augment = h.frame_plan()
            h.propagate(arr)
            if do_update:
                h.update_tracked()
            h.augment_compose(do_augment)
        else:
            h.frame(img, arr)
        t_frames.append(t_img)
    rec = h.get_imu_odometry()
    info = h.frame_info()
    h.close()
    assert info["device_error"] == 0 and info["updated"] == 1, info
    return np.array(t_frames), rec


def columns(rec):
    return np.concatenate([rec["t"][:, None], rec["p"], rec["q"], rec["v"]], axis=1)


def test_replay_writes_the_imu_odometry_file(gpu_required, tmp_path):
    yaml, root = _asl(tmp_path, n=34)
    cfg = abi.config_named("A", enable_equalizer=1)          # the stock settings file _asl writes
    rec_a, rec_b = tmp_path / "rec_a", tmp_path / "rec_b"
    rec_a.mkdir()
    rec_b.mkdir()
    dense_b, dense_c, dense_d, poses_c = tmp_path / "imu_b.dat", tmp_path / "imu_c.dat", tmp_path / "imu_d.dat", tmp_path / "poses_c.dat"
    runs = ([ensure_bin(), yaml, root, "--record", "--record-dir", str(rec_a)],
            [ensure_bin(), yaml, root, "--record", "--record-dir", str(rec_b), "--imu-odometry", str(dense_b), "--imu-odometry-ring", "32"],
            [ensure_bin(), yaml, root, str(poses_c), "--imu-odometry", str(dense_c)])
    for cmd in runs:
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    # the pose file does not know about the flag
    pa, pb = (rec_a / "stamped_pose_ests.dat").read_bytes(), (rec_b / "stamped_pose_ests.dat").read_bytes()
    assert len(pa) > 0 and pa == pb
    P = np.loadtxt(str(rec_b / "stamped_pose_ests.dat"), ndmin=2)
    D, Dc = np.loadtxt(str(dense_b), ndmin=2), np.loadtxt(str(dense_c), ndmin=2)
    assert len(P) >= 8 and D.shape[1] == 1 + 3 + 4 + 3 and np.all(np.isfinite(D))
    # one line per IMU sample consumed after initialisation: the samples behind the image in front of the first filtered frame (that frame's
    # batch starts there: the start-up gate consumes whole batches), up to the last filtered frame's image
    imu, imgs = load_asl(root)
    t_img = [t for t, _ in imgs]
    k0 = t_img.index(P[0, 0])
    t_lo = t_img[k0 - 1] if k0 else -1.0
    want_t = np.array([s[0] for s in imu if t_lo < s[0] <= P[-1, 0]])
    assert len(want_t) > 3 * 32                                          # the ring of 32 wrapped several times and was read every 16 samples
    assert len(D) == len(want_t) and np.array_equal(D[:, 0], want_t)
    # every line, every column, against the ring of a Python handle walked over the same folder: 19 digits carry the records' bits
    for staged, got, what in ((True, D, "recording replay, ring 32"), (False, Dc, "pipelined replay, default ring")):
        t_frames, rec = handle_walk(cfg, root, staged)
        assert np.array_equal(t_frames, P[:, 0]), what
        assert [int(s) for s in rec["seq"]] == list(range(1, len(want_t) + 1)), what
        want = columns(rec)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), float(np.max(np.abs(got - want))))
    # ... and the frames without an update (the first four) end on the sample whose record IS the frame's pose line
    for k in range(4):
        j = int(np.searchsorted(D[:, 0], P[k, 0], side="right")) - 1
        assert D[j, 0] <= P[k, 0] < D[j, 0] + 0.0051 and np.array_equal(D[j, 1:8], P[k, 1:8]), k
    Pc = np.loadtxt(str(poses_c), ndmin=2)
    assert Pc.shape == P.shape and np.max(np.abs(Pc - P)) <= 1e-9
    # a ring smaller than one frame's samples cannot be drained in time: the replay says so and fails, it does not write a short file and exit 0
    r = subprocess.run([ensure_bin(), yaml, root, "--imu-odometry", str(dense_d), "--imu-odometry-ring", "8"], capture_output=True, text=True)
    assert r.returncode != 0 and "overwritten before they were read" in r.stderr and "--imu-odometry-ring" in r.stderr, r.stderr[-2000:]
