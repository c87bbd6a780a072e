"""(Collected with the host tests at the end.)  rvio_replay --imu-odometry FILE --imu-odometry-cov on the synthetic ASL folder of
test_gpu_z_host.py: one line per IMU sample the filter consumed after initialisation, the 11 columns of --imu-odometry followed by the 21
upper-triangle entries of the sample's pose covariance and the 6 of its velocity covariance (System::record_imu_odometry_to(with_cov)).
EVERY appended column is held bit for bit to the covariance ring of a Python handle walked over the same folder by the same host logic
(handle_walk of test_gpu_z_imu_odometry_host.py), on the pipelined replay (default ring, one read at the end) and on the recording replay (a
ring of 32 samples that wraps several times, read every 16).  Without the flag the file is what it was: the same bytes as the first 11 columns
of the file with it.  (tests/test_imu_cov_abi.py holds the line formatter itself to known records.)"""
import subprocess

import numpy as np
import pytest

import oracle as O
from test_gpu_z_host import _asl, load_asl
from test_gpu_z_imu_odometry_host import columns, handle_walk
from test_host import ensure_bin

abi = O.abi
pytestmark = pytest.mark.gpu


def walk_with_cov(cfg, root, staged, monkeypatch):
    """handle_walk with the covariance ring switched on beside its IMU-rate ring: (pose records, covariance records).  handle_walk closes its
    handle, so the covariance ring is read where it reads the pose ring."""
    from rvio_amd import hip
    covs = []
    set0, get0 = hip.RvioHip.set_imu_odometry, hip.RvioHip.get_imu_odometry

    def set1(self, capacity):
        set0(self, capacity)
        self.set_imu_odometry_cov(1)

    def get1(self, *a, **kw):
        covs.append(self.get_imu_odometry_cov(*a, **kw))
        return get0(self, *a, **kw)
    with monkeypatch.context() as mp:
        mp.setattr(hip.RvioHip, "set_imu_odometry", set1)
        mp.setattr(hip.RvioHip, "get_imu_odometry", get1)
        _, rec = handle_walk(cfg, root, staged)
    assert len(covs) == 1
    return rec, covs[0]


def test_replay_appends_the_covariance_columns(gpu_required, tmp_path, monkeypatch):
    yaml, root = _asl(tmp_path, n=34)
    cfg = abi.config_named("A", enable_equalizer=1)          # the stock settings file _asl writes
    rec_dir = tmp_path / "rec"
    rec_dir.mkdir()
    plain, with_cov, with_cov_rec = tmp_path / "imu.dat", tmp_path / "imu_cov.dat", tmp_path / "imu_cov_rec.dat"
    runs = ([ensure_bin(), yaml, root, str(tmp_path / "poses_a.dat"), "--imu-odometry", str(plain)],
            [ensure_bin(), yaml, root, str(tmp_path / "poses_b.dat"), "--imu-odometry", str(with_cov), "--imu-odometry-cov"],
            [ensure_bin(), yaml, root, "--record", "--record-dir", str(rec_dir), "--imu-odometry", str(with_cov_rec), "--imu-odometry-ring", "32", "--imu-odometry-cov"])
    for cmd in runs:
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    # one line per IMU sample consumed after initialisation (the count test_gpu_z_imu_odometry_host.py derives from the folder)
    P = np.loadtxt(str(rec_dir / "stamped_pose_ests.dat"), ndmin=2)
    imu, imgs = load_asl(root)
    t_img = [t for t, _ in imgs]
    k0 = t_img.index(P[0, 0])
    t_lo = t_img[k0 - 1] if k0 else -1.0
    want_t = np.array([s[0] for s in imu if t_lo < s[0] <= P[-1, 0]])
    lines_plain, lines_cov = plain.read_text().splitlines(), with_cov.read_text().splitlines()
    assert len(lines_plain) == len(lines_cov) == len(want_t) > 3 * 32
    # without the flag: 11 columns, the very text the flagged file starts each line with; the pose file does not know about the flag
    assert all(len(l.split(" ")) == 11 for l in lines_plain)
    assert all(c.startswith(p + " ") and len(c.split(" ")) == 38 for p, c in zip(lines_plain, lines_cov))
    assert (tmp_path / "poses_a.dat").read_bytes() == (tmp_path / "poses_b.dat").read_bytes()
    iu6, iu3 = np.triu_indices(6), np.triu_indices(3)
    for staged, path, what in ((False, with_cov, "pipelined replay, default ring"), (True, with_cov_rec, "recording replay, ring 32")):
        got = np.loadtxt(str(path), ndmin=2)
        rec, cov = walk_with_cov(cfg, root, staged, monkeypatch)
        assert len(cov) == len(rec) == len(want_t) and np.array_equal(cov["seq"], rec["seq"]) and np.array_equal(cov["index"], rec["index"]), what
        want = np.concatenate([columns(rec), cov["pose_cov"][:, iu6[0], iu6[1]], cov["vel_cov"][:, iu3[0], iu3[1]]], axis=1)
        assert got.shape == want.shape == (len(want_t), 38), (what, got.shape)
        bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        assert len(bad) == 0, (what, len(bad), bad[:5].tolist())
        assert np.all(cov["pose_cov"][:, np.arange(6), np.arange(6)] > 0), what
