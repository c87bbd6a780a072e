"""(Collected with the host tests at the end.)  rvio_replay --odometry on the synthetic ASL folder of test_gpu_z_host.py: a ring of 8 records
over 40 images is read several times and wraps, and still every filtered frame has its line — seq 1 .. N, the time stamp and pose of the pose
file to the last digit, a symmetric covariance.  Line format (System::record_odometry_to): t seq px py pz qx qy qz qw vx vy vz c00 .. c55."""
import subprocess

import numpy as np
import pytest

from test_gpu_z_host import _asl
from test_host import ensure_bin

pytestmark = pytest.mark.gpu


def test_replay_writes_the_odometry_file(gpu_required, tmp_path):
    yaml, root = _asl(tmp_path, n=40)
    poses, odom = tmp_path / "poses.dat", tmp_path / "odometry.dat"
    r = subprocess.run([ensure_bin(), yaml, root, str(poses), "--max-frames", "40"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([ensure_bin(), yaml, root, "--max-frames", "40", "--odometry", str(odom), "--odometry-ring", "8"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    P, D = np.loadtxt(str(poses), ndmin=2), np.loadtxt(str(odom), ndmin=2)
    assert D.shape == (len(P), 2 + 3 + 4 + 3 + 36) and len(P) > 16 and np.all(np.isfinite(D))      # more than two rings of 8: a read every 4 frames, the ring wraps twice
    assert np.array_equal(D[:, 1], np.arange(1, len(P) + 1))
    assert np.array_equal(D[:, 0], P[:, 0]) and np.array_equal(D[:, 2:9], P[:, 1:8])
    cov = D[:, 12:].reshape(-1, 6, 6)
    assert np.array_equal(cov, cov.transpose(0, 2, 1)) and np.all(np.einsum("kii->ki", cov) > 0)
