"""(Collected with the host tests at the end.)  rvio_replay --landmarks on the synthetic ASL folder of test_gpu_z_host.py: the pipelined
replay and the --sync-every-frame replay write the same cloud file, its blocks sit on filtered frames, and the clouds are populated once the
window is full.  Line format (System::record_landmarks_to): t frame feat xw yw zw xr yr zr."""
import subprocess

import numpy as np
import pytest

from test_gpu_z_host import _asl
from test_host import ensure_bin

pytestmark = pytest.mark.gpu


def test_replay_writes_the_landmark_cloud(gpu_required, tmp_path):
    yaml, root = _asl(tmp_path)
    files = {}
    for mode, extra in (("piped", []), ("sync", ["--sync-every-frame"])):
        poses, lms = tmp_path / ("poses_%s.dat" % mode), tmp_path / ("landmarks_%s.dat" % mode)
        r = subprocess.run([ensure_bin(), yaml, root, str(poses), "--landmarks", str(lms)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        files[mode] = (np.loadtxt(str(poses), ndmin=2), open(str(lms)).read())
    assert files["piped"][1] == files["sync"][1] and len(files["piped"][1]) > 0
    poses = files["piped"][0]
    L = np.loadtxt(str(tmp_path / "landmarks_piped.dat"), ndmin=2)
    assert L.shape[1] == 9 and np.all(np.isfinite(L))
    assert set(L[:, 0].tolist()) <= set(poses[:, 0].tolist())                 # blocks are stamped with filtered frames' times
    frames = np.unique(L[:, 1]).astype(int)
    counts = np.array([np.sum(L[:, 1] == f) for f in frames])
    assert len(frames) >= 5 and np.all(counts[1:] > 0), counts               # once the window is full every update has points
    for f in frames:                                                          # feature indices ascend inside a block
        feat = L[L[:, 1] == f, 2]
        assert np.all(np.diff(feat) > 0)
