"""CPU: the optional settings keys Meas.Iterations / Meas.Tolerance as host/rvio_host.cpp parse_settings reads them, through rvio_replay
--check-settings: absent keys give the single update (1, 0) and are not reported as missing, each key overrides its member alone — and the
parsing of rvio_replay --meas-iters / --meas-tol, which refuses what the library would refuse before anything is opened."""
import json
import subprocess

import pytest

from test_host import EUROC_YAML, ensure_bin


def check(tmp_path, text):
    p = tmp_path / "s.yaml"
    p.write_text(text)
    r = subprocess.run([ensure_bin(), "--check-settings", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout), r.stderr


def test_meas_keys_are_optional_and_override_one_member_each(tmp_path):
    got, err = check(tmp_path, EUROC_YAML)
    assert got["meas"] == {"iterations": 1, "tolerance": 0.0} and "Meas." not in err
    got, err = check(tmp_path, EUROC_YAML + "\nMeas.Iterations: 4\n")
    assert got["meas"] == {"iterations": 4, "tolerance": 0.0} and "Meas." not in err
    got, err = check(tmp_path, EUROC_YAML + "\nMeas.Tolerance: 1e-6\n")
    assert got["meas"] == {"iterations": 1, "tolerance": 1e-6}
    got, err = check(tmp_path, EUROC_YAML + "\nMeas.Iterations: 8\nMeas.Tolerance: 0.001\n")
    assert got["meas"] == {"iterations": 8, "tolerance": 0.001}


@pytest.mark.parametrize("args,word", [(["--meas-iters", "0"], "--meas-iters takes an integer in 1 .. 8"), (["--meas-iters", "9"], "--meas-iters takes"),
                                       (["--meas-iters", "two"], "--meas-iters takes"), (["--meas-tol", "-1e-9"], "--meas-tol takes a finite number >= 0"),
                                       (["--meas-tol", "nan"], "--meas-tol takes"), (["--meas-tol", "x"], "--meas-tol takes")])
def test_the_command_line_refuses_what_the_library_would(tmp_path, args, word):
    r = subprocess.run([ensure_bin(), str(tmp_path / "none.yaml"), str(tmp_path), str(tmp_path / "out.dat")] + args, capture_output=True, text=True)
    assert r.returncode != 0 and word in r.stderr, r.stderr
