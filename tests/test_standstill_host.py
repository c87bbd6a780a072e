"""CPU: the optional Standstill.* settings keys of the C++ host (host/rvio_host.cpp parse_settings), read back through rvio_replay
--check-settings: absent keys give Enable 0 and the values of rvio_standstill_config_default for the IMU densities of the SAME file, each key
overrides its member alone, and none of them is reported as missing."""
import json
import math
import subprocess

from test_host import EUROC_YAML, ensure_bin

KEYS = {"Standstill.Enable": ("enable", 1), "Standstill.SigmaA": ("sigma_a", 0.07), "Standstill.SigmaW": ("sigma_w", 0.004),
        "Standstill.ImuThr": ("imu_thr", 33.0), "Standstill.DispThrPx": ("disp_thr_px", 0.25), "Standstill.MinPairs": ("min_pairs", 7),
        "Standstill.SigmaV": ("sigma_v", 0.02), "Standstill.SigmaBg": ("sigma_bg", 0.001), "Standstill.BiasRows": ("bias_rows", 1),
        "Standstill.Gate": ("gate", 0)}


def check(tmp_path, text):
    p = tmp_path / "s.yaml"
    p.write_text(text)
    r = subprocess.run([ensure_bin(), "--check-settings", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout), r.stderr


def test_standstill_keys_are_optional_and_override_one_member_each(tmp_path):
    got, err = check(tmp_path, EUROC_YAML)
    assert "Standstill" not in err
    sw = 1.6968e-04 * math.sqrt(200.0)
    want = dict(enable=0, sigma_a=2.0e-3 * math.sqrt(200.0), sigma_w=sw, imu_thr=12.0, disp_thr_px=0.5, min_pairs=20, sigma_v=0.05, sigma_bg=sw,
                bias_rows=0, gate=1)
    assert got["standstill"] == want
    # the defaults follow the densities of the file, not the stock ones
    got2, _ = check(tmp_path, EUROC_YAML.replace("IMU.sigma_a: 2.0000e-3", "IMU.sigma_a: 4.0e-3").replace("IMU.dps: 200", "IMU.dps: 100"))
    assert got2["standstill"]["sigma_a"] == 4.0e-3 * math.sqrt(100.0) and got2["standstill"]["sigma_w"] == 1.6968e-04 * math.sqrt(100.0)
    for key, (member, val) in KEYS.items():
        one, err = check(tmp_path, EUROC_YAML + "%s: %r\n" % (key, val))
        assert one["standstill"] == dict(want, **{member: val}), key
        assert "Standstill" not in err
    every, _ = check(tmp_path, EUROC_YAML + "".join("%s: %r\n" % (k, v) for k, (_, v) in KEYS.items()))
    assert every["standstill"] == {m: v for m, v in KEYS.values()}
    # the rest of the settings is what it was
    assert {k: v for k, v in every.items() if k != "standstill"} == {k: v for k, v in got.items() if k != "standstill"}
