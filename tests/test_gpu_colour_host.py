"""rvio_replay (host/: System::MonoVIO above the C-ABI) on an EuRoC ASL folder of COLOUR frames: System sets the handle's image format
from the channel count and Camera.RGB and hands the interleaved bytes over (no pixel is converted on the host), so the pose file must be
byte-identical to the one the same binary writes for the folder that holds the NumPy gray of the same frames as PGM — for Camera.RGB: 1
and for Camera.RGB: 0 (the same colour bytes then mean another gray image: each case has its own gray folder)."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
from test_gpu_colour import gray, tint
from test_host import EUROC_YAML, ensure_bin

abi, rv = O.abi, O.rv
pytestmark = pytest.mark.gpu


def write_asl_images(root, seq, frames, images):
    """mav0/{cam0,imu0} in the EuRoC ASL layout; images[i]: H x W (binary PGM) or H x W x 3 (binary PPM, P6) of frame frames[i]"""
    cam = os.path.join(root, "mav0", "cam0", "data")
    os.makedirs(cam)
    os.makedirs(os.path.join(root, "mav0", "imu0"))
    t0 = 1403636579_000000000
    with open(os.path.join(root, "mav0", "cam0", "data.csv"), "w") as f:
        f.write("#timestamp [ns],filename\n")
        for k, img in zip(frames, images):
            ns = t0 + int(round(seq.frame_time(k) * 1e9))
            name = "%d.%s" % (ns, "ppm" if img.ndim == 3 else "pgm")
            f.write("%d,%s\n" % (ns, name))
            with open(os.path.join(cam, name), "wb") as g:
                g.write((b"P6" if img.ndim == 3 else b"P5") + b"\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + np.ascontiguousarray(img).tobytes())
    with open(os.path.join(root, "mav0", "imu0", "data.csv"), "w") as f:
        f.write("#timestamp [ns],w_RS_S_x [rad s^-1],w_RS_S_y [rad s^-1],w_RS_S_z [rad s^-1],a_RS_S_x [m s^-2],a_RS_S_y [m s^-2],a_RS_S_z [m s^-2]\n")
        for s in seq.imu_all():
            ns = t0 + int(round(float(s["t"]) * 1e9))
            f.write("%d,%s\n" % (ns, ",".join(repr(float(v)) for v in list(s["w"]) + list(s["a"]))))


@pytest.fixture(scope="module")
def colour_frames():
    cfg = abi.config_named("A", enable_equalizer=1)          # the stock settings file = cfg A
    seq = rv.synth.SynthSequence(cfg, duration=4.0)
    frames = list(range(30, 30 + 34))                        # stationary until t = 2 s (frame 40): the start-up gate is exercised
    return seq, frames, [tint(seq.render(k), 2000 + k) for k in frames]


@pytest.mark.parametrize("is_rgb", [1, 0])
def test_replay_of_colour_frames_equals_replay_of_their_gray(gpu_required, tmp_path, colour_frames, is_rgb):
    seq, frames, cols = colour_frames
    yaml = tmp_path / "rvio.yaml"
    assert "Camera.RGB: 0" in EUROC_YAML
    yaml.write_text(EUROC_YAML.replace("Camera.RGB: 0", "Camera.RGB: %d" % is_rgb))
    outs = {}
    for kind, images in (("colour", cols), ("gray", [gray(c, bool(is_rgb)) for c in cols])):
        root = tmp_path / kind
        write_asl_images(str(root), seq, frames, images)
        out = tmp_path / (kind + ".dat")
        r = subprocess.run([ensure_bin(), str(yaml), str(root), str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[kind] = open(str(out), "rb").read()
    assert len(outs["gray"].splitlines()) >= 5
    assert outs["colour"] == outs["gray"]


def test_the_two_orders_give_different_trajectories(gpu_required, tmp_path, colour_frames):
    seq, frames, cols = colour_frames
    root = tmp_path / "colour"
    write_asl_images(str(root), seq, frames, cols)
    outs = []
    for is_rgb in (1, 0):
        yaml = tmp_path / ("rvio%d.yaml" % is_rgb)
        yaml.write_text(EUROC_YAML.replace("Camera.RGB: 0", "Camera.RGB: %d" % is_rgb))
        out = tmp_path / ("o%d.dat" % is_rgb)
        r = subprocess.run([ensure_bin(), str(yaml), str(root), str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(open(str(out), "rb").read())
    assert outs[0] != outs[1]
