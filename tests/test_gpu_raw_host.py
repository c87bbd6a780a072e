"""rvio_replay (host/: System::MonoVIO above the C-ABI) on an EuRoC ASL folder of RAW frames — 16-bit PNGs, and Bayer mosaics as PGM declared by
Camera.Encoding: System sets the handle's image format from the file's bit depth or the settings key and hands the samples over unconverted
(what the reference's node leaves to cv_bridge::toCvShare(msg, MONO8), rvio_mono.cc:64), so the pose file must be byte-identical to the one
the same binary writes for the folder that holds the NumPy gray of the same frames as 8-bit PGM."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import raw_model as M
from test_gpu_raw import tint, widen
from test_host import EUROC_YAML, ensure_bin
from test_raw_host import write_png, write_pnm

abi, rv = O.abi, O.rv
pytestmark = pytest.mark.gpu


def write_asl_images(root, seq, frames, images, png):
    """mav0/{cam0,imu0} in the EuRoC ASL layout; images[i]: the H x W samples of frame frames[i], as PNG or binary PGM"""
    cam = os.path.join(root, "mav0", "cam0", "data")
    os.makedirs(cam)
    os.makedirs(os.path.join(root, "mav0", "imu0"))
    t0 = 1403636579_000000000
    with open(os.path.join(root, "mav0", "cam0", "data.csv"), "w") as f:
        f.write("#timestamp [ns],filename\n")
        for k, img in zip(frames, images):
            ns = t0 + int(round(seq.frame_time(k) * 1e9))
            name = "%d.%s" % (ns, "png" if png else "pgm")
            f.write("%d,%s\n" % (ns, name))
            if png:
                write_png(os.path.join(cam, name), img, filters=(1, 4, 0, 2))
            else:
                write_pnm(os.path.join(cam, name), img)
    with open(os.path.join(root, "mav0", "imu0", "data.csv"), "w") as f:
        f.write("#timestamp [ns],w_RS_S_x [rad s^-1],w_RS_S_y [rad s^-1],w_RS_S_z [rad s^-1],a_RS_S_x [m s^-2],a_RS_S_y [m s^-2],a_RS_S_z [m s^-2]\n")
        for s in seq.imu_all():
            ns = t0 + int(round(float(s["t"]) * 1e9))
            f.write("%d,%s\n" % (ns, ",".join(repr(float(v)) for v in list(s["w"]) + list(s["a"]))))


@pytest.fixture(scope="module")
def gray_frames():
    cfg = abi.config_named("A", enable_equalizer=1)          # the stock settings file = cfg A
    seq = rv.synth.SynthSequence(cfg, duration=4.0)
    frames = list(range(30, 30 + 34))                        # stationary until t = 2 s (frame 40): the start-up gate is exercised
    return seq, frames, [seq.render(k) for k in frames]


def replay(tmp_path, yaml_text, kind, seq, frames, images, png):
    yaml = tmp_path / (kind + ".yaml")
    yaml.write_text(yaml_text)
    root = tmp_path / kind
    write_asl_images(str(root), seq, frames, images, png)
    out = tmp_path / (kind + ".dat")
    r = subprocess.run([ensure_bin(), str(yaml), str(root), str(out)], capture_output=True, text=True)
    return r, (open(str(out), "rb").read() if r.returncode == 0 else b"")


@pytest.mark.parametrize("enc", ["mono16", "bayer_rggb8", "bayer_gbrg16"])
def test_replay_of_raw_frames_equals_replay_of_their_gray(gpu_required, tmp_path, gray_frames, enc):
    seq, frames, grays = gray_frames
    if enc == "mono16":                                       # nothing declared: the file's bit depth says it
        raws, yaml, png = [widen(g, 3000 + k) for k, g in zip(frames, grays)], EUROC_YAML, True
    else:
        cols = [tint(g, 2000 + k) for k, g in zip(frames, grays)]
        raws = [M.mosaic(c if enc.endswith("8") else widen(c, 4000 + k), enc[6:10]) for k, c in zip(frames, cols)]
        yaml, png = EUROC_YAML + "\nCamera.Encoding: %s\n" % enc, enc.endswith("16")
    r, raw_out = replay(tmp_path, yaml, "raw", seq, frames, raws, png)
    assert r.returncode == 0, r.stderr[-3000:]
    r, gray_out = replay(tmp_path, EUROC_YAML, "gray", seq, frames, [M.to_gray(x, enc) for x in raws], False)
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(gray_out.splitlines()) >= 5
    assert raw_out == gray_out


def test_a_contradictory_encoding_stops_the_replay(gpu_required, tmp_path, gray_frames):
    seq, frames, grays = gray_frames
    r, _ = replay(tmp_path, EUROC_YAML + "\nCamera.Encoding: bayer_rggb16\n", "bad", seq, frames, grays, False)
    assert r.returncode != 0 and "contradicts the image" in r.stderr, r.stderr[-2000:]
