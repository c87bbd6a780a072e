"""The host side of raw camera images (host/: load_image, Camera.Encoding, to_gray): 16-bit PNG, PGM and PPM files written here with NumPy and
zlib are decoded by `rvio_replay --check-image FILE [--encoding NAME]`, which prints a checksum of the CONVERTED 8-bit image — it must be the
checksum of tests/raw_model.py's conversion of the same samples.  Both file formats hold 16-bit samples big endian; a Bayer mosaic looks like a
gray file and can only be declared.  No device is involved: to_gray is the host form of the device's arithmetic."""
import json
import struct
import subprocess
import zlib

import numpy as np
import pytest

import raw_model as M
from test_host import BIN, EUROC_YAML, ensure_bin


def write_png(path, img, filters=(0, 1, 2, 3, 4)):
    """8- or 16-bit PNG (gray [h,w], RGB [h,w,3] or RGBA [h,w,4]; uint8 or uint16), row filters cycling through `filters`"""
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    depth = 8 * img.dtype.itemsize
    bpp = ch * depth // 8                                  # bytes per pixel: the distance the filters look back
    rows = np.ascontiguousarray(img.astype(">u2") if depth == 16 else img).view(np.uint8).reshape(h, w * bpp)
    raw = bytearray()
    prev = np.zeros(w * bpp, np.int32)
    zero = np.zeros(bpp, np.int32)
    for y in range(h):
        ft = filters[y % len(filters)]
        cur = rows[y].astype(np.int32)
        a, b, c = np.concatenate((zero, cur[:-bpp])), prev, np.concatenate((zero, prev[:-bpp]))
        if ft == 0:
            pred = np.zeros_like(cur)
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = b
        elif ft == 3:
            pred = (a + b) >> 1
        else:
            p = a + b - c
            pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        raw.append(ft)
        raw += ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    z = zlib.compress(bytes(raw), 1)
    half = len(z) // 2
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, {1: 0, 3: 2, 4: 6}[ch], 0, 0, 0)) +
                chunk(b"IDAT", z[:half]) + chunk(b"IDAT", z[half:]) + chunk(b"IEND", b""))


def write_pnm(path, img, maxval=None):
    """binary PGM (H x W) or PPM (H x W x 3); uint16: maxval 65535 unless given, samples most significant byte first"""
    h, w = img.shape[:2]
    sixteen = img.dtype == np.uint16
    data = (img.astype(">u2") if sixteen else img).tobytes()
    with open(path, "wb") as f:
        f.write((b"P6" if img.ndim == 3 else b"P5") + b"\n# synthetic\n%d %d\n%d\n" % (w, h, maxval or (65535 if sixteen else 255)) + data)


def checksum(g):
    idx = np.arange(g.size) % 251 + 1
    return int(g.sum(dtype=np.int64)), int((g.ravel().astype(np.int64) * idx).sum())


def check(path, *flags):
    return json.loads(subprocess.check_output([ensure_bin(), "--check-image", str(path)] + list(flags)))


H, W = 37, 53


@pytest.fixture(scope="module")
def samples():
    rng = np.random.default_rng(16)
    m16 = rng.integers(0, 65536, (H, W)).astype(np.uint16)
    m16[0, 0], m16[0, 1], m16[-1, -1] = 0, 65535, 0x1234           # the byte order shows
    rgb16 = rng.integers(0, 65536, (H, W, 3)).astype(np.uint16)
    rgba16 = np.concatenate([rgb16, rng.integers(0, 65536, (H, W, 1)).astype(np.uint16)], axis=2)
    m8 = rng.integers(0, 256, (H, W)).astype(np.uint8)
    return dict(m16=m16, rgb16=rgb16, rgba16=rgba16, m8=m8)


def test_mono16_png_and_pgm(tmp_path, samples):
    img = samples["m16"]
    s, ws = checksum(M.to_gray(img, "mono16"))
    want = {"width": W, "height": H, "channels": 1, "bits": 16, "format": 16, "sum": s, "wsum": ws}
    write_png(tmp_path / "a.png", img)
    write_pnm(tmp_path / "a.pgm", img)
    assert check(tmp_path / "a.png") == want
    assert check(tmp_path / "a.pgm") == want
    assert check(tmp_path / "a.png", "--encoding", "mono16") == want
    small = (img >> 4).astype(np.uint16)                             # a 12-bit sensor: maxval 4095 is 16-bit storage all the same
    write_pnm(tmp_path / "b.pgm", small, maxval=4095)
    s, ws = checksum(M.to_gray(small, "mono16"))
    assert check(tmp_path / "b.pgm") == dict(want, sum=s, wsum=ws)


def test_16_bit_colour_png_and_ppm(tmp_path, samples):
    write_png(tmp_path / "c.png", samples["rgb16"])
    write_png(tmp_path / "d.png", samples["rgba16"])
    write_pnm(tmp_path / "e.ppm", samples["rgb16"])
    for name, img, ch in (("c.png", samples["rgb16"], 3), ("d.png", samples["rgba16"], 4), ("e.ppm", samples["rgb16"], 3)):
        for flags, enc in (((), "rgb"), (("--bgr",), "bgr"), (("--encoding", "bgr%s16" % ("a" if ch == 4 else "")), "bgr")):
            full = enc + ("a" if ch == 4 else "") + "16"
            s, ws = checksum(M.to_gray(img, full))
            want = {"width": W, "height": H, "channels": ch, "bits": 16, "format": {"rgb16": 17, "bgr16": 18, "rgba16": 19, "bgra16": 20}[full], "sum": s, "wsum": ws}
            assert check(tmp_path / name, *flags) == want, (name, flags)


@pytest.mark.parametrize("enc", ["bayer_rggb8", "bayer_gbrg8", "bayer_grbg16", "bayer_bggr16"])
def test_declared_mosaics(tmp_path, samples, enc):
    img = samples["m16"] if enc.endswith("16") else samples["m8"]
    s, ws = checksum(M.to_gray(img, enc))
    assert (s, ws) != checksum(M.to_gray(img, "mono16" if enc.endswith("16") else "mono8"))
    want = {"width": W, "height": H, "channels": 1, "bits": 8 * img.dtype.itemsize, "format": M_FORMAT[enc], "sum": s, "wsum": ws}
    write_png(tmp_path / "m.png", img)
    write_pnm(tmp_path / "m.pgm", img)
    assert check(tmp_path / "m.png", "--encoding", enc) == want
    assert check(tmp_path / "m.pgm", "--encoding", enc) == want


M_FORMAT = {"bayer_rggb8": 32, "bayer_bggr8": 33, "bayer_gbrg8": 34, "bayer_grbg8": 35,
            "bayer_rggb16": 48, "bayer_bggr16": 49, "bayer_gbrg16": 50, "bayer_grbg16": 51}


def test_an_8_bit_file_without_an_encoding_prints_what_it_always_printed(tmp_path, samples):
    write_pnm(tmp_path / "g.pgm", samples["m8"])
    s, ws = checksum(samples["m8"])
    assert check(tmp_path / "g.pgm") == {"width": W, "height": H, "channels": 1, "sum": s, "wsum": ws}


def test_a_contradictory_encoding_is_refused(tmp_path, samples):
    write_png(tmp_path / "c.png", samples["rgb16"])
    write_pnm(tmp_path / "g.pgm", samples["m8"])
    write_pnm(tmp_path / "h.pgm", samples["m16"])
    for name, enc in (("c.png", "bayer_rggb16"), ("c.png", "rgb8"), ("c.png", "rgba16"), ("g.pgm", "mono16"), ("g.pgm", "bayer_rggb16"),
                      ("g.pgm", "rgb8"), ("h.pgm", "bayer_rggb8"), ("h.pgm", "mono8")):
        r = subprocess.run([ensure_bin(), "--check-image", str(tmp_path / name), "--encoding", enc], capture_output=True, text=True)
        assert r.returncode != 0 and "contradicts the image" in r.stderr and enc in r.stderr, (name, enc, r.stderr)
    r = subprocess.run([BIN, "--check-image", str(tmp_path / "g.pgm"), "--encoding", "yuv422"], capture_output=True, text=True)
    assert r.returncode != 0 and "unknown encoding" in r.stderr


def test_the_settings_key(tmp_path):
    p = tmp_path / "s.yaml"
    p.write_text(EUROC_YAML)
    assert json.loads(subprocess.check_output([ensure_bin(), "--check-settings", str(p)]))["encoding"] == ""     # absent: as before
    for text, want in (("Camera.Encoding: bayer_grbg8", "bayer_grbg8"), ('Camera.Encoding: "mono16"   # quoted', "mono16")):
        p.write_text(EUROC_YAML + "\n" + text + "\n")
        assert json.loads(subprocess.check_output([BIN, "--check-settings", str(p)]))["encoding"] == want
    p.write_text(EUROC_YAML + "\nCamera.Encoding: yuv422\n")
    r = subprocess.run([BIN, "--check-settings", str(p)], capture_output=True, text=True)
    assert r.returncode != 0 and "unknown encoding" in r.stderr
