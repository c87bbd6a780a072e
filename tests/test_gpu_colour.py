"""Colour camera images on the device (rvio_hip_set_image_format; Tracker.cc:182-196 "Convert to gray scale"): gray_kernel in front of the
frame's image chain, through every image entry point.

The truth is the NumPy form of OpenCV's 8-bit fixed-point cvtColor, Y = (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14 (as
tests/test_host.py::gray writes it; tests/test_gray_arith.py walks the device's arithmetic over all 2^24 triples on the CPU).  Everything
behind the conversion is the mono path, which the rest of the suite pins — so a colour handle fed interleaved pixels must give, BIT FOR
BIT, what a mono handle fed the NumPy gray of the same pixels gives: integers in, the same launches behind.  No tolerances anywhere.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
import scenarios as S

abi, rv = O.abi, O.rv
pytestmark = pytest.mark.gpu

K0 = 38
FMT = {"rgb": abi.RVIO_PIX_RGB8, "bgr": abi.RVIO_PIX_BGR8, "rgba": abi.RVIO_PIX_RGBA8, "bgra": abi.RVIO_PIX_BGRA8}


def gray(img, is_rgb):
    r, g, b = (img[..., 0], img[..., 1], img[..., 2]) if is_rgb else (img[..., 2], img[..., 1], img[..., 0])
    return ((r.astype(np.int64) * 4899 + g.astype(np.int64) * 9617 + b.astype(np.int64) * 1868 + 8192) >> 14).astype(np.uint8)


def gray_of(img, fmt):
    return gray(img, fmt in ("rgb", "rgba"))


def tint(g, seed, num=(5, 4, 3)):
    """a synthetic gray frame as a colour one: R = min(255, 5g/4), G = g, B = 3g/4 (num / 4), plus a seeded +-3 per channel — the texture still
    moves with the scene, and reading the bytes as RGB or as BGR gives different grays"""
    rng = np.random.default_rng(seed)
    g16 = g.astype(np.int64)
    c = np.stack([g16 * num[0] // 4, g16 * num[1] // 4, g16 * num[2] // 4], axis=-1) + rng.integers(-3, 4, g.shape + (3,))
    return np.clip(c, 0, 255).astype(np.uint8)


def random_colour(h, w, ch, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
    img[0, 0, :3], img[h // 2, w - 1, :3], img[h - 1, w - 1, :3], img[1, 1, :3] = 0, 255, 0, 255     # both ends of the range, row ends included
    return img


def eq_off_cfg(w, h, eq=0):
    return abi.config_named("B", enable_equalizer=eq, width=w, height=h, block_x=min(150, w // 4), block_y=min(120, h // 4))


def one_imu():
    imu = np.zeros(1, abi.IMU_DTYPE)
    imu["dt"] = 0.005
    return imu


# ------------------------------------------------------------------ 1, 2: the kernel alone
@pytest.mark.parametrize("fmt", ["rgb", "bgr", "rgba", "bgra"])
def test_wide_form_through_track(gpu_required, fmt):
    """376 x 240 from host memory (dword-aligned staging, W % 4 == 0: four pixels per thread), equaliser off: level 0 of the pyramid is the
    copy of the gray image"""
    from rvio_amd import hip
    w, hh, ch = 376, 240, len(fmt)
    img = random_colour(hh, w, ch, 7 + ch)
    h = hip.RvioHip(eq_off_cfg(w, hh))
    h.set_image_format(FMT[fmt])
    assert h.image_format() == FMT[fmt]
    cand = np.array([[w / 2, hh / 2], [w / 3, hh / 3]], np.float32)
    h.track(img, one_imu(), cand)
    got, _ = h.debug_pyramid(0)
    want = gray_of(img, fmt)
    assert np.array_equal(got, want), int((got != want).sum())
    if ch == 4:                      # alpha is ignored
        img2 = img.copy()
        img2[..., 3] = 255 - img2[..., 3]
        h.track(img2, one_imu(), cand)
        assert np.array_equal(h.debug_pyramid(0)[0], want)
    h.close()


@pytest.mark.parametrize("fmt", ["rgb", "bgr", "rgba", "bgra"])
def test_byte_form_through_track_dev(gpu_required, fmt):
    """750 x 481 (two whole 256-pixel segments and a tail of 238 per row, an odd height) with an odd padded row stride from a device buffer:
    the byte form; the padding bytes are random and change between the two calls, the result does not"""
    from rvio_amd import hip
    import torch
    w, hh, ch = 750, 481, len(fmt)
    stride = w * ch + 7                                # odd for both pixel sizes
    assert stride % 2 == 1
    img = random_colour(hh, w, ch, 70 + ch)
    want = gray_of(img, fmt)
    h = hip.RvioHip(eq_off_cfg(w, hh))
    h.set_image_format(FMT[fmt])
    d_imu = torch.from_numpy(one_imu().view(np.uint8)).cuda()
    d_cand = torch.from_numpy(np.array([[w / 2, hh / 2], [w / 3, hh / 3]], np.float32)).cuda()
    for seed in (1, 2):
        buf = np.random.default_rng(seed).integers(0, 256, (hh, stride), dtype=np.uint8)
        buf[:, : w * ch] = img.reshape(hh, w * ch)
        d_buf = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        h.track_dev(d_buf.data_ptr(), stride, d_imu.data_ptr(), 1, d_cand.data_ptr(), 2)
        got, _ = h.debug_pyramid(0)
        assert np.array_equal(got, want), (seed, int((got != want).sum()))
    h.close()


@pytest.mark.parametrize("fmt", ["rgb", "bgra"])
def test_equaliser_sees_the_gray_image(gpu_required, fmt):
    from rvio_amd import hip
    w, hh, ch = 376, 240, len(fmt)
    img = random_colour(hh, w, ch, 17 + ch)
    img[..., :3] = tint(np.add.outer(np.arange(hh) * 2, np.arange(w)).astype(np.uint8) // 2 + img[..., 0] // 4, 3)   # some structure for the histograms
    h = hip.RvioHip(eq_off_cfg(w, hh, eq=1))
    h.set_image_format(FMT[fmt])
    h.track(img, one_imu(), np.array([[w / 2, hh / 2], [w / 3, hh / 3]], np.float32))
    got, _ = h.debug_pyramid(0)
    want = O.clahe(gray_of(img, fmt))
    assert np.array_equal(got, want), int((got != want).sum())
    h.close()


# ------------------------------------------------------------------ 3 - 7: sequences
def sequence(n=40):
    """the 376 x 240 scenario of tests/scenarios.py (stock equaliser, 100 features, 10-clone window), tinted"""
    cfg = S.small_image_config()
    seq = rv.synth.SynthSequence(cfg, duration=8.0)
    ks = list(range(K0 + 1, K0 + 1 + n))
    grays = [seq.render(k) for k in ks]
    return dict(cfg=cfg, init=seq.init_from_static(K0), imus=[seq.imu_between(k) for k in ks],
                colour=[tint(g, 1000 + i) for i, g in enumerate(grays)])


@pytest.fixture(scope="module")
def seq40():
    return sequence(40)


def snapshot(h):
    p, q = h.pose()
    x, P = h.get_state()
    pts, hl = h.get_points()
    return dict(pose=np.concatenate((p, q)), x=x, P=P, pts=pts, hl=hl, tracks=h.get_tracks(), info=h.frame_info())


def same_snapshot(a, b):
    return (all(np.array_equal(a[k], b[k]) for k in ("pose", "x", "P", "pts", "hl")) and a["info"] == b["info"]
            and all(np.array_equal(u, v) for u, v in zip(a["tracks"], b["tracks"])))


def run_host(d, frames, fmt):
    """frames through rvio_hip_frame (device detector) on a fresh handle; fmt None: a mono handle"""
    from rvio_amd import hip
    h = hip.RvioHip(d["cfg"])
    h.initialize(*d["init"])
    if fmt is not None:
        h.set_image_format(FMT[fmt])
    out = []
    for img, imu in zip(frames, d["imus"]):
        h.frame(img.copy(), imu.copy(), None)            # temporaries: the call must have consumed them on return
        out.append(snapshot(h))
    h.close()
    return out


@pytest.fixture(scope="module")
def host_runs(seq40):
    """the same bytes read as RGB and as BGR, each against a mono handle fed the NumPy gray (one handle alive at a time)"""
    runs = {}
    for fmt in ("rgb", "bgr"):
        runs[fmt] = run_host(seq40, seq40["colour"], fmt)
        runs[fmt + "-mono"] = run_host(seq40, [gray_of(c, fmt) for c in seq40["colour"]], None)
    return runs


@pytest.mark.parametrize("fmt", ["rgb", "bgr"])
def test_colour_sequence_equals_the_mono_sequence(gpu_required, host_runs, fmt):
    a, b = host_runs[fmt], host_runs[fmt + "-mono"]
    assert len(a) == len(b) == 40
    for k, (u, v) in enumerate(zip(a, b)):
        assert same_snapshot(u, v), (fmt, k, u["info"], v["info"])
    assert sum(u["info"]["updated"] == 1 for u in a) >= 5
    assert a[-1]["info"]["device_error"] == 0


def test_the_channel_order_matters(gpu_required, host_runs):
    assert not np.array_equal(host_runs["rgb"][-1]["x"], host_runs["bgr"][-1]["x"])
    assert not np.array_equal(host_runs["rgb"][0]["pts"], host_runs["bgr"][0]["pts"])


def ordering_child(pad):
    """(runs in a child process: the library reads RVIO_NO_RUNAHEAD when it is loaded)  the colour sequence flat out through rvio_hip_frame_dev
    from a row-padded device buffer, sleeping kernels on random streams and rvio_hip_debug_poison(7) between frames, against the synchronised
    mono run"""
    from rvio_amd import hip
    import torch
    d = sequence(40)
    cfg, n = d["cfg"], 40
    h = hip.RvioHip(cfg)
    h.initialize(*d["init"])
    ref = []
    for c, imu in zip(d["colour"], d["imus"]):
        h.frame(gray_of(c, "rgb"), imu, None)
        h.sync()
        p, q = h.pose()
        ref.append(np.concatenate((p, q)))
    ref_end = (h.get_state(), h.get_points())
    h.close()
    stride = cfg.width * 3 + pad
    buf = np.random.default_rng(5).integers(0, 256, (n, cfg.height, stride), dtype=np.uint8)
    for i, c in enumerate(d["colour"]):
        buf[i, :, : cfg.width * 3] = c.reshape(cfg.height, -1)
    d_imgs = torch.from_numpy(buf).cuda()
    d_imus = [torch.from_numpy(i.view(np.uint8)).cuda() for i in d["imus"]]
    torch.cuda.synchronize()
    for seed in (1, 2):
        h = hip.RvioHip(cfg)
        h.initialize(*d["init"])
        h.set_image_format(abi.RVIO_PIX_RGB8)
        rng = np.random.default_rng(seed)
        poses = []
        for i in range(n):
            for _ in range(int(rng.integers(0, 3))):     # 0..2 stalls in front of this frame, any stream, 30..900 us
                h.stall(int(rng.integers(0, 4)), int(rng.integers(30, 900)))
            if i % 6 == 4:
                h.poison(7)                              # NaN bytes in the gray buffers too: a stage that read a stale slot would show
            h.frame_dev(d_imgs[i].data_ptr(), stride, d_imus[i].data_ptr(), len(d["imus"][i]), 0, 0)
            if seed == 1:
                p, q = h.pose()                          # waits for the filter stream only
                poses.append(np.concatenate((p, q)))
        h.sync()
        end = (h.get_state(), h.get_points())
        info = h.frame_info()
        h.close()
        assert info["device_error"] == 0, info
        if poses:
            bad = [i for i in range(n) if not np.array_equal(poses[i], ref[i])]
            assert not bad, ("first differing frame", bad[0])
        for u, v in zip(end, ref_end):
            assert np.array_equal(u[0], v[0]) and np.array_equal(u[1], v[1]), seed
    print("COLOUR_ORDER_OK")


@pytest.mark.parametrize("mode", ["default", "no-runahead"])
def test_gray_buffers_are_ordered_under_any_pacing(gpu_required, mode):
    """four gray buffers in rotation and no wait of their own: the run-ahead image chains (default) and the single image stream
    (RVIO_NO_RUNAHEAD=1) must both reproduce the synchronised mono run bit for bit; a dword-aligned padded stride (wide form) in one mode, an
    odd one (byte form) in the other"""
    code = "import sys; sys.path.insert(0, %r); import test_gpu_colour as T; T.ordering_child(%d)" % (
        os.path.dirname(os.path.abspath(__file__)), 8 if mode == "default" else 5)
    env = dict(os.environ)
    env.pop("RVIO_NO_RUNAHEAD", None)
    if mode == "no-runahead":
        env["RVIO_NO_RUNAHEAD"] = "1"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert out.returncode == 0 and "COLOUR_ORDER_OK" in out.stdout, out.stderr[-3000:]


def test_format_switch_in_mid_sequence(gpu_required, seq40):
    """10 mono frames, rvio_hip_set_image_format(RGB8), 10 colour frames = 20 mono frames (the staging is laid out again, nothing else moves)"""
    from rvio_amd import hip
    d = seq40
    grays = [gray_of(c, "rgb") for c in d["colour"][:20]]
    h = hip.RvioHip(d["cfg"])
    h.initialize(*d["init"])
    got = []
    for i in range(20):
        if i == 10:
            h.set_image_format(abi.RVIO_PIX_RGB8)
        h.frame(grays[i] if i < 10 else d["colour"][i], d["imus"][i], None)
        got.append(snapshot(h))
    h.close()
    want = run_host(dict(d, imus=d["imus"][:20]), grays, None)
    for k, (u, v) in enumerate(zip(got, want)):
        assert same_snapshot(u, v), k


@pytest.mark.parametrize("B", [3, 8])
def test_batch_handles(gpu_required, seq40, B):
    """rvio_hip_frame_batch_dev with a colour format: B instances, each with its own tint, rows and instances padded (B = 3: an odd instance
    stride, the byte form, the latency forms of the image kernels behind it; B = 8: dword-aligned, the wide form, the throughput forms) against
    the same handle type fed the gray images"""
    from rvio_amd import hip
    import torch
    d, n = seq40, 10
    cfg = d["cfg"]
    W, H = cfg.width, cfg.height
    base = [gray_of(c, "rgb") for c in d["colour"][:n]]
    cols = [[tint(base[f], 50 * i + f, num=(5 + i % 4, 4, 3 - i // 4)) for i in range(B)] for f in range(n)]
    stride = W * 3 + (8 if B == 8 else 3)
    img_stride = stride * H + (52 if B == 8 else 37)
    ends = {}
    for kind in ("colour", "mono"):
        h = hip.RvioHip(cfg, batch=B, front_end=True)
        h.initialize(*d["init"])
        if kind == "colour":
            h.set_image_format(abi.RVIO_PIX_RGB8)
        keep = []
        for f in range(n):
            if kind == "colour":
                buf = np.random.default_rng(f).integers(0, 256, B * img_stride, dtype=np.uint8)
                for i in range(B):
                    rows = buf[i * img_stride: i * img_stride + H * stride].reshape(H, stride)
                    rows[:, : W * 3] = cols[f][i].reshape(H, -1)
                args = (stride, img_stride)
            else:
                buf = np.stack([gray_of(cols[f][i], "rgb") for i in range(B)]).reshape(-1)
                args = (W, W * H)
            d_img = torch.from_numpy(buf).cuda()
            d_imu = torch.from_numpy(d["imus"][f].view(np.uint8)).cuda()
            keep += [d_img, d_imu]
            torch.cuda.synchronize()
            h.frame_batch_dev(d_img.data_ptr(), args[0], args[1], d_imu.data_ptr(), 0, len(d["imus"][f]))
        h.sync()
        ends[kind] = [(h.get_points_at(i), h.get_state_at(i)) for i in range(B)]
        h.close()
    for i in range(B):
        (pa, sa), (pb, sb) = ends["colour"][i], ends["mono"][i]
        assert len(pa[0]) > 20 and np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1]), i
        assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]), i
    assert not np.array_equal(ends["colour"][0][0][0], ends["colour"][1][0][0])     # the tints really give different streams


def test_sharded_frame_world_1(gpu_required, seq40):
    from rvio_amd import hip
    import torch
    d, n = seq40, 10
    cfg = d["cfg"]
    ends = {}
    for kind in ("colour", "mono"):
        h = hip.RvioHip(cfg)
        h.initialize(*d["init"])
        if kind == "colour":
            h.set_image_format(abi.RVIO_PIX_BGR8)
        imgs = np.stack([c if kind == "colour" else gray_of(c, "bgr") for c in d["colour"][:n]])
        d_imgs = torch.from_numpy(imgs).cuda()
        d_imus = [torch.from_numpy(i.view(np.uint8)).cuda() for i in d["imus"][:n]]
        torch.cuda.synchronize()
        for i in range(n):
            h.frame_sharded_dev(d_imgs[i].data_ptr(), cfg.width * (3 if kind == "colour" else 1), d_imus[i].data_ptr(), len(d["imus"][i]), 0, 0, 0, 1)
        h.sync()
        ends[kind] = snapshot(h)
        h.close()
    assert same_snapshot(ends["colour"], ends["mono"])
    assert ends["colour"]["info"]["n_clones"] == 9 and ends["colour"]["info"]["n_tracked_out"] > 20 and ends["colour"]["info"]["device_error"] == 0


# ------------------------------------------------------------------ 8: refusals
def test_refusals_and_the_timing_hook(gpu_required, seq40):
    from rvio_amd import hip
    import torch
    d = seq40
    cfg = d["cfg"]
    W = cfg.width
    h = hip.RvioHip(cfg)
    L = h.L
    assert h.image_format() == abi.RVIO_PIX_MONO8                       # off by default
    for bad in (-1, 5, 99):
        assert L.rvio_hip_set_image_format(h.h, bad) == -1               # RVIO_ERR_INVALID
    assert h.image_format() == abi.RVIO_PIX_MONO8
    import ctypes as C
    us = C.c_float(0)
    assert L.rvio_hip_debug_time_kernel(h.h, 11, 5, C.byref(us)) == -3   # RVIO_ERR_UNSUPPORTED without a colour format
    h.initialize(*d["init"])
    d_imu = torch.from_numpy(d["imus"][0].view(np.uint8)).cuda()
    m = len(d["imus"][0])
    for fmt, ch in (("rgb", 3), ("bgra", 4)):
        h.set_image_format(FMT[fmt])
        img = d["colour"][0] if ch == 3 else np.concatenate([d["colour"][0], d["colour"][0][..., :1]], axis=2)
        d_img = torch.from_numpy(np.ascontiguousarray(img)).cuda()
        torch.cuda.synchronize()
        short = W * ch - 1
        vp = C.c_void_p
        assert L.rvio_hip_frame_dev(h.h, vp(d_img.data_ptr()), short, vp(d_imu.data_ptr()), m, None, 0) == -1
        assert L.rvio_hip_track_dev(h.h, vp(d_img.data_ptr()), short, vp(d_imu.data_ptr()), m, None, 0) == -1
        assert L.rvio_hip_frame_begin_dev(h.h, vp(d_img.data_ptr()), short, vp(d_imu.data_ptr()), m, None, 0) == -1
        assert L.rvio_hip_frame_sharded_dev(h.h, vp(d_img.data_ptr()), short, vp(d_imu.data_ptr()), m, None, 0, 0, 1, None, None) == -1
        host = np.ascontiguousarray(img)
        up = C.POINTER(C.c_ubyte)
        imu = np.ascontiguousarray(d["imus"][0])
        ip = imu.ctypes.data_as(C.POINTER(abi.rvio_imu))
        assert L.rvio_hip_frame(h.h, C.cast(host.ctypes.data, up), short, ip, m, None, 0) == -1
        assert L.rvio_hip_track(h.h, C.cast(host.ctypes.data, up), short, ip, m, None, 0) == -1
        h.frame_dev(d_img.data_ptr(), W * ch, d_imu.data_ptr(), m, 0, 0)          # the exact stride is fine
        for iters in (1, 20):
            t = h.time_kernel(11, iters)
            assert t > 0 and math.isfinite(t), t
    h.close()
    hb = hip.RvioHip(cfg, batch=2, front_end=True)
    hb.set_image_format(abi.RVIO_PIX_RGB8)
    d_b = torch.zeros(2 * W * 3 * cfg.height, dtype=torch.uint8, device="cuda")
    assert L.rvio_hip_frame_batch_dev(hb.h, C.c_void_p(d_b.data_ptr()), W * 3 - 1, C.c_size_t(W * 3 * cfg.height), C.c_void_p(d_imu.data_ptr()), 0, m) == -1
    hb.close()
    hf = hip.RvioHip(cfg, batch=2, front_end=False)                      # filter only: it takes no image
    assert L.rvio_hip_set_image_format(hf.h, abi.RVIO_PIX_RGB8) == -3
    assert L.rvio_hip_set_image_format(hf.h, abi.RVIO_PIX_MONO8) == 0
    assert L.rvio_hip_set_image_format(hf.h, 7) == -1
    hf.close()
