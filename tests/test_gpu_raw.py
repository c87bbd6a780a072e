"""Raw camera images on the device (rvio_hip_set_image_format with a 16-bit or a Bayer format: what cv_bridge::toCvShare(msg, MONO8) converts
in front of Tracker::track, rvio_mono.cc:64): raw16_kernel* / bayer_kernel* at the head of the frame's image chain, through every image
entry point.

The truth is tests/raw_model.py, the NumPy model tests/test_raw_arith.py holds the device's arithmetic to on the CPU.  Everything behind the
conversion is the mono path, which the rest of the suite pins — so a raw handle fed the sensor's samples must give, BIT FOR BIT, what a mono
handle fed the NumPy gray of the same samples gives.  No tolerances anywhere.
"""
import ctypes as C
import math

import numpy as np
import pytest

import oracle as O
import raw_model as M
import scenarios as S

abi, rv = O.abi, O.rv
pytestmark = pytest.mark.gpu

K0 = 38
ENC = dict(abi.PIX_ENCODING)
NEW = [e for e, v in sorted(ENC.items(), key=lambda kv: kv[1]) if v >= 16]      # the thirteen raw encodings


def random_raw(h, w, enc, seed):
    """random samples of an encoding's array type, both ends of the range at the corners, the row ends and next to them"""
    bpp, dtype, last = abi.PIX_LAYOUT[ENC[enc]]
    top = 65535 if dtype == "uint16" else 255
    rng = np.random.default_rng(seed)
    img = rng.integers(0, top + 1, (h, w) if last is None else (h, w, last)).astype(dtype)
    img[0, 0], img[h // 2, w - 1], img[h - 1, w - 1], img[1, 1], img[h - 2, w - 2], img[0, w - 1] = 0, top, 0, top, top, top
    return img


def eq_off_cfg(w, h, eq=0):
    return abi.config_named("B", enable_equalizer=eq, width=w, height=h, block_x=min(150, w // 4), block_y=min(120, h // 4))


def one_imu():
    imu = np.zeros(1, abi.IMU_DTYPE)
    imu["dt"] = 0.005
    return imu


def dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return t


# ------------------------------------------------------------------ the kernel alone: every format, three sizes, one handle per size
def test_wide_form_from_host_memory(gpu_required):
    """376 x 240 through rvio_hip_track (dword-aligned staging, W % 4 == 0: four pixels per lane; a whole segment and a tail of 120), equaliser
    off: level 0 of the pyramid is the copy of the converted image"""
    from rvio_amd import hip
    w, hh = 376, 240
    h = hip.RvioHip(eq_off_cfg(w, hh))
    cand = np.array([[w / 2, hh / 2], [w / 3, hh / 3]], np.float32)
    for k, enc in enumerate(NEW):
        img = random_raw(hh, w, enc, 100 + k)
        h.set_image_format(ENC[enc])
        assert h.image_format() == ENC[enc]
        h.track(img, one_imu(), cand)
        got, _ = h.debug_pyramid(0)
        want = M.to_gray(img, enc)
        assert np.array_equal(got, want), (enc, int((got != want).sum()), np.argwhere(got != want)[:4])
        if img.ndim == 3 and img.shape[2] == 4:      # alpha is ignored
            img2 = img.copy()
            img2[..., 3] = ~img2[..., 3]
            h.track(img2, one_imu(), cand)
            assert np.array_equal(h.debug_pyramid(0)[0], want), enc
    h.close()


def test_plain_form_from_a_padded_device_buffer(gpu_required):
    """750 x 481 (two whole 256-pixel segments and a tail of 238, an odd height) from a device buffer whose row stride is W bpp + 7 (8-bit
    mosaics: odd) or W bpp + 6 (16-bit formats: even, no multiple of 4): the plain form; the padding bytes are random and change between the
    two calls, the result does not"""
    from rvio_amd import hip
    w, hh = 750, 481
    h = hip.RvioHip(eq_off_cfg(w, hh))
    d_imu, d_cand = dev(one_imu()), dev(np.array([[w / 2, hh / 2], [w / 3, hh / 3]], np.float32))
    for k, enc in enumerate(NEW):
        bpp = abi.PIX_LAYOUT[ENC[enc]][0]
        stride = w * bpp + (7 if ENC[enc] & 16 == 0 else 6)
        assert stride % 4 != 0
        img = random_raw(hh, w, enc, 200 + k)
        want = M.to_gray(img, enc)
        h.set_image_format(ENC[enc])
        for seed in (1, 2):
            buf = np.random.default_rng(seed).integers(0, 256, (hh, stride), dtype=np.uint8)
            buf[:, : w * bpp] = img.view(np.uint8).reshape(hh, w * bpp)
            d_buf = dev(buf)
            h.track_dev(d_buf.data_ptr(), stride, d_imu.data_ptr(), 1, d_cand.data_ptr(), 2)
            got, _ = h.debug_pyramid(0)
            assert np.array_equal(got, want), (enc, seed, int((got != want).sum()), np.argwhere(got != want)[:4])
    h.close()


def test_one_pixel_row_tail(gpu_required):
    """769 x 243: three whole segments and a tail of ONE pixel, whose right neighbour is the clamped column; odd width and odd height"""
    from rvio_amd import hip
    w, hh = 769, 243
    h = hip.RvioHip(eq_off_cfg(w, hh))
    cand = np.array([[w / 2, hh / 2], [w / 3, hh / 3]], np.float32)
    for k, enc in enumerate(NEW):
        img = random_raw(hh, w, enc, 300 + k)
        h.set_image_format(ENC[enc])
        h.track(img, one_imu(), cand)
        got, _ = h.debug_pyramid(0)
        want = M.to_gray(img, enc)
        assert np.array_equal(got, want), (enc, int((got != want).sum()), np.argwhere(got != want)[:4])
    h.close()


def test_wide_mosaic_form_across_segments_from_a_padded_device_buffer(gpu_required):
    """772 x 243 from a device buffer with a dword-aligned padded stride: the wide forms with three whole segments (the halo sample comes from the
    neighbouring segment) and a tail of ONE group of four, first and last row; padding bytes random"""
    from rvio_amd import hip
    w, hh = 772, 243
    h = hip.RvioHip(eq_off_cfg(w, hh))
    d_imu, d_cand = dev(one_imu()), dev(np.array([[w / 2, hh / 2], [w / 3, hh / 3]], np.float32))
    for k, enc in enumerate(NEW):
        bpp = abi.PIX_LAYOUT[ENC[enc]][0]
        stride = w * bpp + 8
        img = random_raw(hh, w, enc, 400 + k)
        buf = np.random.default_rng(k).integers(0, 256, (hh, stride), dtype=np.uint8)
        buf[:, : w * bpp] = img.view(np.uint8).reshape(hh, w * bpp)
        d_buf = dev(buf)
        h.set_image_format(ENC[enc])
        h.track_dev(d_buf.data_ptr(), stride, d_imu.data_ptr(), 1, d_cand.data_ptr(), 2)
        got, _ = h.debug_pyramid(0)
        want = M.to_gray(img, enc)
        assert np.array_equal(got, want), (enc, int((got != want).sum()), np.argwhere(got != want)[:4])
    h.close()


@pytest.mark.parametrize("enc", ["mono16", "bgr16", "bayer_gbrg8", "bayer_bggr16"])
def test_equaliser_sees_the_converted_image(gpu_required, enc):
    from rvio_amd import hip
    w, hh = 376, 240
    bpp, dtype, last = abi.PIX_LAYOUT[ENC[enc]]
    ramp = (np.add.outer(np.arange(hh) * 2, np.arange(w)) % 256)                 # some structure for the histograms
    img = random_raw(hh, w, enc, 17)
    scale = 257 if dtype == "uint16" else 1
    img = ((img.astype(np.int64) // 4 + (ramp * scale * 3 // 4).reshape((hh, w) + (1,) * (img.ndim - 2)))).astype(dtype)
    h = hip.RvioHip(eq_off_cfg(w, hh, eq=1))
    h.set_image_format(ENC[enc])
    h.track(img, one_imu(), np.array([[w / 2, hh / 2], [w / 3, hh / 3]], np.float32))
    got, _ = h.debug_pyramid(0)
    model = M.to_gray(img, enc)
    assert model.std() > 20
    want = O.clahe(model)
    assert np.array_equal(got, want), int((got != want).sum())
    h.close()


# ------------------------------------------------------------------ sequences
def tint(g, seed, num=(5, 4, 3)):
    """a synthetic gray frame as a colour one: R = min(255, 5g/4), G = g, B = 3g/4, plus a seeded +-3 per channel"""
    rng = np.random.default_rng(seed)
    g16 = g.astype(np.int64)
    c = np.stack([g16 * num[0] // 4, g16 * num[1] // 4, g16 * num[2] // 4], axis=-1) + rng.integers(-3, 4, g.shape + (3,))
    return np.clip(c, 0, 255).astype(np.uint8)


def widen(a, seed):
    """8-bit samples as 16-bit ones: v * 257 plus seeded low-byte noise"""
    noise = np.random.default_rng(seed).integers(-128, 129, a.shape)
    return np.clip(a.astype(np.int64) * 257 + noise, 0, 65535).astype(np.uint16)


def raw_frame(enc, g, seed, inst=0):
    """the synthetic gray frame g as a sensor of that encoding delivers it"""
    num = (5 + inst % 4, 4, 3 - inst // 4)
    if enc == "mono16":
        return widen(g, seed)
    if enc == "bayer_rggb8":
        return M.mosaic(tint(g, seed, num), "rggb")
    if enc == "bayer_grbg16":
        return M.mosaic(widen(tint(g, seed, num), seed + 1), "grbg")
    if enc == "bayer_bggr8":
        return M.mosaic(tint(g, seed, num), "bggr")
    raise KeyError(enc)


@pytest.fixture(scope="module")
def seq40():
    """the 376 x 240 scenario of tests/scenarios.py (stock equaliser, 100 features, 10-clone window)"""
    cfg = S.small_image_config()
    seq = rv.synth.SynthSequence(cfg, duration=8.0)
    ks = list(range(K0 + 1, K0 + 41))
    return dict(cfg=cfg, init=seq.init_from_static(K0), imus=[seq.imu_between(k) for k in ks], grays=[seq.render(k) for k in ks])


def snapshot(h):
    p, q = h.pose()
    x, P = h.get_state()
    pts, hl = h.get_points()
    return dict(pose=np.concatenate((p, q)), x=x, P=P, pts=pts, hl=hl, tracks=h.get_tracks(), info=h.frame_info())


def same_snapshot(a, b):
    return (all(np.array_equal(a[k], b[k]) for k in ("pose", "x", "P", "pts", "hl")) and a["info"] == b["info"]
            and all(np.array_equal(u, v) for u, v in zip(a["tracks"], b["tracks"])))


def run_host(d, frames, fmt, switch=None):
    """frames through rvio_hip_frame (device detector) on a fresh handle; fmt None: a mono handle; switch: {frame index: format} changes on the way"""
    from rvio_amd import hip
    h = hip.RvioHip(d["cfg"])
    h.initialize(*d["init"])
    if fmt is not None:
        h.set_image_format(fmt)
    out = []
    for i, (img, imu) in enumerate(zip(frames, d["imus"])):
        if switch and i in switch:
            h.set_image_format(switch[i])
        h.frame(img.copy(), imu.copy(), None)            # temporaries: the call must have consumed them on return
        out.append(snapshot(h))
    h.close()
    return out


def run_dev(d, frames, fmt, pad):
    """the same through rvio_hip_frame_dev, flat out, from row-padded device buffers: the pose of every frame and the snapshot at the end"""
    from rvio_amd import hip
    bpp = abi.PIX_LAYOUT[fmt][0]
    H, W = d["cfg"].height, d["cfg"].width
    stride = W * bpp + pad
    bufs = []
    for i, f in enumerate(frames):
        buf = np.random.default_rng(i).integers(0, 256, (H, stride), dtype=np.uint8)
        buf[:, : W * bpp] = f.view(np.uint8).reshape(H, W * bpp)
        bufs.append(dev(buf))
    d_imus = [dev(i) for i in d["imus"]]
    h = hip.RvioHip(d["cfg"])
    h.initialize(*d["init"])
    h.set_image_format(fmt)
    poses = []
    for i in range(len(frames)):
        h.frame_dev(bufs[i].data_ptr(), stride, d_imus[i].data_ptr(), len(d["imus"][i]), 0, 0)
        p, q = h.pose()
        poses.append(np.concatenate((p, q)))
    h.sync()
    end = snapshot(h)
    h.close()
    return poses, end


def run_batch(d, frames_of, fmt, B, n, pad, ipad):
    """rvio_hip_frame_batch_dev, B instances with their own images, rows and instances padded: points and state of every instance at the end"""
    from rvio_amd import hip
    bpp = abi.PIX_LAYOUT[fmt][0]
    H, W = d["cfg"].height, d["cfg"].width
    stride = W * bpp + pad
    img_stride = stride * H + ipad
    h = hip.RvioHip(d["cfg"], batch=B, front_end=True)
    h.initialize(*d["init"])
    h.set_image_format(fmt)
    keep = []
    for f in range(n):
        buf = np.random.default_rng(f).integers(0, 256, B * img_stride, dtype=np.uint8)
        for i in range(B):
            rows = buf[i * img_stride: i * img_stride + H * stride].reshape(H, stride)
            rows[:, : W * bpp] = frames_of(f, i).view(np.uint8).reshape(H, W * bpp)
        d_img, d_imu = dev(buf), dev(d["imus"][f])
        keep += [d_img, d_imu]
        h.frame_batch_dev(d_img.data_ptr(), stride, img_stride, d_imu.data_ptr(), 0, len(d["imus"][f]))
    h.sync()
    ends = [(h.get_points_at(i), h.get_state_at(i)) for i in range(B)]
    h.close()
    return ends


@pytest.mark.parametrize("enc", ["mono16", "bayer_rggb8", "bayer_grbg16"])
def test_raw_sequence_equals_the_mono_sequence(gpu_required, seq40, enc):
    """40 pipelined frames through rvio_hip_frame (host buffers), rvio_hip_frame_dev (padded device buffers: the wide form) and a batch handle of
    three instances (odd / 2-aligned paddings: the plain form), each against mono handles fed the NumPy gray"""
    d, fmt = seq40, ENC[enc]
    raws = [raw_frame(enc, g, 1000 + i) for i, g in enumerate(d["grays"])]
    grays = [M.to_gray(r, enc) for r in raws]
    if enc == "mono16":
        assert all(np.array_equal(a, b) for a, b in zip(grays, d["grays"]))      # g * 257 + low-byte noise rounds back to g
    want = run_host(d, grays, None)
    got = run_host(d, raws, fmt)
    assert len(got) == len(want) == 40
    for k, (u, v) in enumerate(zip(got, want)):
        assert same_snapshot(u, v), (enc, "frame", k, u["info"], v["info"])
    assert sum(u["info"]["updated"] == 1 for u in got) >= 5 and got[-1]["info"]["device_error"] == 0
    poses, end = run_dev(d, raws, fmt, 8)
    bad = [k for k in range(40) if not np.array_equal(poses[k], want[k]["pose"])]
    assert not bad, (enc, "frame_dev: first differing frame", bad[0])
    assert same_snapshot(end, want[-1]), (enc, "frame_dev", end["info"], want[-1]["info"])
    B = 3
    cache = {}

    def raw_of(f, i):
        if (f, i) not in cache:
            cache[f, i] = raw_frame(enc, d["grays"][f], 50 * i + f, inst=i)
        return cache[f, i]
    a = run_batch(d, raw_of, fmt, B, 40, 6 if fmt & 16 else 3, 38 if fmt & 16 else 37)
    b = run_batch(d, lambda f, i: M.to_gray(raw_of(f, i), enc), abi.RVIO_PIX_MONO8, B, 40, 0, 0)
    for i in range(B):
        (pa, sa), (pb, sb) = a[i], b[i]
        assert len(pa[0]) > 20 and np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1]), (enc, i)
        assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]), (enc, i)
    if enc != "mono16":
        assert not np.array_equal(a[0][0][0], a[1][0][0])     # the tints really give different streams


def test_format_switch_in_mid_sequence(gpu_required, seq40):
    """10 mono frames, then 10 mono16, then 10 bayer_bggr8 on one handle = 30 mono frames (the staging is laid out again, nothing else moves)"""
    d = dict(seq40, imus=seq40["imus"][:30])
    encs = ["mono8"] * 10 + ["mono16"] * 10 + ["bayer_bggr8"] * 10
    raws = [g if e == "mono8" else raw_frame(e, g, 2000 + i) for i, (e, g) in enumerate(zip(encs, seq40["grays"][:30]))]
    grays = [M.to_gray(r, e) for r, e in zip(raws, encs)]
    got = run_host(d, raws, None, switch={10: ENC["mono16"], 20: ENC["bayer_bggr8"]})
    want = run_host(d, grays, None)
    assert len(got) == 30
    for k, (u, v) in enumerate(zip(got, want)):
        assert same_snapshot(u, v), k


# ------------------------------------------------------------------ refusals and the timing hook
def test_refusals(gpu_required, seq40):
    from rvio_amd import hip
    import torch
    d = seq40
    cfg = d["cfg"]
    W, H = cfg.width, cfg.height
    h = hip.RvioHip(cfg)
    L = h.L
    vp, up = C.c_void_p, C.POINTER(C.c_ubyte)
    for bad in (21, 36, 52, 64, 15, 31, 47, 63, 128 + 16, -16):        # bit patterns outside the table
        assert L.rvio_hip_set_image_format(h.h, bad) == -1, bad
    assert h.image_format() == abi.RVIO_PIX_MONO8
    h.initialize(*d["init"])
    imu = np.ascontiguousarray(d["imus"][0])
    ip, m = imu.ctypes.data_as(C.POINTER(abi.rvio_imu)), len(imu)
    d_imu = dev(imu)
    d_buf = torch.zeros(W * H * 8 + 64, dtype=torch.uint8, device="cuda")
    host = np.zeros(W * H * 8 + 64, np.uint8)
    torch.cuda.synchronize()

    def every_entry_point(ptr_off, stride):
        dp, hp = vp(d_buf.data_ptr() + ptr_off), C.cast(host.ctypes.data, up)
        return [L.rvio_hip_frame_dev(h.h, dp, stride, vp(d_imu.data_ptr()), m, None, 0),
                L.rvio_hip_track_dev(h.h, dp, stride, vp(d_imu.data_ptr()), m, None, 0),
                L.rvio_hip_frame_begin_dev(h.h, dp, stride, vp(d_imu.data_ptr()), m, None, 0),
                L.rvio_hip_frame_sharded_dev(h.h, dp, stride, vp(d_imu.data_ptr()), m, None, 0, 0, 1, None, None)] + \
               ([] if ptr_off else [L.rvio_hip_frame(h.h, hp, stride, ip, m, None, 0), L.rvio_hip_track(h.h, hp, stride, ip, m, None, 0)])

    for enc in ("mono16", "rgba16", "bayer_gbrg8", "bayer_rggb16"):
        bpp = abi.PIX_LAYOUT[ENC[enc]][0]
        h.set_image_format(ENC[enc])
        assert every_entry_point(0, W * bpp - 1) == [-1] * 6, enc                     # a short stride
        if ENC[enc] & 16:
            assert every_entry_point(0, W * bpp + 1) == [-1] * 6, enc                 # an odd stride
            assert b"even" in L.rvio_hip_last_error(h.h)
            assert every_entry_point(1, W * bpp + 2) == [-1] * 4, enc                 # an odd device address
            assert b"even" in L.rvio_hip_last_error(h.h)
        h.frame_dev(d_buf.data_ptr(), W * bpp, d_imu.data_ptr(), m, 0, 0)             # the exact stride is fine
    h.close()
    hb = hip.RvioHip(cfg, batch=2, front_end=True)
    hb.set_image_format(abi.RVIO_PIX_MONO16)
    bd = lambda stride, ist: L.rvio_hip_frame_batch_dev(hb.h, vp(d_buf.data_ptr()), stride, C.c_size_t(ist), vp(d_imu.data_ptr()), 0, m)
    assert bd(W * 2 - 2, W * 2 * H) == -1                                             # short
    assert bd(W * 2 + 1, (W * 2 + 1) * H + 1) == -1                                   # odd row stride
    assert bd(W * 2, W * 2 * H + 1) == -1                                             # odd instance stride
    hb.close()
    hf = hip.RvioHip(cfg, batch=2, front_end=False)                                   # filter only: it takes no image
    for v in sorted(ENC.values()):
        assert L.rvio_hip_set_image_format(hf.h, v) == (0 if v == 0 else -3), v
    assert L.rvio_hip_set_image_format(hf.h, 36) == -1
    hf.close()


def test_the_timing_hook_times_the_conversion_the_frame_launched(gpu_required, seq40):
    from rvio_amd import hip
    d = seq40
    cfg = d["cfg"]
    h = hip.RvioHip(cfg)
    us = C.c_float(0)
    assert h.L.rvio_hip_debug_time_kernel(h.h, 11, 5, C.byref(us)) == -3                # RVIO_ERR_UNSUPPORTED on a MONO8 handle
    h.initialize(*d["init"])
    for enc in ("mono16", "rgb16", "bayer_grbg8", "bayer_bggr16"):
        h.set_image_format(ENC[enc])
        assert h.L.rvio_hip_debug_time_kernel(h.h, 11, 5, C.byref(us)) == -3            # no image of this format has been handed over yet
        h.frame(random_raw(cfg.height, cfg.width, enc, 5), d["imus"][0], None)
        for iters in (1, 20):
            t = h.time_kernel(11, iters)
            assert t > 0 and math.isfinite(t), (enc, t)
    h.set_image_format(abi.RVIO_PIX_MONO8)
    assert h.L.rvio_hip_debug_time_kernel(h.h, 11, 5, C.byref(us)) == -3
    h.close()
