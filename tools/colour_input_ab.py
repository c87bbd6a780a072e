"""What colour camera input costs (rvio_hip_set_image_format: the gray conversion of Tracker.cc:182-196 on the device), measured on ONE warmed
handle at 752 x 480 cfg B, the legs alternating window by window inside one process (other people's work shares the host):

  a  rvio_hip_frame on RGB host frames (the colour bytes are staged, gray_kernel converts them)
  b  what the host did before: host/rvio_host.cpp's scalar to_gray on the frame (tools/colour_input_to_gray.cpp, timed where it runs) and then
     the mono rvio_hip_frame
  c  rvio_hip_frame_dev on resident frames, colour against mono
  d  gray_kernel alone (rvio_hip_debug_time_kernel(11), HIP events), wide and byte form, RGB and RGBA, beside the streaming bound: the bytes it
     must move over the MI355X's HBM bandwidth (6.29 TB/s measured for a float4 copy, 8.0 TB/s by the data sheet)

Every window is K frames that end in a synchronise; a change of format drains the handle outside the timed span.  The mono frames are the
NumPy gray of the colour frames, so every leg walks the same trajectory (the filter sees the same bits whichever leg hands a frame over).

  python tools/colour_input_ab.py [--repeats 3] [--window 70] [--out FILE]      one JSON line (also appended to FILE)
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12


def to_gray_helper():
    src = os.path.join(ROOT, "tools", "colour_input_to_gray.cpp")
    lib = os.path.join(ROOT, "tools", "libcolour_input_to_gray.so")
    deps = [src, os.path.join(ROOT, "host", "rvio_host.cpp"), os.path.join(ROOT, "host", "rvio_host.hpp")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in deps):
        libdir = os.path.join(ROOT, "r-vio_amd")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, os.path.join(ROOT, "host", "rvio_host.cpp"), "-o", lib,
                               "-L" + libdir, "-lrvio_hip", "-lz", "-Wl,-rpath," + libdir])
    L = C.CDLL(lib)
    L.colour_input_to_gray.restype = C.c_double
    L.colour_input_to_gray.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return L


def gray_np(c):
    return ((c[..., 0].astype(np.uint32) * 4899 + c[..., 1].astype(np.uint32) * 9617 + c[..., 2].astype(np.uint32) * 1868 + 8192) >> 14).astype(np.uint8)


def spread(v):
    v = np.asarray(v, float)
    return dict(median=round(float(np.median(v)), 2), min=round(float(v.min()), 2), max=round(float(v.max()), 2), runs=[round(float(x), 2) for x in v])


def run(repeats, K, warm=40):
    import torch
    import bench
    from rvio_amd import abi, hip
    cfg = abi.config_named("B")
    W, H = cfg.width, cfg.height
    legs = ("a_host_rgb", "b_host_to_gray_mono", "c_dev_rgb", "c_dev_mono")
    n_steps = warm + repeats * len(legs) * K + 8
    n_res = bench.resident_frames(n_steps + 1)
    assert n_res > n_steps, "the resident sequence must cover the run (no seam inside a window)"
    seq, imgs, imu_arr, imu_cnt, _, _ = bench.build_inputs(cfg, n_res, workers=bench.render_workers(n_res))
    col = np.empty((n_res, H, W, 3), np.uint8)               # R = min(255, 5g/4), G = g, B = 3g/4
    g16 = imgs.astype(np.uint16)
    col[..., 0], col[..., 1], col[..., 2] = np.minimum(255, g16 * 5 // 4), imgs, g16 * 3 // 4
    del g16
    mono = np.stack([gray_np(c) for c in col])
    helper = to_gray_helper()
    d_col, d_mono = torch.from_numpy(col).cuda(), torch.from_numpy(mono).cuda()
    d_imu = torch.from_numpy(imu_arr.view(np.uint8).reshape(n_res, -1)).cuda()
    torch.cuda.synchronize()
    msb = int(d_imu.shape[1])
    h = hip.RvioHip(cfg)
    h.initialize(*seq.init_from_static(bench.K0))
    scratch = np.empty((H, W), np.uint8)
    step = 0

    def frame(leg):
        nonlocal step
        i, m = step, int(imu_cnt[step])
        step += 1
        if leg == "a_host_rgb":
            h.frame(col[i], imu_arr[i, :m], None)
            return 0.0
        if leg == "b_host_to_gray_mono":
            dt = helper.colour_input_to_gray(col[i].ctypes.data, W, H, 3, 1, scratch.ctypes.data)
            h.frame(scratch, imu_arr[i, :m], None)
            return dt
        if leg == "c_dev_rgb":
            h.frame_dev(d_col.data_ptr() + i * W * H * 3, W * 3, d_imu.data_ptr() + i * msb, m, 0, 0)
        else:
            h.frame_dev(d_mono.data_ptr() + i * W * H, W, d_imu.data_ptr() + i * msb, m, 0, 0)
        return 0.0

    def fmt_of(leg):
        return abi.RVIO_PIX_RGB8 if leg in ("a_host_rgb", "c_dev_rgb") else abi.RVIO_PIX_MONO8

    for leg in legs:                                          # warm every leg: staging, pinned ring, code objects
        h.set_image_format(fmt_of(leg))
        for _ in range(warm // len(legs)):
            frame(leg)
    h.sync()
    us = {leg: [] for leg in legs}
    to_gray_us = []
    for rep in range(repeats):
        for leg in legs:
            h.set_image_format(fmt_of(leg))
            h.sync()
            t0 = time.perf_counter()
            tg = 0.0
            for _ in range(K):
                tg += frame(leg)
            h.sync()
            us[leg].append(1e6 * (time.perf_counter() - t0) / K)
            if leg == "b_host_to_gray_mono":
                to_gray_us.append(1e6 * tg / K)
    info = h.frame_info()
    # d: the kernel alone, on the frame a colour entry point was handed last
    kern = {}
    keep = []
    for name, ch, fmt in (("rgb", 3, abi.RVIO_PIX_RGB8), ("rgba", 4, abi.RVIO_PIX_RGBA8)):
        h.set_image_format(fmt)
        src = col[step] if ch == 3 else np.concatenate([col[step], col[step][..., :1]], axis=2)
        for form, pad in (("wide", 0), ("byte", 1)):
            stride = W * ch + pad
            buf = np.zeros((H, stride), np.uint8)
            buf[:, : W * ch] = src.reshape(H, -1)
            d_buf = torch.from_numpy(buf).cuda()
            keep.append(d_buf)
            torch.cuda.synchronize()
            h.frame_dev(d_buf.data_ptr(), stride, d_imu.data_ptr() + step * msb, int(imu_cnt[step]), 0, 0)
            step += 1
            runs = [h.time_kernel(11, 200) for _ in range(5)]
            nbytes = W * H * (ch + 1)
            kern["%s_%s" % (name, form)] = dict(us=spread(runs), bytes=nbytes, bound_us_at_6p29TBps=round(1e6 * nbytes / HBM_MEASURED, 3),
                                                bound_us_at_8TBps=round(1e6 * nbytes / HBM_SPEC, 3))
    h.close()
    return dict(cfg="B", width=W, height=H, window_frames=K, repeats=repeats, frames_per_leg=K * repeats, device_error=info["device_error"],
                us_per_frame={leg: spread(v) for leg, v in us.items()}, to_gray_us_per_frame=spread(to_gray_us), gray_kernel=kern)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=int, default=70)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    line = json.dumps(run(a.repeats, a.window))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
