"""What the odometry ring costs and what it saves (rvio_hip_set_odometry: odom_kernel behind every augment/compose stage), measured on warmed
handles, the legs of a comparison alternating window by window inside one process (other people's work shares the host); every window ends
in rvio_hip_sync; medians with their spread:

  a  cfg B single stream, rvio_hip_frame_dev on resident frames: ring off / ring on (capacity 256) / ring off with rvio_hip_get_pose behind
     every frame — the third is what a host that wants the pose file did: it prices the per-frame drain the ring removes
  b  a filter-only batch handle (rvio_hip_frame_tracks_dev, the hand-over tables of bench.py's batched_filter leg) at that leg's largest
     batch: filter frames/s with the ring off and on
  c  B = 128: one rvio_hip_get_odometry_all against 128 rvio_hip_get_state_at calls (host clock, the handle idle)
  d  odom_kernel alone (rvio_hip_debug_time_kernel(12), HIP events), one instance and the batch of leg b

  python tools/odometry_cost.py [--repeats 3] [--window 70] [--batch 2048] [--out FILE]      one JSON line (also appended to FILE)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v, nd=2):
    v = np.asarray(v, float)
    return dict(median=round(float(np.median(v)), nd), min=round(float(v.min()), nd), max=round(float(v.max()), nd), runs=[round(float(x), nd) for x in v])


def leg_a(repeats, K, warm=40):
    import torch
    import bench
    from rvio_amd import abi, hip
    cfg = abi.config_named("B")
    W, H = cfg.width, cfg.height
    legs = ("ring_off", "ring_on_256", "ring_off_get_pose_every_frame")
    n_steps = warm + repeats * len(legs) * K + 8
    n_res = bench.resident_frames(n_steps + 1)
    assert n_res > n_steps, "the resident sequence must cover the run (no seam inside a window)"
    seq, imgs, imu_arr, imu_cnt, _, _ = bench.build_inputs(cfg, n_res, workers=bench.render_workers(n_res))
    d_img = torch.from_numpy(imgs).cuda()
    d_imu = torch.from_numpy(imu_arr.view(np.uint8).reshape(n_res, -1)).cuda()
    torch.cuda.synchronize()
    msb = int(d_imu.shape[1])
    h = hip.RvioHip(cfg)
    h.set_odometry(256)
    h.set_odometry(0)
    h.initialize(*seq.init_from_static(bench.K0))
    step = 0

    def frame(leg):
        nonlocal step
        i, m = step, int(imu_cnt[step])
        step += 1
        h.frame_dev(d_img.data_ptr() + i * W * H, W, d_imu.data_ptr() + i * msb, m, 0, 0)
        if leg == "ring_off_get_pose_every_frame":
            h.pose()

    def select(leg):
        h.set_odometry(256 if leg == "ring_on_256" else 0)

    for leg in legs:
        select(leg)
        for _ in range(warm // len(legs)):
            frame(leg)
    h.sync()
    us = {leg: [] for leg in legs}
    for rep in range(repeats):
        for leg in legs:
            select(leg)
            h.sync()
            t0 = time.perf_counter()
            for _ in range(K):
                frame(leg)
            h.sync()
            us[leg].append(1e6 * (time.perf_counter() - t0) / K)
    select("ring_on_256")
    frame("ring_on_256")
    kern = spread([h.time_kernel(12, 200) for _ in range(5)])
    n_ring = len(h.odometry())
    info = h.frame_info()
    h.close()
    return dict(cfg="B", window_frames=K, repeats=repeats, device_error=info["device_error"], records_in_ring=n_ring,
                us_per_frame={leg: spread(v) for leg, v in us.items()}), kern


def filter_tables(cfg, nf, seeds=4):
    """the hand-over tables of `seeds` direct-track sequences run through plain handles, as bench.py's batched_filter leg builds them"""
    import bench
    from rvio_amd import abi, hip
    rv = bench.rv
    Fu, ML, k0 = abi.fu(cfg), cfg.max_track_len, bench.K0
    tabs, inits = [], []
    for sd in range(seeds):
        seq = rv.synth.SynthSequence(cfg, duration=(k0 + nf + 3) / 20.0 + 1.0, seed=sd)
        h = hip.RvioHip(cfg)
        h.initialize(*seq.init_from_static(k0))
        inits.append(h.get_state())
        drv = rv.synth.DirectTrackDriver(seq)
        n_feat, types, lens = np.zeros(nf, np.int32), np.zeros((nf, Fu), np.uint8), np.zeros((nf, Fu), np.int32)
        meas = np.zeros((nf, Fu, ML, 2), np.float32)
        imus = []
        for f in range(nf):
            inp = drv.inputs(k0 + 1 + f)
            h.frame_points(inp["tracked"], inp["status"], inp["imu"], inp["cand"])
            t, l, me = h.get_tracks()
            drv.after(h.get_points()[0])
            n_feat[f] = len(l)
            types[f, : len(l)], lens[f, : len(l)], meas[f, : len(l)] = t, l, me
            imus.append(inp["imu"])
        h.close()
        m = min(len(i) for i in imus)
        tabs.append((n_feat, types, lens, meas, np.stack([i[:m] for i in imus]), m))
    return tabs, inits


def batch_handle(cfg, torch, tabs, inits, B, nf):
    from rvio_amd import hip
    seeds = len(tabs)
    m = min(t[5] for t in tabs)
    idx = np.arange(B) % seeds
    d = [torch.from_numpy(np.stack([tabs[i][k][:nf] for i in idx], 1).copy()).cuda() for k in range(4)]
    imu_h = np.stack([tabs[i][4][:nf, :m] for i in idx], 1).copy()
    d_im = torch.from_numpy(imu_h.view(np.uint8).reshape(nf, B, -1)).cuda()
    h = hip.RvioHip(cfg, batch=B)
    h.set_state(*inits[0])
    for b in range(B):
        if idx[b]:
            h.set_state_at(b, *inits[idx[b]])
    torch.cuda.synchronize()

    def frame(f):
        h.frame_tracks_dev(d_im[f].data_ptr(), m, m, d[0][f].data_ptr(), d[1][f].data_ptr(), d[2][f].data_ptr(), d[3][f].data_ptr())
    return h, frame, (d, d_im)


def leg_b(tabs, inits, B, repeats, K, warm):
    import torch
    from rvio_amd import abi
    cfg = abi.config_named("B", enable_equalizer=0)
    nf = warm + 2 * repeats * K
    h, frame, keep = batch_handle(cfg, torch, tabs, inits, B, nf)
    cap = 64
    h.set_odometry(cap)
    h.set_odometry(0)
    f = 0
    for _ in range(warm):
        frame(f)
        f += 1
    h.sync()
    fps = {"ring_off": [], "ring_on": []}
    for rep in range(repeats):
        for leg in ("ring_off", "ring_on"):
            h.set_odometry(cap if leg == "ring_on" else 0)
            h.sync()
            t0 = time.perf_counter()
            for _ in range(K):
                frame(f)
                f += 1
            h.sync()
            fps[leg].append(B * K / (time.perf_counter() - t0))
    h.set_odometry(cap)
    kern = spread([h.time_kernel(12, 100) for _ in range(5)])
    seqno, _ = h.odometry_all()
    h.close()
    return dict(instances=B, window_frames=K, repeats=repeats, ring_capacity=cap, newest_seq=seqno,
                filter_frames_per_s={k: spread(v, 0) for k, v in fps.items()}), kern


def leg_c(tabs, inits, repeats=5, B=128, frames=20):
    import torch
    from rvio_amd import abi
    cfg = abi.config_named("B", enable_equalizer=0)
    h, frame, keep = batch_handle(cfg, torch, tabs, inits, B, frames)
    h.set_odometry(16)
    for f in range(frames):
        frame(f)
    h.sync()
    h.odometry_all()
    h.get_state_at(0)
    us = {"one_get_odometry_all": [], "128_get_state_at": []}
    for rep in range(repeats):
        t0 = time.perf_counter()
        h.odometry_all()
        us["one_get_odometry_all"].append(1e6 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        for i in range(B):
            h.get_state_at(i)
        us["128_get_state_at"].append(1e6 * (time.perf_counter() - t0))
    n = int(h.odometry(instance=B - 1)["n_clones"][-1])
    h.close()
    return dict(instances=B, n_clones=n, bytes_odometry_all=B * 464, bytes_state_reads=B * 8 * ((26 + 7 * n) + (24 + 6 * n) ** 2), us={k: spread(v) for k, v in us.items()})


def run(repeats, K, B):
    import bench  # noqa: F401  (loads the package the way bench.py does: rvio_amd becomes importable)
    from rvio_amd import abi
    a, kern1 = leg_a(repeats, K)
    print("leg a done", file=sys.stderr, flush=True)
    cfg = abi.config_named("B", enable_equalizer=0)
    Kb, warm = 12, 16
    nf = warm + 2 * repeats * Kb
    tabs, inits = filter_tables(cfg, nf)
    print("tables built", file=sys.stderr, flush=True)
    b, kernB = leg_b(tabs, inits, B, repeats, Kb, warm)
    print("leg b done", file=sys.stderr, flush=True)
    c = leg_c(tabs, inits)
    return dict(a_single_stream=a, b_batched_filter=b, c_fleet_read=c, d_odom_kernel_us={"one_instance": kern1, "batch_%d" % B: kernB})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=int, default=70)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    line = json.dumps(run(a.repeats, a.window, a.batch))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
