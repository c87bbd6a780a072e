"""What the front end launches, for comparing two builds of the library launch by launch (profiles/front_forms_refactor.txt).

    rocprofv3 --kernel-trace --output-format rocpd -d OUT -- python tools/front_trace.py          (once per library: RVIO_HIP_LIB selects it)
    python tools/front_trace.py --list OUT/.../*_results.db > listing.txt                              (then cmp the two listings)

The driver walks every mode and kernel form of front_forms() (launch_plan.h) a handle can be put in: a plain handle with the device detector
(equaliser on and off), a caller-side corner list, the corner source switching every four frames, a colour format on resident frames with a
dword-aligned and an odd row stride (the dword and the byte form of gray_kernel), the throughput forms on one instance
(rvio_hip_debug_kernel_forms), batch handles with their front end at B = 3 and 8, and a window with 6n > 96 (one image chain, no pyramid poll).
Every handle is synchronised before the next one starts.  The listing holds, per kernel name, the sequence of (grid in work-items, workgroup,
dynamic LDS) in dispatch order, and the number of dispatches per queue in the order the queues first appear: two builds that launch the same
things give byte-identical listings."""
import hashlib
import os
import re
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def listing(path):
    db = sqlite3.connect(path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]

    def col(*parts):
        c = [c for c in cols if all(p in c.lower() for p in parts)]
        assert c, (parts, cols)
        return c[0]
    name = "name" if "name" in cols else col("name")
    grid, wg = [col("grid", a) for a in "xyz"], [col("workgroup", a) for a in "xyz"]
    lds = [c for c in cols if "lds" in c.lower() or "group_segment" in c.lower() or "shared" in c.lower()]
    queue = [c for c in cols if "queue" in c.lower()]
    assert lds and queue, cols
    rows = db.execute("select %s, start from kernels order by start" % ", ".join([name] + grid + wg + [lds[0], queue[0]])).fetchall()
    per, queues = {}, {}
    for r in rows:
        per.setdefault(re.sub(r"\(.*", "", r[0]), []).append(tuple(r[1:8]))
        queues[r[8]] = queues.get(r[8], 0) + 1
    out = ["%d dispatches of %d kernel names on %d queues" % (len(rows), len(per), len(queues)),
           "dispatches per queue, in the order the queues first appear: %s" % " ".join(str(n) for n in queues.values()),
           "kernel | dispatches | distinct (grid, workgroup, LDS) | md5 of the sequence"]
    for k in sorted(per):
        out.append("%s | %d | %d | %s" % (k, len(per[k]), len(set(per[k])), hashlib.md5(repr(per[k]).encode()).hexdigest()[:12]))
    return "\n".join(out)


def drive():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pkgload import load_pkg
    rv = load_pkg()
    from rvio_amd import abi, hip
    K0, N = 38, 12

    def inputs(cfg, n=N):
        seq = rv.synth.SynthSequence(cfg, duration=9.0)
        ks = list(range(K0 + 1, K0 + 1 + n))
        cands = []
        for k in ks:
            xy, vis = seq.project(k, noise=False)
            cands.append(seq.candidates(k, xy, vis)[0].astype(np.float32))
        return seq, [seq.render(k) for k in ks], [seq.imu_between(k) for k in ks], cands

    def run(cfg, data, detector, fmt=None, pad=0, throughput=None):
        seq, imgs, imus, cands = data
        h = hip.RvioHip(cfg)
        h.initialize(*seq.init_from_static(K0))
        if throughput is not None:
            h.kernel_forms(throughput)
        if fmt is not None:
            h.set_image_format(fmt)
        keep = []
        for i, (img, imu, cand) in enumerate(zip(imgs, imus, cands)):
            if fmt is not None:
                # the gray image in every channel, rows padded by `pad` bytes, as a RESIDENT frame: rvio_hip_frame would repack the rows into its staging
                # (always dword-aligned at this width), rvio_hip_frame_dev reads the caller's buffer with the caller's stride
                buf = np.zeros((img.shape[0], img.shape[1] * 3 + pad), np.uint8)
                buf[:, :img.shape[1] * 3] = np.repeat(img, 3, axis=1)
                d_img, d_imu = torch.from_numpy(buf).cuda(), torch.from_numpy(np.ascontiguousarray(imu).view(np.uint8)).cuda()
                keep += [d_img, d_imu]
                torch.cuda.synchronize()
                h.frame_dev(d_img.data_ptr(), buf.shape[1], d_imu.data_ptr(), len(imu), 0, 0)
            else:
                h.frame(img, imu, None if detector(i) else cand)
        h.sync()
        if fmt is None and throughput is None and any(detector(i) for i in range(len(imgs))):   # the timing hook's launches of KLT, cornerSubPix and the selection kernel
            h.time_kernel(1, 2), h.time_kernel(6, 2), h.time_kernel(9, 2)
        if fmt is not None:
            h.time_kernel(11, 2)
        h.close()

    small = dict(n_features=40, max_track_len=4)
    for eq in (1, 0):
        cfg = abi.config_named("B", enable_equalizer=eq, **small)
        data = inputs(cfg)
        run(cfg, data, lambda i: True)                    # the device detector: run-ahead, device-side counters
        run(cfg, data, lambda i: False)                   # a caller-side corner list
        run(cfg, data, lambda i: (i // 4) % 2 == 0)       # detector, list, detector, ... every four frames
    cfg = abi.config_named("B", enable_equalizer=1, **small)
    data = inputs(cfg)
    run(cfg, data, lambda i: True, fmt=abi.RVIO_PIX_RGB8, pad=4)     # dword-aligned rows: the wide gray form
    run(cfg, data, lambda i: True, fmt=abi.RVIO_PIX_RGB8, pad=3)     # odd rows: the byte form
    run(cfg, data, lambda i: True, throughput=1)                     # the throughput forms of the image kernels on one instance
    run(cfg, data, lambda i: False, throughput=1)
    cfg = abi.config_named("B", enable_equalizer=1, n_features=40, max_track_len=18)   # 6n = 102: one image chain, no pyramid poll
    run(cfg, inputs(cfg), lambda i: True)
    cfg = abi.config_named("B", enable_equalizer=1, **small)
    seq, imgs, imus, _ = inputs(cfg, 8)
    for B in (3, 8):                                                 # batch handles with their front end: events, no counters; B = 8: throughput forms
        h = hip.RvioHip(cfg, batch=B, front_end=True)
        h.initialize(*seq.init_from_static(K0))
        x0, P0 = h.get_state_at(0)
        for i in range(1, B):
            h.set_state_at(i, x0, P0)
        for img, imu in zip(imgs, imus):
            d_img = torch.from_numpy(np.stack([img] * B)).cuda()
            d_imu = torch.from_numpy(np.ascontiguousarray(imu).view(np.uint8)).cuda()
            torch.cuda.synchronize()
            h.frame_batch_dev(d_img.data_ptr(), cfg.width, cfg.width * cfg.height, d_imu.data_ptr(), 0, len(imu))
            h.sync()
        h.close()
    print("FRONT_TRACE_DONE")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--list":
        print(listing(sys.argv[2]))
    else:
        drive()
