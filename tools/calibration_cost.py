"""What per-instance calibration costs (rvio_hip_set_calibration*: the calibrated kernels read their constants through cam_of(), from the
kernel arguments or from a table of one entry per instance), measured against the PARENT commit's library.  Three steps, each a sub-command:

  resources   on any machine: the touched kernels of two tables written by tools/kernel_resources.py (run once in a checkout of the parent, once
              here) side by side — VGPRs, SGPRs, scratch, instructions — and the check that no touched kernel gained scratch bytes
                python tools/calibration_cost.py resources --parent PARENT.md --this THIS.md --out res.json
  time        on the MI355X: bench.py's headline and its batched_streams / batched_filter legs, one fresh process per run, the variants
              ALTERNATING run by run inside one call (other people's work shares the box): `parent` (the parent's library, through
              RVIO_HIP_LIB), `this` (this build, no setter called: no table) and `this_table` (this build, every batch handle bound to a table of
              identical entries, the config's own calibration: what the indexed path costs, the arithmetic unchanged)
                python tools/calibration_cost.py time --parent-lib PATH/librvio_hip.so [--repeats 3] --out time.json
  report      profiles/calibration.md from the two results; --kernel-stats A.csv B.csv adds which kernel carries a difference: the kernel_stats
              tables of two `rocprofv3 --kernel-trace --stats --output-format csv` runs (each a run of its own) of bench.py's batched_filter
              leg, without and with a table of identical entries
                python tools/calibration_cost.py report --resources res.json --time time.json [--kernel-stats A.csv B.csv] [--out profiles/calibration.md]
"""
import argparse
import contextlib
import io
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOUCHED = ("ransac_kernel", "ransac_book_a_kernel", "ransac_book_kernel", "bookkeep_b_kernel", "feat_build_kernel<16>", "feat_build_kernel<4>",
           "feat_prop_kernel", "geom4_kernel", "landmark_kernel")
VARIANTS = ("parent", "this", "this_table")
LEGS = ("headline_frames_per_s", "batched_streams_frames_per_s", "batched_filter_frames_per_s")


def spread(v, nd=1):
    v = np.asarray(v, float)
    return dict(median=round(float(np.median(v)), nd), min=round(float(v.min()), nd), max=round(float(v.max()), nd), runs=[round(float(x), nd) for x in v])


# ---------------------------------------------------------------- resources
def read_table(path):
    rows = {}
    for ln in open(path):
        m = re.match(r"\| `([^`]+)` \| (\d+) \| (\d+) \| (\d+) \| (\d+) \| (\d+) \| (\d+) \| (\d+) \|", ln)
        if m:
            rows[m.group(1)] = dict(zip(("vgprs", "sgprs", "static_lds", "scratch", "instructions", "mfma_f64", "waves_per_simd"), map(int, m.groups()[1:])))
    return rows


def resources(a):
    par, new = read_table(a.parent), read_table(a.this)
    out, gained = {}, []
    for k in TOUCHED:
        assert k in par and k in new, k
        out[k] = dict(parent=par[k], this=new[k])
        if new[k]["scratch"] > par[k]["scratch"]:
            gained.append(k)
    untouched_moved = sorted(k for k in new if k not in TOUCHED and k in par and new[k] != par[k])
    res = dict(kernels=out, scratch_gained=gained, other_kernels_that_differ=untouched_moved, kernels_in_build=len(new))
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(dict(scratch_gained=gained, other_kernels_that_differ=untouched_moved)))
    if gained:
        raise SystemExit("scratch gained: %s" % gained)


# ---------------------------------------------------------------- time: one run of one variant (a process of its own)
def child(a):
    import bench
    import torch
    from rvio_amd import abi, hip
    if a.table:   # every batch handle computes through a table of identical entries
        init = hip.RvioHip.__init__

        def init_with_table(self, cfg, device=0, batch=None, front_end=False):
            init(self, cfg, device=device, batch=batch, front_end=front_end)
            if batch is not None:
                self.set_calibrations([abi.calibration_from_config(cfg)] * self.batch)
        hip.RvioHip.__init__ = init_with_table
    argv, sys.argv = sys.argv, ["bench.py", "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup), "--no-cpu", "--no-latency"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        bench.main()
    sys.argv = argv
    head = json.loads(buf.getvalue().strip().splitlines()[-1])
    cfg = abi.config_named("B")
    st = bench.batched_streams_leg(cfg, torch, [a.streams], name="B")["sizes"][0]
    fl = bench.batched_filter_leg(cfg, torch, [str(a.batch)], name="B")["sizes"][0]
    assert st["finite"] and fl["finite"]
    print(json.dumps(dict(headline_frames_per_s=head["value"], batched_streams_frames_per_s=st["frames_per_s"], batched_filter_frames_per_s=fl["filter_frames_per_s"],
                          streams=a.streams, instances=a.batch, steps=a.steps, warmup=a.warmup)), flush=True)


def time_all(a):
    assert os.path.exists(a.parent_lib), a.parent_lib
    runs = {v: [] for v in VARIANTS}
    for rep in range(a.repeats):
        for v in VARIANTS:
            env = dict(os.environ)
            if v == "parent":
                env["RVIO_HIP_LIB"] = os.path.abspath(a.parent_lib)
            else:
                env.pop("RVIO_HIP_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "child", "--steps", str(a.steps), "--warmup", str(a.warmup), "--streams", str(a.streams),
                   "--batch", str(a.batch)] + (["--table"] if v == "this_table" else [])
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.run_timeout, cwd=ROOT)
            if r.returncode != 0:   # nothing more is started on the GPU after a run that failed
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit("run %d of %s ended with status %d" % (rep, v, r.returncode))
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            runs[v].append(rec)
            print(rep, v, json.dumps(rec), flush=True)
            res = dict(repeats=rep + 1, runs=runs, summary={v2: {leg: spread([x[leg] for x in runs[v2]]) for leg in LEGS} for v2 in VARIANTS if runs[v2]})
            json.dump(res, open(a.out, "w"), indent=1)


# ---------------------------------------------------------------- report
def report(a):
    res, tm = json.load(open(a.resources)), (json.load(open(a.time)) if a.time and os.path.exists(a.time) else None)
    L = ["# What per-instance calibration costs (`tools/calibration_cost.py`)", "",
         "The calibrated kernels read `Ric, Rci, tic, tci, fx .. k3, fisheye` through `cam_of(cfg, cal, z)` (`csrc/rvio_dev.h`): from the kernel arguments "
         "when no setter was ever called (`cal == nullptr`), else from entry `blockIdx.z` of a table outside the filter slab — scalar loads either way.", "",
         "## Resources of the touched kernels (parent -> this build; `tools/kernel_resources.py` on both code objects)", "",
         "| kernel | VGPRs | SGPRs | scratch (B) | instructions | waves / SIMD by registers |", "|---|---|---|---|---|---|"]
    for k in TOUCHED:
        p, n = res["kernels"][k]["parent"], res["kernels"][k]["this"]
        L.append("| `%s` | %d -> %d | %d -> %d | %d -> %d | %d -> %d | %d -> %d |" % (k, p["vgprs"], n["vgprs"], p["sgprs"], n["sgprs"], p["scratch"], n["scratch"],
                                                                                  p["instructions"], n["instructions"], p["waves_per_simd"], n["waves_per_simd"]))
    L += ["", "Touched kernels that gained scratch bytes: %s.  Other kernels whose row differs from the parent's: %s."
          % (", ".join(res["scratch_gained"]) or "none", ", ".join("`%s`" % k for k in res["other_kernels_that_differ"]) or "none"), ""]
    if tm:
        one = tm["runs"]["parent"][0]
        L += ["## Time on the MI355X (frames/s, higher is better)", "",
              "`bench.py --gpus 1 --steps %d --warmup %d` headline, `batched_streams` at %d streams and `batched_filter` at %d instances; %d runs per variant, "
              "each a fresh process, the variants alternating run by run in one call.  `this_table`: every batch handle bound to a table of identical "
              "entries (the headline is a plain handle: no table there)." % (one["steps"], one["warmup"], one["streams"], one["instances"], tm["repeats"]), "",
              "| leg | parent: median [min .. max] | this build, no table | this build, table of identical entries |", "|---|---|---|---|"]
        for leg in LEGS:
            cells = []
            for v in VARIANTS:
                s = tm["summary"][v][leg]
                cells.append("%.0f [%.0f .. %.0f]" % (s["median"], s["min"], s["max"]))
            L.append("| %s | %s |" % (leg.replace("_frames_per_s", ""), " | ".join(cells)))
        L.append("")
        verdict = []
        for leg in LEGS:
            p = tm["summary"]["parent"][leg]
            for v in VARIANTS[1:]:
                if leg == LEGS[0] and v == "this_table":
                    continue
                s = tm["summary"][v][leg]
                inside = p["min"] <= s["median"] <= p["max"]
                verdict.append("%s / %s: median %s the parent's spread (%+.1f %% against the parent's median)"
                               % (leg.replace("_frames_per_s", ""), v, "inside" if inside else ("ABOVE" if s["median"] > p["max"] else "BELOW"),
                                  100.0 * (s["median"] / p["median"] - 1.0)))
        L += ["- " + v for v in verdict] + [""]
    if a.kernel_stats:
        import csv

        def stats(path):
            return {r["Name"].split("(")[0].replace("void ", ""): (int(r["Calls"]), int(r["TotalDurationNs"])) for r in csv.DictReader(open(path))}
        s0, s1 = stats(a.kernel_stats[0]), stats(a.kernel_stats[1])
        L += ["## Which kernel carries the table's cost (`batched_filter` at 2048 instances under `rocprofv3 --kernel-trace --stats`, a run of its own each)", "",
              "Total device time of the batch handle's kernels over the leg's 56 frames, without a table -> with a table of identical entries (kernels of "
              "more than 1 % of the leg; the other rows of the tables are the plain handles that build the leg's inputs):", "",
              "| kernel | launches | total us, no table | total us, table | difference |", "|---|---|---|---|---|"]
        batch = [k for k in s0 if k in s1 and s0[k][0] in (52, 56) and not k.startswith("__amd")]
        whole = sum(s0[k][1] for k in batch)
        for k in sorted(batch, key=lambda k: -s0[k][1]):
            if s0[k][1] >= 0.01 * whole:
                L.append("| `%s` | %d | %.0f | %.0f | %+.0f us (%+.1f %%) |" % (k, s0[k][0], s0[k][1] / 1e3, s1[k][1] / 1e3, (s1[k][1] - s0[k][1]) / 1e3,
                                                                            100.0 * (s1[k][1] / s0[k][1] - 1.0)))
        L += ["", "Sum over these kernels: %.0f -> %.0f us (%+.1f %%)." % (whole / 1e3, sum(s1[k][1] for k in batch) / 1e3,
                                                                       100.0 * (sum(s1[k][1] for k in batch) / whole - 1.0)), ""]
        L += ["`geom4_kernel` and `feat_build_kernel<4>` are the two kernels of a filter-only batch handle that read calibration.  `propagate_kernel3b` reads none: "
              "in this leg it runs on the handle's second stream BESIDE the per-feature launch (`rvio_hip_frame_tracks_dev`), the two share the chip, and the "
              "duration a trace gives it moves with its neighbour's; the frame waits for the longer of the two.", ""]
    open(a.out, "w").write("\n".join(L))
    print(a.out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("resources")
    p.add_argument("--parent", required=True)
    p.add_argument("--this", required=True)
    p.add_argument("--out", required=True)
    for name in ("time", "child"):
        p = sub.add_parser(name)
        p.add_argument("--steps", type=int, default=200)
        p.add_argument("--warmup", type=int, default=40)
        p.add_argument("--streams", type=int, default=128)
        p.add_argument("--batch", type=int, default=2048)
        if name == "time":
            p.add_argument("--parent-lib", required=True)
            p.add_argument("--repeats", type=int, default=3)
            p.add_argument("--run-timeout", type=int, default=300)
            p.add_argument("--out", required=True)
        else:
            p.add_argument("--table", action="store_true")
    p = sub.add_parser("report")
    p.add_argument("--resources", required=True)
    p.add_argument("--time", default=None)
    p.add_argument("--kernel-stats", nargs=2, default=None, metavar=("NO_TABLE.csv", "TABLE.csv"))
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibration.md"))
    a = ap.parse_args()
    {"resources": resources, "time": time_all, "child": child, "report": report}[a.cmd](a)
