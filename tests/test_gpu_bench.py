"""The driver's own bench command must produce its line (round 2's died of a GPU page fault inside a secondary leg and lost every number
of the round).  Runs bench.py in a child process exactly as the driver does and checks the contract fields."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _run(args, timeout=900):
    env = dict(os.environ)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip().startswith("{")]
    return r, lines


def test_the_drivers_bench_command_prints_its_line(gpu_required):
    r, lines = _run(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 20 and out["warmup"] == 5 and out["n_gpus"] == 1 and out["unit"] == "frames/s" and out["value"] > 0
    assert abs(out["ms_per_step"] * out["value"] - 1e3) < 1e-6 * 1e3
    for leg in ("host_buffers", "pose_latency_unpipelined", "multi_stream", "update_at_load", "batched_streams", "batched_filter"):
        assert leg in out and "error" not in out[leg], (leg, out.get(leg))
    rf = out["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and rf["achieved"] > 0 and rf["peak"] > 0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    hot = [o for o in out["roofline_other"] if "section 8(f)" not in o["kernel"]]
    assert "traffic" in rf and rf["avg_us"] > 0
    # the identity: the hot-path kernel with the largest average in the committed kernel trace of this configuration (round 6: the same kernel in every invocation) —
    # or, for a configuration without a committed trace, the slowest hot-path kernel timed live
    if "trace_avg_us" in rf:
        assert all("trace_avg_us" in o for o in hot) and rf["trace_avg_us"] >= max(o["trace_avg_us"] for o in hot)
        assert "klt_kernel3" in rf["kernel"]                                      # (what profiles/r06_kernel_stats_stream.md says for the stock configuration)
    else:
        assert rf["avg_us"] >= max(o["avg_us"] for o in hot)
    cb = out["cpu_baseline"]
    assert cb["value"] > 0 and cb["cores"] == 1 and cb["kind"] in ("port", "reference") and cb["sample"]
    par = out["parity"]
    assert par["frames"] >= 141 and par["max_state_delta"] <= 1e-6 and par["counters_equal_every_frame"] and par["rank_truncation_nrank_equal"]
    assert out["pose_latency_unpipelined"]["frames"] >= 8 and out["pose_latency_unpipelined"]["updated_last_frame"] == 1
    assert out["last_frame"]["device_error"] == 0


@pytest.mark.parametrize("steps,warmup", [(1, 0), (60, 2)])
def test_short_and_odd_step_counts_do_not_kill_the_line(gpu_required, steps, warmup):
    """(steps, warmup) the pose-latency plan cannot serve from the main sequence: the leg moves to the parity sequence instead of dying"""
    r, lines = _run(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--full", "--no-cpu", "--batch", "", "--batch-streams", "", "--no-streams"])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = json.loads(lines[-1])
    assert out["steps"] == steps and "error" not in out["pose_latency_unpipelined"], out["pose_latency_unpipelined"]


def test_forced_sharded_line_equals_the_single_gpu_updater(gpu_required):
    """bench.py --force-sharded: the sharded frame (rvio_hip_frame_sharded_dev: update_local -> the REAL ncclAllGather on the filter stream ->
    update_global, one C-ABI call per frame) at world 1 against the same frames through the unsharded updater: block sums in rank order, so
    the two agree to rounding — asserted, not just printed (it was null in round 2)."""
    r, lines = _run(["--gpus", "1", "--steps", "60", "--warmup", "5", "--force-sharded", "--full", "--no-cpu", "--batch", "", "--batch-streams", "", "--no-streams"])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = json.loads(lines[-1])
    assert "ncclAllGather" in out["config"]["parallelism"], out["config"]["parallelism"]
    assert out["last_frame"]["updated"] == 1 and out["last_frame"]["device_error"] == 0
    assert out["max_state_delta_sharded_vs_single_gpu"] is not None and out["max_state_delta_sharded_vs_single_gpu"] <= 1e-9, out["max_state_delta_sharded_vs_single_gpu"]


SECONDARY = ("host_buffers", "pose_latency_unpipelined", "multi_stream", "update_at_load", "batched_streams", "batched_filter", "roofline", "cpu_baseline",
             "parity", "latency_ms_p50", "independent_streams", "sharded_cfgE")


def _dump(d):
    import numpy as np
    arrs = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert all(f.endswith(".npy") for f in os.listdir(d)) and {"state", "covariance", "tracker_points"} <= set(arrs)
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values()) and sum(a.nbytes for a in arrs.values()) <= 64 << 20
    assert np.all(np.isfinite(arrs["state"])) and np.all(np.isfinite(arrs["covariance"]))
    return arrs


def test_a_plain_run_times_the_headline_only_and_dumps_the_same_outputs_every_time(gpu_required, tmp_path):
    """no --full: the contract keys and none of the secondary legs; --dump-outputs: two runs with the same arguments, the same arrays"""
    import numpy as np
    dumps = []
    for k in range(2):
        d = str(tmp_path / ("run%d" % k))
        r, lines = _run(["--gpus", "1", "--steps", "20", "--warmup", "5", "--dump-outputs", d])
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert len(lines) == 1, r.stdout.decode()[-2000:]
        out = json.loads(lines[0])
        assert out["steps"] == 20 and out["warmup"] == 5 and out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"]
        assert abs(out["ms_per_step"] * out["value"] - 1e3) < 1e-6 * 1e3 and out["last_frame"]["device_error"] == 0
        assert not [k_ for k_ in SECONDARY if k_ in out], out.keys()
        dumps.append(_dump(d))
        # the dump is the timed handle after its last step: its counters are the line's last_frame (frame_info.npy: the counters in key order)
        sys.path.insert(0, ROOT)
        import bench
        fi = dict(zip(sorted(bench.abi.rvio_frame_info().asdict()), dumps[-1]["frame_info"]))
        assert {k_: fi[k_] for k_ in out["last_frame"]} == out["last_frame"], (fi, out["last_frame"])
    assert dumps[0].keys() == dumps[1].keys()
    for name in dumps[0]:
        assert np.array_equal(dumps[0][name], dumps[1][name]), name


def test_a_run_longer_than_the_resident_sequence_goes_round_its_loop(gpu_required, tmp_path):
    """steps past the resident sequence replay its last trajectory period (bench.loop_frame): twice round it, the filter still tracks"""
    sys.path.insert(0, ROOT)
    import bench
    d = str(tmp_path / "dump")
    steps = bench.LOOP_FIRST + 2 * bench.LOOP_LEN + 10
    r, lines = _run(["--gpus", "1", "--steps", str(steps), "--warmup", "5", "--dump-outputs", d])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = json.loads(lines[-1])
    assert out["steps"] == steps and out["last_frame"]["device_error"] == 0, out["last_frame"]
    lf = out["last_frame"]
    assert lf["n_klt_ok"] >= 100 and lf["n_ransac_inliers"] >= 0.8 * lf["n_klt_ok"], lf      # (a healthy frame of this scene: ~170 tracked, ~all inliers)
    fi = dict(zip(sorted(bench.abi.rvio_frame_info().asdict()), _dump(d)["frame_info"]))
    assert {k_: fi[k_] for k_ in lf} == lf, (fi, lf)
