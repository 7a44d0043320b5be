"""bench.py rehearsals on one GPU: the N=1 line, and world 2 (torch.distributed
.run, gloo for the barriers/collectives, both ranks on device 0) in strong
mode -- n_ranks_seen, the weak line measured beside it, the timed
north-star collective, and the strong shards concatenated in rank order equal
one projection of the global batch bit for bit."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out[-3000:]
    return json.loads(lines[0])


def test_bench_single_gpu_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps",
                        "3", "--warmup", "1", "--points", "300000", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _line(r.stdout)
    assert d["n_gpus"] == 1 and d["n_ranks_seen"] == 1 and d["scaling"] == "weak"
    assert d["value"] > 0 and 0 < d["roofline"]["frac"] < 1.0
    assert d["collective"]["global_n_valid"] > 0.99 * 300000
    assert "traffic_source" in d["roofline"]
    assert d["config4"]["points_total"] == 50_000_000 and d["config4"]["value"] > 0
    # the one-pass round trip and the twelve-launch form it replaces, both timed
    assert 0 < d["config4"]["ms_per_step"] and 0 < d["config4"]["ms_per_step_two_calls"]
    assert d["config5"]["correspondences_total"] == 92_935_075
    assert d["config5"]["final_mean_px"] < 0.01


def test_bench_plain_line_and_dump(tmp_path):
    """without --full the run ends with its timed steps: the headline fields
    and nothing measured beside them; --dump-outputs writes the last step's
    outputs, which equal bit for bit a projection of the same seeded points
    in this process (so the inputs are the same from process to process)"""
    import numpy as np
    import torch

    import bench
    from apex_camera_models import KannalaBrandtModel, samples
    n = 300_000  # over bench.DUMP_MAX_POINTS: the sampled form
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        "2", "--warmup", "1", "--points", str(n), "--dump-outputs",
                        str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _line(r.stdout)
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["dtype"] == "f64"
    assert d["unit"] == "Mpoints/s" and d["higher_is_better"] is True
    assert abs(d["value"] - n / d["ms_per_step"] / 1e3) <= 1e-3 * d["value"]
    assert 0 < d["roofline"]["frac"] < 1.0 and d["roofline"]["traffic"] is None
    for key in ("collective", "config4", "config5", "cpu_baseline", "cpu_baseline_o2",
                "cpu_baseline_all_cores"):
        assert key not in d, key
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert sorted(got) == ["indices", "jacobian", "jacobian_nonfinite", "status", "uv",
                           "uv_nonfinite"]
    for name, arr in got.items():  # finite numbers only, f32 / f64
        assert arr.dtype in (np.float32, np.float64) and np.isfinite(arr).all(), name
    idx = got["indices"].astype(np.int64)
    assert len(idx) == bench.DUMP_MAX_POINTS
    params, (w, h) = samples.SAMPLES[2]
    model = KannalaBrandtModel.new(params)
    model.resolution.width, model.resolution.height = w, h
    uv, st, jac = model.project_batch(bench.seeded_points(n), jacobian=True)
    torch.cuda.synchronize()
    assert np.array_equal(got["status"], st.cpu().numpy()[idx].astype(np.float32))
    assert (got["status"] != 0).any()  # the sample holds failed points (uv NaN)
    # values and non-finite codes (bench.finite_parts) of this process's projection
    for name, full in (("uv", uv.cpu().numpy()[idx]), ("jacobian", jac.cpu().numpy()[:, idx])):
        vals, codes = bench.finite_parts(full)
        assert np.array_equal(got[name], vals), name
        assert np.array_equal(got[name + "_nonfinite"], codes), name
    assert (got["uv_nonfinite"] == 1).any() and (got["jacobian_nonfinite"] == 0).mean() > 0.999


def test_bench_self_launch_world2():
    """the driver's own command form: plain `bench.py --gpus 2`, no launcher;
    bench.py starts both ranks itself (gloo, both on device 0 on this box)"""
    env = dict(os.environ, ACM_BENCH_SAME_DEVICE="1", ACM_BENCH_BACKEND="gloo",
               OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2",
                        "--full", "--steps", "3", "--warmup", "1", "--points", "300000",
                        "--no-cpu-baseline", "--leg4-points", "600001",
                        "--leg5-cells", "2000000", "--leg-steps", "2"],
                       capture_output=True, text=True, timeout=400, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    d = _line(r.stdout)
    assert d["n_gpus"] == d["n_ranks_seen"] == 2 and d["scaling"] == "weak"
    assert d["config"]["global_points"] == 600000
    assert d["strong"]["mode"] == "strong" and d["strong"]["global_points"] == 300000
    assert d["collective"]["ranks"] == 2 and d["collective"]["us"] > 0
    # BASELINE config 4 over both ranks: the all-reduced counts equal the
    # single-process leg's (same global batch, sharded)
    c4 = d["config4"]
    assert c4["points_total"] == 600001 and c4["points_per_rank"] == 300001
    assert c4["allreduce_us"] > 0 and c4["value"] > 0 and len(c4["models"]) == 6
    one = _line(subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "1", "--warmup", "0",
         "--points", "1000", "--no-cpu-baseline", "--legs", "4", "--leg4-points", "600001",
         "--leg-steps", "1"], capture_output=True, text=True, timeout=300, cwd=ROOT).stdout)
    for name, m in c4["models"].items():
        m1 = one["config4"]["models"][name]
        assert m["round_trip_ok"] == m1["round_trip_ok"] > 0.8 * 600001, name
        assert abs(m["rms_round_trip_err"] - m1["rms_round_trip_err"]) <= \
            1e-9 * m1["rms_round_trip_err"] + 1e-300, name
    # BASELINE config 5: row-sharded sample_points + the sharded conversion
    c5 = d["config5"]
    assert c5["correspondences_total"] > c5["correspondences_rank0"] > 0
    assert c5["final_mean_px"] < 0.05 and c5["lm_iterations"] > 0
    assert c5["convert_ms"] > 0 and c5["sample_points_ms"] > 0


def test_bench_world2_strong_rehearsal():
    env = dict(os.environ, ACM_BENCH_SAME_DEVICE="1", ACM_BENCH_BACKEND="gloo",
               OMP_NUM_THREADS="1")
    n = 400_003  # ragged: shards 200002 + 200001
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                        "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(_port()), os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--full", "--steps", "3", "--warmup", "1", "--points",
                        str(n),
                        "--scaling", "strong", "--verify-shards", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=400, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    d = _line(r.stdout)
    assert d["n_gpus"] == 2 and d["n_ranks_seen"] == 2 and d["scaling"] == "strong"
    assert d["config"]["global_points"] == n and d["config"]["points_per_gpu"] == 200002
    assert d["shards_match_single_projection"] is True
    assert d["weak"]["mode"] == "weak" and d["weak"]["global_points"] == 2 * n
    c = d["collective"]
    assert c["ranks"] == 2 and c["us"] > 0 and c["backend"] == "gloo"
    assert c["global_n_valid"] > 0.99 * n
    assert "cpu_baseline" not in d
