"""Times of acm_calibrate on this GPU beside what the library offered before
it: alternating refine_poses (every pose, intrinsics held) with
LevenbergMarquardt.optimize on R X + t (the intrinsics, poses held) until the
total cost is within 1e-6 relative of acm_calibrate's (or --sweeps sweeps
have passed: "alternating_reached" says which).  One JSON line per cell.

Views: K poses a small random motion away from the identity, a shared cloud of
world points x, y in [-1, 1), z in [2, 4); every view observes its own random
subset in ascending point order, every observation the model's own projection
plus 0.5 px of noise.  Start: every pose the true one moved by (0.02, -0.01,
0.015, 0.01, 0.02, -0.015); the intrinsics fx 1.02, fy 0.985, cx + 4, cy - 3,
every further parameter x 0.8 (the start of tests/calibration_ref.py).

Both sides are host-timed between two device synchronisations, 1 warm-up run,
the minimum over --reps runs; the two sides alternate.

  python tools/bench_calibrate.py [--views 8,64,512] [--obs 100,1000] [--reps R]
                                  [--models kb,ds] [--sweeps S]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "apex-camera-models_amd"))
sys.path.insert(0, ROOT)

NAMES = {"pinhole": 0, "radtan": 1, "kb": 2, "ds": 3, "ucm": 4, "eucm": 5, "fov": 6}
START_DELTA = [0.02, -0.01, 0.015, 0.01, 0.02, -0.015]
N_CLOUD = 20000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", default="8,64,512")
    ap.add_argument("--obs", default="100,1000")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--models", default="kb,ds")
    ap.add_argument("--sweeps", type=int, default=100)
    a = ap.parse_args()
    import torch
    from apex_camera_models import Resolution, samples
    from apex_camera_models.camera import MODEL_CLASSES
    from apex_camera_models.optimizer import (LevenbergMarquardt, Pose, calibrate, refine_poses)

    dev = torch.cuda.get_device_name(0)
    views = [int(v) for v in a.views.split(",")]
    k_max = max(views)

    def row(p):
        return [v for r in p.rotation for v in r] + list(p.translation)

    gen = torch.Generator(device="cuda").manual_seed(20251208)
    cloud = torch.rand((N_CLOUD, 3), generator=gen, dtype=torch.float64, device="cuda")
    cloud[:, :2] = 2.0 * cloud[:, :2] - 1.0
    cloud[:, 2] = 2.0 + 2.0 * cloud[:, 2]
    motion = (torch.rand((k_max, 6), generator=gen, dtype=torch.float64, device="cuda") - 0.5).cpu()
    scale = torch.tensor([0.4, 0.2, 0.1, 0.06, 0.08, 0.04], dtype=torch.float64)
    true_poses = [Pose().retract((motion[k] * scale).tolist()) for k in range(k_max)]
    true_t = torch.tensor([row(p) for p in true_poses], dtype=torch.float64, device="cuda")
    start_t = torch.tensor([row(p.retract(START_DELTA)) for p in true_poses], dtype=torch.float64,
                           device="cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for name in a.models.split(","):
        mid = NAMES[name]
        params, (w, h) = samples.SAMPLES[mid]
        cls = MODEL_CLASSES[samples.MODEL_NAMES[mid]]
        truth = cls._from_params(list(params), Resolution(w, h))
        p0 = list(params)
        p0[0] *= 1.02
        p0[1] *= 0.985
        p0[2] += 4.0
        p0[3] -= 3.0
        p0[4:] = [0.8 * v for v in p0[4:]]
        for n_obs in [int(v) for v in a.obs.split(",")]:
            for K in views:
                M = K * n_obs
                point = torch.sort(torch.randint(0, N_CLOUD, (K, n_obs), generator=gen, device="cuda"),
                                   dim=1).values
                Rm, t = true_t[:K, :9].reshape(K, 3, 3), true_t[:K, 9:]
                cam_pts = torch.einsum("kij,knj->kni", Rm, cloud[point]) + t[:, None, :]
                uv, st, _ = truth.project_batch(cam_pts.reshape(M, 3).contiguous())
                uv = torch.where((st == 0)[:, None], uv, torch.full_like(uv, float("nan")))
                uv = (uv + 0.5 * torch.randn(uv.shape, generator=gen, dtype=torch.float64,
                                             device="cuda")).contiguous()
                obs_point = point.reshape(M).to(torch.int32).contiguous()
                gather = obs_point.to(torch.int64)
                offs = torch.arange(K + 1, dtype=torch.int64, device="cuda") * n_obs
                view_of = torch.arange(K, device="cuda").repeat_interleave(n_obs)
                del cam_pts

                def joint():
                    return calibrate(cls._from_params(list(p0), Resolution(w, h)), start_t[:K],
                                     cloud, offs, obs_point, uv)

                def alternating(target):
                    m = cls._from_params(list(p0), Resolution(w, h))
                    poses, cost, sweeps = start_t[:K], float("inf"), 0
                    lm = LevenbergMarquardt()
                    while sweeps < a.sweeps and not cost <= target * (1.0 + 1e-6):
                        sweeps += 1
                        poses = refine_poses(m, poses, cloud, offs, obs_point, uv).poses
                        Rk, tk = poses[:, :9].reshape(K, 3, 3)[view_of], poses[:, 9:][view_of]
                        p_cam = (torch.einsum("mij,mj->mi", Rk, cloud[gather]) + tk).contiguous()
                        cost = lm.optimize(m, p_cam, uv).final_cost
                    return cost, sweeps

                best = {"joint": float("inf"), "alternating": float("inf")}
                _, res = timed(joint)
                target = res.summary.final_cost
                _, (alt_cost, alt_sweeps) = timed(lambda: alternating(target))
                for _ in range(a.reps):
                    best["joint"] = min(best["joint"], timed(joint)[0])
                    best["alternating"] = min(best["alternating"],
                                              timed(lambda: alternating(target))[0])
                print(json.dumps({
                    "what": "acm_calibrate vs alternating refine_poses / LevenbergMarquardt.optimize",
                    "model": name, "views": K, "obs_per_view": n_obs, "device": dev,
                    "calibrate_ms": round(best["joint"], 3),
                    "alternating_ms": round(best["alternating"], 3),
                    "speedup": round(best["alternating"] / best["joint"], 2),
                    "calibrate_cost": target, "alternating_cost": alt_cost,
                    "alternating_reached": bool(alt_cost <= target * (1.0 + 1e-6)),
                    "calibrate_iterations": res.summary.iterations,
                    "calibrate_evaluations": res.summary.evaluations,
                    "calibrate_termination": res.summary.termination,
                    "alternating_sweeps": alt_sweeps,
                    "views_used": res.n_views_used}), flush=True)


if __name__ == "__main__":
    main()
