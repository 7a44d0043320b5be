"""Times of acm_pose_estimate_batch on this GPU, one JSON line per cell, written
to profiles/pose_estimate_perf.log as well (the capability is new: there is no
earlier time to compare with, and the numbers are no gate).

Views: K poses a small random motion away from the identity, a shared cloud of
world points x, y in [-1, 1), z in [2, 4); every view observes its own random
subset (ascending point order, as optimizer.tracks_by_view gives it), every
observation the model's own projection plus 0.5 px of noise; --outliers of
every view's observations (default 40 %) are then moved 50-300 px away.
n_hypotheses = 256, the threshold 3 px.

The call is host-timed between two device synchronisations after one warm-up
run (the minimum over --reps runs).  Beside it, for scale only: the time of
the numpy restatement (tests/pose_estimation_ref.py) on the first view.

  python tools/bench_pose_estimate.py [--views 8,64,512] [--obs 100,1000]
                                      [--reps R] [--models kb,ds] [--out FILE]
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "apex-camera-models_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

NAMES = {"pinhole": 0, "radtan": 1, "kb": 2, "ds": 3, "ucm": 4, "eucm": 5, "fov": 6}
N_CLOUD = 20000
N_HYPOTHESES = 256
THRESHOLD_PX = 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", default="8,64,512")
    ap.add_argument("--obs", default="100,1000")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--models", default="kb,ds")
    ap.add_argument("--outliers", type=float, default=0.4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_estimate_perf.log"))
    a = ap.parse_args()
    import numpy as np
    import torch

    import pose_estimation_ref as P
    from apex_camera_models import Resolution, _lib, samples
    from apex_camera_models.camera import MODEL_CLASSES
    from apex_camera_models.optimizer import Pose

    L = _lib.load()
    sh = torch.cuda.current_stream().cuda_stream
    dev = torch.cuda.get_device_name(0)
    views = [int(v) for v in a.views.split(",")]
    k_max = max(views)

    def row(p):
        return [v for r in p.rotation for v in r] + list(p.translation)

    gen = torch.Generator(device="cuda").manual_seed(20261020)
    cloud = torch.rand((N_CLOUD, 3), generator=gen, dtype=torch.float64, device="cuda")
    cloud[:, :2] = 2.0 * cloud[:, :2] - 1.0
    cloud[:, 2] = 2.0 + 2.0 * cloud[:, 2]
    motion = (torch.rand((k_max, 6), generator=gen, dtype=torch.float64, device="cuda") - 0.5).cpu()
    scale = torch.tensor([0.4, 0.2, 0.1, 0.06, 0.08, 0.04], dtype=torch.float64)
    true_poses = [Pose().retract((motion[k] * scale).tolist()) for k in range(k_max)]
    true_t = torch.tensor([row(p) for p in true_poses], dtype=torch.float64, device="cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    lines = ["# acm_pose_estimate_batch (tools/bench_pose_estimate.py): host-timed between two device "
             "synchronisations, 1 warm-up run, the minimum of %d runs; n_hypotheses %d, threshold %g px, "
             "%g %% outliers; numpy_one_view_ms: tests/pose_estimation_ref.py on the first view, for scale"
             % (a.reps, N_HYPOTHESES, THRESHOLD_PX, 100.0 * a.outliers)]
    for name in a.models.split(","):
        mid = NAMES[name]
        params, (w, h) = samples.SAMPLES[mid]
        m = MODEL_CLASSES[samples.MODEL_NAMES[mid]]._from_params(list(params), Resolution(w, h))
        cam = m.acm_camera()
        angle = math.atan(THRESHOLD_PX / min(params[0], params[1]))
        for n_obs in [int(v) for v in a.obs.split(",")]:
            for K in views:
                M = K * n_obs
                point = torch.sort(torch.randint(0, N_CLOUD, (K, n_obs), generator=gen, device="cuda"),
                                   dim=1).values
                gathered = cloud[point]                                     # (K, n_obs, 3)
                Rm, t = true_t[:K, :9].reshape(K, 3, 3), true_t[:K, 9:]
                cam_pts = torch.einsum("kij,knj->kni", Rm, gathered) + t[:, None, :]
                uv, st, _ = m.project_batch(cam_pts.reshape(M, 3).contiguous())
                uv = torch.where((st == 0)[:, None], uv, torch.full_like(uv, float("nan")))
                uv = uv + 0.5 * torch.randn(uv.shape, generator=gen, dtype=torch.float64, device="cuda")
                gross = torch.rand((M,), generator=gen, dtype=torch.float64, device="cuda") < a.outliers
                r = 50.0 + 250.0 * torch.rand((M,), generator=gen, dtype=torch.float64, device="cuda")
                phi = 2.0 * math.pi * torch.rand((M,), generator=gen, dtype=torch.float64, device="cuda")
                away = torch.stack([r * torch.cos(phi), r * torch.sin(phi)], dim=1)
                uv = torch.where(gross[:, None], uv + away, uv).contiguous()
                obs_point = point.reshape(M).to(torch.int32).contiguous()
                offs = torch.arange(K + 1, dtype=torch.int64, device="cuda") * n_obs
                del cam_pts

                cfg = _lib.PoseEstimateConfig()
                L.acm_pose_estimate_batch_default_config(ctypes.byref(cfg))
                cfg.n_hypotheses = N_HYPOTHESES
                cfg.inlier_angle = angle
                poses = torch.empty((K, 12), dtype=torch.float64, device="cuda")
                status = torch.empty((K,), dtype=torch.uint8, device="cuda")
                n_inl = torch.empty((K,), dtype=torch.int32, device="cuda")
                mask = torch.empty((M,), dtype=torch.uint8, device="cuda")
                wb = L.acm_pose_estimate_batch_workspace_size(K, M)
                ws = torch.empty(((wb + 7) // 8,), dtype=torch.float64, device="cuda")

                def estimate():
                    _lib.check(L.acm_pose_estimate_batch(
                        ctypes.byref(cam), K, poses.data_ptr(), N_CLOUD, cloud.data_ptr(),
                        offs.data_ptr(), M, obs_point.data_ptr(), uv.data_ptr(), ctypes.byref(cfg),
                        status.data_ptr(), n_inl.data_ptr(), mask.data_ptr(), None, ws.data_ptr(), wb,
                        sh))

                timed(estimate)
                best = min(timed(estimate)[0] for _ in range(a.reps))
                # the numpy restatement on the first view
                rays, rst = m.unproject_batch(uv[:n_obs])
                f = (rays / rays.norm(dim=1, keepdim=True)).cpu().numpy()
                usable = ((rst == 0) & torch.isfinite(uv[:n_obs]).all(dim=1)).cpu().numpy() & \
                    np.isfinite(f).all(axis=1)
                X0 = gathered[0].cpu().numpy()
                t0 = time.perf_counter()
                ref = P.ransac(X0, f, usable, N_HYPOTHESES, 1, angle)
                ref_ms = (time.perf_counter() - t0) * 1e3
                dR = (poses[:, :9] - true_t[:K, :9]).abs().max(dim=1).values
                good = (~gross).reshape(K, n_obs).sum(dim=1)
                line = json.dumps({
                    "what": "RANSAC over P3P, one workgroup per view",
                    "model": name, "views": K, "obs_per_view": n_obs, "device": dev,
                    "estimate_ms": round(best, 4),
                    "us_per_view": round(1e3 * best / K, 3),
                    "numpy_one_view_ms": round(ref_ms, 1),
                    "status_counts": torch.bincount(status.to(torch.int64), minlength=3).tolist(),
                    "inliers_over_clean_min": round(float((n_inl / good).min()), 4),
                    "inliers_view0": int(n_inl[0]), "numpy_inliers_view0": int(ref["n_inliers"]),
                    "rotation_entry_error_max": float(dR.max())})
                print(line, flush=True)
                lines.append(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
