"""Times of acm_homography_batch on this GPU, one JSON line per cell, written to
profiles/homography_perf.log as well (the capability is new: there is no
earlier time to compare with, and the numbers are no gate).

Pairs: K true relative poses (tools/bench_relative_pose.py's: a rotation of up
to ~0.2 rad, a baseline of 0.3 .. 0.6), every pair its own random points on the
plane n ~ (0.1, -0.2, 1), d = 3 of camera A's frame (x, y in [-4, 4)); every
match is the model's own projection into both images plus 0.5 px of noise, and
--outliers of every pair's pixels in image B (default 40 %) are then moved
50-300 px away.  n_hypotheses = 256, the threshold 3 px, refit_rounds = 3.

The call is host-timed between two device synchronisations after one warm-up
run (the minimum over --reps runs).  Beside it, for scale only and on the same
matches: acm_relative_pose_batch with its default 512 hypotheses (a planar
scene is degenerate for it, so only its time means anything), and the time of
the numpy restatement (tests/homography_ref.py) on the first pair.

  python tools/bench_homography.py [--pairs 8,64,512] [--matches 100,1000]
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
N_HYPOTHESES = 256
THRESHOLD_PX = 3.0
PLANE = (0.1, -0.2, 1.0, 3.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="8,64,512")
    ap.add_argument("--matches", default="100,1000")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--models", default="kb,ds")
    ap.add_argument("--outliers", type=float, default=0.4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography_perf.log"))
    a = ap.parse_args()
    import numpy as np
    import torch

    import homography_ref as G
    from apex_camera_models import Resolution, _lib, samples
    from apex_camera_models.camera import MODEL_CLASSES
    from apex_camera_models.optimizer import Pose

    L = _lib.load()
    sh = torch.cuda.current_stream().cuda_stream
    dev = torch.cuda.get_device_name(0)
    pairs = [int(v) for v in a.pairs.split(",")]
    k_max = max(pairs)
    nrm = np.array(PLANE[:3]) / np.linalg.norm(PLANE[:3])
    n_t = torch.tensor(nrm, dtype=torch.float64, device="cuda")

    def row(p):
        return [v for r in p.rotation for v in r] + list(p.translation)

    gen = torch.Generator(device="cuda").manual_seed(20261020)

    def rand(*shape):
        return torch.rand(shape, generator=gen, dtype=torch.float64, device="cuda")

    motion = (rand(k_max, 6) - 0.5).cpu()
    motion[:, 0] = torch.where(motion[:, 0] < 0, motion[:, 0] - 0.5, motion[:, 0] + 0.5)
    scale = torch.tensor([0.45, 0.4, 0.6, 0.25, 0.25, 0.25], dtype=torch.float64)
    true_poses = [Pose().retract((motion[k] * scale).tolist()) for k in range(k_max)]
    true_t = torch.tensor([row(p) for p in true_poses], dtype=torch.float64, device="cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    lines = ["# acm_homography_batch (tools/bench_homography.py): host-timed between two device "
             "synchronisations, 1 warm-up run, the minimum of %d runs; n_hypotheses %d, threshold %g px, "
             "refit_rounds 3, %g %% outliers, planar scenes; relative_pose_ms: acm_relative_pose_batch "
             "(512 hypotheses) on the same matches, numpy_one_pair_ms: tests/homography_ref.py on the "
             "first pair, both for scale only" % (a.reps, N_HYPOTHESES, THRESHOLD_PX, 100.0 * a.outliers)]
    for name in a.models.split(","):
        mid = NAMES[name]
        params, (w, h) = samples.SAMPLES[mid]
        m = MODEL_CLASSES[samples.MODEL_NAMES[mid]]._from_params(list(params), Resolution(w, h))
        cam = m.acm_camera()
        angle = math.atan(THRESHOLD_PX / min(params[0], params[1]))
        for n_m in [int(v) for v in a.matches.split(",")]:
            for K in pairs:
                M = K * n_m
                x, y = 8.0 * rand(K, n_m) - 4.0, 8.0 * rand(K, n_m) - 4.0
                X = torch.stack([x, y, (PLANE[3] - nrm[0] * x - nrm[1] * y) / nrm[2]], dim=2)
                Rm, t = true_t[:K, :9].reshape(K, 3, 3), true_t[:K, 9:]
                pb = torch.einsum("kij,knj->kni", Rm, X) + t[:, None, :]

                def pixels(p):
                    uv, st, _ = m.project_batch(p.reshape(M, 3).contiguous())
                    uv = torch.where((st == 0)[:, None], uv, torch.full_like(uv, float("nan")))
                    return uv + 0.5 * torch.randn(uv.shape, generator=gen, dtype=torch.float64,
                                                  device="cuda")

                uv_a, uv_b = pixels(X), pixels(pb)
                gross = rand(M) < a.outliers
                r, phi = 50.0 + 250.0 * rand(M), 2.0 * math.pi * rand(M)
                away = torch.stack([r * torch.cos(phi), r * torch.sin(phi)], dim=1)
                uv_b = torch.where(gross[:, None], uv_b + away, uv_b).contiguous()
                uv_a = uv_a.contiguous()
                offs = torch.arange(K + 1, dtype=torch.int64, device="cuda") * n_m

                cfg = _lib.HomographyConfig()
                L.acm_homography_batch_default_config(ctypes.byref(cfg))
                cfg.n_hypotheses = N_HYPOTHESES
                cfg.inlier_angle = angle
                hom = torch.empty((K, 9), dtype=torch.float64, device="cuda")
                poses = torch.empty((K, 2, 12), dtype=torch.float64, device="cuda")
                planes = torch.empty((K, 2, 4), dtype=torch.float64, device="cuda")
                status = torch.empty((K,), dtype=torch.uint8, device="cuda")
                n_sol = torch.empty((K,), dtype=torch.uint8, device="cuda")
                n_inl = torch.empty((K,), dtype=torch.int32, device="cuda")
                n_front = torch.empty((K, 2), dtype=torch.int32, device="cuda")
                tau = torch.empty((K,), dtype=torch.float64, device="cuda")
                mask = torch.empty((M,), dtype=torch.uint8, device="cuda")
                wb = L.acm_homography_batch_workspace_size(K, M)
                ws = torch.empty(((wb + 7) // 8,), dtype=torch.float64, device="cuda")

                def estimate():
                    _lib.check(L.acm_homography_batch(
                        ctypes.byref(cam), K, offs.data_ptr(), M, uv_a.data_ptr(), uv_b.data_ptr(),
                        ctypes.byref(cfg), hom.data_ptr(), status.data_ptr(), n_inl.data_ptr(),
                        poses.data_ptr(), planes.data_ptr(), n_sol.data_ptr(), n_front.data_ptr(),
                        tau.data_ptr(), mask.data_ptr(), None, ws.data_ptr(), wb, sh))

                timed(estimate)
                best = min(timed(estimate)[0] for _ in range(a.reps))

                # acm_relative_pose_batch on the same matches, for scale
                rcfg = _lib.RelativePoseConfig()
                L.acm_relative_pose_batch_default_config(ctypes.byref(rcfg))
                rcfg.inlier_angle = angle
                rposes = torch.empty((K, 12), dtype=torch.float64, device="cuda")
                rstatus = torch.empty((K,), dtype=torch.uint8, device="cuda")
                rinl = torch.empty((K,), dtype=torch.int32, device="cuda")
                rmask = torch.empty((M,), dtype=torch.uint8, device="cuda")
                rwb = L.acm_relative_pose_batch_workspace_size(K, M)
                rws = torch.empty(((rwb + 7) // 8,), dtype=torch.float64, device="cuda")

                def relpose():
                    _lib.check(L.acm_relative_pose_batch(
                        ctypes.byref(cam), K, rposes.data_ptr(), offs.data_ptr(), M, uv_a.data_ptr(),
                        uv_b.data_ptr(), ctypes.byref(rcfg), rstatus.data_ptr(), rinl.data_ptr(),
                        rmask.data_ptr(), None, rws.data_ptr(), rwb, sh))

                timed(relpose)
                rel_best = min(timed(relpose)[0] for _ in range(a.reps))

                # the numpy restatement on the first pair
                def unit(uv):
                    rays, rst = m.unproject_batch(uv[:n_m].contiguous())
                    f = (rays / rays.norm(dim=1, keepdim=True)).cpu().numpy()
                    ok = ((rst == 0) & torch.isfinite(uv[:n_m]).all(dim=1)).cpu().numpy()
                    return f, ok & np.isfinite(f).all(axis=1)

                (fa, ua), (fb, ub) = unit(uv_a), unit(uv_b)
                t0 = time.perf_counter()
                ref = G.ransac(fa, fb, ua & ub, N_HYPOTHESES, 1, angle)
                ref_ms = (time.perf_counter() - t0) * 1e3
                # |H - H_true| and the better slot's rotation error, per pair
                H0 = Rm + (t / PLANE[3])[:, :, None] * n_t[None, None, :]
                dH = (hom.reshape(K, 3, 3) - H0).abs().amax(dim=(1, 2))
                dR = (poses[:, :, :9] - true_t[:K, None, :9]).abs().amax(dim=2).amin(dim=1)
                good = (~gross).reshape(K, n_m).sum(dim=1)
                line = json.dumps({
                    "what": "RANSAC over the 4-point homography with refit, one workgroup per pair",
                    "model": name, "pairs": K, "matches_per_pair": n_m, "device": dev,
                    "estimate_ms": round(best, 4),
                    "us_per_pair": round(1e3 * best / K, 3),
                    "relative_pose_ms": round(rel_best, 4),
                    "numpy_one_pair_ms": round(ref_ms, 1),
                    "status_counts": torch.bincount(status.to(torch.int64), minlength=3).tolist(),
                    "solutions_counts": torch.bincount(n_sol.to(torch.int64), minlength=3).tolist(),
                    "inliers_over_clean_min": round(float((n_inl / good).min()), 4),
                    "inliers_over_clean_median": round(float((n_inl / good).median()), 4),
                    "inliers_pair0": int(n_inl[0]), "numpy_inliers_pair0": int(ref["n_inliers"]),
                    "h_entry_error_median": float(dH.nanmedian()),
                    "h_entry_error_max": float(dH[~dH.isnan()].max()),
                    "rotation_entry_error_median": float(dR.nanmedian()),
                    "tau_median": float(tau.nanmedian())})
                print(line, flush=True)
                lines.append(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
