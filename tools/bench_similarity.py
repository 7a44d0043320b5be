"""Times of acm_similarity_batch on this GPU, one JSON line per cell, written to
profiles/similarity_perf.log as well (the capability is new: there is no
earlier time to compare with, and the numbers are no gate).

Sets: K similarities (a rotation Exp(N(0, I)), t = N(0, I), s = 2.5), every
set its own random points in the box [+-4, +-3, 6 +- 2]; b = s R a + t plus
noise of 0.01 per axis, and --outliers of every set's b (default 40 %) are
then moved by N(0, I).  n_hypotheses = 256, inlier_distance 0.04,
refit_rounds = 3.

The call is host-timed between two device synchronisations after one warm-up
run (the minimum over --reps runs).  Beside it, for scale only: the time of the
numpy restatement (tests/similarity_ref.py) on the first set.  No hardware
counters are collected.

  python tools/bench_similarity.py [--sets 8,64,512] [--points 100,1000]
                                   [--reps R] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "apex-camera-models_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

N_HYPOTHESES = 256
DISTANCE = 0.04
NOISE = 0.01
SCALE = 2.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="8,64,512")
    ap.add_argument("--points", default="100,1000")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--outliers", type=float, default=0.4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similarity_perf.log"))
    a = ap.parse_args()
    import numpy as np
    import torch

    import similarity_ref as G
    from apex_camera_models import _lib

    L = _lib.load()
    sh = torch.cuda.current_stream().cuda_stream
    dev = torch.cuda.get_device_name(0)
    sets = [int(v) for v in a.sets.split(",")]
    k_max = max(sets)
    rng = np.random.default_rng(20261021)
    R_np = np.stack([G.exp_so3(w) for w in rng.normal(size=(k_max, 3))])
    R_all = torch.as_tensor(R_np, device="cuda")
    t_all = torch.as_tensor(rng.normal(size=(k_max, 3)), device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(20261021)

    def rand(*shape):
        return torch.rand(shape, generator=gen, dtype=torch.float64, device="cuda")

    def randn(*shape):
        return torch.randn(shape, generator=gen, dtype=torch.float64, device="cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    lines = ["# acm_similarity_batch (tools/bench_similarity.py): host-timed between two device "
             "synchronisations, 1 warm-up run, the minimum of %d runs; n_hypotheses %d, "
             "inlier_distance %g, refit_rounds 3, noise %g, %g %% of b moved by N(0, I), s = %g; "
             "numpy_one_set_ms: tests/similarity_ref.py on the first set, for scale only; no "
             "hardware counters collected" % (a.reps, N_HYPOTHESES, DISTANCE, NOISE,
                                              100.0 * a.outliers, SCALE)]
    half = torch.tensor([4.0, 3.0, 2.0], dtype=torch.float64, device="cuda")
    mid = torch.tensor([0.0, 0.0, 6.0], dtype=torch.float64, device="cuda")
    for n_p in [int(v) for v in a.points.split(",")]:
        for K in sets:
            M = K * n_p
            pa = (2.0 * rand(K, n_p, 3) - 1.0) * half + mid
            Rm, t = R_all[:K], t_all[:K]
            pb = SCALE * torch.einsum("kij,knj->kni", Rm, pa) + t[:, None, :] + NOISE * randn(K, n_p, 3)
            moved = rand(K, n_p) < a.outliers
            pb = torch.where(moved[:, :, None], pb + randn(K, n_p, 3), pb)
            pa, pb = pa.reshape(M, 3).contiguous(), pb.reshape(M, 3).contiguous()
            offs = torch.arange(K + 1, dtype=torch.int64, device="cuda") * n_p

            cfg = _lib.SimilarityConfig()
            L.acm_similarity_batch_default_config(ctypes.byref(cfg))
            cfg.n_hypotheses = N_HYPOTHESES
            cfg.inlier_distance = DISTANCE
            sim = torch.empty((K, 13), dtype=torch.float64, device="cuda")
            status = torch.empty((K,), dtype=torch.uint8, device="cuda")
            n_inl = torch.empty((K,), dtype=torch.int32, device="cuda")
            rms = torch.empty((K,), dtype=torch.float64, device="cuda")
            mask = torch.empty((M,), dtype=torch.uint8, device="cuda")
            wb = L.acm_similarity_batch_workspace_size(K, M)
            ws = torch.empty(((wb + 7) // 8,), dtype=torch.float64, device="cuda")

            def estimate():
                _lib.check(L.acm_similarity_batch(
                    K, offs.data_ptr(), M, pa.data_ptr(), pb.data_ptr(), ctypes.byref(cfg),
                    sim.data_ptr(), status.data_ptr(), n_inl.data_ptr(), rms.data_ptr(),
                    mask.data_ptr(), None, ws.data_ptr(), wb, sh))

            timed(estimate)
            best = min(timed(estimate)[0] for _ in range(a.reps))

            # the numpy restatement on the first set
            a0, b0 = pa[:n_p].cpu().numpy(), pb[:n_p].cpu().numpy()
            t0 = time.perf_counter()
            ref = G.ransac(a0, b0, DISTANCE, N_HYPOTHESES, 1)
            ref_ms = (time.perf_counter() - t0) * 1e3
            dR = (sim[:, :9] - Rm.reshape(K, 9)).abs().amax(dim=1)
            ds = (sim[:, 12] / SCALE - 1.0).abs()
            clean = (~moved).sum(dim=1)
            line = json.dumps({
                "what": "RANSAC over the 3-point similarity with refit, one workgroup per set",
                "sets": K, "points_per_set": n_p, "device": dev,
                "estimate_ms": round(best, 4),
                "us_per_set": round(1e3 * best / K, 3),
                "numpy_one_set_ms": round(ref_ms, 1),
                "status_counts": torch.bincount(status.to(torch.int64), minlength=3).tolist(),
                "inliers_over_unmoved_min": round(float((n_inl / clean).min()), 4),
                "inliers_over_unmoved_median": round(float((n_inl / clean).median()), 4),
                "inliers_set0": int(n_inl[0]), "numpy_inliers_set0": int(ref["n_inliers"]),
                "rotation_entry_error_median": float(dR.nanmedian()),
                "rotation_entry_error_max": float(dR[~dR.isnan()].max()),
                "scale_error_median": float(ds.nanmedian()),
                "rms_median": float(rms.nanmedian())})
            print(line, flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
