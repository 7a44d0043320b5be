"""Times of acm_triangulate on this GPU beside a zero-compute probe moving
the same algorithmic bytes (8 + 20 L read, 25 written per point of track
length L; tools/hbm_probe.hip acm_probe_triangulate), one JSON line per cell.

Tracks: a 6-view rig (centres 0.4 apart along x, small rotations), points
x, y in [-1, 1), z in [2, 4), every observation the model's own projection
plus 0.5 px of noise; constant track length 2 and 4, and a mixed 2..6 set.
Each cell: max_iterations = 0 (the midpoint start only) and the default
config, against the probe.

Device events around each call, 3 warm-up calls, the minimum over --reps
windows of the mean of 10 calls; the cells of one comparison alternate.

  python tools/bench_triangulate.py [--points N] [--reps R] [--models kb,ds]
"""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "apex-camera-models_amd"))
sys.path.insert(0, ROOT)
PROBE = os.path.join(HERE, "build", "libhbmprobe.so")

NAMES = {"pinhole": 0, "radtan": 1, "kb": 2, "ds": 3, "ucm": 4, "eucm": 5, "fov": 6}
K_VIEWS = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--models", default="kb,ds")
    a = ap.parse_args()
    import torch
    from apex_camera_models import Resolution, _lib, samples, tracks_from_dense
    from apex_camera_models.camera import MODEL_CLASSES
    from apex_camera_models.optimizer import Pose

    L = _lib.load()
    probe = ctypes.CDLL(PROBE)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    probe.acm_probe_triangulate.argtypes = [sz, vp, vp, vp, vp, vp, vp]
    sh = torch.cuda.current_stream().cuda_stream
    n = a.points
    dev = torch.cuda.get_device_name(0)

    def timed(fn, reps=10):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
               for _ in range(reps)]
        for e0, e1 in evs:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return sum(e0.elapsed_time(e1) for e0, e1 in evs) / reps

    def compare(cells, nbytes):
        best = {k: float("inf") for k in cells}
        for _ in range(a.reps):
            for k, fn in cells.items():
                best[k] = min(best[k], timed(fn))
        return {k: {"ms": round(best[k], 4), "TBps": round(nbytes / best[k] / 1e9, 3)}
                for k in cells}

    poses = []
    for k in range(K_VIEWS):
        s, b, c = k - 2.5, (k % 3) - 1, k % 2
        rot = Pose().retract([0.0, 0.0, 0.0, 0.03 * b, -0.04 * s, 0.02 * c])
        R = torch.tensor(rot.rotation, dtype=torch.float64)
        centre = torch.tensor([0.4 * s, 0.15 * b, 0.05 * c], dtype=torch.float64)
        poses.append(Pose(rot.rotation, (-(R @ centre)).tolist()))
    poses_t = torch.tensor([[v for row in p.rotation for v in row] + p.translation for p in poses],
                           dtype=torch.float64, device="cuda")

    gen = torch.Generator(device="cuda").manual_seed(20251205)
    X = torch.rand((n, 3), generator=gen, dtype=torch.float64, device="cuda")
    X[:, :2] = 2.0 * X[:, :2] - 1.0
    X[:, 2] = 2.0 + 2.0 * X[:, 2]
    mixed = torch.randint(2, K_VIEWS + 1, (n,), generator=gen, device="cuda")

    for name in a.models.split(","):
        mid = NAMES[name]
        params, (w, h) = samples.SAMPLES[mid]
        m = MODEL_CLASSES[samples.MODEL_NAMES[mid]]._from_params(list(params), Resolution(w, h))
        cam = m.acm_camera()
        dense = torch.empty((K_VIEWS, n, 2), dtype=torch.float64, device="cuda")
        for k, p in enumerate(poses):
            R = torch.tensor(p.rotation, dtype=torch.float64, device="cuda")
            t = torch.tensor(p.translation, dtype=torch.float64, device="cuda")
            uv, st, _ = m.project_batch(X @ R.T + t)
            dense[k] = torch.where((st == 0)[:, None], uv, torch.full_like(uv, float("nan")))
        dense += 0.5 * torch.randn(dense.shape, generator=gen, dtype=torch.float64, device="cuda")
        view_of = torch.arange(K_VIEWS, device="cuda")[:, None]
        for label, lengths in (("L=2", torch.full((n,), 2, device="cuda")),
                               ("L=4", torch.full((n,), 4, device="cuda")),
                               ("L=2..6", mixed)):
            keep = view_of < lengths[None, :]
            offs, view, uv = tracks_from_dense(
                torch.where(keep[:, :, None], dense, torch.full_like(dense, float("nan"))))
            nobs = view.shape[0]
            pts = torch.empty((n, 3), dtype=torch.float64, device="cuda")
            status = torch.empty((n,), dtype=torch.uint8, device="cuda")
            wb = L.acm_triangulate_workspace_size(n, nobs)
            ws = torch.empty(((wb + 7) // 8,), dtype=torch.float64, device="cuda")

            def call(max_iterations):
                cfg = _lib.TriangulateConfig()
                L.acm_triangulate_default_config(ctypes.byref(cfg))
                if max_iterations is not None:
                    cfg.max_iterations = max_iterations
                return lambda: _lib.check(L.acm_triangulate(
                    ctypes.byref(cam), K_VIEWS, poses_t.data_ptr(), n, offs.data_ptr(), nobs,
                    view.data_ptr(), uv.data_ptr(), ctypes.byref(cfg), pts.data_ptr(),
                    status.data_ptr(), None, None, None, ws.data_ptr(), wb, sh))

            nbytes = 8 * n + 20 * nobs + 25 * n
            r = compare({
                "start_only": call(0),
                "default": call(None),
                "probe": lambda: probe.acm_probe_triangulate(
                    n, offs.data_ptr(), view.data_ptr(), uv.data_ptr(), pts.data_ptr(),
                    status.data_ptr(), sh),
            }, nbytes)
            call(None)()
            torch.cuda.synchronize()
            counts = torch.bincount(status.to(torch.int64), minlength=4).tolist()
            for k in ("start_only", "default"):
                r[k]["x_probe"] = round(r[k]["ms"] / r["probe"]["ms"], 2)
            print(json.dumps({"what": "triangulate vs zero-compute probe", "model": name,
                              "tracks": label, "points": n, "observations": nobs,
                              "bytes": nbytes, "status_counts": counts, "device": dev,
                              "cells": r}), flush=True)


if __name__ == "__main__":
    main()
