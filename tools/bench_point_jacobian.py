"""Times of the point-Jacobian and pose normal-equations kernels on this GPU
against their yardsticks, one JSON line per cell:

  * acm_project_point_jacobian (89 B per point) against the zero-compute
    mimic of tools/hbm_probe.hip moving the same 89 B per point (3 Jacobian
    columns), and, for comparison, acm_project + parameter Jacobian
    (k_project_al) against its own mimic (P columns);
  * acm_pose_normal_equations against acm_normal_equations for the same
    model and n (both read 40 B per point).

Device events around each call, 3 warm-up calls, the minimum over --reps
windows of the mean of 20 calls; the cells of one comparison alternate.

  python tools/bench_point_jacobian.py [--points N] [--reps R] [--models kb,ds]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--models", default="kb,ds")
    a = ap.parse_args()
    import torch
    from apex_camera_models import Resolution, _lib, samples
    from apex_camera_models.camera import MODEL_CLASSES
    from apex_camera_models.optimizer import Pose

    L = _lib.load()
    probe = ctypes.CDLL(PROBE)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    probe.acm_probe_mimic.argtypes = [sz, vp, vp, vp, vp, ci, ci, ci, vp]
    sh = torch.cuda.current_stream().cuda_stream
    n = a.points

    def timed(fn, reps=20):
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

    def compare(cells):
        """cells: {name: (fn, bytes)}; alternates them, min over reps."""
        best = {k: float("inf") for k in cells}
        for _ in range(a.reps):
            for k, (fn, _) in cells.items():
                best[k] = min(best[k], timed(fn))
        return {k: {"ms": round(best[k], 4), "TBps": round(cells[k][1] / best[k] / 1e9, 3)}
                for k in cells}

    pts = samples.synthetic_points_device(n)
    uv = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    st = torch.empty((n,), dtype=torch.uint8, device="cuda")
    jac = torch.empty((9, n, 2), dtype=torch.float64, device="cuda")
    dev = torch.cuda.get_device_name(0)
    for name in a.models.split(","):
        mid = NAMES[name]
        params, (w, h) = samples.SAMPLES[mid]
        m = MODEL_CLASSES[samples.MODEL_NAMES[mid]]._from_params(list(params), Resolution(w, h))
        cam = m.acm_camera()
        P = m.NUM_PARAMS
        r = compare({
            "point_jacobian": (lambda: _lib.check(L.acm_project_point_jacobian(
                ctypes.byref(cam), n, pts.data_ptr(), 0, uv.data_ptr(), st.data_ptr(),
                jac.data_ptr(), sh)), 89 * n),
            "mimic_89B": (lambda: probe.acm_probe_mimic(
                n, pts.data_ptr(), uv.data_ptr(), st.data_ptr(), jac.data_ptr(), 3, 1, 0, sh),
                89 * n),
            "project_param_jacobian": (lambda: _lib.check(L.acm_project(
                ctypes.byref(cam), n, pts.data_ptr(), 0, uv.data_ptr(), st.data_ptr(),
                jac.data_ptr(), sh)), (41 + 16 * P) * n),
            "mimic_param_jacobian": (lambda: probe.acm_probe_mimic(
                n, pts.data_ptr(), uv.data_ptr(), st.data_ptr(), jac.data_ptr(), P, 1, 0, sh),
                (41 + 16 * P) * n),
        })
        r["point_jacobian"]["of_ceiling"] = round(
            r["mimic_89B"]["ms"] / r["point_jacobian"]["ms"], 3)
        r["project_param_jacobian"]["of_ceiling"] = round(
            r["mimic_param_jacobian"]["ms"] / r["project_param_jacobian"]["ms"], 3)
        print(json.dumps({"what": "project + point Jacobian vs zero-compute mimic", "model": name,
                          "points": n, "device": dev, "cells": r}), flush=True)

        # observations: the model's own projections (NaN where they fail)
        m.project_batch(pts, out=(uv, st, None))
        pose = Pose().retract([0.01, -0.02, 0.015, 0.004, -0.003, 0.005]).acm_pose()
        res = torch.empty((128,), dtype=torch.float64, device="cuda")
        wb_p = L.acm_pose_normal_equations_workspace_size(n)
        wb_c = L.acm_normal_equations_workspace_size(mid, n)
        ws = torch.empty(((max(wb_p, wb_c) + 7) // 8,), dtype=torch.float64, device="cuda")
        r = compare({
            "pose_normal_equations": (lambda: _lib.check(L.acm_pose_normal_equations(
                ctypes.byref(cam), ctypes.byref(pose), n, pts.data_ptr(), 0, uv.data_ptr(),
                res.data_ptr(), ws.data_ptr(), wb_p, sh)), 40 * n),
            "normal_equations": (lambda: _lib.check(L.acm_normal_equations(
                ctypes.byref(cam), n, pts.data_ptr(), 0, uv.data_ptr(), 0, res.data_ptr(),
                ws.data_ptr(), wb_c, sh)), 40 * n),
        })
        r["pose_normal_equations"]["vs_normal_equations"] = round(
            r["pose_normal_equations"]["ms"] / r["normal_equations"]["ms"], 3)
        print(json.dumps({"what": "pose normal equations vs parameter normal equations",
                          "model": name, "points": n, "device": dev, "cells": r}), flush=True)


if __name__ == "__main__":
    main()
