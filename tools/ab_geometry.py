"""Same bits from two builds of libacm.so on the batched geometry solvers:
every output array of acm_pose_normal_equations, acm_triangulate,
acm_pose_optimize_batch, acm_calibrate, acm_p3p / acm_pose_estimate_batch and
acm_relative_pose_8pt / acm_relative_pose_batch, at the GPU tests' own input
builders (their COUNTS, the spoiled inputs, KB / DS / UCM / RadTan), digested
per library and compared.  Each library runs in a process of its own, chosen
by ACM_LIB_PATH.

  python tools/ab_geometry.py --libs old/libacm.so,apex-camera-models_amd/lib/libacm.so

The inputs come from private helpers of the GPU test modules (_run, _csr,
_spoiled, _family_on_device, ...): when one of those tests is reorganised this
tool has to follow.

Prints one line per array (name, digest per library) and the count that
differ; exit status 1 when any does."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def digest(out_path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "apex-camera-models_amd"), os.path.join(ROOT, "tests")]
    import numpy as np
    import torch

    import calibration_ref as C
    import point_jacobian_ref as R
    import triangulation_ref as T
    import test_gpu_calibrate as TC
    import test_gpu_pose as TP
    import test_gpu_pose_batch as PB
    import test_gpu_pose_estimate as PE
    import test_gpu_relative_pose as RP
    import test_gpu_triangulate as TT
    from apex_camera_models import samples

    MIDS = (2, 3, 4, 1)  # KB, DS, UCM, RadTan
    out = {}


    def dig(a):
        a = np.ascontiguousarray(np.asarray(a))
        return hashlib.sha256(a.tobytes()).hexdigest()[:16]


    def put(name, d):
        if not isinstance(d, dict):
            d = {str(i): v for i, v in enumerate(d)}
        for k, v in d.items():
            out[f"{name}.{k}"] = dig(v)


    def spoil_offsets(offsets, m):
        o = np.array(offsets).copy()
        o[0], o[-1] = -5, m + 7
        return o


    for mid in MIDS:
        nm = samples.MODEL_NAMES[mid]
        # acm_pose_normal_equations
        pose = TP.TRUE_POSE.retract(TP.START_DELTA)
        for layout in ("aos", "soa"):
            for n in TP.NE_SIZES:
                world = R.tiled(TP._world_base(mid), n)
                obs = TP._observations(mid, world, TP._noise()[:n])
                w_t = torch.as_tensor(world if layout == "aos" else np.ascontiguousarray(world.T),
                                      device="cuda")
                put(f"pose_ne.{nm}.{layout}.{n}",
                    {"result": TP._ne_call(mid, pose, w_t, torch.as_tensor(obs, device="cuda"), layout)})
        # acm_triangulate
        kind = "wide" if mid in (2, 3) else "narrow"  # the wide rig is the fisheye models'
        avail = len(T.scene(kind)[1]) - 1
        for n in TT.START_SIZES + (TT.N_NOISY,):
            if n > avail:
                continue
            _, offsets, view, uv = TT._prefix(kind, mid, n, 0.5)
            put(f"triangulate.{nm}.{kind}.{n}", TT._c_triangulate(mid, T.poses12(kind), offsets, view, uv))
        _, offsets, view, uv = TT._prefix(kind, mid, 257, 0.5)
        view, uv = view.copy(), uv.copy()
        j = np.arange(len(view))
        uv[j % 37 == 5, 0] = np.nan
        uv[j % 53 == 7, 1] = np.inf
        view[j % 41 == 11] = -1
        view[j % 43 == 13] = T.K_VIEWS
        put(f"triangulate.{nm}.spoiled",
            TT._c_triangulate(mid, T.poses12(kind), spoil_offsets(offsets, len(view)), view, uv))
        # acm_pose_optimize_batch
        K = len(PB.COUNTS)
        world = PB._world(mid, K)
        offsets, point, uv = PB._csr(mid, PB.COUNTS, noisy=True, spoil=True)
        start = np.stack([PB._row(PB._start_pose(k)) for k in range(K)])
        put(f"pose_batch.{nm}", PB._run(mid, start, world, offsets, point, uv))
        put(f"pose_batch.{nm}.offsets_outside",
            PB._run(mid, start, world, spoil_offsets(offsets, len(point)), point, uv))
        put(f"pose_batch.{nm}.two_iterations", PB._run(mid, start, world, offsets, point, uv, 2))
        # acm_calibrate
        offsets, point, uv = TC._sums_csr(mid)
        start = np.stack([PB._row(PB._start_pose(0))] * len(TC.COUNTS))
        w1 = PB._world(mid, 1)
        put(f"calibrate.{nm}.sums", TC._run(mid, C.true_params(mid), start, w1, offsets, point, uv,
                                            max_iterations=0))
        put(f"calibrate.{nm}.counts", TC._run(mid, C.true_params(mid), start, w1, offsets, point, uv))
        put(f"calibrate.{nm}.scene_noisy", TC._scene_run(mid, 0.5))
        put(f"calibrate.{nm}.scene_exact", TC._scene_run(mid))
        # acm_pose_estimate_batch
        K = len(PE.COUNTS)
        world = PB._world(mid, K)
        offsets, point, uv = PB._csr(mid, PE.COUNTS, noisy=False, spoil=False)
        put(f"pose_estimate.{nm}.exact", PE._run(mid, world, offsets, point, uv, inlier_angle=1e-6))
        put(f"pose_estimate.{nm}.spoiled", PE._run(mid, *PE._spoiled(mid), inlier_angle=1e-6))
        offsets, point, uv, _ = PE._outlier_views(mid)
        put(f"pose_estimate.{nm}.outliers",
            PE._run(mid, PB._world(mid, len(PE.OUTLIER_COUNTS)), offsets, point, uv,
                    inlier_angle=PE._angle_of(mid, 2.0), n_hypotheses=600, seed=3))
        # acm_relative_pose_batch
        offsets, uv_a, uv_b, _ = RP.scene(mid, RP.COUNTS)
        put(f"relative_pose.{nm}.exact", RP.run(mid, offsets, uv_a, uv_b, inlier_angle=1e-6))
        put(f"relative_pose.{nm}.spoiled", RP.run(mid, *RP.spoiled(mid), inlier_angle=1e-6))
        for rounds in ((0, 3) if mid in (2, 3) else ()):  # the noisy scene is the fisheye models'
            put(f"relative_pose.{nm}.noisy.refit{rounds}", RP.noisy_on_device(mid, rounds))

    # the long unstaged track, acm_p3p, acm_relative_pose_8pt
    put("triangulate.kb.long_track", TT._c_triangulate(2, T.poses12("wide"),
                                                       *TT._csr(TT._independence_problem())))
    _, poses, count = PE._family_on_device()
    put("p3p.family", {"poses": poses, "count": count})
    _, _, res = RP._family_on_device()
    put("relative_pose_8pt.family", res)

    json.dump(out, open(out_path, "w"), indent=0, sort_keys=True)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--digest":
        return digest(sys.argv[2])
    if len(sys.argv) != 3 or sys.argv[1] != "--libs":
        sys.exit(__doc__)
    libs = [os.path.abspath(p) for p in sys.argv[2].split(",")]
    res = []
    with tempfile.TemporaryDirectory() as d:
        for i, lib in enumerate(libs):
            path = os.path.join(d, f"{i}.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--digest", path], check=True,
                           env=dict(os.environ, ACM_LIB_PATH=lib), stdout=subprocess.DEVNULL)
            res.append(json.load(open(path)))
    names = sorted(set().union(*res))
    differ = 0
    print(f"{'array':70s} " + " ".join(os.path.relpath(p, ROOT) for p in libs))
    for k in names:
        row = [r.get(k, "-") for r in res]
        bad = len(set(row)) != 1
        differ += bad
        print(f"{k:70s} " + " ".join(row) + ("  DIFFERENT" if bad else ""))
    print(f"{len(names)} arrays, {differ} differ")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
