"""acm_homography_4pt and acm_homography_batch on the GPU: the 4-point
homography solver and RANSAC with a refit over it, one workgroup per view
pair.

The solver's accuracy tests run the tuples of homography_ref (4096 general
4-tuples, 200 of each special family) under the bounds of
tests/test_homography_ref.py: median error <= 10 x the numpy reference's
median on the same tuples, worst <= 100 x its worst.  The pairs of the RANSAC
tests are points on the plane n ~ (0.1, -0.2, 1), d = 3 of camera A's frame
seen through test_gpu_relative_pose.true_pose, a motion that differs per pair
-- x in [-1, 1), y in [-0.7, 0.7) for the zero-noise test, which fits every
model's image, x, y in [-4, 4) for the noisy tests of the two fisheye models.
The pixels are the oracle's projections, the bearings the numpy side uses are
tests/bearing_ref.py's (the oracle's unprojection under the kernel's bearing
rule, RadTan polished; test_gpu_relative_pose.bearings).

A gross outlier is drawn by rejection: its transfer sine at the true H
exceeds 10 sin(inlier_angle).

Measured on an MI355X (profiles/homography_perf.log).
acm_homography_4pt returns the bits of the host build of homography.hpp on all
257 tuples compared; on the 4096 tuples worst error 2.6e-10 (reference
1.9e-10), median 7.2e-15 (9.7e-15), |H - H_true| worst 4.3e-11 (3.1e-11);
special families worst / median: rotation 2.8e-14 / 3.9e-16, tau = 1e-3
3.6e-10 / 1.6e-12, plane at 75 degrees 1.7e-11 / 8.7e-15.  Zero noise: worst
|H - H_true| over a model's pairs 5.4e-15 (FOV) .. 2.5e-13 (DS), matched
solution 4.8e-14 .. 1.3e-12, each within 2.1 x the reference's.  Noise and
outliers, seed 1: the inlier counts equal the numpy RANSAC's in all eight
pairs and are all clean matches (KB 24, 67, 189, 643; DS 28, 74, 225, 760), no
moved match in a mask, no borderline match, pose errors equal to the
reference's (3.3e-3 .. 3.1e-2 rad), |H - H_reference| 2.8e-15 .. 2.2e-12; the
counts without the refit are the same, and equal the reference's without it:
the hypotheses agree one by one.  Pure rotation: one solution, tau 6e-16 (KB),
1.4e-15 (Pinhole), |R - R_true| 1.1e-16.  General scene: 42 inliers of 274
usable, the reference's 42.  End to end: 189 tracks, all ACM_TRI_OK, median
distance from the plane 0.160 baselines against 0.155 from the true pose;
estimate_relative_poses on the same pair: OK, 167 inliers, 0.19 rad off.
"""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import camera_zoo as Z
import homography_ref as G
import oracle
import relative_pose_ref as Q
from apex_camera_models import _lib, samples
from apex_camera_models.optimizer import (HomographyConfig, RelativePoseConfig,
                                          estimate_homographies, estimate_relative_poses,
                                          homography_4pt, triangulate, two_view_tracks)
from test_gpu_relative_pose import _angle_of, _model, bearings, project, records, true_pose
from test_homography_ref import CSRC, DRIVER, check_against_reference

pytestmark = pytest.mark.gpu

KB, DS, PINHOLE = _lib.KANNALA_BRANDT, _lib.DOUBLE_SPHERE, _lib.PINHOLE
OK, TOO_FEW, NO_MODEL = _lib.HOMOGRAPHY_OK, _lib.HOMOGRAPHY_TOO_FEW_MATCHES, _lib.HOMOGRAPHY_NO_MODEL
# too few matches, the minimal sample, lanes with and without a hypothesis'
# worth of matches, both sides of the LDS / workspace boundary
COUNTS = (0, 3, 4, 5, 64, 257, 1024, 1025, 2000)
NOISY_COUNTS = (40, 100, 300, 1025)
NOISE_PX, THRESHOLD_PX = 0.5, 3.0
PLANE_N = np.array([0.1, -0.2, 1.0]) / np.linalg.norm([0.1, -0.2, 1.0])
PLANE_D = 3.0


# ------------------------------------------------------- acm_homography_4pt
def _rows(out):
    """homography_4pt's six tensors as homography_ref.unpack's rows (n, 45)."""
    hom, poses, planes, tau, count, front = [x.cpu().numpy() for x in out]
    n = len(count)
    return np.concatenate([count.reshape(n, 1).astype(np.float64), hom, poses.reshape(n, 24),
                           planes.reshape(n, 8), tau.reshape(n, 1), front.astype(np.float64)], axis=1)


@functools.lru_cache(maxsize=None)
def _family_on_device():
    fa, fb = G.family()[:2]
    scale = np.linspace(0.5, 3.0, len(fa))[:, None, None]  # bearings need not be unit
    a, b = fa * scale, fb / scale
    res = _rows(homography_4pt(torch.as_tensor(a, device="cuda"), torch.as_tensor(b, device="cuda")))
    for x in (a, b, res):
        x.setflags(write=False)
    return a, b, res


@functools.lru_cache(maxsize=None)
def _family_on_host():
    """The first 257 tuples through the host build of homography.hpp."""
    import tempfile
    a, b, _ = _family_on_device()
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "homography_host_driver")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, DRIVER, "-o",
                        exe], check=True)
        inp, out = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        np.concatenate([a[:257].reshape(257, 12), b[:257].reshape(257, 12)], axis=1).tofile(inp)
        subprocess.run([exe, inp, out, "4"], check=True)
        return np.fromfile(out).reshape(257, 45)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_4pt_sizes(n):
    """Measured on an MI355X: the same bits as the host build for every n."""
    a, b, want = _family_on_device()
    a_t = torch.as_tensor(a[:n].copy(), device="cuda")
    b_t = torch.as_tensor(b[:n].copy(), device="cuda")
    # the C call, on buffers with a guard row behind the outputs
    dev = "cuda"
    hom = torch.full((n + 1, 9), -7.0, dtype=torch.float64, device=dev)
    poses = torch.full((n + 1, 24), -7.0, dtype=torch.float64, device=dev)
    planes = torch.full((n + 1, 8), -7.0, dtype=torch.float64, device=dev)
    tau = torch.full((n + 1,), -7.0, dtype=torch.float64, device=dev)
    count = torch.full((n + 1,), 99, dtype=torch.uint8, device=dev)
    front = torch.full((n + 1, 2), 99, dtype=torch.uint8, device=dev)
    L = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    rc = L.acm_homography_4pt(n, a_t.data_ptr() if n else None, b_t.data_ptr() if n else None,
                              hom.data_ptr(), poses.data_ptr(), planes.data_ptr(), tau.data_ptr(),
                              count.data_ptr(), front.data_ptr(), stream)
    assert rc == 0, _lib.last_error()
    got = _rows((hom, poses, planes, tau, count, front))
    assert (got[n, 1:43] == -7.0).all() and (got[n, [0, 43, 44]] == 99).all(), "wrote past n"
    assert got[:n].tobytes() == want[:n].tobytes(), "a problem's result depends on n"
    # the host build of the same code: both are within the family's worst
    # error (3e-10) of the truth, so within 1e-9 of each other
    host = _family_on_host()
    if n:
        assert (got[:n, [0, 43, 44]] == host[:n, [0, 43, 44]]).all()
        diff = np.abs(got[:n] - host[:n]).max()
        same = got[:n].tobytes() == host[:n].tobytes()
        print(f"acm_homography_4pt n = {n}: largest difference to the host build {diff:.3e}"
              f"{' (the same bits)' if same else ''}")
        assert diff <= 1e-9
    # without tau: the same results
    hom2 = torch.full((n + 1, 9), -7.0, dtype=torch.float64, device=dev)
    rc = L.acm_homography_4pt(n, a_t.data_ptr() if n else None, b_t.data_ptr() if n else None,
                              hom2.data_ptr(), poses.data_ptr(), planes.data_ptr(), None,
                              count.data_ptr(), front.data_ptr(), stream)
    assert rc == 0, _lib.last_error()
    assert hom2.cpu().numpy().tobytes() == hom.cpu().numpy().tobytes()


def test_4pt_accuracy():
    _, _, res = _family_on_device()
    check_against_reference("acm_homography_4pt", res, G.family(), G.family_accuracy(), 2)


@pytest.mark.parametrize("kind", G.SPECIAL)
def test_4pt_special_families(kind):
    fa, fb = G.special(kind)[:2]
    res = _rows(homography_4pt(torch.as_tensor(np.array(fa), device="cuda"),
                               torch.as_tensor(np.array(fb), device="cuda")))
    check_against_reference(f"acm_homography_4pt, {kind}", res, G.special(kind),
                            G.special_accuracy(kind), 1 if kind == "rotation" else 2)
    if kind == "rotation":
        assert (res[:, 19:22] == 0.0).all() and (res[:, 34:38] == 0.0).all()  # t, the plane
        assert (res[:, 43] == 4).all() and (res[:, 44] == 0).all()


def test_4pt_failures():
    fa, fb = G.failing_tuples()
    res = _rows(homography_4pt(torch.as_tensor(fa, device="cuda"), torch.as_tensor(fb, device="cuda")))
    assert (res[:, 0] == 0).all() and np.isnan(res[:, 1:43]).all() and (res[:, 43:] == 0).all()


# ----------------------------------------------------- acm_homography_batch
def plane_points(rng, m, half_x, half_y):
    x, y = rng.uniform(-half_x, half_x, m), rng.uniform(-half_y, half_y, m)
    z = (PLANE_D - PLANE_N[0] * x - PLANE_N[1] * y) / PLANE_N[2]
    return np.column_stack([x, y, z])


@functools.lru_cache(maxsize=None)
def scene(key, counts, wide=False):
    """(offsets, uv_a, uv_b, X): exact pixels of points on the plane, pair k
    seen through true_pose(key, k); X are the points in camera A's frame.
    key: a model id (its sample camera) or a zoo camera's name."""
    rng = np.random.default_rng(20261024 + Z.camera_of(key)[0])
    offsets = np.zeros(len(counts) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(counts)
    m = int(offsets[-1])
    X = plane_points(rng, m, 4.0, 4.0) if wide else plane_points(rng, m, 1.0, 0.7)
    uv_a = project(key, X)
    uv_b = np.empty_like(uv_a)
    for k in range(len(counts)):
        Rm, t = true_pose(key, k)
        sl = slice(offsets[k], offsets[k + 1])
        uv_b[sl] = project(key, X[sl] @ Rm.T + t)
    for arr in (offsets, uv_a, uv_b, X):
        arr.setflags(write=False)
    return offsets, uv_a, uv_b, X


def run(key, offsets, uv_a, uv_b, bare=False, **kw):
    """The C call; numpy outputs, every output prefilled with a sentinel.
    bare: without the nullable outputs."""
    L = _lib.load()
    c = _lib.HomographyConfig()
    L.acm_homography_batch_default_config(ctypes.byref(c))
    for name, v in kw.items():
        setattr(c, name, v)
    k, m = len(offsets) - 1, len(uv_a)
    dev = "cuda"
    o_t = torch.as_tensor(np.array(offsets), device=dev)
    a_t = torch.as_tensor(np.array(uv_a), device=dev)
    b_t = torch.as_tensor(np.array(uv_b), device=dev)
    hom = torch.full((k + 1, 9), -7.0, dtype=torch.float64, device=dev)
    status = torch.full((k + 1,), 255, dtype=torch.uint8, device=dev)
    n_inl = torch.full((k + 1,), -1, dtype=torch.int32, device=dev)
    poses = torch.full((k + 1, 2, 12), -7.0, dtype=torch.float64, device=dev)
    planes = torch.full((k + 1, 2, 4), -7.0, dtype=torch.float64, device=dev)
    n_sol = torch.full((k + 1,), 99, dtype=torch.uint8, device=dev)
    n_front = torch.full((k + 1, 2), -1, dtype=torch.int32, device=dev)
    tau = torch.full((k + 1,), -7.0, dtype=torch.float64, device=dev)
    n_use = torch.full((k + 1,), -1, dtype=torch.int32, device=dev)
    mask = torch.full((m + 1,), 77, dtype=torch.uint8, device=dev)
    ws_bytes = L.acm_homography_batch_workspace_size(k, m)
    ws = torch.full(((ws_bytes + 7) // 8 + 1,), -3.0, dtype=torch.float64, device=dev)
    cam = _model(key).acm_camera()
    opt = [None] * 7 if bare else [x.data_ptr() for x in (poses, planes, n_sol, n_front, tau, mask,
                                                           n_use)]
    rc = L.acm_homography_batch(
        ctypes.byref(cam), k, o_t.data_ptr(), m, a_t.data_ptr() if m else None,
        b_t.data_ptr() if m else None, ctypes.byref(c), hom.data_ptr(), status.data_ptr(),
        n_inl.data_ptr(), *opt, ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.last_error()
    out = {"homography": hom, "status": status, "n_inliers": n_inl, "poses": poses, "planes": planes,
           "n_solutions": n_sol, "n_front": n_front, "translation": tau, "n_usable": n_use}
    out = {key: v.cpu().numpy() for key, v in out.items()}
    assert (out["homography"][k] == -7.0).all() and out["status"][k] == 255 and \
        out["n_inliers"][k] == -1 and (out["poses"][k] == -7.0).all() and \
        (out["planes"][k] == -7.0).all() and out["n_solutions"][k] == 99 and \
        (out["n_front"][k] == -1).all() and out["translation"][k] == -7.0 and \
        out["n_usable"][k] == -1, "an output was written past n_pairs"
    out = {key: v[:k] for key, v in out.items()}
    mask = mask.cpu().numpy()
    assert mask[m] == 77, "the mask was written past n_matches"
    assert float(ws[-1]) == -3.0, "the workspace was written past its size"
    out["mask"] = mask[:m]
    return out


def solution(got, k):
    """Pair k of run()'s output as a homography_ref solve()-like dict."""
    return dict(count=int(got["n_solutions"][k]), H=got["homography"][k].reshape(3, 3),
                R=got["poses"][k][:, :9].reshape(2, 3, 3), t=got["poses"][k][:, 9:],
                planes=got["planes"][k], tau=float(got["translation"][k]),
                n_front=got["n_front"][k])


def pose_error(sol, R0, t0):
    """The smaller of the slots' max(rotation error, translation direction
    error), radians."""
    return min(max(Q.angles(sol["R"][s], sol["t"][s], R0, t0)) for s in range(sol["count"]))


def rule(H, fa, fb, usable, angle):
    """The inlier rule at H (3, 3): (mask, relative distance of every match's
    transfer test to the threshold)."""
    sin2 = math.sin(angle) ** 2
    fa = np.where(usable[:, None], fa, 0.0)
    fb = np.where(usable[:, None], fb, 0.0)
    ok, _ = G.inliers(H, fa, fb, usable, sin2)
    with np.errstate(invalid="ignore", divide="ignore"):
        e, dot = G.transfer(H, fa, fb)
        rel = np.abs(e - sin2) / sin2
    return ok, np.where(usable & (dot > 0), rel, np.inf)


def check_failed(got, k, sl, status, n_inliers=0):
    assert got["status"][k] == status, (k, got["status"][k])
    assert got["n_inliers"][k] == n_inliers, (k, got["n_inliers"][k])
    assert np.isnan(got["homography"][k]).all() and np.isnan(got["poses"][k]).all()
    assert np.isnan(got["planes"][k]).all() and np.isnan(got["translation"][k])
    assert got["n_solutions"][k] == 0 and (got["n_front"][k] == 0).all()
    assert (got["mask"][sl] == 0).all()


@pytest.mark.parametrize("mid", sorted(samples.SAMPLES))
def test_zero_noise_every_model(mid):
    """The figures of each pair are printed before they are checked.  Measured
    on an MI355X, worst |H - H_true| / matched solution over the pairs
    (reference): Pinhole 5.0e-14 / 4.1e-13 (1.4e-13 / 1.1e-12), RadTan 1.3e-14 /
    7.6e-14 (1.7e-14 / 1.2e-13), KB 2.0e-14 / 1.4e-13 (7.4e-14 / 3.9e-13), DS
    2.5e-13 / 1.3e-12 (1.2e-13 / 6.1e-13), UCM 3.0e-14 / 2.2e-13 (2.9e-14 /
    2.2e-13), EUCM 7.5e-15 / 5.1e-14 (2.1e-14 / 1.4e-13), FOV 5.4e-15 / 4.8e-14
    (7.2e-15 / 6.6e-14)."""
    offsets, uv_a, uv_b, _ = scene(mid, COUNTS)
    got = run(mid, offsets, uv_a, uv_b, inlier_angle=1e-6)
    fa, fb, usable = records(mid, uv_a, uv_b)
    name = samples.MODEL_NAMES[mid]
    figures = {}
    for k, c in enumerate(COUNTS):
        sl = slice(offsets[k], offsets[k + 1])
        if int(usable[sl].sum()) < 4:
            continue
        R0, t0 = true_pose(mid, k)
        H0 = G.true_h(R0, t0, PLANE_N, PLANE_D)
        ref = G.solve(fa[sl], fb[sl])
        ref_h = np.abs(ref["H"] - H0).max()
        ref_e = G.solution_error(ref, R0, t0, PLANE_N, PLANE_D)
        sol = solution(got, k)
        ok = got["status"][k] == OK and sol["count"] == 2
        h = np.abs(sol["H"] - H0).max() if ok else math.nan
        e = G.solution_error(sol, R0, t0, PLANE_N, PLANE_D) if ok else math.nan
        figures[k] = (h, e, ref_h, ref_e)
        print(f"homography {name} zero noise, pair of {c}: status {got['status'][k]}, "
              f"{got['n_inliers'][k]} inliers of {got['n_usable'][k]} usable, |H - H_true| {h:.3e} "
              f"(reference {ref_h:.3e}), matched solution {e:.3e} (reference {ref_e:.3e}), tau "
              f"{sol['tau']:.4f}, n_front {sol['n_front'].tolist()}")
    worst = [0.0, 0.0, 0.0, 0.0]
    for k, c in enumerate(COUNTS):
        sl = slice(offsets[k], offsets[k + 1])
        nu = int(usable[sl].sum())
        assert nu == c, "the scene should be usable throughout"
        assert got["n_usable"][k] == nu, (k, c, got["n_usable"][k], nu)
        if nu < 4:
            check_failed(got, k, sl, TOO_FEW)
            continue
        assert got["status"][k] == OK, (k, c, got["status"][k], got["n_inliers"][k], nu)
        assert got["n_inliers"][k] == nu, (k, c, got["n_inliers"][k], nu)
        assert (got["mask"][sl] == 1).all()
        sol = solution(got, k)
        assert sol["count"] == 2 and sol["n_front"][0] == nu
        G.check_solutions([sol], fa[sl][None], fb[sl][None], *[np.asarray(x)[None] for x in
                                                              (*true_pose(mid, k), PLANE_N, PLANE_D)])
        h, e, ref_h, ref_e = figures[k]
        worst = [max(a, b) for a, b in zip(worst, figures[k])]
        assert h <= max(1e-9, 10.0 * ref_h), (k, c, h, ref_h)
        assert e <= max(1e-9, 10.0 * ref_e), (k, c, e, ref_e)
    print(f"homography {name} zero noise: |H - H_true| {worst[0]:.3e} (reference {worst[2]:.3e}), "
          f"matched solution {worst[1]:.3e} (reference {worst[3]:.3e})")


@functools.lru_cache(maxsize=None)
def noisy_scene(mid):
    """Pairs of NOISY_COUNTS matches on the wide plane: N(0, 0.5 px) noise on
    both pixels, and 25-40 % of each pair's pixels in B moved 50-300 px, drawn
    again until the moved pixel is usable and its transfer sine at the true H
    exceeds 10 sin(angle).  Returns (offsets, uv_a, uv_b, moved (m,) bool)."""
    offsets, uv_a, uv_b, _ = scene(mid, NOISY_COUNTS, wide=True)
    rng = np.random.default_rng(20261025 + mid)
    m = len(uv_a)
    uv_a = uv_a + rng.normal(0.0, NOISE_PX, (m, 2))
    uv_b = uv_b + rng.normal(0.0, NOISE_PX, (m, 2))
    fa, _ = bearings(mid, uv_a)
    sin_min = 10.0 * math.sin(_angle_of(mid, THRESHOLD_PX))
    moved = np.zeros(m, dtype=bool)
    for k, c in enumerate(NOISY_COUNTS):
        H0 = G.true_h(*true_pose(mid, k), PLANE_N, PLANE_D)
        n_out = int(round(rng.uniform(0.25, 0.4) * c))
        for j in offsets[k] + rng.choice(c, n_out, replace=False):
            while True:
                r, phi = rng.uniform(50.0, 300.0), rng.uniform(0.0, 2.0 * math.pi)
                cand = uv_b[j] + r * np.array([math.cos(phi), math.sin(phi)])
                g, ok = bearings(mid, cand[None])
                e, dot = G.transfer(H0, fa[j:j + 1], g)
                if ok[0] and (dot[0] <= 0 or e[0] > sin_min ** 2):
                    uv_b[j] = cand
                    moved[j] = True
                    break
    for arr in (uv_a, uv_b, moved):
        arr.setflags(write=False)
    return offsets, uv_a, uv_b, moved


# The seed of the noisy tests, chosen on the CPU with the reference alone: of
# the seeds 1 .. 8 it is the first for which the numpy RANSAC returns OK for
# all eight pairs with every clean match's pair found (no moved match in a
# mask) and no match within 1e-9 (relative) of the threshold.
NOISY_SEED = 1


@functools.lru_cache(maxsize=None)
def noisy_reference(mid, k, refit_rounds=3):
    offsets, uv_a, uv_b, _ = noisy_scene(mid)
    sl = slice(offsets[k], offsets[k + 1])
    fa, fb, usable = records(mid, uv_a[sl], uv_b[sl])
    return G.ransac(fa, fb, usable, 256, NOISY_SEED, _angle_of(mid, THRESHOLD_PX),
                    refit_rounds=refit_rounds)


@functools.lru_cache(maxsize=None)
def noisy_on_device(mid, refit_rounds):
    offsets, uv_a, uv_b, _ = noisy_scene(mid)
    return run(mid, offsets, uv_a, uv_b, n_hypotheses=256, seed=NOISY_SEED,
               inlier_angle=_angle_of(mid, THRESHOLD_PX), refit_rounds=refit_rounds)


@pytest.mark.parametrize("mid", [KB, DS])
def test_noise_and_outliers(mid):
    """Measured on an MI355X: the counts and pose errors of the module
    docstring; tau 0.128 / 0.149 / 0.171 / 0.091 (KB; true 0.121 / 0.148 / 0.172
    / 0.092) and 0.143 / 0.134 / 0.155 / 0.115 (DS; within 3e-4 of the truth)."""
    offsets, uv_a, uv_b, moved = noisy_scene(mid)
    angle = _angle_of(mid, THRESHOLD_PX)
    got = noisy_on_device(mid, 3)
    fa, fb, usable = records(mid, uv_a, uv_b)
    assert usable.all()
    assert not got["mask"][moved].any(), "a moved match is in the mask"
    for k, c in enumerate(NOISY_COUNTS):
        sl = slice(offsets[k], offsets[k + 1])
        ref = noisy_reference(mid, k)
        assert ref["status"] == 0 and got["status"][k] == OK, (k, ref["status"], got["status"][k])
        _, rel = rule(ref["H"], fa[sl], fb[sl], usable[sl], angle)
        borderline = int((rel <= 1e-9).sum())
        R0, t0 = true_pose(mid, k)
        sol = solution(got, k)
        ref_err, err = pose_error(ref["sol"], R0, t0), pose_error(sol, R0, t0)
        print(f"homography {samples.MODEL_NAMES[mid]} pair of {c}: {got['n_inliers'][k]} inliers "
              f"(reference {ref['n_inliers']}, {ref['refits']} refits, {borderline} borderline), "
              f"{int(moved[sl].sum())} moved, pose error {err:.3e} rad (reference {ref_err:.3e}), "
              f"tau {sol['tau']:.4f} (true {np.linalg.norm(t0) / PLANE_D:.4f}), |H - H_ref| "
              f"{np.abs(sol['H'] - ref['H']).max():.3e}")
        assert got["n_inliers"][k] >= ref["n_inliers"] - borderline, \
            (k, got["n_inliers"][k], ref["n_inliers"])
        # the mask is the rule at the returned H
        want, rel = rule(sol["H"], fa[sl], fb[sl], usable[sl], angle)
        differ = want != (got["mask"][sl] != 0)
        assert (rel[differ] <= 1e-9).all(), (k, np.nonzero(differ)[0], rel[differ])
        assert int(got["mask"][sl].sum()) == got["n_inliers"][k]
        assert sol["count"] == 2 and sol["n_front"][0] <= got["n_inliers"][k]
        assert err <= 2.0 * ref_err, (k, err, ref_err)


@pytest.mark.parametrize("mid", [KB, DS])
def test_without_the_refit(mid):
    """refit_rounds = 0: never more inliers than with the refit.  The device
    scores H itself, so without the refit its winner is the reference's
    hypothesis by hypothesis: the counts are printed side by side."""
    fit, raw = noisy_on_device(mid, 3), noisy_on_device(mid, 0)
    ref = [noisy_reference(mid, k, 0)["n_inliers"] for k in range(len(NOISY_COUNTS))]
    print(f"homography {samples.MODEL_NAMES[mid]} inliers without / with the refit: "
          f"{raw['n_inliers'].tolist()} / {fit['n_inliers'].tolist()}; the reference without: {ref}")
    assert (raw["status"] == OK).all() and (fit["status"] == OK).all()
    assert (raw["n_inliers"] <= fit["n_inliers"]).all()


@pytest.mark.parametrize("mid", [KB, PINHOLE])
def test_pure_rotation(mid):
    rng = np.random.default_rng(31 + mid)
    n = 200
    X = np.column_stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-0.7, 0.7, n),
                         rng.uniform(2.5, 6.0, n)])
    R0 = Q.exp_so3(np.array([0.05, -0.08, 0.1]))
    uv_a, uv_b = project(mid, X), project(mid, X @ R0.T)
    off = np.array([0, n], dtype=np.int64)
    got = run(mid, off, uv_a, uv_b, inlier_angle=1e-6)
    fa, fb, usable = records(mid, uv_a, uv_b)
    ref = G.solve(fa, fb)
    sol = solution(got, 0)
    err, ref_err = np.abs(sol["R"][0] - R0).max(), np.abs(ref["R"][0] - R0).max()
    print(f"homography {samples.MODEL_NAMES[mid]} pure rotation: status {got['status'][0]}, "
          f"{got['n_inliers'][0]} inliers, {sol['count']} solution, tau {sol['tau']:.3e}, |R - "
          f"R_true| {err:.3e} (reference {ref_err:.3e}), |H - R_true| "
          f"{np.abs(sol['H'] - R0).max():.3e}")
    assert got["status"][0] == OK and got["n_inliers"][0] == n and (got["mask"] == 1).all()
    assert sol["count"] == 1 and (sol["t"][0] == 0.0).all() and (sol["planes"][0] == 0.0).all()
    assert np.isnan(sol["R"][1]).all() and sol["n_front"].tolist() == [n, 0]
    assert sol["tau"] <= G.ROTATION_FLOOR
    assert err <= max(1e-9, 10.0 * ref_err)


def pixels(mid, pts):
    """The oracle's projections; NaN where a point does not project."""
    params, (w, h) = samples.SAMPLES[mid]
    uv, st, _ = oracle.project(mid, params, w, h, np.ascontiguousarray(pts))
    return np.where((st == 0)[:, None], uv, np.nan)


def test_general_scene_is_not_a_plane():
    """relative_pose_ref._scene, 300 matches, 5e-3 rad: the homography's
    inlier count tells the caller that the scene is no plane."""
    mid, n, angle = KB, 300, 5e-3
    rng = np.random.default_rng(41)
    R0, t0 = Q.exp_so3(np.array([0.2, -0.3, 0.1])), np.array([0.3, -0.2, 0.5])
    d, _ = Q._scene(rng, 1, n, R0[None], t0[None])
    X = d[0] * rng.uniform(2.0, 8.0, n)[:, None]
    uv_a, uv_b = pixels(mid, X), pixels(mid, X @ R0.T + t0)
    off = np.array([0, n], dtype=np.int64)
    got = run(mid, off, uv_a, uv_b, inlier_angle=angle)
    fa, fb, usable = records(mid, uv_a, uv_b)
    ref = G.ransac(fa, fb, usable, 256, 1, angle)
    _, rel = rule(ref["H"], fa, fb, usable, angle)
    borderline = int((rel <= 1e-9).sum())
    print(f"homography on a general scene: {got['n_inliers'][0]} inliers of {got['n_usable'][0]} "
          f"usable (reference {ref['n_inliers']}, {borderline} borderline), tau "
          f"{got['translation'][0]:.3f}")
    assert got["n_usable"][0] == int(usable.sum()) and usable.sum() >= 200
    assert got["status"][0] == OK and ref["status"] == 0
    assert abs(int(got["n_inliers"][0]) - ref["n_inliers"]) <= borderline
    assert 2 * got["n_inliers"][0] < usable.sum()


def spoiled(mid):
    offsets, uv_a, uv_b, _ = scene(mid, COUNTS)
    uv_a, uv_b, offsets = uv_a.copy(), uv_b.copy(), offsets.copy()
    j = np.arange(len(uv_a))
    uv_a[j % 37 == 5, 0] = np.nan
    uv_b[j % 53 == 7, 1] = np.inf
    uv_b[j % 41 == 11] = np.nan
    uv_a[j % 43 == 13] = [1e5, -1e5]   # far outside the image
    uv_b[j % 47 == 17] = [-4e3, 6e3]
    offsets[0], offsets[-1] = -5, len(uv_a) + 7  # outside [0, n_matches]
    return offsets, uv_a, uv_b


@pytest.mark.parametrize("mid", [KB, DS])
def test_spoiled_inputs(mid):
    offsets, uv_a, uv_b = spoiled(mid)
    m = len(uv_a)
    got = run(mid, offsets, uv_a, uv_b, inlier_angle=1e-6)
    fa, fb, usable = records(mid, uv_a, uv_b)
    assert (~usable).sum() > 100
    clamped = np.clip(offsets, 0, m)
    assert not (got["mask"][~usable] != 0).any(), "an unusable match is in the mask"
    assert set(np.unique(got["mask"])) <= {0, 1}, "a mask entry of a pair's range was not written"
    for k in range(len(COUNTS)):
        sl = slice(clamped[k], clamped[k + 1])
        nu = int(usable[sl].sum())
        assert got["n_usable"][k] == nu, (k, got["n_usable"][k], nu)
        if nu < 4:
            check_failed(got, k, sl, TOO_FEW)
        else:
            assert got["status"][k] == OK, (k, got["status"][k])
            assert got["n_inliers"][k] == nu == int(got["mask"][sl].sum())
    # the nullable outputs: the same results without them
    bare = run(mid, offsets, uv_a, uv_b, bare=True, inlier_angle=1e-6)
    assert (bare["mask"] == 77).all() and (bare["n_usable"] == -1).all()
    assert (bare["poses"] == -7.0).all() and (bare["n_solutions"] == 99).all()
    for key in ("homography", "status", "n_inliers"):
        assert bare[key].tobytes() == got[key].tobytes(), key
    # decreasing offsets: empty ranges, nothing read
    down = run(mid, np.array([50, 20, 10, 60], dtype=np.int64), uv_a[:100], uv_b[:100],
               inlier_angle=1e-6)
    assert down["n_usable"][:2].tolist() == [0, 0] and (down["status"][:2] == TOO_FEW).all()


@pytest.mark.parametrize("mid", [KB, DS])
def test_determinism_and_batch_independence(mid):
    offsets, uv_a, uv_b, _ = noisy_scene(mid)
    angle = _angle_of(mid, THRESHOLD_PX)
    first = run(mid, offsets, uv_a, uv_b, inlier_angle=angle)
    again = run(mid, offsets, uv_a, uv_b, inlier_angle=angle)
    for key in first:
        assert first[key].tobytes() == again[key].tobytes(), key
    # one pair alone, and first / in the middle / last of another batch
    filler = slice(offsets[0], offsets[1])
    fc = NOISY_COUNTS[0]
    per_pair = [key for key in first if key != "mask"]
    for k in (1, 3):
        sl = slice(offsets[k], offsets[k + 1])
        c = NOISY_COUNTS[k]
        alone = run(mid, np.array([0, c], dtype=np.int64), uv_a[sl], uv_b[sl], inlier_angle=angle)
        for place in range(3):
            counts, parts_a, parts_b = [fc, fc], [uv_a[filler]] * 2, [uv_b[filler]] * 2
            counts.insert(place, c)
            parts_a.insert(place, uv_a[sl])
            parts_b.insert(place, uv_b[sl])
            off = np.zeros(4, dtype=np.int64)
            off[1:] = np.cumsum(counts)
            batch = run(mid, off, np.concatenate(parts_a), np.concatenate(parts_b),
                        inlier_angle=angle)
            for key in per_pair:
                assert batch[key][place].tobytes() == alone[key][0].tobytes() == \
                    first[key][k].tobytes(), (k, place, key)
            assert batch["mask"][off[place]:off[place + 1]].tobytes() == alone["mask"].tobytes() == \
                first["mask"][sl].tobytes(), (k, place)
        assert alone["status"][0] == OK


@pytest.mark.parametrize("mid", [KB, DS])
def test_hypothesis_count(mid):
    offsets, uv_a, uv_b, _ = noisy_scene(mid)
    angle = _angle_of(mid, THRESHOLD_PX)
    fa, fb, usable = records(mid, uv_a, uv_b)
    h256 = run(mid, offsets, uv_a, uv_b, n_hypotheses=256, inlier_angle=angle, refit_rounds=0)
    h300 = run(mid, offsets, uv_a, uv_b, n_hypotheses=300, inlier_angle=angle, refit_rounds=0)
    assert (h256["status"] == OK).all()
    # more hypotheses under the same key: never a worse winner
    assert (h300["n_inliers"] >= h256["n_inliers"]).all(), (h300["n_inliers"], h256["n_inliers"])
    # one hypothesis: no model, or a result consistent with itself
    h1 = run(mid, offsets, uv_a, uv_b, n_hypotheses=1, inlier_angle=angle)
    for k in range(len(NOISY_COUNTS)):
        sl = slice(offsets[k], offsets[k + 1])
        if h1["status"][k] == NO_MODEL:
            check_failed(h1, k, sl, NO_MODEL, h1["n_inliers"][k])
            assert h1["n_inliers"][k] < 4
        else:
            assert h1["status"][k] == OK and h1["n_inliers"][k] >= 4
            assert int(h1["mask"][sl].sum()) == h1["n_inliers"][k]
            want, rel = rule(h1["homography"][k].reshape(3, 3), fa[sl], fb[sl], usable[sl], angle)
            differ = want != (h1["mask"][sl] != 0)
            assert (rel[differ] <= 1e-9).all()
    # min_inliers above the reachable count: the best count, without the refit
    high = run(mid, offsets, uv_a, uv_b, n_hypotheses=256, inlier_angle=angle, min_inliers=5000)
    for k in range(len(NOISY_COUNTS)):
        check_failed(high, k, slice(offsets[k], offsets[k + 1]), NO_MODEL, h256["n_inliers"][k])


def test_end_to_end_planar_pair():
    """estimate_homographies -> the slot that matches the truth ->
    two_view_tracks -> triangulate on the noisy KB pair of 300 matches: every
    inlier track triangulates, and the points lie as close to the true plane
    (in units of the baseline) as those from the true pose."""
    mid, k = KB, 2
    offsets, uv_a, uv_b, moved = noisy_scene(mid)
    sl = slice(offsets[k], offsets[k + 1])
    off = np.array([0, NOISY_COUNTS[k]], dtype=np.int64)
    model = _model(mid)
    a_t = torch.as_tensor(uv_a[sl].copy(), device="cuda")
    b_t = torch.as_tensor(uv_b[sl].copy(), device="cuda")
    res = estimate_homographies(model, off, a_t, b_t, HomographyConfig(seed=NOISY_SEED),
                                threshold_px=THRESHOLD_PX)
    assert res.status.cpu().numpy()[0] == OK
    want = noisy_on_device(mid, 3)
    assert res.inlier_mask.cpu().numpy().tobytes() == want["mask"][sl].tobytes()
    assert res.homography.cpu().numpy()[0].tobytes() == want["homography"][k].tobytes()
    assert res.poses.cpu().numpy()[0].tobytes() == want["poses"][k].tobytes()
    assert res.poses.shape == (1, 2, 12) and res.planes.shape == (1, 2, 4)
    R0, t0 = true_pose(mid, k)
    poses = res.poses.cpu().numpy()[0]
    errs = [max(Q.angles(p[:9].reshape(3, 3), p[9:], R0, t0)) for p in poses]
    slot = int(np.argmin(errs))
    chosen = res.pose_slot(torch.tensor([slot]))
    assert chosen.cpu().numpy().tobytes() == res.pose_slot(slot).cpu().numpy().tobytes() == \
        poses[slot:slot + 1].tobytes()
    view_poses, t_off, t_view, t_uv, match = two_view_tracks(off, a_t, b_t, res.inlier_mask, chosen)
    n = int(res.n_inliers.cpu().numpy()[0])
    assert t_off.shape[0] == n + 1 and t_view.shape[0] == 2 * n and view_poses.shape == (2, 12)
    assert not moved[sl][match.cpu().numpy()].any()
    tri = triangulate(model, view_poses, t_off, t_view, t_uv)
    assert (tri.status.cpu().numpy() == _lib.TRI_OK).all()
    base = np.linalg.norm(t0)
    truth = torch.as_tensor(np.stack([np.r_[np.eye(3).ravel(), np.zeros(3)],
                                      np.r_[R0.ravel(), t0]]), device="cuda")
    best = triangulate(model, truth, t_off, t_view, t_uv)
    assert (best.status.cpu().numpy() == _lib.TRI_OK).all()
    # distance from the true plane in units of the baseline
    dist = np.abs(tri.points.cpu().numpy() @ PLANE_N - PLANE_D / base)
    ref = np.abs(best.points.cpu().numpy() @ PLANE_N - PLANE_D) / base
    err, ref_err = np.median(dist), np.median(ref)
    rp = estimate_relative_poses(model, off, a_t, b_t, RelativePoseConfig(seed=NOISY_SEED),
                                 threshold_px=THRESHOLD_PX)
    rp_pose = rp.poses.cpu().numpy()[0]
    rp_err = (max(Q.angles(rp_pose[:9].reshape(3, 3), rp_pose[9:], R0, t0))
              if np.isfinite(rp_pose).all() else math.nan)
    print(f"planar pair end to end: slot {slot} (pose errors {errs[0]:.3e}, {errs[1]:.3e} rad), {n} "
          f"tracks, median distance from the plane {err:.3e} baselines (from the true pose "
          f"{ref_err:.3e}); estimate_relative_poses on the same pair: status "
          f"{rp.status.cpu().numpy()[0]}, {rp.n_inliers.cpu().numpy()[0]} inliers, pose error "
          f"{rp_err:.3e} rad")
    assert err <= 2.0 * ref_err
