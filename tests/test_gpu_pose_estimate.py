"""acm_p3p and acm_pose_estimate_batch on the GPU: the minimal solver and
RANSAC over it, one workgroup per view.

The P3P accuracy tests run the 4096 triplets of pose_estimation_ref.family()
and bound the device by 10 x the numpy reference's own worst values over the
same triplets (a different algorithm for the quartic and a different rounding,
both in f64).  The views of the RANSAC tests are built as
tests/test_gpu_pose_batch.py builds its own (its helpers are imported): the
world points of view k are point_jacobian_ref's 250-point base set moved by
the inverse of that view's true pose, so the edge rows (behind the camera, NaN,
Inf) are in every long view.

Measured on an MI355X.  acm_p3p on the 4096 triplets:
worst backward residual 1.715e-13 (reference 2.270e-13, bound 10 x), worst
true-pose error of the best solution 3.242e-10 (reference 1.140e-10, bound
10 x), |R^T R - I| 1.1e-15.  Zero noise after refinement, rotation error (rad)
/ translation error: Pinhole 1.2e-13 / 7.4e-14, RadTan 1.4e-8 / 8.0e-9, KB
3.8e-14 / 2.4e-14, DS 7.8e-14 / 5.5e-14, EUCM 2.7e-11 / 1.6e-11, FOV 3.2e-13 /
1.9e-13 (bound 1e-6).  Outliers: the inlier counts equal the numpy RANSAC's in
all ten views (KB 5, 13, 46, 214, 568; DS 6, 14, 42, 217, 588), no observation
near the threshold, no gross outlier in a mask, refined costs equal to the
LM's from the true pose to 9 digits.

UCM: Ucm::unproject keeps the reference's 1 - r^2 denominator (DESIGN.md
section 9), which bends the ray of an exact pixel by up to 1.5e-2 rad (median
4.7e-3) on this set; the kernel takes that call's status and the projection's
inverse (1 + r^2) as the bearing, so UCM runs the zero-noise case like the
other models: 9.0e-12 rad / 5.9e-12 after refinement.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import bearing_ref as BR
import camera_zoo as Z
import pose_estimation_ref as P
import test_gpu_pose_batch as B
from apex_camera_models import _lib, samples
from apex_camera_models.optimizer import (PoseBatchConfig, PoseEstimateConfig, estimate_poses, p3p,
                                          refine_poses)

pytestmark = pytest.mark.gpu

KB, DS = _lib.KANNALA_BRANDT, _lib.DOUBLE_SPHERE
N_BASE = B.N_BASE
OK, TOO_FEW, NO_MODEL = _lib.POSE_EST_OK, _lib.POSE_EST_TOO_FEW_OBSERVATIONS, _lib.POSE_EST_NO_MODEL
# the lane, wave, workgroup and staging boundaries
COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1024, 1025, 2000)
OUTLIER_COUNTS = (8, 20, 64, 300, 1025)
LM_ITERATIONS = 100


# ------------------------------------------------------------------ acm_p3p
@functools.lru_cache(maxsize=None)
def _family_on_device():
    f, X, _, _ = P.family()
    scale = np.linspace(0.5, 3.0, len(f))[:, None, None]  # bearings need not be unit
    poses, count = p3p(torch.as_tensor(f * scale, device="cuda"), torch.as_tensor(X.copy(), device="cuda"))
    poses, count = poses.cpu().numpy(), count.cpu().numpy()
    poses.setflags(write=False)
    count.setflags(write=False)
    return f * scale, poses, count


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4096])
def test_p3p_sizes(n):
    fs, want_poses, want_count = _family_on_device()
    _, X, _, _ = P.family()
    f_t = torch.as_tensor(fs[:n].copy(), device="cuda")
    x_t = torch.as_tensor(X[:n].copy(), device="cuda")
    # the C call, on buffers with a guard row behind the outputs
    poses = torch.full((n + 1, 4, 12), -7.0, dtype=torch.float64, device="cuda")
    count = torch.full((n + 1,), 99, dtype=torch.uint8, device="cuda")
    rc = _lib.load().acm_p3p(n, f_t.data_ptr() if n else None, x_t.data_ptr() if n else None,
                             poses.data_ptr(), count.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.last_error()
    poses, count = poses.cpu().numpy(), count.cpu().numpy()
    assert (poses[n] == -7.0).all() and count[n] == 99, "wrote past n"
    assert count[:n].tobytes() == want_count[:n].tobytes()
    assert poses[:n].tobytes() == want_poses[:n].tobytes(), "a triplet's result depends on n"
    assert (count[:n] >= 1).all() and (count[:n] <= 4).all()


def test_p3p_accuracy():
    """Measured on an MI355X: the reference's worst backward residual 2.270e-13
    and worst true-pose error 1.140e-10; the GPU's 1.715e-13 and 3.242e-10."""
    f, X, R0, t0 = P.family()
    ref_res, ref_err, none = P.family_accuracy()
    assert none == 0
    _, poses, count = _family_on_device()
    res, err, orth = P.check_solutions(poses, count, f, X, R0, t0)
    print(f"acm_p3p: worst backward residual {res:.3e} (reference {ref_res:.3e}), worst true-pose "
          f"error of the best solution {err:.3e} (reference {ref_err:.3e}), |R^T R - I| {orth:.1e}, "
          f"counts {np.bincount(count, minlength=5).tolist()}")
    assert orth <= 1e-12
    assert res <= 10.0 * ref_res
    assert err <= 10.0 * ref_err


def test_p3p_degenerate_triplets():
    f, X = P.degenerate_triplets()
    poses, count = p3p(torch.as_tensor(f, device="cuda"), torch.as_tensor(X, device="cuda"))
    assert (count.cpu().numpy() == 0).all(), count
    assert np.isnan(poses.cpu().numpy()).all()


# ------------------------------------------------- acm_pose_estimate_batch
def _angle_of(mid, threshold_px):
    """mid: a model id (its sample camera) or a zoo camera's name, here and below"""
    _, params, _ = Z.camera_of(mid)
    return math.atan(threshold_px / min(params[0], params[1]))


def _run(mid, world, offsets, point, uv, want_mask=True, want_usable=True, **kw):
    """The C call; numpy outputs, every output prefilled with a sentinel."""
    L = _lib.load()
    c = _lib.PoseEstimateConfig()
    L.acm_pose_estimate_batch_default_config(ctypes.byref(c))
    for key, v in kw.items():
        setattr(c, key, v)
    k, n, m = len(offsets) - 1, len(world), len(point)
    dev = "cuda"
    w_t = torch.as_tensor(np.array(world), device=dev)
    o_t = torch.as_tensor(np.array(offsets), device=dev)
    i_t = torch.as_tensor(np.array(point), device=dev)
    u_t = torch.as_tensor(np.array(uv), device=dev)
    poses = torch.full((k, 12), -7.0, dtype=torch.float64, device=dev)
    status = torch.full((k,), 255, dtype=torch.uint8, device=dev)
    n_inl = torch.full((k,), -1, dtype=torch.int32, device=dev)
    n_use = torch.full((k,), -1, dtype=torch.int32, device=dev)
    mask = torch.full((m + 1,), 77, dtype=torch.uint8, device=dev)
    ws_bytes = L.acm_pose_estimate_batch_workspace_size(k, m)
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device=dev)
    cam = B._model(mid).acm_camera()
    rc = L.acm_pose_estimate_batch(
        ctypes.byref(cam), k, poses.data_ptr(), n, w_t.data_ptr(), o_t.data_ptr(), m,
        i_t.data_ptr() if m else None, u_t.data_ptr() if m else None, ctypes.byref(c),
        status.data_ptr(), n_inl.data_ptr(), mask.data_ptr() if want_mask else None,
        n_use.data_ptr() if want_usable else None, ws.data_ptr(), ws_bytes,
        torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.last_error()
    mask = mask.cpu().numpy()
    assert mask[m] == 77, "the mask was written past n_observations"
    return {"poses": poses.cpu().numpy(), "status": status.cpu().numpy(),
            "n_inliers": n_inl.cpu().numpy(), "n_usable": n_use.cpu().numpy(), "mask": mask[:m]}


def _dev(*arrays):
    """Device copies (the cached inputs are read-only numpy arrays)."""
    return [torch.as_tensor(np.array(a), device="cuda") for a in arrays]


def _records(mid, world, point, uv):
    """The usable rule: (X (m, 3), f (m, 3), usable (m,)) with the bearings of
    tests/bearing_ref.py (no RadTan polish in pose estimation)."""
    point = np.asarray(point, dtype=np.int64)
    in_range = (point >= 0) & (point < len(world))
    X = np.asarray(world)[np.where(in_range, point, 0)]
    f, pixel_ok = BR.bearings(mid, uv, False)
    usable = in_range & np.isfinite(X).all(axis=1) & pixel_ok
    return X, f, usable


def _rule(row, X, f, usable, angle):
    """The inlier rule at the pose `row` (12,): (mask, relative distance of
    every observation's test to the threshold)."""
    Rm, t = row[:9].reshape(3, 3), row[9:]
    cos2 = math.cos(angle) ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        p = X @ Rm.T + t
        d = (f * p).sum(axis=1)
        pp = (p * p).sum(axis=1)
        ok = usable & (d > 0) & (d * d >= cos2 * pp)
        rel = np.abs(d * d - cos2 * pp) / (cos2 * pp)
    return ok, np.where(usable & (d > 0), rel, np.inf)


@pytest.mark.parametrize("mid", sorted(samples.SAMPLES))
def test_zero_noise_every_model(mid):
    K = len(COUNTS)
    world = B._world(mid, K)
    offsets, point, uv = B._csr(mid, COUNTS, noisy=False, spoil=False)
    got = _run(mid, world, offsets, point, uv, inlier_angle=1e-6)
    _, _, usable = _records(mid, world, point, uv)
    seen = set()
    for k in range(K):
        sl = slice(offsets[k], offsets[k + 1])
        nu = int(usable[sl].sum())
        assert got["n_usable"][k] == nu, (k, COUNTS[k], got["n_usable"][k], nu)
        if nu < 4:
            assert got["status"][k] == TOO_FEW, (k, COUNTS[k], got["status"][k])
            assert np.isnan(got["poses"][k]).all() and got["n_inliers"][k] == 0
            assert (got["mask"][sl] == 0).all()
            seen.add("few")
            continue
        seen.add("ok")
        assert got["status"][k] == OK, (k, COUNTS[k], got["status"][k], got["n_inliers"][k], nu)
        assert got["n_inliers"][k] == nu, (k, COUNTS[k], got["n_inliers"][k], nu)
        assert int(got["mask"][sl].sum()) == got["n_inliers"][k]
        assert set(np.unique(got["mask"][sl])) <= {0, 1}
    assert seen == {"few", "ok"}
    # refined over the inliers: test_gpu_pose_batch.py's zero-noise bound
    res = estimate_poses(B._model(mid), *_dev(world, offsets, point, uv),
                         PoseEstimateConfig(inlier_angle=1e-6), refine=True,
                         refine_config=PoseBatchConfig(max_iterations=LM_ITERATIONS))
    assert res.status.cpu().numpy().tobytes() == got["status"].tobytes()
    assert res.inlier_mask.cpu().numpy().tobytes() == got["mask"].tobytes()
    poses = res.poses.cpu().numpy()
    worst = [0.0, 0.0]
    for k in range(K):
        if got["status"][k] != OK:
            assert np.isnan(poses[k]).all()
            continue
        ang, dt, orth = B._pose_errors(poses[k], B._true_pose(k))
        worst = [max(a, b) for a, b in zip(worst, (ang, dt))]
        assert ang <= 1e-6 and dt <= 1e-6, (k, COUNTS[k], ang, dt)
        assert orth <= 1e-12, (k, orth)
    print(f"pose estimate {samples.MODEL_NAMES[mid]} zero noise: rotation error {worst[0]:.3e} rad, "
          f"translation error {worst[1]:.3e} after refinement; n_usable {got['n_usable'].tolist()}")


@functools.lru_cache(maxsize=None)
def _outlier_views(mid):
    """Views of OUTLIER_COUNTS observations: 25-50 % of each moved 50-300 px
    away from the true pixel, the rest with N(0, 0.5 px) noise clipped at 1.5
    px.  Returns (offsets, point, uv, gross (m,) bool)."""
    offsets, point, uv = B._csr(mid, OUTLIER_COUNTS, noisy=False, spoil=False)
    rng = np.random.default_rng(20261020 + mid)
    m = len(point)
    uv = uv + np.clip(rng.normal(0.0, 0.5, (m, 2)), -1.5, 1.5)
    gross = np.zeros(m, dtype=bool)
    for k, c in enumerate(OUTLIER_COUNTS):
        n_out = int(round(rng.uniform(0.25, 0.5) * c))
        gross[offsets[k] + rng.choice(c, n_out, replace=False)] = True
    r = rng.uniform(50.0, 300.0, m)
    phi = rng.uniform(0.0, 2.0 * math.pi, m)
    true_uv = B._true_pixels(mid, len(OUTLIER_COUNTS))[point]
    uv[gross] = (true_uv + np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1))[gross]
    for a in (offsets, point, uv, gross):
        a.setflags(write=False)
    return offsets, point, uv, gross


def _costs(mid, poses, world, offsets, point, uv):
    at = refine_poses(B._model(mid), poses, world, offsets, point, uv, PoseBatchConfig(max_iterations=0))
    return at.cost.cpu().numpy(), at.n_valid.cpu().numpy()


@pytest.mark.parametrize("mid", [KB, DS])
def test_outliers(mid):
    K = len(OUTLIER_COUNTS)
    world = B._world(mid, K)
    offsets, point, uv, gross = _outlier_views(mid)
    angle = _angle_of(mid, 3.0)
    model = B._model(mid)
    w_t, o_t, i_t, u_t = _dev(world, offsets, point, uv)
    res = estimate_poses(model, w_t, o_t, i_t, u_t, PoseEstimateConfig(n_hypotheses=256),
                         threshold_px=3.0)
    status, mask = res.status.cpu().numpy(), res.inlier_mask.cpu().numpy()
    n_inl, poses = res.n_inliers.cpu().numpy(), res.poses.cpu().numpy()
    X, f, usable = _records(mid, world, point, uv)
    assert not mask[gross].any(), "a gross outlier is in the winning mask"
    for k in range(K):
        sl = slice(offsets[k], offsets[k + 1])
        ref = P.ransac(X[sl], f[sl], usable[sl], 256, 1, angle)
        assert ref["status"] == 0 and status[k] == OK, (k, ref["status"], status[k])
        row = np.concatenate([ref["R"].ravel(), ref["t"]])
        _, rel = _rule(row, X[sl], f[sl], usable[sl], angle)
        near = int((rel <= 1e-6).sum())
        print(f"pose estimate {samples.MODEL_NAMES[mid]} view of {OUTLIER_COUNTS[k]}: {n_inl[k]} "
              f"inliers (reference {ref['n_inliers']}, {near} near the threshold), "
              f"{int(gross[sl].sum())} gross outliers, {int(usable[sl].sum())} usable")
        assert n_inl[k] >= ref["n_inliers"] - near, (k, n_inl[k], ref["n_inliers"], near)
        # the mask is the rule at the returned pose
        want, rel = _rule(poses[k], X[sl], f[sl], usable[sl], angle)
        differ = want != (mask[sl] != 0)
        assert (rel[differ] <= 1e-8).all(), (k, np.nonzero(differ)[0], rel[differ])
        assert int(differ.sum()) <= 2, (k, int(differ.sum()))
        assert int(mask[sl].sum()) == n_inl[k]
    # refined over the inliers: as good as the LM started at the true pose
    cfg = PoseBatchConfig(max_iterations=LM_ITERATIONS)
    fine = estimate_poses(model, w_t, o_t, i_t, u_t, PoseEstimateConfig(n_hypotheses=256),
                          threshold_px=3.0, refine=True, refine_config=cfg)
    assert fine.inlier_mask.cpu().numpy().tobytes() == mask.tobytes()
    kept = torch.as_tensor(np.where(mask != 0, point, -1).astype(np.int32), device="cuda")
    truth = np.stack([B._row(B._true_pose(k)) for k in range(K)])
    best = refine_poses(model, torch.as_tensor(truth, device="cuda"), w_t, o_t, kept, u_t, cfg)
    got_cost, got_nv = _costs(mid, fine.poses, w_t, o_t, kept, u_t)
    want_cost, want_nv = best.cost.cpu().numpy(), best.n_valid.cpu().numpy()
    for k in range(K):
        print(f"pose estimate {samples.MODEL_NAMES[mid]} view of {OUTLIER_COUNTS[k]}: refined cost "
              f"{got_cost[k]:.9e}, from the true pose {want_cost[k]:.9e}")
        assert got_nv[k] == want_nv[k] == n_inl[k], (k, got_nv[k], want_nv[k], n_inl[k])
        assert got_cost[k] <= (1.0 + 1e-6) * want_cost[k], (k, got_cost[k], want_cost[k])


def _spoiled(mid):
    K = len(COUNTS)
    world = np.array(B._world(mid, K))
    offsets, point, uv = B._csr(mid, COUNTS, noisy=False, spoil=True)
    world[N_BASE * 13 + 40:N_BASE * 13 + 60:3, 1] = np.nan     # NaN world points in the long view
    offsets = offsets.copy()
    offsets[0], offsets[-1] = -5, len(point) + 7               # outside [0, n_observations]
    return world, offsets, point, uv


@pytest.mark.parametrize("mid", [KB, DS])
def test_spoiled_inputs(mid):
    world, offsets, point, uv = _spoiled(mid)
    m = len(point)
    got = _run(mid, world, offsets, point, uv, inlier_angle=1e-6)
    X, f, usable = _records(mid, world, point, uv)
    assert (~usable).sum() > 100 and not np.isfinite(uv).all() and (point < 0).any() and \
        (point >= len(world)).any()
    clamped = np.clip(offsets, 0, m)
    assert not (got["mask"][~usable] != 0).any(), "an unusable observation is in the mask"
    assert set(np.unique(got["mask"])) <= {0, 1}, "a mask entry of a view's range was not written"
    for k in range(len(COUNTS)):
        sl = slice(clamped[k], clamped[k + 1])
        nu = int(usable[sl].sum())
        assert got["n_usable"][k] == nu, (k, got["n_usable"][k], nu)
        if nu < 4:
            assert got["status"][k] == TOO_FEW and got["n_inliers"][k] == 0
            assert np.isnan(got["poses"][k]).all() and (got["mask"][sl] == 0).all()
        else:
            assert got["status"][k] == OK, (k, got["status"][k])
            assert got["n_inliers"][k] == nu == int(got["mask"][sl].sum())
    # the nullable outputs: the same results without them
    bare = _run(mid, world, offsets, point, uv, want_mask=False, want_usable=False, inlier_angle=1e-6)
    assert (bare["mask"] == 77).all() and (bare["n_usable"] == -1).all()
    for key in ("poses", "status", "n_inliers"):
        assert bare[key].tobytes() == got[key].tobytes(), key


@pytest.mark.parametrize("mid", [KB, DS])
def test_determinism_and_batch_independence(mid):
    world, offsets, point, uv = _spoiled(mid)
    m = len(point)
    offsets = np.clip(offsets, 0, m)
    first = _run(mid, world, offsets, point, uv)
    again = _run(mid, world, offsets, point, uv)
    for key in first:
        assert first[key].tobytes() == again[key].tobytes(), key
    # one view alone, and first / in the middle / last of another batch
    for k in (4, 9, 12, 13):
        sl = slice(offsets[k], offsets[k + 1])
        c = COUNTS[k]
        alone = _run(mid, world, np.array([0, c], dtype=np.int64), point[sl], uv[sl])
        filler_p, filler_u = point[offsets[5]:offsets[6]], uv[offsets[5]:offsets[6]]
        fc = len(filler_p)
        for place in range(3):
            counts = [fc, fc]
            counts.insert(place, c)
            parts_p = [filler_p, filler_p]
            parts_u = [filler_u, filler_u]
            parts_p.insert(place, point[sl])
            parts_u.insert(place, uv[sl])
            off = np.zeros(4, dtype=np.int64)
            off[1:] = np.cumsum(counts)
            batch = _run(mid, world, off, np.concatenate(parts_p), np.concatenate(parts_u))
            for key in ("poses", "status", "n_inliers", "n_usable"):
                assert batch[key][place].tobytes() == alone[key][0].tobytes() == \
                    first[key][k].tobytes(), (k, place, key)
            assert batch["mask"][off[place]:off[place + 1]].tobytes() == alone["mask"].tobytes() == \
                first["mask"][sl].tobytes(), (k, place)
        assert c < 256 or alone["status"][0] == OK


@pytest.mark.parametrize("mid", [KB, DS])
def test_hypothesis_count(mid):
    world = B._world(mid, len(OUTLIER_COUNTS))
    offsets, point, uv, _ = _outlier_views(mid)
    angle = _angle_of(mid, 3.0)
    h256 = _run(mid, world, offsets, point, uv, n_hypotheses=256, inlier_angle=angle)
    h300 = _run(mid, world, offsets, point, uv, n_hypotheses=300, inlier_angle=angle)
    assert (h256["status"] == OK).all()
    assert (h300["n_inliers"] >= h256["n_inliers"]).all(), (h300["n_inliers"], h256["n_inliers"])
    # one hypothesis: no model, or a result consistent with itself
    h1 = _run(mid, world, offsets, point, uv, n_hypotheses=1, inlier_angle=angle)
    X, f, usable = _records(mid, world, point, uv)
    for k in range(len(OUTLIER_COUNTS)):
        sl = slice(offsets[k], offsets[k + 1])
        assert h1["n_inliers"][k] <= h256["n_inliers"][k]
        if h1["status"][k] == NO_MODEL:
            assert np.isnan(h1["poses"][k]).all() and (h1["mask"][sl] == 0).all()
            assert h1["n_inliers"][k] < 4
        else:
            assert h1["status"][k] == OK and h1["n_inliers"][k] >= 4
            assert int(h1["mask"][sl].sum()) == h1["n_inliers"][k]
            want, rel = _rule(h1["poses"][k], X[sl], f[sl], usable[sl], angle)
            differ = want != (h1["mask"][sl] != 0)
            assert (rel[differ] <= 1e-8).all() and int(differ.sum()) <= 2
    # min_inliers above the reachable count
    high = _run(mid, world, offsets, point, uv, n_hypotheses=256, inlier_angle=angle,
                min_inliers=2000)
    assert (high["status"] == NO_MODEL).all()
    assert np.isnan(high["poses"]).all() and (high["mask"] == 0).all()
    assert high["n_inliers"].tobytes() == h256["n_inliers"].tobytes()
