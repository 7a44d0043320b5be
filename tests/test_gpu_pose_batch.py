"""acm_pose_optimize_batch on the GPU: every view's 6-DoF LM in one launch.

Inputs are built from point_jacobian_ref's 250-point base set as
tests/test_gpu_pose.py builds its own: the world points of a view are the base
set moved by the inverse of that view's true pose, so the set's edge rows
(behind the camera, NaN, Inf) are in every view.

Sums (max_iterations = 0), all seven models at their sample cameras and the
solver subset of tests/camera_zoo.py (views of 2, 257 and 1000 observations
there): per view the 21 + 6 + 1 sums against float64 terms
from the 50-digit point Jacobians, summed with math.fsum, per entry |gpu -
exact| <= max(1e-10 |exact|, 1e-13 sum |terms|) (test_pose_normal_equations'
bound).  Solver: the bounds of tests/test_gpu_pose.py.

Measured on an MI355X: sums, worst |gpu - exact| /
bound Pinhole 2.0e-4, RadTan 5.3e-4, KB 1.2e-3, DS 3.9e-4, UCM 2.9e-4, EUCM
1.0e-3, FOV 2.0e-4; zoo cameras 3.1e-6 (pinhole_aniso) ... 9.1e-4
(eucm_alpha_half).  Zero noise (bound 1e-6): KB rotation error
4.9e-11 rad, translation error 2.6e-9 after 43-46 iterations; the other six
models <= 1.0e-10 after 4-5.  Noise: cost / scipy <= 1 + 1.7e-8; largest
relative difference to acm_pose_optimize's cost KB 5.0e-15, DS 6.6e-15.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import camera_zoo as Z
import oracle
import point_jacobian_ref as R
import triangulation_ref as T
from apex_camera_models import _lib, samples
from apex_camera_models.optimizer import (Pose, PoseBatchConfig, alternate_bundle_adjustment,
                                          refine_poses)

pytestmark = pytest.mark.gpu

KB, DS = _lib.KANNALA_BRANDT, _lib.DOUBLE_SPHERE
TRUE_DELTA = np.array([0.3, -0.1, 0.2, 0.1, -0.2, 0.15])
START_DELTA = [0.02, -0.01, 0.015, 0.01, 0.02, -0.015]
# the lane, wave, workgroup and staging boundaries
COUNTS = (0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1000, 1024, 1025, 3000)
ZOO_COUNTS = (2, 257, 1000)  # too few to take part; across a wave and a workgroup seam
ALL_MODELS = tuple(sorted(samples.SAMPLES))
N_BASE = R.N_BASE
# The solver bounds below are tests/test_gpu_pose.py's, which runs
# acm_pose_optimize under acm_lm_default_config: 100 iterations.  The batched
# default is 20; from these starts the LM (either entry point, the same
# iterates) takes 3-4 iterations for DS and 43-44 for KB, whose first steps are
# rejected five times over, so the recovery and optimum tests run both solvers
# with the limit the bounds were set under.
LM_ITERATIONS = 100


def _model(mid):
    """mid: a model id (its sample camera) or a zoo camera's name, here and below"""
    return Z.device_model(mid)


def _Rt(pose):
    return np.array(pose.rotation), np.array(pose.translation)


def _row(pose):
    return np.concatenate([np.array(pose.rotation).ravel(), np.array(pose.translation)])


def _pose_of_row(row):
    return Pose(np.asarray(row[:9]).reshape(3, 3).tolist(), list(row[9:]))


def _true_pose(k):
    """Distinct true poses: view k's is the identity moved by (1 + k / 10) TRUE_DELTA."""
    return Pose().retract(list(TRUE_DELTA * (1.0 + 0.1 * k)))


def _start_pose(k):
    """Each view its own start: its true pose moved by (1 - k / 40) START_DELTA."""
    return _true_pose(k).retract(list(np.array(START_DELTA) * (1.0 - 0.025 * k)))


@functools.lru_cache(maxsize=None)
def _world(mid, n_views):
    """(250 n_views, 3): block k is the base set moved by the inverse of view
    k's true pose (read-only)."""
    blocks = []
    for k in range(n_views):
        Rm, t = _Rt(_true_pose(k))
        with np.errstate(invalid="ignore"):
            blocks.append((R.base_points(mid) - t) @ Rm)  # R^T (p - t), row vectors
    w = np.concatenate(blocks)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _noise():
    n = np.random.default_rng(20251206).normal(0.0, 0.5, (16001, 2))
    n.setflags(write=False)
    return n


@functools.lru_cache(maxsize=None)
def _true_pixels(mid, n_views):
    """(250 n_views, 2): the device projection of every world point through
    its own view's true pose, NaN where it fails (as test_gpu_pose.py)."""
    world = _world(mid, n_views)
    cam_pts = np.empty_like(world)
    for k in range(n_views):
        Rm, t = _Rt(_true_pose(k))
        with np.errstate(invalid="ignore"):
            cam_pts[N_BASE * k:N_BASE * (k + 1)] = world[N_BASE * k:N_BASE * (k + 1)] @ Rm.T + t
    uv, _, _ = _model(mid).project_batch(torch.as_tensor(cam_pts, device="cuda"))
    out = uv.cpu().numpy()
    out.setflags(write=False)
    return out


def _csr(mid, counts, noisy, spoil):
    """View k observes `counts[k]` points of its own block, tiled from a
    start that differs per view.  spoil: NaN pixels and out-of-range indices
    are put in at fixed places.  Returns (offsets, obs_point, obs_uv)."""
    k_views = len(counts)
    offsets = np.zeros(k_views + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(counts)
    m = int(offsets[-1])
    point = np.empty(m, dtype=np.int32)
    for k, c in enumerate(counts):
        point[offsets[k]:offsets[k + 1]] = N_BASE * k + (np.arange(c) + 17 * k) % N_BASE
    uv = _true_pixels(mid, k_views)[point].copy()
    if noisy:
        uv += _noise()[:m]
    if spoil:
        j = np.arange(m)
        uv[j % 37 == 5, 0] = np.nan
        uv[j % 53 == 7, 1] = np.inf
        point[j % 41 == 11] = -1
        point[j % 43 == 13] = N_BASE * k_views  # == n_points
    return offsets, point, uv


def _run(mid, poses, world, offsets, point, uv, max_iterations=None):
    """The C call; numpy outputs.  poses: (K, 12)."""
    L = _lib.load()
    c = _lib.PoseBatchConfig()
    L.acm_pose_optimize_batch_default_config(ctypes.byref(c))
    if max_iterations is not None:
        c.max_iterations = max_iterations
    k, n, m = len(poses), len(world), len(point)
    dev = "cuda"
    p_t = torch.as_tensor(np.ascontiguousarray(poses), device=dev).clone()
    w_t = torch.as_tensor(np.array(world), device=dev)
    o_t = torch.as_tensor(np.ascontiguousarray(offsets), device=dev)
    i_t = torch.as_tensor(np.ascontiguousarray(point), device=dev)
    u_t = torch.as_tensor(np.ascontiguousarray(uv), device=dev)
    status = torch.full((k,), 255, dtype=torch.uint8, device=dev)
    cost = torch.full((k,), -1.0, dtype=torch.float64, device=dev)
    n_valid = torch.full((k,), -1, dtype=torch.int32, device=dev)
    iters = torch.full((k,), -1, dtype=torch.int32, device=dev)
    info = torch.full((k, 21), -1.0, dtype=torch.float64, device=dev)
    ws_bytes = L.acm_pose_optimize_batch_workspace_size(k, m)
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device=dev)
    cam = _model(mid).acm_camera()
    rc = L.acm_pose_optimize_batch(
        ctypes.byref(cam), k, p_t.data_ptr(), n, w_t.data_ptr(), o_t.data_ptr(), m,
        i_t.data_ptr() if m else None, u_t.data_ptr() if m else None, ctypes.byref(c),
        status.data_ptr(), cost.data_ptr(), n_valid.data_ptr(), iters.data_ptr(), info.data_ptr(),
        ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.last_error()
    return {"poses": p_t.cpu().numpy(), "status": status.cpu().numpy(), "cost": cost.cpu().numpy(),
            "n_valid": n_valid.cpu().numpy(), "iterations": iters.cpu().numpy(),
            "information": info.cpu().numpy()}


@functools.lru_cache(maxsize=None)
def _view_reference(mid, k, n_views):
    """At view k's start pose, per point of its block: the 2 x 6 pose
    Jacobian from the mp point Jacobians (250, 2, 6), the 50-digit projection
    (250, 2) and the rows that have a reference."""
    Rm, t = _Rt(_start_pose(k))
    with np.errstate(invalid="ignore"):
        p = _world(mid, n_views)[N_BASE * k:N_BASE * (k + 1)] @ Rm.T + t
    have = R.reference_rows(mid, p)
    Jp = R.mp_jacobians(mid, p)
    uv = R.mp_project(mid, p, have)
    J6 = np.full((len(p), 2, 6), np.nan)
    for i in np.nonzero(have)[0]:
        x, y, z = p[i]
        neg_skew = np.array([[0.0, z, -y], [-z, 0.0, x], [y, -x, 0.0]])  # -[p]x
        J6[i] = Jp[i] @ np.hstack([np.eye(3), neg_skew])
    return J6, uv, have


@pytest.mark.parametrize("mid", ALL_MODELS + Z.SOLVER_SUBSET)
def test_sums_against_50_digits(mid):
    counts = COUNTS if mid in ALL_MODELS else ZOO_COUNTS
    K = len(counts)
    world = _world(mid, K)
    offsets, point, uv = _csr(mid, counts, noisy=True, spoil=True)
    start = np.stack([_row(_start_pose(k)) for k in range(K)])
    got = _run(mid, start, world, offsets, point, uv, max_iterations=0)
    assert got["poses"].tobytes() == start.tobytes(), "max_iterations = 0 moved a pose"
    assert not np.isfinite(world).all(), "the base set should carry NaN / Inf world points"
    worst, seen = 0.0, set()
    for k in range(K):
        sl = slice(offsets[k], offsets[k + 1])
        idx, obs = point[sl].astype(np.int64), uv[sl]
        in_range = (idx >= 0) & (idx < len(world))
        local = np.where(in_range, idx - N_BASE * k, 0)
        assert ((local >= 0) & (local < N_BASE)).all()
        # only the points a view names need a reference
        if counts[k] == 0:
            valid = np.zeros(0, dtype=bool)
        else:
            J6b, uvb, haveb = _view_reference(mid, k, K)
            assert int(haveb.sum()) >= 240, "more than 10 base rows without a reference"
            valid = in_range & haveb[local] & np.isfinite(obs).all(axis=1) & \
                np.isfinite(world[np.where(in_range, idx, 0)]).all(axis=1)
        nv = int(valid.sum())
        assert got["n_valid"][k] == nv, (k, counts[k], got["n_valid"][k], nv)
        assert got["iterations"][k] == 0
        if nv < 3:
            assert got["status"][k] == _lib.POSE_TOO_FEW_OBSERVATIONS, (k, counts[k])
            assert math.isnan(got["cost"][k]) and (got["information"][k] == 0.0).all()
            seen.add("few")
            continue
        assert got["status"][k] == _lib.POSE_OK, (k, counts[k], got["status"][k])
        seen.add("ok")
        J = J6b[local][valid]                 # (m, 2, 6)
        r = (uvb[local] - obs)[valid]         # (m, 2)
        want, mag = [], []

        def put(terms):
            want.append(math.fsum(terms))
            mag.append(math.fsum(np.abs(terms)))
        for a in range(6):
            for b in range(a, 6):
                put(np.concatenate([J[:, 0, a] * J[:, 0, b], J[:, 1, a] * J[:, 1, b]]))
        put(0.5 * np.concatenate([r[:, 0] ** 2, r[:, 1] ** 2]))
        want, mag = np.array(want), np.array(mag)
        have_v = np.concatenate([got["information"][k], [got["cost"][k]]])
        err = np.abs(have_v - want)
        bound = np.maximum(1e-10 * np.abs(want), 1e-13 * mag)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        worst = max(worst, float(ratio.max()))
        assert (err <= bound).all(), (k, counts[k], int(np.argmax(ratio)), float(ratio.max()))
    assert seen == {"few", "ok"}
    print(f"pose batch sums {Z.label(mid)}: worst |gpu - exact| / bound = {worst:.3e}")


def _same(a, b, k_a, k_b, what):
    for key in ("poses", "status", "cost", "n_valid", "iterations", "information"):
        assert a[key][k_a].tobytes() == b[key][k_b].tobytes(), (what, key, k_a, k_b)


@pytest.mark.parametrize("mid", [KB, DS])
def test_batch_independence(mid):
    K = len(COUNTS)
    world = _world(mid, K)
    offsets, point, uv = _csr(mid, COUNTS, noisy=True, spoil=True)
    start = np.stack([_row(_start_pose(k)) for k in range(K)])
    batch = _run(mid, start, world, offsets, point, uv)
    again = _run(mid, start, world, offsets, point, uv)
    # the batch reversed: view K - 1 - k first
    r_counts = COUNTS[::-1]
    r_off = np.zeros(K + 1, dtype=np.int64)
    r_off[1:] = np.cumsum(r_counts)
    r_point = np.concatenate([point[offsets[k]:offsets[k + 1]] for k in range(K - 1, -1, -1)])
    r_uv = np.concatenate([uv[offsets[k]:offsets[k + 1]] for k in range(K - 1, -1, -1)])
    rev = _run(mid, start[::-1], world, r_off, r_point, r_uv)
    moved = 0
    for k in range(K):
        _same(batch, again, k, k, "second call")
        _same(batch, rev, k, K - 1 - k, "reversed batch")
        sl = slice(offsets[k], offsets[k + 1])
        alone = _run(mid, start[k:k + 1], world, np.array([0, COUNTS[k]], dtype=np.int64),
                     point[sl], uv[sl])
        _same(batch, alone, k, 0, "alone")
        moved += int(batch["iterations"][k] > 0)
    assert moved >= 8, "the default config should have iterated on the long views"
    print(f"pose batch independence {samples.MODEL_NAMES[mid]}: status {batch['status'].tolist()}, "
          f"iterations {batch['iterations'].tolist()}, cost {batch['cost'].tolist()}")


def _pose_errors(row, true_pose):
    Rt, tt = _Rt(true_pose)
    Re, te = row[:9].reshape(3, 3), row[9:]
    c = (np.trace(Re @ Rt.T) - 1.0) / 2.0
    s = np.linalg.norm(Re @ Rt.T - (Re @ Rt.T).T) / (2.0 * math.sqrt(2.0))  # sin(angle)
    return math.atan2(s, c), float(np.linalg.norm(te - tt)), float(np.abs(Re @ Re.T - np.eye(3)).max())


@pytest.mark.parametrize("mid", sorted(samples.SAMPLES))
def test_zero_noise_recovery(mid):
    K, n = 8, 2000
    world = _world(mid, K)
    offsets, point, uv = _csr(mid, (n,) * K, noisy=False, spoil=False)
    start = np.stack([_row(_true_pose(k).retract(START_DELTA)) for k in range(K)])
    got = _run(mid, start, world, offsets, point, uv, max_iterations=LM_ITERATIONS)
    worst = [0.0, 0.0, 0.0]
    for k in range(K):
        ang, dt, orth = _pose_errors(got["poses"][k], _true_pose(k))
        worst = [max(a, b) for a, b in zip(worst, (ang, dt, orth))]
        assert got["status"][k] == _lib.POSE_OK, (k, got["status"][k], got["iterations"][k])
        assert ang <= 1e-6 and dt <= 1e-6, (k, ang, dt)
        assert orth <= 1e-12, (k, orth)
    print(f"pose batch {samples.MODEL_NAMES[mid]} zero noise: rotation error {worst[0]:.3e} rad, "
          f"translation error {worst[1]:.3e}, |R R^T - I| {worst[2]:.1e}, iterations "
          f"{got['iterations'].tolist()}")


def _scipy_cost(mid, start, world, obs):
    from scipy.optimize import least_squares
    params, (w, h) = samples.SAMPLES[mid]

    def resid(d):
        Rm, t = _Rt(start.retract(list(d)))
        with np.errstate(invalid="ignore"):
            uv, st, _ = oracle.project(mid, params, w, h, world @ Rm.T + t)
        r = uv - obs
        r[(st != 0) | ~np.isfinite(r).all(axis=1)] = 0.0
        return r.ravel()
    sol = least_squares(resid, np.zeros(6), method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    return float(sol.cost)


def _single_cost(mid, start, world_t, obs_t):
    """acm_pose_optimize on one view's gathered arrays."""
    L = _lib.load()
    n = obs_t.shape[0]
    cfg = _lib.LmConfig()
    L.acm_lm_default_config(ctypes.byref(cfg))
    assert cfg.max_iterations == LM_ITERATIONS
    ws_bytes = L.acm_pose_optimize_workspace_size(n)
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device="cuda")
    cam, ap, summ = _model(mid).acm_camera(), start.acm_pose(), _lib.LmSummary()
    rc = L.acm_pose_optimize(ctypes.byref(cam), ctypes.byref(ap), n, world_t.data_ptr(),
                             _lib.LAYOUT_AOS, obs_t.data_ptr(), ctypes.byref(cfg),
                             _lib.ALLREDUCE_FN(), None, ctypes.byref(summ), ws.data_ptr(), ws_bytes,
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.last_error()
    return summ.final_cost


@pytest.mark.parametrize("mid", [KB, DS])
def test_reaches_scipy_optimum_with_noise(mid):
    K, n = 6, 2000
    world = _world(mid, K)
    offsets, point, uv = _csr(mid, (n,) * K, noisy=True, spoil=False)
    starts = [_true_pose(k).retract(START_DELTA) for k in range(K)]
    got = _run(mid, np.stack([_row(p) for p in starts]), world, offsets, point, uv,
               max_iterations=LM_ITERATIONS)
    rel = 0.0
    for k in range(K):
        sl = slice(offsets[k], offsets[k + 1])
        w_k, obs_k = world[point[sl]], uv[sl]
        ref = _scipy_cost(mid, starts[k], w_k, obs_k)
        one = _single_cost(mid, starts[k], torch.as_tensor(w_k, device="cuda"),
                           torch.as_tensor(obs_k, device="cuda"))
        rel = max(rel, abs(got["cost"][k] - one) / one)
        print(f"pose batch {samples.MODEL_NAMES[mid]} noisy view {k}: cost {got['cost'][k]:.9e} "
              f"({got['iterations'][k]} it, status {got['status'][k]}), scipy {ref:.9e}, "
              f"acm_pose_optimize {one:.9e}")
        assert got["cost"][k] <= ref * 1.02 + 1e-9, (k, got["cost"][k], ref)
    print(f"pose batch {samples.MODEL_NAMES[mid]} noisy: largest relative difference to "
          f"acm_pose_optimize's cost {rel:.3e}")


def test_refine_poses_matches_c_call():
    mid, K = DS, 5
    counts = (300, 1024, 1500, 2, 700)
    world = _world(mid, K)
    offsets, point, uv = _csr(mid, counts, noisy=True, spoil=True)
    start = np.stack([_row(_start_pose(k)) for k in range(K)])
    want = _run(mid, start, world, offsets, point, uv)
    p_t = torch.as_tensor(start, device="cuda")
    w_t, o_t = torch.as_tensor(world.copy(), device="cuda"), torch.as_tensor(offsets, device="cuda")
    i_t, u_t = torch.as_tensor(point, device="cuda"), torch.as_tensor(uv, device="cuda")
    keep = [t.clone() for t in (p_t, w_t, o_t, i_t, u_t)]
    res = refine_poses(_model(mid), p_t, w_t, o_t, i_t, u_t, PoseBatchConfig(),
                       want_information=True)
    for key in ("poses", "status", "cost", "n_valid", "iterations", "information"):
        assert getattr(res, key).cpu().numpy().tobytes() == want[key].tobytes(), key
    for before, after in zip(keep, (p_t, w_t, o_t, i_t, u_t)):
        assert before.cpu().numpy().tobytes() == after.cpu().numpy().tobytes()
    assert res.poses.data_ptr() != p_t.data_ptr()
    # a sequence of Pose, no information
    res2 = refine_poses(_model(mid), [_pose_of_row(r) for r in start], w_t, o_t, i_t, u_t)
    assert res2.information is None
    assert res2.poses.cpu().numpy().tobytes() == want["poses"].tobytes()


@pytest.mark.parametrize("mid", [KB, DS])
def test_alternate_bundle_adjustment(mid):
    n, sweeps = 500, 3
    X, offsets, view = T.scene("narrow")
    offsets, view = offsets[:n + 1], view[:offsets[n]]
    uv = T.observations("narrow", mid, 0.5)[:offsets[n]]
    truth = T.poses12("narrow")
    start = truth.copy()
    for k in range(1, T.K_VIEWS):
        start[k] = _row(_pose_of_row(truth[k]).retract(START_DELTA))
    # every observation projects Ok on the oracle at the perturbed start
    params, (w, h) = samples.SAMPLES[mid]
    Rs, ts = start[:, :9].reshape(-1, 3, 3), start[:, 9:]
    p = np.einsum("mij,mj->mi", Rs[view], X[T.point_of(offsets)]) + ts[view]
    uv0, st0, _ = oracle.project(mid, params, w, h, p)
    assert (st0 == 0).all()
    assert (np.abs(uv0 - [w / 2, h / 2]) < [0.4 * w, 0.4 * h]).all(), "not comfortably inside the image"
    start_t = torch.as_tensor(start, device="cuda")
    before = start_t.clone()
    poses, tri, costs = alternate_bundle_adjustment(_model(mid), start_t, offsets, view, uv, sweeps)
    hist = [float(c) for c in costs]
    print(f"alternating BA {samples.MODEL_NAMES[mid]}: cost history {hist}")
    assert len(hist) == 1 + 2 * sweeps and all(math.isfinite(c) for c in hist)
    for a, b in zip(hist, hist[1:]):
        assert b <= a * (1.0 + 1e-9), hist
    assert hist[-1] < hist[0]
    assert start_t.cpu().numpy().tobytes() == before.cpu().numpy().tobytes()
    assert poses[0].cpu().numpy().tobytes() == start[0].tobytes()
    assert tri.points.shape == (n, 3)
