"""acm_calibrate on the GPU: the intrinsics and every view's pose in one LM.

Sums (max_iterations = 0), all seven models at their sample cameras and the
solver subset of tests/camera_zoo.py (views of 2, 257 and 1000 observations
there): the views are built as tests/test_gpu_pose_batch.py
builds them (point_jacobian_ref's 250-point base set with its NaN / Inf /
behind-the-camera rows, noisy pixels, spoiled pixels and indices), all views
over one block of world points and one start pose so that one 50-digit
reference (mp point Jacobians, mp_models.jacobian, mp projections) serves
every view.  Every entry of view_system against float64 terms summed with
math.fsum: |gpu - exact| <= max(1e-10 |exact|, 1e-13 sum |terms|), the bound
of test_gpu_pose_batch.py.

Solver: the scene, start and references of tests/calibration_ref.py.  The
zero-noise bounds (1e-4 on the intrinsics, floor 1e-2, and on the poses) are
the CPU restatement's 5.8e-6 with about 17 x margin; the noise margin (1.02
scipy + 1e-9) and the pose bound of the fixed-intrinsics test (1e-6) are
test_gpu_pose_batch.py's.

Measured on an MI355X: sums, worst |gpu - exact| /
bound Pinhole 1.0e-3, RadTan 1.0e-3, KB 2.1e-3, DS 1.1e-3, UCM 3.3e-3, EUCM
2.7e-3, FOV 3.1e-3; zoo cameras 3.0e-5 (pinhole_aniso) ... 7.5e-3
(eucm_alpha_half).  Zero noise: intrinsics error at most 5.8e-6 (KB;
RadTan 3.7e-6, the others <= 1.4e-8), pose errors <= 6.4e-9, 4-13 iterations,
all as the numpy restatement.  Noise: cost / scipy <= 1 + 4.7e-9.  Bounded
DoubleSphere: alpha on its bound, cost equal to bounded scipy's to 10 digits.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import calibration_ref as C
import camera_zoo as Z
import mp_models
import point_jacobian_ref as R
import test_gpu_pose_batch as PB
from apex_camera_models import _lib, samples
from apex_camera_models.optimizer import (CalibrationConfig, CalibrationResult, calibrate,
                                          tracks_by_view)

pytestmark = pytest.mark.gpu

KB, DS = _lib.KANNALA_BRANDT, _lib.DOUBLE_SPHERE
MODELS = sorted(samples.SAMPLES)
COUNTS = PB.COUNTS
N_BASE = R.N_BASE
TOLERANCE_STOPS = (1, 2, 3)  # ACM_LM_COST, ACM_LM_PARAMETER, ACM_LM_GRADIENT


def _model(mid, params=None):
    """mid: a model id (its sample camera) or a zoo camera's name, here and below"""
    return Z.device_model(mid, params)


def _run(mid, params, poses, world, offsets, point, uv, max_iterations=None, fixed_mask=0,
         bounds=None):
    """The C call; numpy outputs."""
    L = _lib.load()
    c = _lib.CalibrateConfig()
    L.acm_calibrate_default_config(ctypes.byref(c))
    if max_iterations is not None:
        c.max_iterations = max_iterations
    c.fixed_mask = fixed_mask
    if bounds:
        c.has_bounds = 1
        for j, (lo, hi) in bounds.items():
            c.lower[j], c.upper[j] = lo, hi
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
    system = torch.full((k, 16, 16), -1.0, dtype=torch.float64, device=dev)
    ws_bytes = L.acm_calibrate_workspace_size(Z.camera_of(mid)[0], k, m)
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device=dev)
    cam = _model(mid, params).acm_camera()
    summ = _lib.CalibrateSummary()
    rc = L.acm_calibrate(
        ctypes.byref(cam), k, p_t.data_ptr(), n, w_t.data_ptr(), o_t.data_ptr(), m,
        i_t.data_ptr() if m else None, u_t.data_ptr() if m else None, ctypes.byref(c),
        ctypes.byref(summ), status.data_ptr(), cost.data_ptr(), n_valid.data_ptr(),
        system.data_ptr(), ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.last_error()
    P = cam.num_params
    return {"params": np.array(list(cam.params)[:P]), "poses": p_t.cpu().numpy(),
            "status": status.cpu().numpy(), "cost": cost.cpu().numpy(),
            "n_valid": n_valid.cpu().numpy(), "system": system.cpu().numpy(),
            "information": np.array(list(summ.information)[:P * P]).reshape(P, P),
            "iterations": summ.iterations, "termination": summ.termination,
            "evaluations": summ.evaluations, "n_views_used": summ.n_views_used,
            "initial_cost": summ.initial_cost, "final_cost": summ.final_cost,
            "total_valid": summ.n_valid}


# ------------------------------------------------------------------- sums
@functools.lru_cache(maxsize=None)
def _sums_reference(mid):
    """For the 250 world points of PB._world(mid, 1) at PB._start_pose(0): the
    augmented rows M (250, 2, 16) without the residual, the 50-digit
    projections (250, 2) and the rows that have a reference."""
    J6, uv, have = PB._view_reference(mid, 0, 1)
    model, params, _ = Z.camera_of(mid)
    Rm, t = PB._Rt(PB._start_pose(0))
    with np.errstate(invalid="ignore"):
        p = PB._world(mid, 1) @ Rm.T + t
    P = len(params)
    M = np.zeros((N_BASE, 2, 16))
    M[:, :, :6] = np.where(have[:, None, None], J6, 0.0)
    for i in np.nonzero(have)[0]:
        Ju, Jv = mp_models.jacobian(model, list(params), p[i])
        M[i, 0, 6:6 + P] = [float(v) for v in Ju]
        M[i, 1, 6:6 + P] = [float(v) for v in Jv]
    M.setflags(write=False)
    return M, uv, have


def _sums_csr(mid, counts):
    """View k observes counts[k] points of the one block, tiled from 17 k."""
    K = len(counts)
    offsets = np.zeros(K + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(counts)
    m = int(offsets[-1])
    point = np.empty(m, dtype=np.int32)
    for k, c in enumerate(counts):
        point[offsets[k]:offsets[k + 1]] = (np.arange(c) + 17 * k) % N_BASE
    uv = PB._true_pixels(mid, 1)[point] + PB._noise()[:m]
    j = np.arange(m)
    uv[j % 37 == 5, 0] = np.nan
    uv[j % 53 == 7, 1] = np.inf
    point[j % 41 == 11] = -1
    point[j % 43 == 13] = N_BASE  # == n_points
    return offsets, point, uv


@pytest.mark.parametrize("mid", tuple(MODELS) + Z.SOLVER_SUBSET)
def test_sums_against_50_digits(mid):
    counts = COUNTS if mid in MODELS else PB.ZOO_COUNTS
    K = len(counts)
    world = PB._world(mid, 1)
    offsets, point, uv = _sums_csr(mid, counts)
    start = np.stack([PB._row(PB._start_pose(0))] * K)
    params = C.true_params(mid)
    P = len(params)
    got = _run(mid, params, start, world, offsets, point, uv, max_iterations=0)
    assert got["poses"].tobytes() == start.tobytes(), "max_iterations = 0 moved a pose"
    assert got["params"].tobytes() == params.tobytes(), "max_iterations = 0 moved the intrinsics"
    assert got["iterations"] == 0 and got["evaluations"] == 1
    assert not np.isfinite(world).all(), "the base set should carry NaN / Inf world points"
    M, uvb, have = _sums_reference(mid)
    assert int(have.sum()) >= 240, "more than 10 base rows without a reference"
    worst, seen, used, total_cost, total_valid = 0.0, set(), 0, [], 0
    for k in range(K):
        sl = slice(offsets[k], offsets[k + 1])
        idx, obs = point[sl].astype(np.int64), uv[sl]
        in_range = (idx >= 0) & (idx < len(world))
        local = np.where(in_range, idx, 0)
        valid = in_range & have[local] & np.isfinite(obs).all(axis=1) & \
            np.isfinite(world[local]).all(axis=1)
        nv = int(valid.sum())
        assert got["n_valid"][k] == nv, (k, counts[k], got["n_valid"][k], nv)
        S = got["system"][k]
        assert S.tobytes() == S.T.copy().tobytes(), (k, "the system is not symmetric")
        assert (S[6 + P:15, :] == 0.0).all() and (S[:, 6 + P:15] == 0.0).all(), (k, "padding")
        rows = M[local][valid].copy()                      # (m, 2, 16)
        rows[:, :, 15] = (uvb[local] - obs)[valid]
        flat = rows.reshape(-1, 16)
        if nv < 3:
            assert got["status"][k] == _lib.POSE_TOO_FEW_OBSERVATIONS, (k, counts[k])
            assert math.isnan(got["cost"][k])
            seen.add("few")
        else:
            assert got["status"][k] == _lib.POSE_OK, (k, counts[k], got["status"][k])
            seen.add("ok")
            used += 1
            total_valid += nv
        for a in range(16):
            for b in range(a, 16):
                terms = flat[:, a] * flat[:, b]
                want, mag = math.fsum(terms), math.fsum(np.abs(terms))
                err = abs(S[a, b] - want)
                bound = max(1e-10 * abs(want), 1e-13 * mag)
                if err > 0.0:
                    worst = max(worst, err / bound if bound > 0 else math.inf)
                assert err <= bound, (k, counts[k], a, b, S[a, b], want, err / max(bound, 1e-300))
        if nv >= 3:
            assert got["cost"][k] == 0.5 * S[15, 15]
            total_cost.append(got["cost"][k])
    assert seen == {"few", "ok"}
    assert got["n_views_used"] == used and got["total_valid"] == total_valid
    assert abs(got["initial_cost"] - math.fsum(total_cost)) <= 1e-12 * got["initial_cost"]
    assert got["final_cost"] == got["initial_cost"]
    print(f"calibrate sums {Z.label(mid)}: worst |gpu - exact| / bound = {worst:.3e}")


# ----------------------------------------------------------------- solver
def _scene_run(mid, noise=0.0, params=None, poses=None, **kw):
    world, offsets, point, _, _ = C.scene(mid)
    return _run(mid, C.start_params(mid) if params is None else params,
                C.start_poses() if poses is None else poses, world, offsets, point,
                C.observed(mid, noise), **kw)


@pytest.mark.parametrize("mid", MODELS)
def test_zero_noise_recovery(mid):
    got = _scene_run(mid)
    err = C.param_errors(mid, got["params"])
    ang, dt = zip(*[C.pose_errors(got["poses"][k], C.true_poses()[k]) for k in range(C.K_VIEWS)])
    print(f"calibrate {samples.MODEL_NAMES[mid]} zero noise: {got['iterations']} iterations "
          f"({got['evaluations']} evaluations), termination {got['termination']}, cost "
          f"{got['initial_cost']:.3e} -> {got['final_cost']:.3e}, intrinsics error "
          f"{err.max():.3e}, rotation error {max(ang):.3e} rad, translation error {max(dt):.3e}")
    assert got["termination"] in TOLERANCE_STOPS, got["termination"]
    assert got["n_views_used"] == C.K_VIEWS and got["total_valid"] == 600
    assert (got["status"] == _lib.POSE_OK).all()
    assert got["final_cost"] <= 1e-12 * got["initial_cost"]
    assert err.max() <= 1e-4, err
    assert max(ang) <= 1e-4 and max(dt) <= 1e-4, (ang, dt)
    assert abs(got["cost"].sum() - got["final_cost"]) <= 1e-9 * got["final_cost"] + 1e-300


@pytest.mark.parametrize("mid", MODELS)
def test_reaches_scipy_optimum_with_noise(mid):
    ref, _, _ = C.scipy_solution(mid, 0.5)
    got = _scene_run(mid, 0.5)
    print(f"calibrate {samples.MODEL_NAMES[mid]} noisy: cost {got['final_cost']:.9e} "
          f"({got['iterations']} it, termination {got['termination']}), scipy {ref:.9e}")
    assert got["final_cost"] <= ref * 1.02 + 1e-9, (got["final_cost"], ref)


@pytest.mark.parametrize("mid", [KB, DS])
def test_fixed_parameters(mid):
    truth = C.true_params(mid)
    P = len(truth)
    got = _scene_run(mid, params=truth, fixed_mask=(1 << P) - 1)
    assert got["params"].tobytes() == truth.tobytes()
    assert got["termination"] in TOLERANCE_STOPS
    assert (got["information"] == 0.0).all()
    worst = [0.0, 0.0]
    for k in range(C.K_VIEWS):
        ang, dt = C.pose_errors(got["poses"][k], C.true_poses()[k])
        worst = [max(worst[0], ang), max(worst[1], dt)]
        assert ang <= 1e-6 and dt <= 1e-6, (k, ang, dt)
    print(f"calibrate {samples.MODEL_NAMES[mid]} intrinsics fixed: rotation error {worst[0]:.3e} "
          f"rad, translation error {worst[1]:.3e}, {got['iterations']} iterations")
    # one parameter fixed at its (wrong) start value: it stays, the others move
    start = C.start_params(mid)
    for j in (0, P - 1):
        one = _scene_run(mid, fixed_mask=1 << j)
        assert one["params"][j].tobytes() == start[j].tobytes(), j
        moved = np.delete(one["params"] != start, j)
        assert moved.all(), (j, one["params"], start)
        assert (one["information"][j] == 0.0).all() and (one["information"][:, j] == 0.0).all()
        assert one["final_cost"] < one["initial_cost"]


def test_bounds():
    mid = DS
    ref, theta, _ = C.scipy_solution(mid, 0.5, C.DS_ALPHA_UPPER)
    assert abs(theta[C.DS_ALPHA] - C.DS_ALPHA_UPPER) <= 1e-9
    got = _scene_run(mid, 0.5, bounds={C.DS_ALPHA: (0.0, C.DS_ALPHA_UPPER)})
    print(f"calibrate DS bounded: alpha {got['params'][C.DS_ALPHA]!r}, cost "
          f"{got['final_cost']:.9e} ({got['iterations']} it, termination {got['termination']}), "
          f"bounded scipy {ref:.9e}")
    assert 0.0 <= got["params"][C.DS_ALPHA] <= C.DS_ALPHA_UPPER
    assert got["final_cost"] <= ref * 1.02 + 1e-9, (got["final_cost"], ref)


def _with_few_view(at, world, offsets, point, uv, poses):
    """The batch with a two-observation view inserted at position `at`."""
    o = int(offsets[at])
    n_off = np.concatenate([offsets[:at + 1], offsets[at:] + 2])
    n_point = np.concatenate([point[:o], point[:2], point[o:]])
    n_uv = np.concatenate([uv[:o], uv[:2], uv[o:]])
    n_poses = np.concatenate([poses[:at], poses[:1], poses[at:]])
    return n_off, n_point, n_uv, n_poses


@pytest.mark.parametrize("mid", [KB, DS])
def test_repeatable_and_independent_of_idle_views(mid):
    world, offsets, point, _, _ = C.scene(mid)
    uv, poses, params = C.observed(mid, 0.5), np.array(C.start_poses()), C.start_params(mid)
    a = _run(mid, params, poses, world, offsets, point, uv)
    b = _run(mid, params, poses, world, offsets, point, uv)
    for key in ("params", "poses", "status", "cost", "n_valid", "system", "information"):
        assert a[key].tobytes() == b[key].tobytes(), key
    for key in ("iterations", "termination", "evaluations", "final_cost", "initial_cost"):
        assert a[key] == b[key], key
    assert a["iterations"] > 0
    for at in (0, 3, C.K_VIEWS):
        n_off, n_point, n_uv, n_poses = _with_few_view(at, world, offsets, point, uv, poses)
        c = _run(mid, params, n_poses, world, n_off, n_point, n_uv)
        rest = [k for k in range(C.K_VIEWS + 1) if k != at]
        assert c["status"][at] == _lib.POSE_TOO_FEW_OBSERVATIONS and c["n_valid"][at] == 2
        assert c["poses"][at].tobytes() == n_poses[at].tobytes()
        assert math.isnan(c["cost"][at])
        assert c["n_views_used"] == C.K_VIEWS
        assert c["params"].tobytes() == a["params"].tobytes(), at
        assert c["information"].tobytes() == a["information"].tobytes(), at
        for key in ("poses", "status", "cost", "n_valid", "system"):
            assert c[key][rest].tobytes() == a[key].tobytes(), (at, key)
        assert (c["iterations"], c["final_cost"]) == (a["iterations"], a["final_cost"])


def test_no_participating_view_fails_and_leaves_the_camera():
    mid = DS
    world, offsets, point, _, _ = C.scene(mid)
    uv, poses, params = C.observed(mid), np.array(C.start_poses()), C.start_params(mid)
    off = np.arange(C.K_VIEWS + 1, dtype=np.int64) * 2  # two observations per view
    got = _run(mid, params, poses, world, off, point, uv)
    assert got["termination"] == 4 and got["n_views_used"] == 0 and got["iterations"] == 0
    assert got["params"].tobytes() == params.tobytes() and got["poses"].tobytes() == poses.tobytes()
    assert (got["status"] == _lib.POSE_TOO_FEW_OBSERVATIONS).all() and (got["n_valid"] == 2).all()
    assert (got["information"] == 0.0).all()


def test_python_api_round_trip():
    mid = DS
    world, offsets, point, _, _ = C.scene(mid)
    uv, poses, params = C.observed(mid, 0.5), np.array(C.start_poses()), C.start_params(mid)
    want = _run(mid, params, poses, world, offsets, point, uv)
    # every point is one track seen by the one view of its block
    n = len(world)
    t_off = torch.arange(n + 1, dtype=torch.int64, device="cuda")
    t_view = torch.as_tensor(np.repeat(np.arange(C.K_VIEWS), C.N_PER_VIEW).astype(np.int32),
                             device="cuda")
    t_uv = torch.as_tensor(np.array(uv), device="cuda")
    v_off, v_point, v_uv = tracks_by_view(t_off, t_view, t_uv, C.K_VIEWS)
    assert v_off.cpu().numpy().tobytes() == offsets.tobytes()
    assert v_point.cpu().numpy().tobytes() == point.tobytes()
    model = _model(mid, params)
    p_t, w_t = torch.as_tensor(poses, device="cuda"), torch.as_tensor(np.array(world), device="cuda")
    keep = [t.clone() for t in (p_t, w_t, v_off, v_point, v_uv)]
    res = calibrate(model, p_t, w_t, v_off, v_point, v_uv, CalibrationConfig(),
                    want_view_system=True)
    assert isinstance(res, CalibrationResult)
    assert list(model.params()) == list(params), "the caller's model was modified"
    assert res.model is not model and type(res.model) is type(model)
    assert np.array(res.model.params()).tobytes() == want["params"].tobytes()
    assert (res.model.resolution.width, res.model.resolution.height) == samples.SAMPLES[mid][1]
    for key, val in (("poses", res.poses), ("status", res.status), ("cost", res.cost),
                     ("n_valid", res.n_valid), ("system", res.view_system)):
        assert val.cpu().numpy().tobytes() == want[key].tobytes(), key
    assert res.information.numpy().tobytes() == want["information"].tobytes()
    assert res.summary.final_cost == want["final_cost"]
    assert res.summary.iterations == want["iterations"]
    assert res.summary.termination == _lib.LM_TERMINATION[want["termination"]]
    assert res.n_views_used == C.K_VIEWS
    for before, after in zip(keep, (p_t, w_t, v_off, v_point, v_uv)):
        assert before.cpu().numpy().tobytes() == after.cpu().numpy().tobytes()
    assert res.poses.data_ptr() != p_t.data_ptr()
    # fixed takes indices; no view_system unless asked for
    fx = calibrate(model, p_t, w_t, v_off, v_point, v_uv, fixed=[C.DS_ALPHA])
    assert fx.view_system is None
    assert fx.model.params()[C.DS_ALPHA] == params[C.DS_ALPHA]
    assert fx.model.params()[0] != params[0]
