"""The fused pose normal equations and the 6-DoF pose LM on the GPU.

Normal equations, all seven models at their sample cameras and the solver
subset of tests/camera_zoo.py (sizes 257 and 1000 there): per-point terms
built in float64 from the 50-digit point
Jacobians (tests/point_jacobian_ref.py), [I | -[p]x] and the residuals, summed
with math.fsum; per entry |gpu - exact| <= max(1e-10 |exact|, 1e-13 sum
|terms|).  Solver: zero-noise recovery of the true pose, and the optimum of a
noisy problem against scipy's TRF on the oracle residuals.

Measured on an MI355X (zero noise, 2000 points, start 0.03 rad / 0.03 off;
bound 1e-6): KB rotation error 3.7e-12 rad, translation error 1.7e-10; DS
3.0e-11 rad, 2.9e-11.  Normal equations, worst |gpu - exact| / bound: Pinhole
2.7e-4, RadTan 1.2e-4, KB 5.9e-4, DS 9.0e-4, UCM 1.7e-3, EUCM 1.4e-3, FOV
2.4e-4; zoo cameras 3.8e-6 (pinhole_aniso) ... 1.5e-2 (eucm_alpha_half).
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
from apex_camera_models import _lib, refine_pose, samples
from apex_camera_models.optimizer import LevenbergMarquardtConfig, Pose

pytestmark = pytest.mark.gpu

KB, DS = _lib.KANNALA_BRANDT, _lib.DOUBLE_SPHERE
TRUE_POSE = Pose().retract([0.3, -0.1, 0.2, 0.1, -0.2, 0.15])  # rotation vector, then t
START_DELTA = [0.02, -0.01, 0.015, 0.01, 0.02, -0.015]
NE_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, 4099)
ZOO_NE_SIZES = (257, 1000)  # across a wave and a workgroup seam
ALL_MODELS = tuple(sorted(samples.SAMPLES))


def _model(mid):
    """mid: a model id (its sample camera) or a zoo camera's name, here and below"""
    return Z.device_model(mid)


def _Rt(pose):
    return np.array(pose.rotation), np.array(pose.translation)


@functools.lru_cache(maxsize=None)
def _world_base(mid):
    """The base set moved by the inverse of TRUE_POSE (250 world points)."""
    Rm, t = _Rt(TRUE_POSE)
    with np.errstate(invalid="ignore"):
        w = (R.base_points(mid) - t) @ Rm  # R^T (p - t), row vectors
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _noise():
    return np.random.default_rng(20251205).normal(0.0, 0.5, (4099, 2))


def _observations(mid, world, noise):
    """project_batch at the true pose (NaN where it fails) + noise."""
    Rm, t = _Rt(TRUE_POSE)
    with np.errstate(invalid="ignore"):
        cam_pts = world @ Rm.T + t
    uv, _, _ = _model(mid).project_batch(torch.as_tensor(cam_pts, device="cuda"))
    obs = uv.cpu().numpy()
    return obs + noise if noise is not None else obs


@functools.lru_cache(maxsize=None)
def _eval_reference(mid):
    """At the evaluation pose (TRUE_POSE retracted by START_DELTA), per base
    point: p (250, 3), the 2 x 6 pose Jacobian from the mp point Jacobians
    (250, 2, 6), the 50-digit projection (250, 2), and the valid rows."""
    Rm, t = _Rt(TRUE_POSE.retract(START_DELTA))
    with np.errstate(invalid="ignore"):
        p = _world_base(mid) @ Rm.T + t
    have = R.reference_rows(mid, p)
    Jp = R.mp_jacobians(mid, p)
    uv = R.mp_project(mid, p, have)
    J6 = np.full((len(p), 2, 6), np.nan)
    for i in np.nonzero(have)[0]:
        x, y, z = p[i]
        neg_skew = np.array([[0.0, z, -y], [-z, 0.0, x], [y, -x, 0.0]])  # -[p]x
        J6[i] = Jp[i] @ np.hstack([np.eye(3), neg_skew])
    return p, J6, uv, have


def _ne_call(mid, pose, world_t, obs_t, layout):
    L = _lib.load()
    n = obs_t.shape[0]
    ws_bytes = L.acm_pose_normal_equations_workspace_size(n)
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device="cuda")
    res = torch.full((44,), float("nan"), dtype=torch.float64, device="cuda")
    cam, ap = _model(mid).acm_camera(), pose.acm_pose()
    _lib.check(L.acm_pose_normal_equations(
        ctypes.byref(cam), ctypes.byref(ap), n, world_t.data_ptr(),
        _lib.LAYOUT_SOA if layout == "soa" else _lib.LAYOUT_AOS, obs_t.data_ptr(),
        res.data_ptr(), ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream))
    return res.cpu().numpy()


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("mid", ALL_MODELS + Z.SOLVER_SUBSET)
def test_pose_normal_equations(mid, layout):
    _, J6b, uvb, haveb = _eval_reference(mid)
    assert int(haveb.sum()) >= 240, "more than 10 base rows without a reference"
    pose = TRUE_POSE.retract(START_DELTA)
    worst = 0.0
    for n in (NE_SIZES if mid in ALL_MODELS else ZOO_NE_SIZES):
        idx = np.arange(n) % 250
        world = R.tiled(_world_base(mid), n)
        obs = _observations(mid, world, _noise()[:n])
        valid = haveb[idx] & np.isfinite(obs).all(axis=1)
        world_t = torch.as_tensor(world if layout == "aos" else np.ascontiguousarray(world.T),
                                  device="cuda")
        obs_t = torch.as_tensor(obs, device="cuda")
        got = _ne_call(mid, pose, world_t, obs_t, layout)
        again = _ne_call(mid, pose, world_t, obs_t, layout)
        assert got.tobytes() == again.tobytes(), "two calls differ"
        A = got[:36].reshape(6, 6)
        assert A.tobytes() == np.ascontiguousarray(A.T).tobytes(), "JtJ not symmetric bit for bit"
        assert got[43] == float(valid.sum()), (n, got[43], valid.sum())
        J = J6b[idx][valid]                   # (m, 2, 6)
        r = (uvb[idx] - obs)[valid]           # (m, 2)
        want = np.zeros(44)
        mag = np.zeros(44)

        def put(k, terms):
            want[k] = math.fsum(terms)
            mag[k] = math.fsum(np.abs(terms))
        for a in range(6):
            for b in range(6):
                put(a * 6 + b, np.concatenate([J[:, 0, a] * J[:, 0, b], J[:, 1, a] * J[:, 1, b]]))
            put(36 + a, np.concatenate([J[:, 0, a] * r[:, 0], J[:, 1, a] * r[:, 1]]))
        put(42, 0.5 * np.concatenate([r[:, 0] ** 2, r[:, 1] ** 2]))
        err = np.abs(got[:43] - want[:43])
        bound = np.maximum(1e-10 * np.abs(want[:43]), 1e-13 * mag[:43])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        worst = max(worst, float(ratio.max()))
        assert (err <= bound).all(), (n, int(np.argmax(ratio)), float(ratio.max()))
    print(f"pose NE {Z.label(mid)} {layout}: worst |gpu - exact| / bound = {worst:.3e}")


def _c_optimize(mid, start, world_t, obs_t, allreduce=None, bounds=False):
    L = _lib.load()
    n = obs_t.shape[0]
    cfg = _lib.LmConfig()
    L.acm_lm_default_config(ctypes.byref(cfg))
    cfg.has_bounds = 1 if bounds else 0
    ws_bytes = L.acm_pose_optimize_workspace_size(n)
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device="cuda")
    cam, ap, summ = _model(mid).acm_camera(), start.acm_pose(), _lib.LmSummary()
    cb = _lib.ALLREDUCE_FN(allreduce) if allreduce else _lib.ALLREDUCE_FN()
    rc = L.acm_pose_optimize(ctypes.byref(cam), ctypes.byref(ap), n, world_t.data_ptr(),
                             _lib.LAYOUT_AOS, obs_t.data_ptr(), ctypes.byref(cfg), cb, None,
                             ctypes.byref(summ), ws.data_ptr(), ws_bytes,
                             torch.cuda.current_stream().cuda_stream)
    return rc, ap, summ


def _problem(mid, n, noisy):
    world = R.tiled(_world_base(mid), n)
    obs = _observations(mid, world, _noise()[:n] if noisy else None)
    return world, obs, torch.as_tensor(world, device="cuda"), torch.as_tensor(obs, device="cuda")


def _pose_errors(ap):
    Rt, tt = _Rt(TRUE_POSE)
    Re, te = np.array(list(ap.r)).reshape(3, 3), np.array(list(ap.t))
    c = (np.trace(Re @ Rt.T) - 1.0) / 2.0
    s = np.linalg.norm(Re @ Rt.T - (Re @ Rt.T).T) / (2.0 * math.sqrt(2.0))  # sin(angle)
    return math.atan2(s, c), float(np.linalg.norm(te - tt)), float(np.abs(Re @ Re.T - np.eye(3)).max())


@pytest.mark.parametrize("mid", [KB, DS])
def test_pose_solver_recovers_true_pose_without_noise(mid):
    _, _, world_t, obs_t = _problem(mid, 2000, noisy=False)
    rc, ap, summ = _c_optimize(mid, TRUE_POSE.retract(START_DELTA), world_t, obs_t)
    assert rc == 0, _lib.last_error()
    ang, dt, orth = _pose_errors(ap)
    print(f"pose LM {samples.MODEL_NAMES[mid]} zero noise: {_lib.LM_TERMINATION[summ.termination]} "
          f"after {summ.iterations} iterations / {summ.evaluations} evaluations, cost "
          f"{summ.initial_cost:.3e} -> {summ.final_cost:.3e}, n_valid {summ.n_valid:.0f}, "
          f"rotation error {ang:.3e} rad, translation error {dt:.3e}, |R R^T - I| {orth:.1e}")
    assert _lib.LM_TERMINATION[summ.termination] in ("CostTolerance", "ParameterTolerance",
                                                      "GradientTolerance")
    assert ang <= 1e-6 and dt <= 1e-6
    assert orth <= 1e-12


def _scipy_cost(mid, start, world, obs):
    from scipy.optimize import least_squares
    model, params, (w, h) = Z.camera_of(mid)

    def resid(d):
        Rm, t = _Rt(start.retract(list(d)))
        with np.errstate(invalid="ignore"):
            uv, st, _ = oracle.project(model, params, w, h, world @ Rm.T + t)
        r = uv - obs
        r[(st != 0) | ~np.isfinite(r).all(axis=1)] = 0.0
        return r.ravel()
    sol = least_squares(resid, np.zeros(6), method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    return float(sol.cost)


@pytest.mark.parametrize("mid", [KB, DS])
def test_pose_solver_reaches_scipy_optimum_with_noise(mid):
    world, obs, world_t, obs_t = _problem(mid, 2000, noisy=True)
    start = TRUE_POSE.retract(START_DELTA)
    rc, ap, summ = _c_optimize(mid, start, world_t, obs_t)
    assert rc == 0, _lib.last_error()
    ref = _scipy_cost(mid, start, world, obs)
    print(f"pose LM {samples.MODEL_NAMES[mid]} noisy: gpu cost {summ.final_cost:.9e} "
          f"({_lib.LM_TERMINATION[summ.termination]}, {summ.iterations} it), scipy {ref:.9e}")
    assert summ.final_cost <= ref * 1.02 + 1e-9


def test_allreduce_hook_called_once_per_evaluation():
    _, _, world_t, obs_t = _problem(KB, 2000, noisy=True)
    start = TRUE_POSE.retract(START_DELTA)
    calls = []

    def identity(ctx, buf, count, stream):
        calls.append(count)
        return 0
    rc0, ap0, s0 = _c_optimize(KB, start, world_t, obs_t)
    rc1, ap1, s1 = _c_optimize(KB, start, world_t, obs_t, allreduce=identity)
    assert rc0 == 0 and rc1 == 0
    assert calls == [44] * s1.evaluations and s1.evaluations >= 2
    assert bytes(ap0) == bytes(ap1) and bytes(s0) == bytes(s1)


def test_refine_pose_matches_c_call_and_rejects_bounds():
    _, _, world_t, obs_t = _problem(DS, 2000, noisy=True)
    start = TRUE_POSE.retract(START_DELTA)
    rc, ap, summ = _c_optimize(DS, start, world_t, obs_t)
    assert rc == 0
    pose, res = refine_pose(_model(DS), start, world_t, obs_t, LevenbergMarquardtConfig())
    assert bytes(pose.acm_pose()) == bytes(ap)
    assert res.iterations == summ.iterations and res.final_cost == summ.final_cost
    assert res.n_valid == int(summ.n_valid)
    assert start.rotation == TRUE_POSE.retract(START_DELTA).rotation  # the input is not modified
    with pytest.raises(_lib.AcmError):
        refine_pose(_model(DS), start, world_t, obs_t, bounds={0: (-1.0, 1.0)})
    assert _c_optimize(DS, start, world_t, obs_t, bounds=True)[0] == _lib.ERR_INVALID_ARGUMENT
