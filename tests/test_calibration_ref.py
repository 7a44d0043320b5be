"""The calibration reference on the CPU (tests/calibration_ref.py): the scene
is fully observable, scipy recovers the true intrinsics at zero noise, the
numpy restatement of acm_calibrate's LM stops by a tolerance within 20
iterations, and the bounded DoubleSphere problem of the GPU test really ends
on its bound.

Measured here: 600 of 600 observations Ok for all seven models; the LM's
intrinsics error at zero noise is at most 5.8e-6 relative (floor 1e-2; KB),
which is where the GPU test's 1e-4 comes from.
"""
import numpy as np
import pytest

import calibration_ref as C
from apex_camera_models import _lib, samples

MODELS = sorted(samples.SAMPLES)


@pytest.mark.parametrize("mid", MODELS)
def test_every_grid_observation_is_ok(mid):
    world, offsets, point, uv, n_ok = C.scene(mid)
    assert n_ok == C.K_VIEWS * C.N_PER_VIEW == 600 == len(world) == len(uv)
    assert np.isfinite(world).all() and np.isfinite(uv).all()
    # and still Ok from the start intrinsics and poses
    _, nv = C.residuals(mid, C.start_params(mid), np.array(C.start_poses()), uv)
    assert nv == 600


@pytest.mark.parametrize("mid", MODELS)
def test_scipy_recovers_the_true_intrinsics(mid):
    cost, theta, poses = C.scipy_solution(mid)
    err = C.param_errors(mid, theta)
    print(f"scipy {samples.MODEL_NAMES[mid]}: cost {cost:.3e}, worst intrinsics error {err.max():.3e}")
    assert err.max() <= 1e-4, err
    for k in range(C.K_VIEWS):
        ang, dt = C.pose_errors(poses[k], C.true_poses()[k])
        assert ang <= 1e-4 and dt <= 1e-4, (k, ang, dt)


@pytest.mark.parametrize("mid", MODELS)
def test_numpy_lm_stops_by_a_tolerance(mid):
    got = C.numpy_lm(mid)
    err = C.param_errors(mid, got["theta"])
    print(f"numpy LM {samples.MODEL_NAMES[mid]}: {got['iterations']} iterations, "
          f"{got['termination']}, cost {got['initial_cost']:.3e} -> {got['cost']:.3e}, worst "
          f"intrinsics error {err.max():.3e}")
    assert got["termination"] in ("cost", "parameter", "gradient")
    assert got["iterations"] <= 20
    assert got["n_valid"] == 600
    assert err.max() <= 1e-4, err


def test_bounded_scipy_solution_sits_on_the_bound():
    mid = _lib.DOUBLE_SPHERE
    assert C.true_params(mid)[C.DS_ALPHA] > C.DS_ALPHA_UPPER
    free, _, _ = C.scipy_solution(mid, 0.5)
    cost, theta, _ = C.scipy_solution(mid, 0.5, C.DS_ALPHA_UPPER)
    print(f"bounded scipy: alpha {theta[C.DS_ALPHA]!r}, cost {cost:.6f} (free {free:.6f})")
    assert abs(theta[C.DS_ALPHA] - C.DS_ALPHA_UPPER) <= 1e-9
    assert cost >= free
