"""Pins tests/point_jacobian_ref.py (the reference of the point-Jacobian and
pose tests): its 50-digit mp.diff Jacobians against central differences of
the CPU oracle's projection, and the shape of the base set."""
import numpy as np
import pytest

import oracle
import point_jacobian_ref as R
from apex_camera_models import samples


@pytest.mark.parametrize("model", range(7))
def test_base_set_shape_and_grid_projects(model):
    params, (w, h) = samples.SAMPLES[model]
    pts = R.base_points(model)
    assert pts.shape == (250, 3)
    _, st, _ = oracle.project(model, params, w, h, pts)
    assert (st[:R.N_GRID] == 0).all(), np.nonzero(st[:R.N_GRID])[0]
    assert np.array_equal(pts[R.ON_AXIS], [0.0, 0.0, 1.5])
    assert np.array_equal(pts[R.NEAR_AXIS], [1e-7, -2e-7, 1.0])
    # the eight edge rows: non-finite inputs never get a reference row
    have = R.reference_rows(model, pts)
    assert not have[np.nonzero(~np.isfinite(pts).all(axis=1))[0]].any()
    t = R.tiled(pts, 257)
    assert np.array_equal(t[250:], pts[:7]) and np.array_equal(t[:250], pts, equal_nan=True)


@pytest.mark.parametrize("model", range(7))
def test_mp_jacobian_matches_oracle_central_differences(model):
    """For every model, at step 1e-6 |p|, within 1e-6 of the block's largest
    entry (central differences: truncation ~ step^2, rounding ~ 1e-16 |uv| /
    step ~ 1e-7 of the entries at worst -- the bound is the issue's)."""
    params, (w, h) = samples.SAMPLES[model]
    pts = np.array(R.base_points(model)[:R.N_GRID])
    J = R.base_jacobians(model)[:R.N_GRID]
    assert np.isfinite(J).all()
    step = 1e-6 * np.linalg.norm(pts, axis=1)
    fd = np.empty_like(J)
    for c in range(3):
        hi, lo = pts.copy(), pts.copy()
        hi[:, c] += step
        lo[:, c] -= step
        uh, sh, _ = oracle.project(model, params, w, h, hi)
        ul, sl, _ = oracle.project(model, params, w, h, lo)
        assert (sh == 0).all() and (sl == 0).all()
        fd[:, :, c] = (uh - ul) / (hi[:, c] - lo[:, c])[:, None]
    scale = np.abs(J).max(axis=(1, 2))
    err = np.abs(fd - J).max(axis=(1, 2)) / scale
    print(samples.MODEL_NAMES[model], "max |fd - mp| / max|J| =", err.max())
    assert err.max() <= 1e-6
