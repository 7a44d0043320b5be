"""Pins the references at the cameras of tests/camera_zoo.py before they judge
a kernel there (tests/test_gpu_camera_zoo.py and the zoo cases of the solver
tests): the oracle's alpha <= 0.5 arms, k3 terms and large-w FOV branch have no
golden file and no reference known answer behind them.

For every zoo camera: the parameters validate; the inputs the GPU tests build
exist (every base-grid pixel unprojects, at least 240 of the 250 base points
project); the oracle agrees with the 50-digit restatement of tests/mp_models.py
within the bounds tests/test_oracle.py holds it to at the sample cameras; and
the 50-digit point Jacobian agrees with central differences of the oracle
within the bound of tests/test_point_jacobian_ref.py.
"""
import ctypes

import numpy as np
import pytest

import camera_zoo as Z
import mp_models
import oracle as O
import point_jacobian_ref as R

RADTAN, KB = 1, 2


def _grid_pixels(w, h):
    """the 12 x 10 pixel grid of point_jacobian_ref.base_points"""
    jj, ii = np.meshgrid(np.arange(12), np.arange(10))
    return np.stack([w * (0.1 + 0.8 * (jj.ravel() + 0.5) / 12),
                     h * (0.1 + 0.8 * (ii.ravel() + 0.5) / 10)], axis=1)


def test_zoo_keeps_its_coverage():
    """at least two cameras per model, alpha below / at / above 0.5 for DS, UCM
    and EUCM, a RadTan camera with k3 != 0, and the solver subset is in the zoo"""
    assert len(set(Z.NAMES)) == len(Z.NAMES)
    for model in range(7):
        assert sum(z[1] == model for z in Z.ZOO) >= 2, model
    for model in (3, 4, 5):
        alphas = [z[2][4] for z in Z.ZOO if z[1] == model]
        assert any(a < 0.5 for a in alphas) and 0.5 in alphas and any(a > 0.5 for a in alphas)
    assert any(z[1] == RADTAN and z[2][8] != 0.0 for z in Z.ZOO)
    assert any(z[1] == 3 and z[2][5] > 0.0 for z in Z.ZOO)
    assert set(Z.SOLVER_SUBSET) <= set(Z.NAMES) and "fov_max" not in Z.SOLVER_SUBSET
    assert {Z.camera_of(n)[0] for n in Z.SOLVER_SUBSET} == set(range(7))
    # a model id resolves to the sample camera itself
    from apex_camera_models import samples
    for model in range(7):
        assert Z.camera_of(model) == (model, samples.SAMPLES[model][0], samples.SAMPLES[model][1])


@pytest.mark.parametrize("name", Z.NAMES)
def test_parameters_validate(name):
    from apex_camera_models import _lib
    model, params, (w, h) = Z.camera_of(name)
    L = _lib.load()
    cam = _lib.AcmCamera()
    rc = L.acm_camera_init(ctypes.byref(cam), model, (ctypes.c_double * len(params))(*params),
                           len(params), w, h)
    assert rc == 0, _lib.last_error()
    assert L.acm_validate_params(ctypes.byref(cam)) == 0  # ACM_VALID


@pytest.mark.parametrize("name", Z.NAMES)
def test_base_set_exists(name):
    model, params, (w, h) = Z.camera_of(name)
    _, st = O.unproject(model, params, w, h, _grid_pixels(w, h))
    assert (st == 0).all(), np.nonzero(st)[0]
    pts = R.base_points(name)
    assert pts.shape == (R.N_BASE, 3)
    _, st, _ = O.project(model, params, w, h, pts)
    assert int((st == 0).sum()) >= 240, int((st == 0).sum())
    assert int(R.reference_rows(name, pts).sum()) >= 240


@pytest.mark.parametrize("name", Z.NAMES)
def test_oracle_project_matches_mpmath(name):
    """test_oracle.py's bound (1e-12 of max(|pixel|, 1)) on every base point
    that has a reference row, and on the wide set's Ok points (z <= 0 among
    them for the omnidirectional models)."""
    model, params, (w, h) = Z.camera_of(name)
    rng = np.random.default_rng(7)
    wide = np.stack([rng.uniform(-3, 3, 60), rng.uniform(-3, 3, 60), rng.uniform(-1, 2, 60)], 1)
    pts = np.concatenate([R.base_points(name), wide])
    uv, st, _ = O.project(model, params, w, h, pts)
    rows = np.nonzero((st == 0) & np.isfinite(pts).all(axis=1))[0]
    assert len(rows) >= 240
    worst = 0.0
    for i in rows:
        ref = mp_models.project(model, params, pts[i])
        for a, b in zip(uv[i], ref):
            err = abs(a - float(b)) / max(abs(float(b)), 1.0)
            worst = max(worst, err)
            assert err <= 1e-12, (name, i, pts[i].tolist(), a, float(b))
    print(f"{name}: oracle vs mp projection, worst relative error {worst:.2e}")


@pytest.mark.parametrize("name", Z.NAMES)
def test_oracle_jacobian_matches_mpmath(name):
    """test_oracle.py's bound and scale on every fifth base point."""
    model, params, (w, h) = Z.camera_of(name)
    pts = R.base_points(name)[::5]
    _, st, J = O.project(model, params, w, h, pts, want_jac=True)
    checked, worst = 0, 0.0
    for i in range(len(pts)):
        if st[i] != 0 or not np.isfinite(pts[i]).all():
            continue
        Ju, Jv = mp_models.jacobian(model, params, pts[i])
        scale = max(max(abs(float(t)) for t in Ju + Jv), 1.0)
        for k in range(len(params)):
            for a, b in ((J[k, i, 0], Ju[k]), (J[k, i, 1], Jv[k])):
                err = abs(a - float(b)) / max(abs(float(b)), 1e-6 * scale)
                worst = max(worst, err)
                assert err <= 1e-10, (name, i, k, a, float(b))
        checked += 1
    assert checked >= 45
    print(f"{name}: oracle vs mp parameter Jacobian, worst error {worst:.2e}")


@pytest.mark.parametrize("name", [n for n in Z.NAMES if n != "kb_strong"])
def test_oracle_unproject_matches_mpmath(name):
    """Every base-grid pixel: closed-form rays within 1e-12, the Newton models
    within their 1e-6 stop (test_oracle.py).  kb_strong is left out: theta_d
    is not monotone there and mp.findroot lands on another root; its
    unprojection is held to the oracle by test_gpu_parity.py's NEWTON_STRESS."""
    model, params, (w, h) = Z.camera_of(name)
    px = _grid_pixels(w, h)
    ray, st = O.unproject(model, params, w, h, px)
    assert (st == 0).all()
    tol = 1e-6 if model in (RADTAN, KB) else 1e-12
    worst = 0.0
    for i in range(len(px)):
        ref = mp_models.unproject(model, params, px[i])
        for a, b in zip(ray[i], ref):
            worst = max(worst, abs(a - float(b)))
            assert abs(a - float(b)) <= tol, (name, i, a, float(b))
    print(f"{name}: oracle vs mp rays, worst absolute error {worst:.2e} (bound {tol:.0e})")


@pytest.mark.parametrize("name", Z.NAMES)
def test_mp_point_jacobian_matches_oracle_central_differences(name):
    """As tests/test_point_jacobian_ref.py: step 1e-6 |p|, within 1e-6 of the
    block's largest entry, on the 240 grid points."""
    model, params, (w, h) = Z.camera_of(name)
    pts = np.array(R.base_points(name)[:R.N_GRID])
    J = R.base_jacobians(name)[:R.N_GRID]
    assert np.isfinite(J).all()
    step = 1e-6 * np.linalg.norm(pts, axis=1)
    fd = np.empty_like(J)
    for c in range(3):
        hi, lo = pts.copy(), pts.copy()
        hi[:, c] += step
        lo[:, c] -= step
        uh, sh, _ = O.project(model, params, w, h, hi)
        ul, sl, _ = O.project(model, params, w, h, lo)
        assert (sh == 0).all() and (sl == 0).all()
        fd[:, :, c] = (uh - ul) / (hi[:, c] - lo[:, c])[:, None]
    scale = np.abs(J).max(axis=(1, 2))
    err = np.abs(fd - J).max(axis=(1, 2)) / scale
    print(name, "max |fd - mp| / max|J| =", err.max())
    assert err.max() <= 1e-6
