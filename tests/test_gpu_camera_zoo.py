"""The per-point kernels at the cameras of tests/camera_zoo.py: the branches
and regimes the sample cameras never enter (alpha <= 0.5 and alpha = 0.5
exactly for DS / UCM / EUCM, DS with xi > 0, RadTan with k3 != 0, FOV where
rd w passes pi / 2 and 2, strongly distorted KB).

References are computed here, once per camera: the CPU oracle (pinned at
these cameras by tests/test_camera_zoo_ref.py) and the 50-digit point
Jacobian of tests/point_jacobian_ref.py.  Bounds are the ones the sample
cameras are held to in tests/test_gpu_parity.py, test_gpu_exact.py and
test_gpu_point_jacobian.py: statuses bit-exact; f64 values within 1e-10
(rel_err with floor 1, jac_err per point); bit-identical where the model has
no transcendental; RadTan's fast Newton within 64 ulp of 1.

Inputs per camera: the camera's 250-point base set, samples.EDGE_POINTS, and
500 points x, y ~ U(-3, 3), z ~ U(-1, 2) (z <= 0 reaches the omnidirectional
conditions); for the unprojection a 41 x 33 pixel grid from -20 to w + 20 and
h + 20 plus the border pixels of tests/golden/make_golden.py.
"""
import functools

import numpy as np
import pytest

import camera_zoo as Z
import normal_equations_ref as NE
import oracle as O
import point_jacobian_ref as R
from _backends import GpuBackend, rel_err
from apex_camera_models import samples
from test_gpu_exact import atan2_args, glibc_misrounds, same_bits
from test_gpu_parity import (EXACT_RAYS_UNPROJECT, NO_TRANSCENDENTAL_PROJECT, TOL, jac_err,
                             ulps_of_one)

pytestmark = pytest.mark.gpu

RADTAN, KB, FOV = 1, 2, 6
LAYOUTS = ["aos", "soa"]


@pytest.fixture(scope="module")
def be():
    return GpuBackend()


@functools.lru_cache(maxsize=None)
def _points(name):
    """(780, 3): base set, edge points, wide set (read-only)."""
    rng = np.random.default_rng(20251205)
    wide = np.stack([rng.uniform(-3, 3, 500), rng.uniform(-3, 3, 500),
                     rng.uniform(-1.0, 2.0, 500)], 1)
    pts = np.concatenate([R.base_points(name), samples.EDGE_POINTS, wide])
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _pixels(name):
    """(1360, 2): the grid over and beyond the image, then the border pixels."""
    _, params, (w, h) = Z.camera_of(name)
    gx, gy = np.meshgrid(np.linspace(-20, w + 20, 41), np.linspace(-20, h + 20, 33))
    border = np.array([[0.0, 0.0], [w - 1e-9, h - 1e-9], [float(w), 0.0], [0.0, float(h)],
                       [-1e-300, 5.0], [params[2], params[3]], [np.nan, 1.0]])
    px = np.concatenate([np.stack([gx.ravel(), gy.ravel()], 1), border])
    px.setflags(write=False)
    return px


@functools.lru_cache(maxsize=None)
def _oracle_project(name):
    model, params, (w, h) = Z.camera_of(name)
    out = O.project(model, params, w, h, _points(name), want_jac=True)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_unproject(name):
    model, params, (w, h) = Z.camera_of(name)
    out = O.unproject(model, params, w, h, _pixels(name))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _mp_point_jacobians(name):
    """(780, 2, 3), NaN rows where the point is not finite or not Ok on the oracle."""
    return R.mp_jacobians(name, _points(name))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", Z.NAMES)
def test_project_jacobian(be, name, layout):
    model, params, (w, h) = Z.camera_of(name)
    pts = _points(name)
    uv0, st0, J0 = _oracle_project(name)
    uv, st, J = be.project(model, params, w, h, pts, want_jac=True, layout=layout)
    assert np.array_equal(st, st0), np.nonzero(st != st0)[0][:5]
    e_uv, e_j = rel_err(uv, uv0, floor=1.0), jac_err(J, J0)
    print(f"zoo project {name} {layout}: uv err / bound {e_uv / TOL:.3e}, "
          f"J err / bound {e_j / TOL:.3e}")
    assert e_uv <= TOL and e_j <= TOL
    assert np.all(J[:, st != 0] == 0.0)
    if model in NO_TRANSCENDENTAL_PROJECT:
        assert np.array_equal(uv, uv0, equal_nan=True)
        assert np.array_equal(J, J0, equal_nan=True)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", [n for n in Z.NAMES if Z.camera_of(n)[0] in (KB, FOV)])
def test_project_exact_math(be, name, layout):
    """test_gpu_exact.py's criterion: with ACM_EXACT_MATH statuses equal the
    oracle's and uv / J are bit-identical on every row except Ok rows whose
    atan2 argument glibc misrounds (at most 0.5% of the Ok rows).

    The 0.5% cap is a statement about a rate (glibc misrounds about 0.2% of
    arguments), so it needs a sample on which a rate means something: on the
    ~600 Ok rows of _points alone the expected count is 1.2 and the cap 3,
    which independent rows exceed a few times in a hundred, and the base
    grid's mirror-image rows share their atan2 arguments (measured: 4 and 5
    rows, each one a glibc misrounding).  So, as test_gpu_exact.exact_points
    does, 20 000 points of the bench distribution and the points around the
    axis test and z = EPS are added: expected count ~40, cap ~100."""
    import torch
    model, params, (w, h) = Z.camera_of(name)
    rng = np.random.default_rng(31)
    n = 20_000
    bench = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(0.5, 4.0, n)], 1)
    e = 2.0 ** rng.uniform(-60, 0, 1000)
    ax = np.stack([e * rng.uniform(-1, 1, 1000), e * rng.uniform(-1, 1, 1000),
                   rng.uniform(1e-3, 4, 1000)], 1)
    zz = np.stack([rng.uniform(-1, 1, 200), rng.uniform(-1, 1, 200),
                   samples.EPS * rng.uniform(0.5, 2, 200)], 1)
    xyz = np.concatenate([_points(name), bench, ax, zz])
    xyz = xyz[np.isfinite(xyz).all(1)]
    m = be._model(model, params, w, h)
    t = torch.as_tensor(xyz if layout == "aos" else xyz.T.copy(), device="cuda")
    uv, st, J = (a.cpu().numpy() for a in m.project_batch(t, jacobian=True, layout=layout,
                                                          exact=True))
    uv0, st0, J0 = O.project(model, params, w, h, xyz, want_jac=True)
    assert np.array_equal(st, st0)
    row_ok = same_bits(uv, uv0).all(1) & same_bits(J, J0).all(axis=(0, 2))
    bad = np.nonzero(~row_ok)[0]
    assert (st0[bad] == 0).all()
    ya, xa = atan2_args(model, params, xyz)
    unexplained = [(i, xyz[i].tolist(), uv[i].tolist(), uv0[i].tolist()) for i in bad
                   if not glibc_misrounds(ya[i], xa[i])]
    n_ok = int((st0 == 0).sum())
    print(f"zoo exact {name} {layout}: {n_ok} Ok points, {len(bad)} differ, "
          f"{len(unexplained)} of them not at a glibc atan2 misrounding")
    assert not unexplained, unexplained[:5]
    assert len(bad) <= 0.005 * n_ok, (len(bad), n_ok)


def test_fov_grids_enter_both_large_angle_branches():
    """rd w > 2 leaves the polynomial sin / cos for the library's; pi / 2 <
    rd w <= 2 has cos(rd w) < 0: fov_max must hold pixels of the first kind
    and fov_mid of the second, or the unprojection cases below prove nothing
    about those branches."""
    def rdw(name):
        _, p, _ = Z.camera_of(name)
        px = _pixels(name)
        px = px[np.isfinite(px).all(1)]
        return np.hypot((px[:, 0] - p[2]) / p[0], (px[:, 1] - p[3]) / p[1]) * p[4]
    a, b = rdw("fov_max"), rdw("fov_mid")
    assert int((a > 2.0).sum()) >= 100
    assert int(((b > np.pi / 2) & (b <= 2.0)).sum()) >= 100 and not (b > 2.0).any()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", Z.NAMES)
def test_unproject(be, name, layout):
    model, params, (w, h) = Z.camera_of(name)
    px = _pixels(name)
    rays0, st0 = _oracle_unproject(name)
    ok = st0 == 0
    rays, st = be.unproject(model, params, w, h, px, layout=layout)
    assert np.array_equal(st, st0), np.nonzero(st != st0)[0][:5]
    if model in EXACT_RAYS_UNPROJECT:
        assert np.array_equal(rays, rays0, equal_nan=True)
        print(f"zoo unproject {name} {layout}: {int(ok.sum())} Ok rays bit-identical")
    elif model == RADTAN:
        u = ulps_of_one(rays[ok], rays0[ok])
        print(f"zoo unproject {name} {layout}: fast Newton {u:.1f} ulp of 1 (bound 64)")
        assert u <= 64
        assert rel_err(rays, rays0, floor=1.0) <= TOL
    else:
        e = rel_err(rays, rays0, floor=1.0)
        print(f"zoo unproject {name} {layout}: ray err / bound {e / TOL:.3e}")
        assert e <= TOL
    if model in (RADTAN, FOV):  # ACM_REFERENCE_NEWTON
        rays_r, st_r = be.unproject(model, params, w, h, px, layout=layout,
                                    reference_newton=True)
        assert np.array_equal(st_r, st0)
        if model == RADTAN:
            assert np.array_equal(rays_r, rays0, equal_nan=True)
        else:
            e = rel_err(rays_r, rays0, floor=1.0)
            print(f"zoo unproject {name} {layout} reference loop: ray err / bound {e / TOL:.3e}")
            assert e <= TOL


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", Z.NAMES)
def test_point_jacobian(be, name, layout):
    import torch
    model, params, (w, h) = Z.camera_of(name)
    pts = _points(name)
    _, st0, _ = _oracle_project(name)
    jref = _mp_point_jacobians(name)
    have = ~np.isnan(jref[:, 0, 0])
    assert int(have[:R.N_BASE].sum()) >= 240
    m = be._model(model, params, w, h)
    t = torch.as_tensor(pts if layout == "aos" else np.ascontiguousarray(pts.T), device="cuda")
    uv_p, st_p, _ = m.project_batch(t, layout=layout)
    uv, st, jac = m.project_point_jacobian_batch(t, layout=layout)
    torch.cuda.synchronize()
    assert torch.equal(uv.contiguous().view(torch.int64), uv_p.contiguous().view(torch.int64))
    assert torch.equal(st, st_p)
    st_h = st.cpu().numpy()
    assert np.array_equal(st_h, st0)
    J = jac.permute(1, 2, 0).cpu().numpy()  # (n, 2, 3)
    assert (J[st_h != 0] == 0.0).all()
    assert np.isfinite(J[have]).all()
    scale = np.abs(jref[have]).max(axis=(1, 2))
    err = np.abs(J[have] - jref[have]).max(axis=(1, 2)) / scale
    print(f"zoo point jacobian {name} {layout}: max err / max|J_point| / bound = "
          f"{err.max() / TOL:.3e} over {int(have.sum())} rows")
    assert err.max() <= TOL, (float(err.max()), pts[have][err.argmax()].tolist())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", Z.NAMES)
def test_project_unproject_fused(be, name, layout):
    """acm_project_unproject writes what acm_project followed by
    acm_unproject of its pixels writes, bit for bit."""
    model, params, (w, h) = Z.camera_of(name)
    pts = _points(name)
    uv, st, rays, st2 = be.round_trip(model, params, w, h, pts, layout=layout)
    uv_a, st_a, _ = be.project(model, params, w, h, pts, want_jac=False, layout=layout)
    rays_a, st2_a = be.unproject(model, params, w, h, uv_a, layout=layout)
    for x, y in ((uv, uv_a), (st, st_a), (rays, rays_a), (st2, st2_a)):
        assert x.tobytes() == y.tobytes() or np.array_equal(x, y, equal_nan=True)


def _factor(name, xyz, obs, policy):
    import torch
    from apex_camera_models import factors
    from apex_camera_models.camera import Resolution
    model, _, (w, h) = Z.camera_of(name)
    return factors.CameraParamsFactor.__subclasses__()[model](
        torch.as_tensor(xyz), torch.as_tensor(obs), Resolution(w, h), invalid_policy=policy)


@functools.lru_cache(maxsize=None)
def _factor_inputs(name):
    """Finite points and their observations: the oracle's pixels + N(0, 0.5)
    (3.0 where the projection fails), read-only."""
    pts = _points(name)
    uv0, st0, _ = _oracle_project(name)
    keep = np.isfinite(pts).all(1) & ((st0 != 0) | np.isfinite(uv0).all(1))
    xyz = np.ascontiguousarray(pts[keep])
    obs = np.where(np.isnan(uv0[keep]), 3.0, uv0[keep]) + \
        np.random.default_rng(20251208).normal(0.0, 0.5, (int(keep.sum()), 2))
    xyz.setflags(write=False)
    obs.setflags(write=False)
    return xyz, obs


@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("name", Z.NAMES)
def test_residual_jacobian(name, policy):
    model, params, (w, h) = Z.camera_of(name)
    xyz, obs = _factor_inputs(name)
    r, J = _factor(name, xyz, obs, policy).linearize(params)
    r = r.cpu().numpy().reshape(-1, 2)
    Jn = J.t().contiguous().cpu().numpy().reshape(len(params), -1, 2)
    r0, J0, _ = O.residual_jacobian(model, params, w, h, xyz, obs, policy)
    e_r, e_j = rel_err(r, r0, floor=1.0), jac_err(Jn, J0)
    print(f"zoo residual jacobian {name} policy {policy}: r err / bound {e_r / TOL:.3e}, "
          f"J err / bound {e_j / TOL:.3e}")
    assert e_r <= TOL and e_j <= TOL


@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("name", Z.NAMES)
def test_normal_equations(name, policy):
    model, params, (w, h) = Z.camera_of(name)
    xyz, obs = _factor_inputs(name)
    P = len(params)
    A0, b0, c0, nv0 = O.normal_equations(model, params, w, h, xyz, obs, policy)
    f = _factor(name, xyz, obs, policy)
    res = f.normal_equations(params)
    A, b, c, nv = [t.cpu().numpy() for t in f.unpack_normal_equations(res, P)]
    assert int(nv) == nv0
    e = max(np.abs(A - A0).max() / np.abs(A0).max(),
            np.abs(b - b0).max() / max(np.abs(b0).max(), 1.0),
            abs(c - c0) / max(abs(c0), 1.0))
    print(f"zoo normal equations {name} policy {policy}: n_valid {nv0}, "
          f"worst err / bound {e / TOL:.3e}")
    assert np.abs(A - A0).max() <= TOL * np.abs(A0).max()
    assert np.abs(b - b0).max() <= TOL * max(np.abs(b0).max(), 1.0)
    assert abs(c - c0) <= TOL * max(abs(c0), 1.0)
    # and every entry on its own, against the exact sum of the oracle's
    # per-point terms: max(1e-10 |exact|, 1e-13 sum |terms|)
    # (tests/normal_equations_ref.py)
    want, mag, n_valid = NE.oracle_terms_exact(model, params, w, h, xyz, obs, policy)
    assert n_valid == nv0
    worst = NE.check(res.cpu().numpy(), want, mag, n_valid)
    print(f"zoo normal equations {name} policy {policy}: worst |gpu - exact| / bound = {worst:.3e}")
