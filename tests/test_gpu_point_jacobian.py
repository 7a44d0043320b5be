"""acm_project_point_jacobian on the GPU: d(u, v)/d(x, y, z) of all seven
models against the 50-digit reference of tests/point_jacobian_ref.py, uv and
status bit-identical to acm_project, and the line-aligned store windows at
every size / buffer offset (guard words around every output view).

Measured on an MI355X (largest error of an Ok row, relative to the largest
of the point's six reference entries; bound 1e-10): Pinhole 1.8e-16, RadTan
3.5e-16, KB 6.4e-16, DS 4.6e-16, UCM 3.6e-16, EUCM 5.8e-16, FOV 4.4e-16.
"""
import numpy as np
import pytest
import torch

import point_jacobian_ref as R
from apex_camera_models import Resolution, _lib, samples
from apex_camera_models.camera import MODEL_CLASSES

pytestmark = pytest.mark.gpu

SIZES = (1, 7, 8, 9, 250, 255, 256, 257, 263, 264, 1000, 4099)
OFFSETS = (0, 16, 48)  # bytes past a 128-B line
SENT = -7.25e77
SENT_U8 = 0xA5
TOL = 1e-10


def _model(mid):
    params, (w, h) = samples.SAMPLES[mid]
    return MODEL_CLASSES[samples.MODEL_NAMES[mid]]._from_params(list(params), Resolution(w, h))


def _view(count, off_bytes, dtype):
    """A `count`-element view starting off_bytes past a 128-B line of a
    sentinel-filled buffer, with at least one 128-B line of guard before
    and after."""
    item = 8 if dtype == torch.float64 else 1
    lead = 128 // item + off_bytes // item  # one whole line of guard, then the offset
    fill = SENT if dtype == torch.float64 else SENT_U8
    big = torch.full((lead + count + 128 // item,), fill, dtype=dtype, device="cuda")
    assert big.data_ptr() % 128 == 0
    v = big[lead:lead + count]
    assert v.data_ptr() % 128 == off_bytes
    return big, v, lead


def _guards_intact(big, lead, count):
    h = big.cpu().numpy()
    fill = SENT if h.dtype == np.float64 else SENT_U8
    return bool((h[:lead] == fill).all() and (h[lead + count:] == fill).all())


def _bits(t):
    return t.contiguous().view(torch.int64)


def _check(mid, layout, exact):
    m = _model(mid)
    base = R.base_points(mid)
    jref = R.base_jacobians(mid)          # (250, 2, 3), NaN rows without a reference
    have = ~np.isnan(jref[:, 0, 0])
    scale = np.abs(jref).max(axis=(1, 2))
    worst = 0.0
    for n in SIZES:
        pts_h = R.tiled(base, n)
        pts = torch.as_tensor(pts_h if layout == "aos" else np.ascontiguousarray(pts_h.T),
                              device="cuda")
        uv0, st0, _ = m.project_batch(pts, layout=layout, exact=exact)
        st0_h = st0.cpu().numpy()
        if n >= 250:
            assert int((st0_h[:250] == 0).sum()) >= 240, "fewer than 240 of the base set project"
        for off in OFFSETS:
            buv, uv, luv = _view(2 * n, off, torch.float64)
            bj, jac, lj = _view(6 * n, off, torch.float64)
            bst, st, lst = _view(n, off, torch.uint8)
            out = m.project_point_jacobian_batch(pts, layout=layout, exact=exact,
                                                 out=(uv.view(n, 2), st, jac.view(3, n, 2)))
            torch.cuda.synchronize()
            tag = (samples.MODEL_NAMES[mid], layout, exact, n, off)
            assert _guards_intact(buv, luv, 2 * n), tag
            assert _guards_intact(bj, lj, 6 * n), tag
            assert _guards_intact(bst, lst, n), tag
            assert torch.equal(_bits(out[0]), _bits(uv0)), tag
            assert torch.equal(st, st0), tag
            J = jac.view(3, n, 2).permute(1, 2, 0).cpu().numpy()  # (n, 2, 3)
            failed = st0_h != 0
            assert (J[failed] == 0.0).all(), tag
            idx = np.arange(n) % 250
            ok = ~failed & have[idx]
            # every finite point the oracle holds Ok is Ok here, and no other finite one
            assert np.array_equal(ok, have[idx]), tag
            assert np.array_equal(~failed & np.isfinite(pts_h).all(axis=1), ok), tag
            assert np.isfinite(J[ok]).all(), tag
            err = np.abs(J[ok] - jref[idx[ok]]).max(axis=(1, 2)) / scale[idx[ok]]
            worst = max(worst, float(err.max()))
            assert err.max() <= TOL, (tag, float(err.max()), int(idx[ok][err.argmax()]))
    print(f"point jacobian {samples.MODEL_NAMES[mid]} {layout} exact={exact}: "
          f"max err / max|J_point| = {worst:.3e}")


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("mid", range(7))
def test_point_jacobian_matches_reference(mid, layout):
    _check(mid, layout, False)


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("mid", [_lib.KANNALA_BRANDT, _lib.FOV])
def test_point_jacobian_exact_math(mid, layout):
    _check(mid, layout, True)


def test_exact_flag_is_ignored_by_the_other_models():
    for mid in (_lib.PINHOLE, _lib.RADTAN, _lib.DOUBLE_SPHERE, _lib.UCM, _lib.EUCM):
        m = _model(mid)
        pts = torch.as_tensor(R.tiled(R.base_points(mid), 257), device="cuda")
        a = m.project_point_jacobian_batch(pts)
        b = m.project_point_jacobian_batch(pts, exact=True)
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.uint8).flatten(), y.view(torch.uint8).flatten())


@pytest.mark.parametrize("exact", [False, True])
def test_axis_limits(exact):
    """KB at x = y = 0: [[fx/z, 0, 0], [0, fy/z, 0]].  FOV inside r^2 <
    1.49e-8 (the on-axis and the near-axis point): [[fx rd, 0, 0], [0, fy rd,
    0]], rd = 2 tan(w/2) / w.  The structural zeros are exact."""
    m = _model(_lib.KANNALA_BRANDT)
    pts = torch.as_tensor(R.base_points(_lib.KANNALA_BRANDT)[[R.ON_AXIS, R.NEAR_AXIS]].copy(),
                          device="cuda")
    _, st, jac = m.project_point_jacobian_batch(pts, exact=exact)
    J = jac.permute(1, 2, 0).cpu().numpy()
    assert (st.cpu().numpy() == 0).all() and np.isfinite(J).all()
    fx, fy = m.params()[:2]
    want = np.array([[fx / 1.5, 0.0, 0.0], [0.0, fy / 1.5, 0.0]])
    assert np.abs(J[0] - want).max() <= TOL * fx / 1.5
    assert J[0][want == 0.0].tolist() == [0.0] * 4
    f = _model(_lib.FOV)
    fx, fy, _, _, w = f.params()
    rd = 2.0 * np.tan(w / 2.0) / w
    pts = torch.as_tensor(R.base_points(_lib.FOV)[[R.ON_AXIS, R.NEAR_AXIS]].copy(), device="cuda")
    _, st, jac = f.project_point_jacobian_batch(pts, exact=exact)
    J = jac.permute(1, 2, 0).cpu().numpy()
    assert (st.cpu().numpy() == 0).all()
    want = np.array([[fx * rd, 0.0, 0.0], [0.0, fy * rd, 0.0]])
    for k in range(2):
        assert np.abs(J[k] - want).max() <= TOL * fx * rd
        assert J[k][want == 0.0].tolist() == [0.0] * 4


def test_empty_batch():
    m = _model(_lib.DOUBLE_SPHERE)
    uv, st, jac = m.project_point_jacobian_batch(torch.empty((0, 3), dtype=torch.float64,
                                                             device="cuda"))
    assert uv.shape == (0, 2) and st.shape == (0,) and jac.shape == (3, 0, 2)
