"""acm_project_f32 (k_project_f32, the one float instantiation of
camera_models.hpp) against the references of tests/f32_ref.py, through
project_batch with float32 tensors: all 26 cameras, both layouts.

The camera parameters and the points are rounded to f32 first and every
reference is evaluated at those values, so the bounds hold the kernel's own
arithmetic: pixels within K_UV 2^-24 S, every Jacobian entry within its
camera's K_J 2^-24 max(|J0|, column median), statuses equal to the exact
decision wherever binary32 arithmetic can make it.  Neither constant comes
from the kernel (f32_ref.py says where they come from).

Each test prints its worst ratio against its bound.
"""
import functools

import numpy as np
import pytest

import boundary_probes as B
import camera_zoo as Z
import f32_ref as F
import point_jacobian_ref as R

pytestmark = pytest.mark.gpu

KB, DS = 2, 3
LAYOUTS = ["aos", "soa"]
NT_THRESHOLD = 64 << 20  # bytes of output above which the library stores non-temporally
F_SENTINEL, ST_SENTINEL = -7.03125e5, 0xAB


def _project(key, pts32, layout, jacobian=True, out=None):
    """project_batch of f32 points (float64 array holding f32 values, or a
    float32 device tensor (n, 3)) on the camera with f32-rounded parameters."""
    import torch
    m = Z.device_model(key, F.params32(key))
    t = pts32 if isinstance(pts32, torch.Tensor) else torch.as_tensor(
        np.asarray(pts32).astype(np.float32), device="cuda")
    assert t.dtype == torch.float32
    if layout == "soa":
        t = t.t().contiguous()
    return m.project_batch(t, jacobian=jacobian, layout=layout, out=out)


@functools.lru_cache(maxsize=None)
def _kernel(key, layout):
    """(uv, status, J) of the camera's point set as numpy arrays (read-only)."""
    out = tuple(a.cpu().numpy() for a in _project(key, F.point_set(key), layout))
    assert out[0].dtype == np.float32 and out[2].dtype == np.float32
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _axis_reference(key):
    return F.make_reference(key, F.kb_axis_points(), lo=2.0 ** -60)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("key", F.KEYS, ids=Z.label)
def test_pixels(key, layout):
    ref = F.reference(key)
    uv, st, _ = _kernel(key, layout)
    rows = ref.rows & (st == 0)
    n = int(rows.sum())
    worst, where = F.uv_ratio(uv, ref, rows)
    print(f"f32 pixels {Z.label(key)} {layout}: {n} compared rows, worst |uv - uv*| = "
          f"{worst:.3f} x 2^-24 S, / bound {worst / F.K_UV:.3f}")
    assert n >= 240
    assert worst <= F.K_UV, (worst, ref.pts[where].tolist(), uv[where].tolist(),
                             ref.uv[where].tolist())
    if ref.model == KB:  # the axis test r < EPS shapes values: its probes belong here
        ax = _axis_reference(key)
        uv_a, st_a, _ = (a.cpu().numpy() for a in _project(key, ax.pts, layout))
        assert ax.rows.all() and (st_a == 0).all()
        worst, where = F.uv_ratio(uv_a, ax, ax.rows)
        print(f"f32 pixels {Z.label(key)} {layout}: axis probes worst {worst:.3f} x 2^-24 S, "
              f"/ bound {worst / F.K_UV:.3f}")
        assert worst <= F.K_UV, (worst, ax.pts[where].tolist())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("key", F.KEYS, ids=Z.label)
def test_jacobian(key, layout):
    ref = F.reference(key)
    _, st, J = _kernel(key, layout)
    rows = ref.rows & (st == 0)
    k_j = F.K_J[key]
    worst, (q, i, a) = F.jac_ratio(J, ref.J0, rows)
    print(f"f32 jacobian {Z.label(key)} {layout}: {int(rows.sum())} compared rows, worst entry "
          f"{worst:.3f} x 2^-24 scale (parameter {q}), / bound {worst / k_j:.3f}")
    assert int(rows.sum()) >= 240
    assert worst <= k_j, (worst, q, a, ref.pts[i].tolist(), float(J[q, i, a]),
                          float(ref.J0[q, i, a]))
    # the literals of camera_models.hpp, on every Ok row of the batch
    assert F.structural_exact(J, st == 0)
    if ref.model == KB:
        # the axis branch shapes the Jacobian too (x_r = y_r = 0 below r =
        # 2^-52): the axis probes, but for the +-2 steps around the root where
        # the binary32 r may fall on either side of it.  theta ~ 2^-52 there,
        # so theta^3 .. theta^9 underflow in f32: each has an absolute error
        # below the smallest normal 2^-126, times fx x_r <= fx.
        ax = _axis_reference(key)
        _, st_a, J_a = (t.cpu().numpy() for t in _project(key, ax.pts, layout))
        away = np.abs(np.tile(np.arange(2 * B.F32_STEPS + 1) - B.F32_STEPS, 3)) > 2
        floor = 2.0 ** -126 * max(ax.params[0], ax.params[1])
        worst, (q, i, a) = F.jac_ratio(J_a, ax.J0, away, floor=floor)
        print(f"f32 jacobian {Z.label(key)} {layout}: axis probes worst {worst:.3f} x 2^-24 "
              f"scale (parameter {q}), / bound {worst / k_j:.3f}")
        assert worst <= k_j, (worst, q, a, ax.pts[i].tolist(), float(J_a[q, i, a]),
                              float(ax.J0[q, i, a]))
        assert F.structural_exact(J_a, st_a == 0)
        on_axis = np.hypot(ax.pts[:, 0], ax.pts[:, 1]) < B.EPS
        assert (J_a[:, on_axis & away][[0, 1, 4, 5, 6, 7]] == 0.0).all()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("key", F.KEYS, ids=Z.label)
def test_statuses(key, layout):
    """Equal to the exact status wherever the binary32 evaluation agrees with
    it (no rate), one of the two where they differ."""
    ref = F.reference(key)
    _, st, _ = _kernel(key, layout)
    rows = ref.status_rows
    agree = rows & (ref.st_exact == ref.st24)
    differ = rows & ~agree
    bad = np.nonzero(agree & (st != ref.st_exact))[0]
    print(f"f32 statuses {Z.label(key)} {layout}: {int(agree.sum())} rows where binary32 = exact, "
          f"{len(bad)} of them differ on the kernel; {int(differ.sum())} rows where they differ")
    assert len(bad) == 0, [(ref.pts[i].tolist(), int(st[i]), int(ref.st_exact[i])) for i in bad[:5]]
    assert ((st == ref.st_exact) | (st == ref.st24))[differ].all()


@functools.lru_cache(maxsize=None)
def _probe_references():
    """[(label, key, points, exact statuses, W)]: W the half-width in f32 steps
    of the interval on which the binary32 status differs from the exact one."""
    out = []
    for lab, key, pts in B.probes_f32():
        model, _, res = Z.camera_of(key)
        se, s24 = F.statuses(model, F.params32(key), res, pts, np.ones(len(pts), dtype=bool))
        d = np.nonzero(se != s24)[0]
        w = int(np.abs(d - B.F32_STEPS).max()) if len(d) else 0
        out.append((lab, key, pts, se, w))
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
def test_threshold_probes(layout):
    """Along each probe line: outside +-max(4W, 2) f32 steps of the root the
    kernel's status is the exact one; inside, one of the two that meet there."""
    refs = _probe_references()
    failures = []
    for key in sorted({k for _, k, _, _, _ in refs}, key=str):
        mine = [r for r in refs if r[1] == key]
        st_all = _project(key, np.concatenate([r[2] for r in mine]), layout,
                          jacobian=False)[1].cpu().numpy().reshape(len(mine), -1)
        for (lab, _, pts, se, w), st in zip(mine, st_all):
            k = np.arange(len(pts)) - B.F32_STEPS
            inside = np.abs(k) <= max(4 * w, 2)
            flips = (np.nonzero(st[1:] != st[:-1])[0] + 1 - B.F32_STEPS).tolist()
            print(f"f32 probe {lab} {layout}: statuses {se[0]} -> {se[-1]}, W = {w}, "
                  f"kernel flips at step {flips}")
            if not (np.array_equal(st[~inside], se[~inside])
                    and np.isin(st[inside], (se[0], se[-1])).all()):
                failures.append((lab, st.tolist()))
    assert not failures, failures


def _contract_points():
    f = np.float32
    big = 3e38
    rows = [[np.nan, 0.0, 1.0], [0.0, np.nan, 1.0], [0.0, 0.0, np.nan], [np.inf, 0.0, 1.0],
            [0.0, -np.inf, 1.0], [0.0, 0.0, np.inf], [0.0, 0.0, -np.inf], [0.0, 0.0, 0.0],
            [-0.0, -0.0, -0.0], [0.1, 0.2, -0.0], [-0.0, 0.0, 1.0], [1e-40, 0.0, 1.0],
            [0.1, 0.1, 1e-45], [0.1, 0.1, -1e-45], [1e-40, -1e-40, 1e-40], [big, 0.0, 1.0],
            [0.0, 0.0, big], [big, big, big], [-big, big, -big], [1e39, 0.0, 1.0],
            [0.0, 0.0, 1e39], [0.0, -1e39, 1.0], [-1e300, 1e300, -1e300],
            [0.1, -0.2, 1.5], [0.0, 0.0, 2.0], [0.3, 0.1, -1.0]]
    with np.errstate(over="ignore"):
        return np.array(rows, dtype=np.float64).astype(f)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("model", range(7))
def test_contract_rows(model, layout):
    """NaN, +-inf, zeros, -0.0, f32 denormals, 3e38 and f64 values that round
    to +-inf: no reference, but the call succeeds (project_batch raises on a
    non-zero return), every output slot is written, and every row whose
    status is not Ok has uv NaN and a zero Jacobian."""
    import torch
    pts = _contract_points()
    n, P = len(pts), len(F.params32(model))
    assert np.isinf(pts[19:23]).any(axis=1).all()
    uv = torch.full((n, 2), F_SENTINEL, dtype=torch.float32, device="cuda")
    st = torch.full((n,), ST_SENTINEL, dtype=torch.uint8, device="cuda")
    J = torch.full((P, n, 2), F_SENTINEL, dtype=torch.float32, device="cuda")
    _project(model, torch.as_tensor(pts, device="cuda"), layout, out=(uv, st, J))
    uv, st, J = uv.cpu().numpy(), st.cpu().numpy(), J.cpu().numpy()
    assert (st <= 4).all(), st
    assert not (uv == np.float32(F_SENTINEL)).any() and not (J == np.float32(F_SENTINEL)).any()
    bad = st != 0
    print(f"f32 contract rows model {model} {layout}: {int(bad.sum())} of {n} rows fail")
    assert bad.sum() >= 3
    assert np.isnan(uv[bad]).all()
    assert (J[:, bad] == 0.0).all()
    assert F.structural_exact(J, ~bad)


SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, 65537)


@pytest.mark.parametrize("jacobian", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("model", [KB, DS])
def test_shapes(model, layout, jacobian):
    """Ragged batch sizes through out= buffers with a sentinel guard behind
    each: the first n rows are bit-identical to the 65537 batch, the guards
    stay untouched, n = 0 touches nothing."""
    import torch
    P = len(F.params32(model))
    G = 64
    pts = torch.as_tensor(R.tiled(F.point_set(model), SIZES[-1]).astype(np.float32), device="cuda")

    def run(n):
        buf_uv = torch.full((2 * n + G,), F_SENTINEL, dtype=torch.float32, device="cuda")
        buf_st = torch.full((n + G,), ST_SENTINEL, dtype=torch.uint8, device="cuda")
        buf_j = torch.full((2 * n * P + G,), F_SENTINEL, dtype=torch.float32, device="cuda")
        out = (buf_uv[:2 * n].view(n, 2), buf_st[:n],
               buf_j[:2 * n * P].view(P, n, 2) if jacobian else None)
        _project(model, pts[:n], layout, jacobian=jacobian, out=out)
        guards_ok = (bool((buf_uv[2 * n:] == F_SENTINEL).all())
                     and bool((buf_st[n:] == ST_SENTINEL).all())
                     and bool((buf_j[2 * n * P if jacobian else 0:] == F_SENTINEL).all()))
        return out, guards_ok

    (uv0, st0, J0), ok = run(SIZES[-1])
    assert ok
    assert int((st0 == 0).sum()) > SIZES[-1] // 2 and int((st0 != 0).sum()) > 100
    for n in (0,) + SIZES[:-1]:
        (uv, st, J), ok = run(n)
        assert ok, n
        assert torch.equal(uv.view(torch.int32), uv0[:n].view(torch.int32)), n
        assert torch.equal(st, st0[:n]), n
        if jacobian:
            assert torch.equal(J.view(torch.int32), J0[:, :n].contiguous().view(torch.int32)), n
    print(f"f32 shapes model {model} {layout} jacobian={jacobian}: {len(SIZES) + 1} sizes "
          f"bit-identical, guards intact")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("model,jacobian", [(KB, True), (0, False)])
def test_non_temporal_stores(model, jacobian, layout):
    """1000 points above the size at which the library switches to
    non-temporal stores (n (9 + 8P) bytes of output with the Jacobian, 9 n
    without, above 64 MiB), against the same points in four chunks below it:
    uv, status and J bit-identical, compared on the device."""
    import torch
    P = len(F.params32(model))
    per_point = 9 + (8 * P if jacobian else 0)
    n = NT_THRESHOLD // per_point + 1 + 1000
    assert (n - 1000) * per_point > NT_THRESHOLD >= (n // 4 + 1) * per_point
    base = torch.as_tensor(F.point_set(model).astype(np.float32), device="cuda")
    pts = base[torch.arange(n, device="cuda") % len(base)]
    uv, st, J = _project(model, pts, layout, jacobian=jacobian)
    assert int((st == 0).sum()) > n // 3 and int((st != 0).sum()) > n // 100
    cuts = [0, n // 4, n // 2, 3 * (n // 4), n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        uv_c, st_c, J_c = _project(model, pts[a:b], layout, jacobian=jacobian)
        assert torch.equal(uv[a:b].view(torch.int32), uv_c.view(torch.int32))
        assert torch.equal(st[a:b], st_c)
        if jacobian:
            assert torch.equal(J[:, a:b].contiguous().view(torch.int32), J_c.view(torch.int32))
    print(f"f32 non-temporal model {model} {layout}: n = {n} "
          f"({n * per_point / 2 ** 20:.2f} MiB out) bit-identical to four chunks")
