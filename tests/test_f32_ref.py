"""The yardsticks of tests/f32_ref.py, checked on the references alone (no
GPU): the two frozen constants against what they were measured from, the
point sets against the conditions the GPU tests rely on, and the rules
against planted errors."""
import mpmath
import numpy as np
import pytest

import boundary_probes as B
import f32_ref as F
from camera_zoo import label
from test_gpu_parity import jac_err


def test_inputs_are_f32_values():
    for key in (2, "fov_max"):
        p = np.array(F.params32(key))
        assert np.array_equal(p, p.astype(np.float32).astype(np.float64))
        pts = F.point_set(key)
        fin = np.isfinite(pts)
        assert np.array_equal(pts[fin], pts[fin].astype(np.float32).astype(np.float64))
    assert F.round32([1e39, -1e39, 1e-300, 1e-40]).tolist()[:3] == [np.inf, -np.inf, 0.0]
    assert len(F.KEYS) == 26


def test_emulate_status_default_is_binary64():
    """The precision argument leaves the existing callers' decision as it was,
    and 24 bits differs from it where f32 cannot resolve the f64 probes."""
    model, params, (w, h), kind, pts = B.probes()[0]
    with mpmath.workprec(53):
        want = [B._st_project(model, params, w, h, pt) for pt in pts]
    assert [B.emulate_status(model, params, w, h, kind, pt) for pt in pts] == want
    assert [B.emulate_status(model, params, w, h, kind, pt, prec=53) for pt in pts] == want


@pytest.mark.parametrize("key", F.KEYS, ids=label)
def test_point_set_and_uv_yardstick(key):
    """At least 240 compared rows, at most 1% of the set where the binary32
    and the exact status disagree, and the 24-bit evaluation of the model at
    or below K_UV / 8 in units of 2^-24 S."""
    ref = F.reference(key)
    n_rows = int(ref.rows.sum())
    differ = int((ref.st_exact[ref.status_rows] != ref.st24[ref.status_rows]).sum())
    worst = F.measure_uv24(key)
    print(f"f32 reference {label(key)}: {n_rows} compared rows of {len(ref.pts)}, "
          f"{int(ref.status_rows.sum())} status rows, {differ} where binary32 != exact, "
          f"24-bit evaluation worst {worst:.3f} x 2^-24 S (K_UV / 8 = {F.K_UV / 8:.3f})")
    assert n_rows >= 240
    assert differ <= 0.01 * len(ref.pts)
    assert worst <= F.K_UV / 8


@pytest.mark.parametrize("key", F.KEYS, ids=label)
def test_oracle_jacobian_yardstick(key):
    """The camera's K_J / 8 is what the f64 oracle's Jacobian loses in units of
    2^-53 times the Jacobian scale against 50-digit derivatives over every
    compared row: not less (the bound would be too tight to mean 8 x) and not
    over 10% more (an inflated entry would loosen the GPU test unnoticed)."""
    worst, n = F.measure_oracle_jac(key)
    base = F.K_J[key] / 8
    print(f"f32 reference {label(key)}: oracle J worst {worst:.3f} x 2^-53 scale over {n} rows "
          f"(K_J / 8 = {base:.3f})")
    assert n >= 240
    assert 0.9 * base <= worst <= base


def test_point_set_is_the_zoo_set():
    """f32_ref.point_set restates test_gpu_camera_zoo._points (which needs no
    GPU): the same rows, rounded to f32, at every camera."""
    import test_gpu_camera_zoo as zoo
    for key in F.KEYS:
        assert np.array_equal(F.point_set(key), F.points32(zoo._points(key)), equal_nan=True)


def test_rules_fail_on_planted_errors():
    """The pixel rule fails on a reference moved by 2e-6 S in one pixel, and
    the Jacobian rule on KB's k4 column scaled by 1 + 1e-5 -- which jac_err's
    per-point-largest-entry scale passes at 1e-4."""
    ref = F.reference(2)
    rows = ref.rows
    assert F.uv_ratio(ref.uv, ref, rows)[0] == 0.0
    uv = ref.uv.copy()
    i = int(np.nonzero(rows)[0][17])
    uv[i, 1] += 2e-6 * ref.S[i, 1]
    worst, where = F.uv_ratio(uv, ref, rows)
    assert worst > F.K_UV and where == i
    J = ref.J0.copy()
    assert F.jac_ratio(J, ref.J0, rows)[0] == 0.0 and F.structural_exact(J, rows)
    J[7] *= 1.0 + 1e-5
    worst, (q, _, _) = F.jac_ratio(J, ref.J0, rows)
    assert worst > F.K_J[2] and q == 7
    assert jac_err(J[:, rows], ref.J0[:, rows]) < 1e-4
    J = ref.J0.copy()
    J[2, i, 0] = np.nextafter(1.0, 2.0)
    assert not F.structural_exact(J, rows)


def test_probe_lines_f32():
    """Every f32 probe line holds f32 values, steps one f32 at a time, and
    changes its exact status at the root (index F32_STEPS) and nowhere else."""
    lines = B.probes_f32()
    assert len({lab for lab, _, _ in lines}) == len(lines)
    for lab, key, pts in lines:
        assert pts.shape == (2 * B.F32_STEPS + 1, 3)
        assert np.array_equal(pts, F.points32(pts)), lab
        model, _, (w, h) = F.camera_of(key)
        p32 = F.params32(key)
        st = [B.emulate_status(model, p32, w, h, "project", pt, prec=170, f32_thresholds=True)
              for pt in pts]
        flips = [i for i in range(1, len(st)) if st[i] != st[i - 1]]
        assert len(flips) == 1 and flips[0] in (B.F32_STEPS, B.F32_STEPS + 1), (lab, st)


def test_kb_axis_points_straddle_the_axis_test():
    pts = F.kb_axis_points()
    r = np.hypot(pts[:, 0], pts[:, 1])
    assert (r < B.EPS).sum() >= 60 and (r >= B.EPS).sum() >= 60
