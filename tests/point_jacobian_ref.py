"""Reference data for the point-Jacobian and pose tests (not a test).

Every function takes a camera key (camera_zoo.camera_of): a model id for the
sample camera of samples.SAMPLES, or the name of a zoo camera.

Base set (250 points per camera): a 12 x 10
pixel grid u = w (0.1 + 0.8 (j + 0.5) / 12), v = h (0.1 + 0.8 (i + 0.5) / 10)
unprojected with the CPU oracle, each ray scaled by 0.7 and by 2.5 (240
points), then (0, 0, 1.5) and (1e-7, -2e-7, 1.0) (on / near the axis), then
eight rows of samples.EDGE_POINTS (behind the camera, at the centre, NaN,
Inf).  Larger shapes tile it: point i = base[i mod 250]; 250 is no multiple
of 64 or 256, so every wave / workgroup seam lands on different data.

Reference Jacobian d(u, v)/d(x, y, z): mp.diff of mp_models.project in each
of x, y, z at 50 digits (tests/test_point_jacobian_ref.py pins it to central
differences of the oracle).  Computed once per model / point set and cached;
callers must not modify the returned arrays.
"""
import functools

import mpmath as mp
import numpy as np

import mp_models
import oracle
from camera_zoo import camera_of
from apex_camera_models import samples

N_GRID = 240
N_BASE = 250
ON_AXIS, NEAR_AXIS = 240, 241
# samples.EDGE_POINTS rows: centre, behind, near centre on the axis, behind,
# Inf, Inf, NaN, NaN
EDGE_ROWS = (0, 1, 2, 16, 26, 27, 28, 29)


@functools.lru_cache(maxsize=None)
def base_points(key):
    """(250, 3) float64 (read-only)."""
    model, params, (w, h) = camera_of(key)
    jj, ii = np.meshgrid(np.arange(12), np.arange(10))
    u = w * (0.1 + 0.8 * (jj.ravel() + 0.5) / 12)
    v = h * (0.1 + 0.8 * (ii.ravel() + 0.5) / 10)
    rays, st = oracle.unproject(model, params, w, h, np.stack([u, v], axis=1))
    assert (st == 0).all(), "grid pixel failed to unproject on the oracle"
    pts = np.concatenate([0.7 * rays, 2.5 * rays, [[0.0, 0.0, 1.5], [1e-7, -2e-7, 1.0]],
                          samples.EDGE_POINTS[list(EDGE_ROWS)]])
    assert pts.shape == (N_BASE, 3)
    pts.setflags(write=False)
    return pts


def tiled(base, n):
    """(n, 3): point i = base[i mod len(base)]."""
    return base[np.arange(n) % len(base)]


def mp_point_jacobian(model, params, pt):
    """(2, 3) float64: rows u, v; columns d/dx, d/dy, d/dz (50-digit mp.diff)."""
    J = np.empty((2, 3))
    for c in range(3):
        for r in range(2):
            def f(t, c=c, r=r):
                q = [mp.mpf(pt[0]), mp.mpf(pt[1]), mp.mpf(pt[2])]
                q[c] = t
                return mp_models.project(model, params, q)[r]
            J[r, c] = float(mp.diff(f, mp.mpf(pt[c])))
    return J


def reference_rows(key, pts):
    """Which rows of pts get a reference: finite input and Ok on the oracle."""
    model, params, (w, h) = camera_of(key)
    _, st, _ = oracle.project(model, params, w, h, pts)
    return (st == 0) & np.isfinite(pts).all(axis=1)


def mp_jacobians(key, pts):
    """(len(pts), 2, 3) float64, NaN rows where reference_rows is False."""
    model, params, _ = camera_of(key)
    have = reference_rows(key, pts)
    J = np.full((len(pts), 2, 3), np.nan)
    for i in np.nonzero(have)[0]:
        J[i] = mp_point_jacobian(model, params, pts[i])
    J.setflags(write=False)
    return J


@functools.lru_cache(maxsize=None)
def base_jacobians(key):
    """mp_jacobians of base_points(key) (read-only, cached)."""
    return mp_jacobians(key, base_points(key))


def mp_project(key, pts, rows):
    """(len(pts), 2) float64 50-digit projections of the rows in `rows` (NaN elsewhere)."""
    model, params, _ = camera_of(key)
    uv = np.full((len(pts), 2), np.nan)
    for i in np.nonzero(rows)[0]:
        u, v = mp_models.project(model, params, pts[i])
        uv[i] = float(u), float(v)
    return uv
