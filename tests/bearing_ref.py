"""The RANSAC solvers' pixel bearing, stated once in numpy (not a test).

acm_pose_estimate_batch, acm_relative_pose_batch and acm_homography_batch
turn every pixel into a unit ray, or call it unusable, by one rule
(include/acm.h).  bearings() is that rule on top of the CPU oracle's
unprojection; tests/test_bearing_ref.py pins it to the 50-digit forward model
of every sample and zoo camera, and the GPU tests compare the kernels with it.

A pixel is usable when it is finite, the model's unprojection (the oracle's)
returns OK and the direction is finite.  The direction is the unprojection's,
with four exceptions, each the projection's inverse where the unprojection
is not:
  KB      the root of theta_d(theta) = |m| by the reference's Newton
          iteration and one more step (kb_newton).  The unprojection clamps
          |m| to pi / 2 as the reference does, which bends the ray by up to
          58 px in the sample camera's corners, and stops at |delta| < 1e-6,
          9e-9 px off under kb_strong's distortion; a pixel the iteration
          does not converge for is unusable
  UCM     denom = 1 + r^2 (the unprojection keeps the reference's 1 - r^2)
  RadTan  two more Newton steps on the distortion (`polish`, the two-view
          solvers' case) after the unprojection's own, which stop at 1e-6
  FOV     (mx s / (rd 2 tan(w/2)), my s / (rd 2 tan(w/2)), c) with (s, c) =
          sincos(rd w): no division by cos(rd w), which is negative beyond 90
          degrees and turns the unprojection's ray into its antipode; a pixel
          with rd w >= pi is no image of any ray and is unusable

Every key is camera_zoo.camera_of's: a model id (the sample camera) or a zoo
name.
"""
import math

import numpy as np

import oracle
from camera_zoo import camera_of

PINHOLE, RADTAN, KB, DS, UCM, EUCM, FOV = range(7)
EPS = 2.220446049250313e-16
EPS_SQRT = 1.4901161193847656e-08
GRID = (61, 41)     # pixels across and down, image plus margin
MARGIN = 0.25


def fov_psi(params, uv):
    """(mx, my, rd, 2 tan(w/2), rd w, general): the FOV model's quantities of
    pixels uv (m, 2); `general` is False on the axis (rd <= sqrt(eps)) and for
    2 tan(w/2) <= sqrt(eps), where the bearing stays the unprojection's."""
    mx, my = (uv[:, 0] - params[2]) / params[0], (uv[:, 1] - params[3]) / params[1]
    rd = np.sqrt(mx * mx + my * my)
    mul2 = 2.0 * math.tan(params[4] / 2.0)
    return mx, my, rd, mul2, rd * params[4], (rd > EPS_SQRT) & (mul2 > EPS_SQRT)


def kb_newton(params, ru, active):
    """The reference's Newton iteration on theta_d(theta) = ru (from theta =
    ru, at most 10 steps, until |delta| < 1e-6; a derivative below f64's
    epsilon ends it unconverged) for the entries `active`, without the
    unprojection's clamp of ru to pi / 2, and one more step for those that
    converged.  The kernel's operations in the kernel's order: the iterates
    are the same doubles.  Returns (theta, converged)."""
    k1, k2, k3, k4 = params[4:8]
    theta = np.array(ru, dtype=np.float64)
    active = np.array(active, dtype=bool)
    converged = np.zeros(len(theta), dtype=bool)

    def step(th):
        t2 = th * th
        t4 = t2 * t2
        t6 = t4 * t2
        t8 = t4 * t4
        a1, a2, a3, a4 = k1 * t2, k2 * t4, k3 * t6, k4 * t8
        f = th * (1.0 + a1 + a2 + a3 + a4) - ru
        fp = 1.0 + (3.0 * a1) + (5.0 * a2) + (7.0 * a3) + (9.0 * a4)
        return f, fp

    for _ in range(10):
        f, fp = step(theta)
        active &= ~(np.abs(fp) < EPS)
        delta = f / fp
        theta = np.where(active, theta - delta, theta)
        done = active & (np.abs(delta) < 1e-6)
        converged |= done
        active &= ~done
    f, fp = step(theta)
    theta = np.where(converged, theta - f / fp, theta)
    return theta, converged


def bearings(key, uv, polish):
    """(f (m, 3), usable (m,)) of pixels uv (m, 2).  polish: RadTan's two
    extra Newton steps (the two-view solvers); pose estimation takes none."""
    mid, params, (w, h) = camera_of(key)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    fin = np.isfinite(uv).all(axis=1)
    safe = np.where(fin[:, None], uv, 0.0)
    model_ok = np.ones(len(uv), dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rays, st = oracle.unproject(mid, params, w, h, safe)
        if mid == UCM:
            alpha = params[4]
            gamma, xi = 1.0 - alpha, alpha / (1.0 - alpha)
            mx = (safe[:, 0] - params[2]) / params[0] * gamma
            my = (safe[:, 1] - params[3]) / params[1] * gamma
            r2 = mx * mx + my * my
            coeff = (xi + np.sqrt(1.0 + (1.0 - xi * xi) * r2)) / (1.0 + r2)
            rays = np.stack([coeff * mx, coeff * my, coeff - xi], axis=1)
        if mid == RADTAN and polish:
            k1, k2, p1, p2, k3 = params[4:9]
            tx, ty = (safe[:, 0] - params[2]) / params[0], (safe[:, 1] - params[3]) / params[1]
            x, y = rays[:, 0] / rays[:, 2], rays[:, 1] / rays[:, 2]
            for _ in range(2):
                r2 = x * x + y * y
                radial = 1.0 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
                ex = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x) - tx
                ey = y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y - ty
                dr = 2.0 * (k1 + 2.0 * k2 * r2 + 3.0 * k3 * r2 ** 2)
                a00 = radial + dr * x * x + 2.0 * p1 * y + 6.0 * p2 * x
                a01 = dr * x * y + 2.0 * p1 * x + 2.0 * p2 * y
                a11 = radial + dr * y * y + 6.0 * p1 * y + 2.0 * p2 * x
                det = a00 * a11 - a01 * a01
                x, y = x - (a11 * ex - a01 * ey) / det, y - (a00 * ey - a01 * ex) / det
            rays = np.stack([x, y, np.ones_like(x)], axis=1)
        if mid == FOV:
            mx, my, rd, mul2, psi, general = fov_psi(params, safe)
            model_ok = ~general | (psi < math.pi)          # NaN and Inf fail the compare
            ru = np.sin(psi) / (rd * mul2)
            rays = np.where(general[:, None], np.stack([mx * ru, my * ru, np.cos(psi)], axis=1),
                            rays)
        if mid == KB:
            mx, my = (safe[:, 0] - params[2]) / params[0], (safe[:, 1] - params[3]) / params[1]
            ru = np.sqrt(mx * mx + my * my)
            off_axis = ru > 1e-6
            theta, converged = kb_newton(params, ru, off_axis)
            model_ok = ~off_axis | converged
            q = np.sin(theta) / ru
            rays = np.where(off_axis[:, None],
                            np.stack([mx * q, my * q, np.cos(theta)], axis=1), rays)
        f = rays / np.linalg.norm(rays, axis=1)[:, None]
    usable = fin & (st == 0) & model_ok & np.isfinite(f).all(axis=1)
    return f, usable


def grid(key):
    """(uv (2501, 2), inside (2501,)): GRID pixels over the camera's image and
    a margin of MARGIN times its size on every side; `inside` marks those in
    [0, width) x [0, height)."""
    _, _, (w, h) = camera_of(key)
    u = np.linspace(-MARGIN * w, (1.0 + MARGIN) * w, GRID[0])
    v = np.linspace(-MARGIN * h, (1.0 + MARGIN) * h, GRID[1])
    uv = np.stack(np.meshgrid(u, v, indexing="xy"), axis=2).reshape(-1, 2)
    inside = (uv[:, 0] >= 0) & (uv[:, 0] < w) & (uv[:, 1] >= 0) & (uv[:, 1] < h)
    return uv, inside


def near_threshold(key, uv, rel=1e-9):
    """(m,) bool: pixels at which a computed quantity that decides `usable`
    lies within `rel` (relative) of its threshold, so that another rounding of
    the same formula may decide otherwise.  The image bounds of Pinhole, RadTan
    and KB compare the pixel itself and are exact in every implementation: no
    pixel is near those."""
    mid, params, _ = camera_of(key)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    mx, my = (uv[:, 0] - params[2]) / params[0], (uv[:, 1] - params[3]) / params[1]
    r2 = mx * mx + my * my
    pairs = []  # (quantity, threshold)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if mid == KB:
            pairs.append((np.sqrt(r2), 1e-6))
        elif mid == DS:
            a = params[4]
            if a > 0.5:
                pairs.append((r2, 1.0 / (2.0 * a - 1.0)))
            mz = (1.0 - a * a * r2) / (a * np.sqrt(1.0 - (2.0 * a - 1.0) * r2) + (1.0 - a))
            pairs.append((mz * mz + r2, 1e-3))
        elif mid == UCM:
            a = params[4]
            g = 1.0 - a
            pairs.append((1.0 - g * g * r2, 1e-3))
            if a > 0.5:
                pairs.append((g * g * r2, g * g / (2.0 * a - 1.0)))
        elif mid == EUCM:
            a, b = params[4], params[5]
            pairs.append((1.0 - (a - (1.0 - a)) * b * r2, 1e-3))
            if a > 0.5:
                pairs.append((r2, 1.0 / b * (2.0 * a - 1.0)))
        elif mid == FOV:
            pairs.append((fov_psi(params, uv)[4], math.pi))
        near = np.zeros(len(uv), dtype=bool)
        for q, t in pairs:
            near |= np.abs(q - t) <= rel * abs(t)
    return near
