"""CPU reference for the calibration tests (not a test).

Scene: the K = 6 poses of triangulation_ref.rig("wide").  View k observes its
own block of 100 world points: the pixels of a 10 x 10 grid
  u = (0.1 + 0.8 (jx + 0.5 + 0.03 k) / 10) w,  v = (0.1 + 0.8 (jy + 0.5 + 0.03 k) / 10) h
(j = 10 jy + jx) unprojected by the oracle with the intrinsics of camera `mid`
(camera_zoo.camera_of: a model id for its sample camera, or a zoo name), each
unit ray scaled to the distance 1.5 + 2.5 frac(0.6180339887 j
+ 0.1 k) and moved to the world by the inverse true pose.  The observed pixel
is the oracle's re-projection (+ N(0, noise) pixels, seed 20251207).

Start: fx 1.02, fy 0.985, cx + 4, cy - 3, every further parameter x 0.8; pose
k moved (left perturbation, R <- Exp(phi) R, t <- Exp(phi) t + rho) by
(-1)^k (1 - 0.1 k) (0.02, -0.01, 0.015, 0.01, 0.02, -0.015).

scipy_solution(): scipy TRF over [theta, 6 K local deltas about the start
poses] on the oracle's residuals.  numpy_lm(): the Levenberg-Marquardt that
acm_calibrate documents (include/acm.h) restated with dense normal equations
and central-difference Jacobians of the oracle.  Everything is cached;
callers must not modify the returned arrays.
"""
import functools

import numpy as np

import oracle
import triangulation_ref as T
from camera_zoo import camera_of

K_VIEWS = T.K_VIEWS
N_SIDE = 10
N_PER_VIEW = N_SIDE * N_SIDE
START_DELTA = np.array([0.02, -0.01, 0.015, 0.01, 0.02, -0.015])
SEED = 20251207
DS_ALPHA = 4          # index of alpha in DoubleSphere's parameters
DS_ALPHA_UPPER = 0.55  # the bound of the bounded test; the true value is 0.5657


def retract(pose, delta):
    """(12,) pose moved by the left perturbation delta = (rho, phi)."""
    R, t = pose[:9].reshape(3, 3), pose[9:]
    E = T.exp_so3(delta[3:])
    return np.concatenate([(E @ R).ravel(), E @ t + delta[:3]])


def true_poses():
    return T.poses12("wide")


@functools.lru_cache(maxsize=None)
def start_poses():
    p = true_poses()
    out = np.stack([retract(p[k], (-1.0) ** k * (1.0 - 0.1 * k) * START_DELTA)
                    for k in range(K_VIEWS)])
    out.setflags(write=False)
    return out


def true_params(mid):
    return np.array(camera_of(mid)[1], dtype=np.float64)


def start_params(mid):
    p = true_params(mid).copy()
    p[0] *= 1.02
    p[1] *= 0.985
    p[2] += 4.0
    p[3] -= 3.0
    p[4:] *= 0.8
    return p


@functools.lru_cache(maxsize=None)
def scene(mid):
    """(world (600, 3), offsets (7,) int64, obs_point (600,) int32, uv (600, 2),
    n_ok): view k's block is rows 100 k .. 100 k + 99; n_ok counts the grid
    pixels that unprojected and re-projected Ok on the oracle."""
    model, params, (w, h) = camera_of(mid)
    poses = true_poses()
    world, uvs, n_ok = [], [], 0
    j = np.arange(N_PER_VIEW)
    for k in range(K_VIEWS):
        f = 0.1 + 0.8 * (np.stack([j % N_SIDE, j // N_SIDE], axis=1) + 0.5 + 0.03 * k) / N_SIDE
        px = f * [w, h]
        rays, st = oracle.unproject(model, params, w, h, px)
        depth = 1.5 + 2.5 * np.mod(0.6180339887 * j + 0.1 * k, 1.0)
        p = rays * depth[:, None]
        uv, st2, _ = oracle.project(model, params, w, h, p)
        n_ok += int(((st == 0) & (st2 == 0)).sum())
        R, t = poses[k, :9].reshape(3, 3), poses[k, 9:]
        world.append((p - t) @ R)  # R^T (p - t), row vectors
        uvs.append(uv)
    offsets = np.arange(K_VIEWS + 1, dtype=np.int64) * N_PER_VIEW
    out = (np.concatenate(world), offsets, np.arange(K_VIEWS * N_PER_VIEW, dtype=np.int32),
           np.concatenate(uvs), n_ok)
    for a in out[:4]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def observed(mid, noise_px=0.0):
    uv = scene(mid)[3]
    if noise_px:
        uv = uv + np.random.default_rng(SEED).normal(0.0, noise_px, uv.shape)
        uv.setflags(write=False)
    return uv


def residuals(mid, theta, poses, uv):
    """((600, 2) residuals with invalid rows 0, n_valid) on the oracle."""
    model, _, (w, h) = camera_of(mid)
    world = scene(mid)[0]
    r = np.zeros((len(world), 2))
    nv = 0
    for k in range(K_VIEWS):
        sl = slice(N_PER_VIEW * k, N_PER_VIEW * (k + 1))
        R, t = poses[k, :9].reshape(3, 3), poses[k, 9:]
        with np.errstate(all="ignore"):
            p, st, _ = oracle.project(model, list(theta), w, h, world[sl] @ R.T + t)
            d = p - uv[sl]
        ok = (st == 0) & np.isfinite(d).all(axis=1)
        d[~ok] = 0.0
        r[sl] = d
        nv += int(ok.sum())
    return r, nv


@functools.lru_cache(maxsize=None)
def scipy_solution(mid, noise_px=0.0, alpha_upper=None):
    """(cost, theta, poses (K, 12)) of scipy's TRF from the start."""
    from scipy.optimize import least_squares
    uv, x0, P = observed(mid, noise_px), start_params(mid), len(true_params(mid))
    sp = start_poses()

    def unpack(z):
        return z[:P], np.stack([retract(sp[k], z[P + 6 * k:P + 6 * k + 6]) for k in range(K_VIEWS)])

    def f(z):
        th, poses = unpack(z)
        return residuals(mid, th, poses, uv)[0].ravel()
    z0 = np.concatenate([x0, np.zeros(6 * K_VIEWS)])
    lo, hi = np.full(len(z0), -np.inf), np.full(len(z0), np.inf)
    if alpha_upper is not None:
        hi[DS_ALPHA] = alpha_upper
        z0[DS_ALPHA] = min(z0[DS_ALPHA], alpha_upper)
    sol = least_squares(f, z0, method="trf", bounds=(lo, hi), x_scale="jac", xtol=1e-15,
                        ftol=1e-15, gtol=1e-15, max_nfev=400)
    th, poses = unpack(sol.x)
    return float(sol.cost), th.copy(), poses


def _jacobian(mid, theta, poses, uv):
    """Central differences of the residuals in [theta | K x 6 local pose deltas]."""
    P, cols = len(theta), []
    for j in range(P):
        hstep = 1e-6 * max(abs(theta[j]), 1e-2)
        a, b = theta.copy(), theta.copy()
        a[j] += hstep
        b[j] -= hstep
        cols.append((residuals(mid, a, poses, uv)[0] - residuals(mid, b, poses, uv)[0]).ravel()
                    / (2 * hstep))
    for k in range(K_VIEWS):
        for c in range(6):
            d = np.zeros(6)
            d[c] = 1e-6
            a, b = poses.copy(), poses.copy()
            a[k], b[k] = retract(poses[k], d), retract(poses[k], -d)
            cols.append((residuals(mid, theta, a, uv)[0] - residuals(mid, theta, b, uv)[0]).ravel()
                        / 2e-6)
    return np.stack(cols, axis=1)


@functools.lru_cache(maxsize=None)
def numpy_lm(mid, noise_px=0.0, max_iterations=50, ctol=1e-6, ptol=1e-8, gtol=1e-6, mu0=1e-4):
    """acm_calibrate's loop with dense normal equations (no bounds, nothing
    fixed).  Returns a dict: theta, poses, cost, initial_cost, iterations,
    termination ("cost" / "parameter" / "gradient" / "max" / "failed")."""
    uv = observed(mid, noise_px)
    x, poses = start_params(mid), np.array(start_poses())
    P = len(x)
    r, nv = residuals(mid, x, poses, uv)
    F = 0.5 * float((r * r).sum())
    F0 = F
    J = _jacobian(mid, x, poses, uv)
    A, g = J.T @ J, J.T @ r.ravel()
    dmax = float(np.diag(A).max())
    mu, nu, it, term = mu0, 2.0, 0, "max"
    if np.abs(g).max() <= gtol:
        term = "gradient"
    while term == "max" and it < max_iterations:
        it += 1
        Ad = A + np.diag(mu * np.maximum(np.diag(A), 1e-12 * max(dmax, 1.0)))
        try:
            Lc = np.linalg.cholesky(Ad)
            h = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, g))
        except np.linalg.LinAlgError:
            h = None
        if h is None:
            mu *= nu
            nu *= 2.0
            continue
        if np.linalg.norm(h) <= ptol * (np.linalg.norm(x) + ptol):
            term = "parameter"
            break
        xn = x + h[:P]
        pn = np.stack([retract(poses[k], h[P + 6 * k:P + 6 * k + 6]) for k in range(K_VIEWS)])
        rn, nvn = residuals(mid, xn, pn, uv)
        Fn = 0.5 * float((rn * rn).sum())
        pred = -(g @ h + 0.5 * h @ A @ h)
        rho = (F - Fn) / pred if (np.isfinite(Fn) and pred > 0 and nvn >= nv) else -1.0
        if rho > 0:
            dF, Fold = F - Fn, F
            x, poses, r, nv, F = xn, pn, rn, nvn, Fn
            J = _jacobian(mid, x, poses, uv)
            A, g = J.T @ J, J.T @ r.ravel()
            mu *= max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3)
            nu = 2.0
            if np.abs(g).max() <= gtol:
                term = "gradient"
            elif dF <= ctol * Fold:
                term = "cost"
        else:
            mu *= nu
            nu *= 2.0
            if not np.isfinite(mu) or mu > 1e32:
                term = "failed"
    return {"theta": x, "poses": poses, "cost": F, "initial_cost": F0, "iterations": it,
            "termination": term, "n_valid": nv}


def param_errors(mid, theta):
    """|p - p*| / max(|p*|, 1e-2) per parameter."""
    ref = true_params(mid)
    return np.abs(np.asarray(theta) - ref) / np.maximum(np.abs(ref), 1e-2)


def pose_errors(pose, true_pose):
    """(rotation angle, translation distance) between two (12,) poses."""
    Re, Rt = pose[:9].reshape(3, 3), true_pose[:9].reshape(3, 3)
    D = Re @ Rt.T
    c = (np.trace(D) - 1.0) / 2.0
    s = np.linalg.norm(D - D.T) / (2.0 * np.sqrt(2.0))
    return float(np.arctan2(s, c)), float(np.linalg.norm(pose[9:] - true_pose[9:]))
