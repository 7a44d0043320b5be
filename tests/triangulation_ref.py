"""CPU reference for the triangulation tests (not a test).

Rigs (K = 6 views, world -> camera p = R X + t, t = -R c):
  wide   c_k = (0.4 (k - 2.5), 0.15 ((k mod 3) - 1), 0.05 (k mod 2)),
         R_k = Exp((0.03 ((k mod 3) - 1), -0.04 (k - 2.5), 0.02 (k mod 2)));
         points x, y ~ U[-1, 1), z ~ U[2, 4), seed 20251205
  narrow c_k = (0.15 (k - 2.5), 0.05 ((k mod 3) - 1), 0.02 (k mod 2)),
         R_k = Exp((0.01 ((k mod 3) - 1), -0.015 (k - 2.5), 0.02 (k mod 2)));
         points x in +-0.3, y in +-0.2, z in [2, 4)
  medium c_k = (0.3 (k - 2.5), 0.1 ((k mod 3) - 1), 0.04 (k mod 2)),
         R_k = Exp((0.02 ((k mod 3) - 1), -0.03 (k - 2.5), 0.02 (k mod 2)));
         the narrow rig's points: a baseline long enough that the midpoint's
         cond(A) stays below 2000, with every pixel inside the image of the
         models that reject pixels outside it (Pinhole, RadTan)
  tight  c_k = (0.03 (k - 2.5), 0.02 ((k mod 3) - 1), 0.01 (k mod 2)),
         R_k = Exp((0.004 ((k mod 3) - 1), -0.004 (k - 2.5), 0.01 (k mod 2)));
         points x, y in +-0.1, z in [2, 4): |x / z| stays below 0.1, for a
         bounded image whose principal point is close to its border
rig_kind(mid) names the widest of them on which camera `mid` sees every point.
Each track is a random subset of 2..6 views, in view order.  `mid` below is a
camera key (camera_zoo.camera_of): a model id for its sample camera, or a zoo
camera's name.

midpoint(): the numpy restatement of acm_triangulate's start from
oracle.unproject rays: d = R^T ray, c = -R^T t, A = sum (I - d d^T),
b = sum (I - d d^T) c, X0 = A^-1 b.  residuals(): the oracle residuals of one
track for scipy.  Everything is computed once and cached; callers must not
modify the returned arrays.
"""
import functools

import numpy as np

import oracle
from camera_zoo import camera_of

K_VIEWS = 6
SEED = 20251205
N_MAX = 4099


def exp_so3(phi):
    """Rodrigues' formula."""
    phi = np.asarray(phi, dtype=np.float64)
    th = float(np.linalg.norm(phi))
    Kx = np.array([[0.0, -phi[2], phi[1]], [phi[2], 0.0, -phi[0]], [-phi[1], phi[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + Kx
    return np.eye(3) + (np.sin(th) / th) * Kx + ((1.0 - np.cos(th)) / th ** 2) * (Kx @ Kx)


@functools.lru_cache(maxsize=None)
def rig(kind):
    """(R (K, 3, 3), t (K, 3), centres (K, 3)), read-only."""
    cs, Rs = [], []
    for k in range(K_VIEWS):
        a, b, c = k - 2.5, (k % 3) - 1, k % 2
        if kind == "wide":
            cs.append([0.4 * a, 0.15 * b, 0.05 * c])
            Rs.append(exp_so3([0.03 * b, -0.04 * a, 0.02 * c]))
        elif kind == "medium":
            cs.append([0.3 * a, 0.1 * b, 0.04 * c])
            Rs.append(exp_so3([0.02 * b, -0.03 * a, 0.02 * c]))
        elif kind == "tight":
            cs.append([0.03 * a, 0.02 * b, 0.01 * c])
            Rs.append(exp_so3([0.004 * b, -0.004 * a, 0.01 * c]))
        else:
            cs.append([0.15 * a, 0.05 * b, 0.02 * c])
            Rs.append(exp_so3([0.01 * b, -0.015 * a, 0.02 * c]))
    R, c = np.array(Rs), np.array(cs)
    t = -np.einsum("kij,kj->ki", R, c)
    for arr in (R, t, c):
        arr.setflags(write=False)
    return R, t, c


# cameras that reject pixels outside the image and do not see the whole wide scene
_RIG_KIND = {0: "medium", 1: "medium", "radtan_k3_tangential": "medium", "pinhole_aniso": "tight"}


def rig_kind(mid):
    """The rig and scene the tests use for camera `mid`; observations() asserts
    that every projection on it is Ok."""
    return _RIG_KIND.get(mid, "wide")


def poses12(kind):
    """(K, 12) float64: acm_pose's layout, R row-major then t."""
    R, t, _ = rig(kind)
    return np.concatenate([R.reshape(K_VIEWS, 9), t], axis=1)


@functools.lru_cache(maxsize=None)
def scene(kind):
    """N_MAX points and their tracks: (X (N, 3), offsets (N + 1,) int64,
    view (M,) int32), read-only.  The first n points with offsets[: n + 1] and
    view[: offsets[n]] are a scene of n points."""
    rng = np.random.default_rng(SEED)
    if kind == "wide":
        xy = rng.uniform(-1.0, 1.0, (N_MAX, 2))
    elif kind == "tight":
        xy = rng.uniform(-1.0, 1.0, (N_MAX, 2)) * [0.1, 0.1]
    else:
        xy = rng.uniform(-1.0, 1.0, (N_MAX, 2)) * [0.3, 0.2]
    z = rng.uniform(2.0, 4.0, N_MAX)
    X = np.concatenate([xy, z[:, None]], axis=1)
    lengths = rng.integers(2, K_VIEWS + 1, N_MAX)
    views = [np.sort(rng.permutation(K_VIEWS)[:L]) for L in lengths]
    offsets = np.zeros(N_MAX + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(lengths)
    view = np.concatenate(views).astype(np.int32)
    for arr in (X, offsets, view):
        arr.setflags(write=False)
    return X, offsets, view


def point_of(offsets):
    """(M,) the point index of every observation."""
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))


def camera_points(kind, X, offsets, view):
    """(M, 3): R X + t of every observation."""
    R, t, _ = rig(kind)
    return np.einsum("mij,mj->mi", R[view], X[point_of(offsets)]) + t[view]


@functools.lru_cache(maxsize=None)
def observations(kind, mid, noise_px=0.0):
    """(M, 2) oracle projections of scene(kind) through camera `mid`
    (+ N(0, noise_px) pixels, seed SEED + 1).  Asserts that every projection
    is Ok on the oracle."""
    model, params, (w, h) = camera_of(mid)
    X, offsets, view = scene(kind)
    uv, st, _ = oracle.project(model, params, w, h, camera_points(kind, X, offsets, view))
    assert (st == 0).all(), (kind, mid, "an oracle projection of the rig is not Ok")
    if noise_px:
        uv = uv + np.random.default_rng(SEED + 1).normal(0.0, noise_px, uv.shape)
    uv.setflags(write=False)
    return uv


def midpoint(kind, mid, offsets, view, uv):
    """The numpy midpoint per track: (X0 (N, 3), cond(A) (N,), usable (N,)).
    Unusable observations (oracle unprojection not Ok, non-finite pixel, view
    out of range) are skipped; X0 is NaN where fewer than 2 are usable."""
    model, params, (w, h) = camera_of(mid)
    R, t, _ = rig(kind)
    rays, st = oracle.unproject(model, params, w, h, np.nan_to_num(uv, nan=-1.0))
    ok = (st == 0) & np.isfinite(uv).all(axis=1) & (view >= 0) & (view < K_VIEWS)
    n = len(offsets) - 1
    X0 = np.full((n, 3), np.nan)
    cond = np.full(n, np.inf)
    usable = np.zeros(n, dtype=np.int64)
    for i in range(n):
        A = np.zeros((3, 3))
        b = np.zeros(3)
        for j in range(offsets[i], offsets[i + 1]):
            if not ok[j]:
                continue
            Rk, tk = R[view[j]], t[view[j]]
            d = Rk.T @ rays[j]
            c = -(Rk.T @ tk)
            P = np.eye(3) - np.outer(d, d)
            A += P
            b += P @ c
            usable[i] += 1
        if usable[i] >= 2:
            cond[i] = np.linalg.cond(A)
            X0[i] = np.linalg.solve(A, b)
    return X0, cond, usable


def residuals(kind, mid, views, uvs, X):
    """Oracle residuals (2 m,) of one track at X; 0 where the projection is
    not Ok (as tests/test_gpu_pose.py's scipy reference)."""
    model, params, (w, h) = camera_of(mid)
    R, t, _ = rig(kind)
    p = R[views] @ np.asarray(X) + t[views]
    uv, st, _ = oracle.project(model, params, w, h, p)
    r = uv - uvs
    r[(st != 0) | ~np.isfinite(r).all(axis=1)] = 0.0
    return r.ravel()


def scipy_cost(kind, mid, views, uvs, start):
    """0.5 sum r^2 at scipy's TRF optimum from `start`."""
    from scipy.optimize import least_squares
    sol = least_squares(lambda X: residuals(kind, mid, views, uvs, X), np.asarray(start),
                        method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    return float(sol.cost)
