"""numpy restatement of acm_p3p and acm_pose_estimate_batch (not a test).

P3P is Grunert's route as include/acm.h states it, with np.roots for the
quartic: the quartic in v = s3 / s1, u = s2 / s1 from the linear relation, s1
from the law of cosines, three Gauss-Newton steps on the three law-of-cosines
equations in (s1, s2, s3), then R, t from the orthonormal frames of (s_i f_i)
and (X_i).  The sampler is splitmix64 with Python integers, the inlier rule and
the RANSAC key are the header's.
"""
import functools
import math

import numpy as np

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
N_DRAWS = 8
# a solution is kept when its law-of-cosines residuals are at most this times
# a^2 + b^2 + c^2 after the polish (the device applies the same rule)
RESIDUAL_TOL = 1e-12
# a triplet is degenerate when the sine of an angle of the world triangle, or
# of the angle between two bearings, is at most this
DEGENERATE_SIN = 1e-10


def splitmix64(z):
    z &= MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def draw(seed, h, d, cnt):
    """Draw d (0..7) of hypothesis h: a local index in [0, cnt)."""
    ctr = 8 * h + d + 1
    return (splitmix64(seed + ctr * GOLDEN) * cnt) >> 64


def sample(seed, h, cnt, usable):
    """The three local indices of hypothesis h, or None when it is void."""
    got = []
    for d in range(N_DRAWS):
        j = draw(seed, h, d, cnt)
        if usable[j] and j not in got:
            got.append(j)
            if len(got) == 3:
                return got
    return None


def _frame(p1, p2, p3):
    e1 = p2 - p1
    e1 = e1 / np.linalg.norm(e1)
    e3 = np.cross(e1, p3 - p1)
    e3 = e3 / np.linalg.norm(e3)
    return np.stack([e1, np.cross(e3, e1), e3], axis=1)  # columns


def pose_from_depths(f, X, s):
    P = f * np.asarray(s)[:, None]
    Rm = _frame(P[0], P[1], P[2]) @ _frame(X[0], X[1], X[2]).T
    t = P.mean(axis=0) - Rm @ X.mean(axis=0)
    return Rm, t


def degenerate(f, X):
    """f: (3, 3) unit bearings, X: (3, 3) world points."""
    if not (np.isfinite(f).all() and np.isfinite(X).all()):
        return True
    d12, d13, d23 = X[1] - X[0], X[2] - X[0], X[2] - X[1]
    c2, b2, a2 = d12 @ d12, d13 @ d13, d23 @ d23
    if not (a2 > 0 and b2 > 0 and c2 > 0):
        return True
    n = np.cross(d12, d13)
    if not (n @ n > DEGENERATE_SIN ** 2 * b2 * c2):
        return True
    for i, j in ((0, 1), (0, 2), (1, 2)):
        w = np.cross(f[i], f[j])
        if not (w @ w > DEGENERATE_SIN ** 2):
            return True
    return False


def p3p(bearings, points_world):
    """bearings (3, 3), points_world (3, 3) -> list of (R, t), at most 4."""
    f = np.asarray(bearings, dtype=np.float64)
    X = np.asarray(points_world, dtype=np.float64)
    with np.errstate(all="ignore"):
        f = f / np.linalg.norm(f, axis=1)[:, None]
        if degenerate(f, X):
            return []
        a2 = (X[1] - X[2]) @ (X[1] - X[2])
        b2 = (X[0] - X[2]) @ (X[0] - X[2])
        c2 = (X[0] - X[1]) @ (X[0] - X[1])
        ca, cb, cg = f[1] @ f[2], f[0] @ f[2], f[0] @ f[1]
        q, p = (a2 - c2) / b2, (a2 + c2) / b2
        A4 = (q - 1) ** 2 - 4 * (c2 / b2) * ca ** 2
        A3 = 4 * (q * (1 - q) * cb - (1 - p) * ca * cg + 2 * (c2 / b2) * ca ** 2 * cb)
        A2 = 2 * (q * q - 1 + 2 * q * q * cb ** 2 + 2 * ((b2 - c2) / b2) * ca ** 2
                  - 4 * p * ca * cb * cg + 2 * ((b2 - a2) / b2) * cg ** 2)
        A1 = 4 * (-q * (1 + q) * cb + 2 * (a2 / b2) * cg ** 2 * cb - (1 - p) * ca * cg)
        A0 = (1 + q) ** 2 - 4 * (a2 / b2) * cg ** 2
        coef = np.array([A4, A3, A2, A1, A0])
        if not np.isfinite(coef).all():
            return []
        roots = np.roots(coef)
        out = []
        for r in sorted(roots, key=lambda z: z.real):
            if abs(r.imag) > 1e-6 * max(1.0, abs(r.real)):
                continue
            v = r.real
            if not v > 0:
                continue
            u = ((q - 1) * v * v - 2 * q * cb * v + 1 + q) / (2 * (cg - v * ca))
            if not u > 0:
                continue
            s1 = math.sqrt(b2) / math.sqrt(1 + v * v - 2 * v * cb)
            s = np.array([s1, u * s1, v * s1])
            s = polish(s, ca, cb, cg, a2, b2, c2)
            if s is None:
                continue
            if any(np.abs(s - o).max() <= 1e-9 * np.abs(s).max() for o in out):
                continue  # a double root found twice
            out.append(s)
        return [pose_from_depths(f, X, s) for s in out]


def _residual(s, ca, cb, cg, a2, b2, c2):
    return np.array([s[1] * s[1] + s[2] * s[2] - 2 * s[1] * s[2] * ca - a2,
                     s[0] * s[0] + s[2] * s[2] - 2 * s[0] * s[2] * cb - b2,
                     s[0] * s[0] + s[1] * s[1] - 2 * s[0] * s[1] * cg - c2])


def polish(s, ca, cb, cg, a2, b2, c2):
    for _ in range(3):
        g = _residual(s, ca, cb, cg, a2, b2, c2)
        J = np.array([[0.0, 2 * s[1] - 2 * s[2] * ca, 2 * s[2] - 2 * s[1] * ca],
                      [2 * s[0] - 2 * s[2] * cb, 0.0, 2 * s[2] - 2 * s[0] * cb],
                      [2 * s[0] - 2 * s[1] * cg, 2 * s[1] - 2 * s[0] * cg, 0.0]])
        det = np.linalg.det(J)
        if not (np.isfinite(det) and det != 0.0):
            return None
        s = s - np.linalg.solve(J, g)
    if not (np.isfinite(s).all() and (s > 0).all()):
        return None
    g = _residual(s, ca, cb, cg, a2, b2, c2)
    if not (np.abs(g).max() <= RESIDUAL_TOL * (a2 + b2 + c2)):
        return None
    return s


# ------------------------------------------------------------------ triplets
def random_triplets(n, seed=20261020):
    """The family of the accuracy tests: camera-frame points x, y ~ U[-1.5,
    1.5), z ~ U[2, 5); pose R = Exp(N(0, 0.5)^3), t ~ U[-0.5, 0.5)^3.  Returns
    (bearings (n, 3, 3) -- unit --, world points (n, 3, 3), R (n, 3, 3), t (n, 3))."""
    rng = np.random.default_rng(seed)
    pc = np.empty((n, 3, 3))
    pc[..., :2] = rng.uniform(-1.5, 1.5, (n, 3, 2))
    pc[..., 2] = rng.uniform(2.0, 5.0, (n, 3))
    w = rng.normal(0.0, 0.5, (n, 3))
    t = rng.uniform(-0.5, 0.5, (n, 3))
    Rm = np.stack([exp_so3(x) for x in w])
    X = np.einsum("nji,nkj->nki", Rm, pc - t[:, None, :])  # R^T (p - t)
    f = pc / np.linalg.norm(pc, axis=2)[..., None]
    return f, X, Rm, t


def exp_so3(w):
    th = np.linalg.norm(w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * (K @ K)


def backward_residual(Rm, t, f, X):
    p = X @ Rm.T + t
    return float(np.abs(p / np.linalg.norm(p, axis=1)[:, None] - f).max())


def pose_error(Rm, t, R0, t0):
    return float(max(np.abs(Rm - R0).max(), np.abs(t - t0).max()))


def reference_accuracy(f, X, R0, t0):
    """Over the triplets: (worst backward residual of any reference solution,
    worst true-pose error of the best reference solution, triplets with no
    solution)."""
    worst_res, worst_err, none = 0.0, 0.0, 0
    for i in range(len(f)):
        sols = p3p(f[i], X[i])
        if not sols:
            none += 1
            continue
        worst_res = max(worst_res, max(backward_residual(Rm, t, f[i], X[i]) for Rm, t in sols))
        worst_err = max(worst_err, min(pose_error(Rm, t, R0[i], t0[i]) for Rm, t in sols))
    return worst_res, worst_err, none


N_FAMILY = 4096


@functools.lru_cache(maxsize=None)
def family():
    """The N_FAMILY triplets of the accuracy tests (read-only)."""
    out = random_triplets(N_FAMILY)
    for arr in out:
        arr.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def family_accuracy():
    """reference_accuracy over family(), computed once per process."""
    return reference_accuracy(*family())


def check_solutions(poses, count, f, X, R0, t0):
    """poses (n, 4, 12), count (n,): the worst backward residual of any
    returned solution, the worst true-pose error of the best one, the worst
    |R^T R - I|; asserts count in 0 .. 4, det > 0 and NaN beyond the count."""
    worst_res = worst_err = worst_orth = 0.0
    for i in range(len(f)):
        c = int(count[i])
        assert 0 <= c <= 4, (i, c)
        assert np.isnan(poses[i, c:]).all(), i
        assert np.isfinite(poses[i, :c]).all(), i
        best = np.inf
        for k in range(c):
            Rm, t = poses[i, k, :9].reshape(3, 3), poses[i, k, 9:]
            assert np.linalg.det(Rm) > 0, (i, k)
            worst_orth = max(worst_orth, float(np.abs(Rm.T @ Rm - np.eye(3)).max()))
            worst_res = max(worst_res, backward_residual(Rm, t, f[i], X[i]))
            best = min(best, pose_error(Rm, t, R0[i], t0[i]))
        worst_err = max(worst_err, best)
    return worst_res, worst_err, worst_orth


def degenerate_triplets():
    """(bearings (6, 3, 3), points (6, 3, 3)): collinear points, a repeated
    point, a repeated bearing, a NaN bearing, an Inf point, a zero bearing."""
    f, X, _, _ = random_triplets(6, seed=5)
    f, X = f.copy(), X.copy()
    X[0, 2] = X[0, 0] + 0.3 * (X[0, 1] - X[0, 0])
    X[1, 1] = X[1, 0]
    f[2, 2] = f[2, 0]
    f[3, 1, 0] = np.nan
    X[4, 2, 1] = np.inf
    f[5, 0] = 0.0
    return f, X


# -------------------------------------------------------------------- RANSAC
def inliers(Rm, t, X, f, usable, cos2):
    """(mask, score): the header's rule over the usable observations, in order."""
    with np.errstate(invalid="ignore"):
        p = X @ Rm.T + t
        d = (f * p).sum(axis=1)
        pp = (p * p).sum(axis=1)
        ok = usable & (d > 0) & (d * d >= cos2 * pp)
    # cumsum adds in order, as the kernel's lane does
    score = float(np.cumsum(1.0 - d[ok] * d[ok] / pp[ok])[-1]) if ok.any() else 0.0
    return ok, score


def ransac(X, f, usable, n_hypotheses=256, seed=1, inlier_angle=5e-3, min_inliers=4):
    """One view.  X (cnt, 3) world points, f (cnt, 3) unit bearings, usable
    (cnt,) bool.  Returns dict(status, R, t, n_inliers, mask, h, solution)."""
    cnt = len(X)
    usable = np.asarray(usable, dtype=bool)
    none = dict(R=None, t=None, mask=np.zeros(cnt, dtype=bool), h=-1, solution=-1)
    if usable.sum() < 4:
        return dict(none, status=1, n_inliers=0)
    cos2 = math.cos(inlier_angle) ** 2
    best = None  # (-count, score, h, k)
    keep = None
    for h in range(n_hypotheses):
        tri = sample(seed, h, cnt, usable)
        if tri is None:
            continue
        for k, (Rm, t) in enumerate(p3p(f[tri], X[tri])):
            ok, score = inliers(Rm, t, X, f, usable, cos2)
            key = (-int(ok.sum()), score, h, k)
            if best is None or key < best:
                best, keep = key, (Rm, t, ok)
    if best is None:
        return dict(none, status=2, n_inliers=0)
    if -best[0] < min_inliers:
        return dict(none, status=2, n_inliers=-best[0])
    return dict(status=0, R=keep[0], t=keep[1], n_inliers=-best[0], mask=keep[2], h=best[2],
                solution=best[3])
