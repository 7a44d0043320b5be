"""numpy restatement of acm_relative_pose_8pt and acm_relative_pose_batch (not
a test).

An independent route to the same answer: the null vector of the stacked rows
f_b (x) f_a comes from numpy.linalg.svd (the device streams Givens rotations
and runs inverse iteration), and E is decomposed by the textbook SVD recipe
(the device uses Horn's closed form).  The cheirality rule, the sampler
(splitmix64 with Python integers), the inlier rule, the RANSAC key and the
refit are the header's.
"""
import functools
import math

import numpy as np

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
N_DRAWS = 16
N_SAMPLE = 8


def splitmix64(z):
    z &= MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def draw(seed, h, d, cnt):
    """Draw d (0..15) of hypothesis h: a local index in [0, cnt)."""
    ctr = 16 * h + d + 1
    return (splitmix64(seed + ctr * GOLDEN) * cnt) >> 64


def sample(seed, h, cnt, usable):
    """The eight local indices of hypothesis h, or None when it is void."""
    got = []
    for d in range(N_DRAWS):
        j = draw(seed, h, d, cnt)
        if usable[j] and j not in got:
            got.append(j)
            if len(got) == N_SAMPLE:
                return got
    return None


def exp_so3(w):
    th = np.linalg.norm(w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * (K @ K)


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def front(Rm, t, fa, fb):
    """(n,) bool: the match is in front of both cameras of (R, t)."""
    g = fa @ Rm.T
    c = (g * fb).sum(axis=1)
    fbt, gt = fb @ t, g @ t
    return (c * fbt - gt > 0) & (fbt - c * gt > 0)


def solve(fa, fb):
    """fa, fb (n, 3), n >= 8, any length.  Returns dict(R, t, E, n_front, s8)
    -- E of unit Frobenius norm signed as [t]x R, s8 the second-smallest
    singular value of the rows (the smallest is 0 for n = 8) -- or None."""
    fa = np.asarray(fa, dtype=np.float64)
    fb = np.asarray(fb, dtype=np.float64)
    with np.errstate(all="ignore"):
        fa = fa / np.linalg.norm(fa, axis=1)[:, None]
        fb = fb / np.linalg.norm(fb, axis=1)[:, None]
    if len(fa) < 8 or not (np.isfinite(fa).all() and np.isfinite(fb).all()):
        return None
    A = (fb[:, :, None] * fa[:, None, :]).reshape(len(fa), 9)
    _, s, Vt = np.linalg.svd(A, full_matrices=True)
    s9 = np.concatenate([s, np.zeros(9 - len(s))]) if len(s) < 9 else s
    E = Vt[8].reshape(3, 3)
    U, _, Wt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Wt) < 0:
        Wt = -Wt
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    best = None
    for Rm in (U @ W @ Wt, U @ W.T @ Wt):
        for t in (U[:, 2], -U[:, 2]):
            n = int(front(Rm, t, fa, fb).sum())
            if best is None or n > best[0]:
                best = (n, Rm, t)
    n, Rm, t = best
    Et = skew(t) @ Rm
    return dict(R=Rm, t=t, E=Et / np.linalg.norm(Et), n_front=n, s8=float(s9[7]))


def pose_error(Rm, t, R0, t0):
    """max-abs error in (R, t / |t|)."""
    return float(max(np.abs(Rm - R0).max(), np.abs(t - t0 / np.linalg.norm(t0)).max()))


def angles(Rm, t, R0, t0):
    """(rotation error, angle between the translation directions), radians."""
    c = (np.trace(Rm.T @ R0) - 1.0) / 2.0
    s = np.linalg.norm(Rm - R0) / math.sqrt(2.0)  # 2 sqrt(2) sin(angle / 2) / sqrt(2)
    rot = 2.0 * math.asin(min(1.0, s / 2.0)) if c > 0.9 else math.acos(max(-1.0, min(1.0, c)))
    u, v = t / np.linalg.norm(t), t0 / np.linalg.norm(t0)
    return rot, math.atan2(np.linalg.norm(np.cross(u, v)), float(u @ v))


# ------------------------------------------------------------------- tuples
N_FAMILY = 4096
N_SPECIAL = 200
SPECIAL = ("x", "y", "z", "roll_forward", "half_turn_x")


def _scene(rng, n, rows, Rm, t):
    """rows matches per problem seen through (R[i], t[i]): unit bearings
    (n, rows, 3) in A and in B."""
    d = rng.normal(size=(n, rows, 3))
    d[..., 2] = np.abs(d[..., 2]) + 0.2
    d /= np.linalg.norm(d, axis=2)[..., None]
    X = d * rng.uniform(2.0, 8.0, (n, rows))[..., None]
    pb = np.einsum("nij,nkj->nki", Rm, X) + t[:, None, :]
    return d, pb / np.linalg.norm(pb, axis=2)[..., None]


def random_tuples(n, rows=8, seed=20261020):
    """The family of the accuracy tests: directions N(0, I) with z replaced by
    |z| + 0.2, normalised; depths in [2, 8); R = Exp(0.3 N(0, I)); t in [-0.5,
    0.5)^3.  Returns (fa (n, rows, 3), fb, R (n, 3, 3), t (n, 3))."""
    rng = np.random.default_rng(seed)
    Rm = np.stack([exp_so3(w) for w in 0.3 * rng.normal(size=(n, 3))])
    t = rng.uniform(-0.5, 0.5, (n, 3))
    fa, fb = _scene(rng, n, rows, Rm, t)
    return fa, fb, Rm, t


def special_tuples(kind, n=N_SPECIAL, seed=20261021):
    """Motions that put zeros into E: R = I with t along x, y or z, a 90 degree
    roll with forward motion, a 180 degree rotation about x."""
    rng = np.random.default_rng(seed + SPECIAL.index(kind))
    length = rng.uniform(0.2, 1.0, n)
    t = np.zeros((n, 3))
    Rm = np.tile(np.eye(3), (n, 1, 1))
    if kind in ("x", "y", "z"):
        t[:, "xyz".index(kind)] = length
    elif kind == "roll_forward":
        Rm[:] = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
        t[:, 2] = length
    else:
        Rm[:] = np.diag([1.0, -1.0, -1.0])
        t[:] = rng.uniform(-0.5, 0.5, (n, 3))
    fa, fb = _scene(rng, n, 8, Rm, t)
    return fa, fb, Rm, t


def _frozen(out):
    for arr in out:
        arr.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def family():
    """The N_FAMILY 8-tuples of the accuracy tests (read-only)."""
    return _frozen(random_tuples(N_FAMILY))


@functools.lru_cache(maxsize=None)
def special(kind):
    return _frozen(special_tuples(kind))


def reference_accuracy(fa, fb, R0, t0):
    """(errors (n,) -- max-abs in (R, t^) --, s8 (n,), n_front (n,)) of the
    reference over the tuples."""
    err, s8, nf = np.empty(len(fa)), np.empty(len(fa)), np.empty(len(fa), dtype=int)
    for i in range(len(fa)):
        sol = solve(fa[i], fb[i])
        err[i] = pose_error(sol["R"], sol["t"], R0[i], t0[i])
        s8[i], nf[i] = sol["s8"], sol["n_front"]
    return err, s8, nf


@functools.lru_cache(maxsize=None)
def family_accuracy():
    return _frozen(reference_accuracy(*family()))


@functools.lru_cache(maxsize=None)
def special_accuracy(kind):
    return _frozen(reference_accuracy(*special(kind)))


def check_solutions(poses, essential, n_front, fa, fb, R0, t0, s8):
    """poses (n, 12), essential (n, 9), n_front (n,) of a solver under test:
    (errors (n,), worst |R^T R - I|, worst |f_b^T E f_a| over the tuples with
    s8 >= 1e-3); asserts det > 0, |E| = 1 and E ~ [t]x R."""
    n = len(fa)
    err = np.empty(n)
    orth = resid = 0.0
    for i in range(n):
        Rm, t, E = poses[i, :9].reshape(3, 3), poses[i, 9:], essential[i].reshape(3, 3)
        assert np.isfinite(poses[i]).all() and np.isfinite(E).all(), i
        assert np.linalg.det(Rm) > 0, i
        assert abs(np.linalg.norm(E) - 1.0) <= 1e-12, i
        assert abs(np.linalg.norm(t) - 1.0) <= 1e-12, i
        orth = max(orth, float(np.abs(Rm.T @ Rm - np.eye(3)).max()))
        err[i] = pose_error(Rm, t, R0[i], t0[i])
        if s8[i] >= 1e-3:
            resid = max(resid, float(np.abs(np.einsum("ki,ij,kj->k", fb[i], E, fa[i])).max()))
            Et = skew(t) @ Rm
            assert np.abs(Et / np.linalg.norm(Et) - E).max() <= 1e-6, i
    return err, orth, resid


def failing_tuples():
    """(fa (4, 8, 3), fb): a NaN bearing, an Inf bearing, a zero bearing in A,
    a zero bearing in B."""
    fa, fb, _, _ = random_tuples(4, seed=5)
    fa, fb = fa.copy(), fb.copy()
    fa[0, 3, 1] = np.nan
    fb[1, 7, 0] = np.inf
    fa[2, 0] = 0.0
    fb[3, 5] = 0.0
    return fa, fb


# -------------------------------------------------------------------- RANSAC
def epipolar(Rm, t, fa, fb):
    """(d^2 / (n . n), n . n): the squared sine of the angle between f_b and
    the epipolar plane of f_a, and the squared parallax term."""
    g = fa @ Rm.T
    n = np.cross(t, g)
    d = (fb * n).sum(axis=1)
    nn = (n * n).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return d * d / nn, nn, d


def inliers(Rm, t, fa, fb, usable, sin2):
    """(mask, score): the header's rule over the usable matches, in order."""
    with np.errstate(invalid="ignore", divide="ignore"):
        e, nn, d = epipolar(Rm, t, fa, fb)
        ok = usable & (nn > 0) & (d * d <= sin2 * nn) & front(Rm, t, fa, fb)
    score = float(np.cumsum(e[ok])[-1]) if ok.any() else 0.0
    return ok, score


def ransac(fa, fb, usable, n_hypotheses=512, seed=1, inlier_angle=5e-3, min_inliers=8,
           refit_rounds=3):
    """One pair.  fa, fb (cnt, 3) unit bearings, usable (cnt,) bool.  Returns
    dict(status, R, t, n_inliers, mask, h, refits)."""
    cnt = len(fa)
    usable = np.asarray(usable, dtype=bool)
    none = dict(R=None, t=None, mask=np.zeros(cnt, dtype=bool), h=-1, refits=0)
    if usable.sum() < 8:
        return dict(none, status=1, n_inliers=0)
    fa = np.where(usable[:, None], fa, 0.0)
    fb = np.where(usable[:, None], fb, 0.0)
    sin2 = math.sin(inlier_angle) ** 2
    best = keep = None  # (-count, score, h)
    for h in range(n_hypotheses):
        idx = sample(seed, h, cnt, usable)
        if idx is None:
            continue
        sol = solve(fa[idx], fb[idx])
        if sol is None or not (np.isfinite(sol["R"]).all() and np.isfinite(sol["t"]).all()):
            continue
        ok, score = inliers(sol["R"], sol["t"], fa, fb, usable, sin2)
        key = (-int(ok.sum()), score, h)
        if best is None or key < best:
            best, keep = key, (sol["R"], sol["t"], ok)
    if best is None:
        return dict(none, status=2, n_inliers=0)
    if -best[0] < min_inliers:
        return dict(none, status=2, n_inliers=-best[0])
    refits = 0
    for _ in range(refit_rounds):
        sol = solve(fa[keep[2]], fb[keep[2]])
        if sol is None:
            break
        ok, score = inliers(sol["R"], sol["t"], fa, fb, usable, sin2)
        if (-int(ok.sum()), score) < best[:2]:
            best, keep = (-int(ok.sum()), score, best[2]), (sol["R"], sol["t"], ok)
            refits += 1
        else:
            break
    return dict(status=0, R=keep[0], t=keep[1], n_inliers=-best[0], mask=keep[2], h=best[2],
                refits=refits)


def gross_outliers(rng, Rm, t, fa, n, sin_min):
    """n unit bearings in B, uniform on the sphere, each drawn again until its
    epipolar sine against fa[i] at the true pose exceeds sin_min: the epipolar
    constraint is one-dimensional, so a random bearing satisfies it by chance
    unless the generator rules that out."""
    out = np.empty((n, 3))
    for i in range(n):
        while True:
            g = rng.normal(size=3)
            g /= np.linalg.norm(g)
            e, nn, _ = epipolar(Rm, t / np.linalg.norm(t), fa[i:i + 1], g[None])
            if nn[0] > 0 and e[0] > sin_min ** 2:
                out[i] = g
                break
    return out
