"""The numpy restatement of acm_similarity_3pt / acm_similarity_batch
(include/acm.h): the least-squares similarity b ~ s R a + t between two 3-D
point sets and the RANSAC over its 3-point form.

The fit is Umeyama's: the SVD of M = sum (b - bm)(a - am)^T with the
determinant correction -- on purpose not the kernel's algorithm (Horn's
quaternion through a Jacobi eigensolver).  The void rules are the kernel's,
stated once, in `fit`: the eigenvalues of Horn's N follow from M's singular
values, lambda_1 = s1 + s2 + d s3 and lambda_2 = s1 - s2 - d s3 with d = det(U)
det(V).  The RANSAC is the header's: the draw, the sample rule, the inlier
rule, the key and the refit rule.
"""
import functools
import math

import numpy as np

from relative_pose_ref import GOLDEN, exp_so3, splitmix64

N_DRAWS = 6
N_SAMPLE = 3
GAP = 1e-9  # void unless lambda_1 - lambda_2 > GAP lambda_1
OK, TOO_FEW_POINTS, NO_MODEL = 0, 1, 2


def draw(seed, h, d, cnt):
    """Draw d (0..5) of hypothesis h: a local index in [0, cnt)."""
    ctr = N_DRAWS * h + d + 1
    return (splitmix64(seed + ctr * GOLDEN) * cnt) >> 64


def sample(seed, h, cnt, usable):
    """The three local indices of hypothesis h, or None when it is void."""
    got = []
    for d in range(N_DRAWS):
        j = draw(seed, h, d, cnt)
        if usable[j] and j not in got:
            got.append(j)
            if len(got) == N_SAMPLE:
                return got
    return None


# ----------------------------------------------------------------- the fit
def fit(a, b, rigid=False):
    """(R, t, s) of the n >= 3 correspondences a, b (n, 3), or None: void."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    if len(a) < 3 or not (np.isfinite(a).all() and np.isfinite(b).all()):
        return None
    am, bm = a.mean(axis=0), b.mean(axis=0)
    da, db = a - am, b - bm
    M = db.T @ da
    Saa = float((da * da).sum())
    if not (np.isfinite(M).all() and np.isfinite(Saa) and Saa > 0.0):
        return None
    U, sv, Vt = np.linalg.svd(M)
    d = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) > 0 else -1.0
    lam1, lam2 = sv[0] + sv[1] + d * sv[2], sv[0] - sv[1] - d * sv[2]
    if not (lam1 > 0.0 and lam1 - lam2 > GAP * lam1):
        return None
    R = U @ np.diag([1.0, 1.0, d]) @ Vt
    s = 1.0 if rigid else lam1 / Saa
    if not s > 0.0:
        return None
    t = bm - s * (R @ am)
    if not (np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(s)):
        return None
    return R, t, s


def pack(model):
    """13 doubles (R row-major, t, s); NaN for None."""
    if model is None:
        return np.full(13, np.nan)
    return np.concatenate([model[0].reshape(9), model[1], [model[2]]])


def unpack(row):
    row = np.asarray(row, dtype=float)
    return row[:9].reshape(3, 3), row[9:12], float(row[12])


def apply(model, a):
    R, t, s = model
    return s * (np.asarray(a) @ R.T) + t


def model_error(model, R0, t0, s0):
    """max( max|R - R0|, max|t - t0| / max(1, max|t0|), |s / s0 - 1| )"""
    R, t, s = model
    return max(np.abs(R - R0).max(), np.abs(t - t0).max() / max(1.0, np.abs(t0).max()),
               abs(s / s0 - 1.0))


# ------------------------------------------------------------- the families
N_FAMILY = 4096
N_SPECIAL = 200
SPECIAL = ("scale_small", "scale_large", "half_turn", "identity", "thin")


def sin2_first_vertex(a):
    """sin^2 of the angle at the first vertex of the triangles a (n, 3, 3)."""
    u, v = a[:, 1] - a[:, 0], a[:, 2] - a[:, 0]
    c = np.cross(u, v)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (c * c).sum(axis=1) / ((u * u).sum(axis=1) * (v * v).sum(axis=1))


def _triangles(rng, n):
    """a = 2 N(0, I) + 10 N(0, I) per triple (off the origin), drawn again
    until sin^2 of the angle at the first vertex is >= 0.01"""
    a = np.empty((n, 3, 3))
    todo = np.arange(n)
    while len(todo):
        a[todo] = 2.0 * rng.normal(size=(len(todo), 3, 3)) + 10.0 * rng.normal(size=(len(todo), 1, 3))
        todo = todo[~(sin2_first_vertex(a[todo]) >= 0.01)]
    return a


def _motion(rng, n):
    R0 = np.stack([exp_so3(w) for w in rng.normal(size=(n, 3))])
    s0 = np.exp(rng.uniform(math.log(0.1), math.log(10.0), n))
    t0 = 10.0 * rng.normal(size=(n, 3))
    return R0, t0, s0


def _image(a, R0, t0, s0):
    return s0[:, None, None] * np.einsum("nij,nkj->nki", R0, a) + t0[:, None, :]


def random_triples(n, seed=20261021):
    rng = np.random.default_rng(seed)
    a = _triangles(rng, n)
    R0, t0, s0 = _motion(rng, n)
    return a, _image(a, R0, t0, s0), R0, t0, s0


def special_triples(kind, n=N_SPECIAL, seed=20261022):
    rng = np.random.default_rng(seed + SPECIAL.index(kind))
    a = _triangles(rng, n)
    R0, t0, s0 = _motion(rng, n)
    if kind == "scale_small":
        s0[:] = 1e-3
    elif kind == "scale_large":
        s0[:] = 1e3
    elif kind == "half_turn":  # the quaternion's q0 ~ 0
        axis = rng.normal(size=(n, 3))
        axis /= np.linalg.norm(axis, axis=1)[:, None]
        R0 = np.stack([exp_so3((math.pi - 1e-6) * w) for w in axis])
    elif kind == "identity":
        R0 = np.broadcast_to(np.eye(3), (n, 3, 3)).copy()
        t0[:] = 0.0
        s0[:] = 1.0
    elif kind == "thin":  # sin^2 = 1e-6 of the angle at the first vertex
        u = rng.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=1)[:, None]
        v = np.cross(u, rng.normal(size=(n, 3)))
        v /= np.linalg.norm(v, axis=1)[:, None]
        sn = 1e-3
        l1, l2 = rng.uniform(1.0, 3.0, (2, n))
        a[:, 1] = a[:, 0] + l1[:, None] * u
        a[:, 2] = a[:, 0] + l2[:, None] * (math.sqrt(1.0 - sn * sn) * u + sn * v)
    return a, _image(a, R0, t0, s0), R0, t0, s0


def _frozen(out):
    for arr in out:
        arr.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def family():
    """The N_FAMILY triples of the accuracy tests (read-only):
    (a (n, 3, 3), b (n, 3, 3), R (n, 3, 3), t (n, 3), s (n,))."""
    return _frozen(random_triples(N_FAMILY))


@functools.lru_cache(maxsize=None)
def special(kind):
    return _frozen(special_triples(kind))


def reference_accuracy(a, b, R0, t0, s0, rigid=False):
    """The reference's error (n,) over the triples; NaN where it is void."""
    err = np.full(len(a), np.nan)
    for i in range(len(a)):
        got = fit(a[i], b[i], rigid)
        if got is not None:
            err[i] = model_error(got, R0[i], t0[i], s0[i])
    return err


@functools.lru_cache(maxsize=None)
def family_accuracy():
    return _frozen((reference_accuracy(*family()),))[0]


@functools.lru_cache(maxsize=None)
def special_accuracy(kind):
    return _frozen((reference_accuracy(*special(kind)),))[0]


def failing_triples():
    """(a, b) (5, 3, 3): collinear, two coincident points, all coincident, a
    NaN, an Inf."""
    a, b = (np.array(x[:5]) for x in family()[:2])
    R0, t0, s0 = (x[:5] for x in family()[2:])
    a[0, 2] = a[0, 0] + 0.37 * (a[0, 1] - a[0, 0])
    a[1, 1] = a[1, 0]
    a[2, 1] = a[2, 0]
    a[2, 2] = a[2, 0]
    b[:3] = _image(a[:3], R0[:3], t0[:3], s0[:3])
    a[3, 1, 2] = np.nan
    b[4, 0, 0] = np.inf
    return a, b


def offset_set(n, offset=1e6, seed=5):
    """n exact correspondences with `offset` added to every coordinate of a:
    (a (n, 3), b (n, 3), R, t, s).  A raw-moment fit cancels here."""
    rng = np.random.default_rng(seed + n)
    a = 2.0 * rng.normal(size=(n, 3))
    if n == 3:
        a = _triangles(rng, 1)[0] - 10.0
    a = a + offset
    R0, t0, s0 = (x[0] for x in _motion(rng, 1))
    return a, s0 * (a @ R0.T) + t0, R0, t0, s0


# ------------------------------------------------------------------- scenes
def scene(rng, n, s0=2.5, noise=0.01, moved=0.4, rigid=False):
    """n correspondences in the box [+-4, +-3, 6 +- 2]: b = s R a + t + noise
    N(0, I) per axis, a fraction `moved` of b displaced by N(0, I).  Returns
    (a, b, R, t, s, far): far marks b more than 0.2 from the true transform."""
    a = rng.uniform(-1.0, 1.0, (n, 3)) * np.array([4.0, 3.0, 2.0]) + np.array([0.0, 0.0, 6.0])
    R0 = exp_so3(rng.normal(size=3))
    t0 = rng.normal(size=3)
    s0 = 1.0 if rigid else s0
    b = s0 * (a @ R0.T) + t0
    truth = b.copy()
    b = b + noise * rng.normal(size=(n, 3))
    bad = np.zeros(n, dtype=bool)
    bad[rng.permutation(n)[:int(round(moved * n))]] = True
    b[bad] += rng.normal(size=(int(bad.sum()), 3))
    far = np.linalg.norm(b - truth, axis=1) > 0.2
    return a, b, R0, t0, s0, far


# ------------------------------------------------------------------- RANSAC
def residual2(model, a, b):
    e = b - apply(model, a)
    return (e * e).sum(axis=1)


def inliers(model, a, b, usable, d2):
    """(mask, score): the header's rule over the usable correspondences."""
    with np.errstate(invalid="ignore"):
        e = residual2(model, a, b)
        ok = usable & (e <= d2)
    score = float(np.cumsum(e[ok])[-1]) if ok.any() else 0.0
    return ok, score


def usable_rows(a, b):
    return np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1)


def ransac(a, b, inlier_distance, n_hypotheses=256, seed=1, min_inliers=3, refit_rounds=3,
           rigid=False):
    """One set.  a, b (cnt, 3).  Returns dict(status, model, n_inliers, mask,
    rms, n_usable, h, refits)."""
    a, b = np.asarray(a, dtype=float).reshape(-1, 3), np.asarray(b, dtype=float).reshape(-1, 3)
    cnt = len(a)
    usable = usable_rows(a, b)
    none = dict(model=None, mask=np.zeros(cnt, dtype=bool), rms=np.nan, h=-1, refits=0,
                n_usable=int(usable.sum()))
    if usable.sum() < 3:
        return dict(none, status=TOO_FEW_POINTS, n_inliers=0)
    a = np.where(usable[:, None], a, 0.0)
    b = np.where(usable[:, None], b, 0.0)
    d2 = inlier_distance * inlier_distance
    best = keep = None  # (-count, score, h)
    for h in range(n_hypotheses):
        idx = sample(seed, h, cnt, usable)
        if idx is None:
            continue
        got = fit(a[idx], b[idx], rigid)
        if got is None:
            continue
        ok, score = inliers(got, a, b, usable, d2)
        key = (-int(ok.sum()), score, h)
        if best is None or key < best:
            best, keep = key, (got, ok)
    if best is None:
        return dict(none, status=NO_MODEL, n_inliers=0)
    if -best[0] < min_inliers:
        return dict(none, status=NO_MODEL, n_inliers=-best[0])
    refits = 0
    for _ in range(refit_rounds):
        got = fit(a[keep[1]], b[keep[1]], rigid)
        if got is None:
            break
        ok, score = inliers(got, a, b, usable, d2)
        if (-int(ok.sum()), score) < best[:2]:
            best, keep = (-int(ok.sum()), score, best[2]), (got, ok)
            refits += 1
        else:
            break
    got, ok = keep
    e = residual2(got, a[ok], b[ok])
    return dict(status=OK, model=got, n_inliers=-best[0], mask=ok, rms=math.sqrt(e.sum() / ok.sum()),
                h=best[2], refits=refits, n_usable=int(usable.sum()))
