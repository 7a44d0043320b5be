"""numpy restatement of acm_homography_4pt and acm_homography_batch (not a
test).

An independent route to the same answer: the null vector of the stacked rows
[f_b]x (x) f_a and the singular values and vectors of H come from
numpy.linalg.svd (the device streams Givens rotations, runs inverse iteration
and a fixed-sweep Jacobi on H^T H).  The decomposition formula (Ma, Soatto,
Kosecka, Sastry 5.3), the sign and ordering rules, the sampler (splitmix64
with Python integers), the inlier rule, the RANSAC key and the refit are the
header's.
"""
import functools
import math

import numpy as np

from relative_pose_ref import GOLDEN, exp_so3, splitmix64

N_DRAWS = 8
N_SAMPLE = 4
SINGULAR = 2.0 ** -40       # sigma_3^2 <= SINGULAR sigma_1^2: no model
ROTATION_FLOOR = 2.0 ** -24  # tau at or below it: a rotation, one solution
COLLINEAR = 2.0 ** -40      # a minimal sample with three bearings in one plane


def draw(seed, h, d, cnt):
    """Draw d (0..7) of hypothesis h: a local index in [0, cnt)."""
    ctr = 8 * h + d + 1
    return (splitmix64(seed + ctr * GOLDEN) * cnt) >> 64


def sample(seed, h, cnt, usable):
    """The four local indices of hypothesis h, or None when it is void."""
    got = []
    for d in range(N_DRAWS):
        j = draw(seed, h, d, cnt)
        if usable[j] and j not in got:
            got.append(j)
            if len(got) == N_SAMPLE:
                return got
    return None


def rows(fa, fb):
    """(3 n, 9): the rows [f_b]x (x) f_a, so that rows @ vec(H) = f_b x (H f_a)."""
    n = len(fa)
    z = np.zeros((n, 3))
    r0 = np.concatenate([z, -fb[:, 2:3] * fa, fb[:, 1:2] * fa], axis=1)
    r1 = np.concatenate([fb[:, 2:3] * fa, z, -fb[:, 0:1] * fa], axis=1)
    r2 = np.concatenate([-fb[:, 1:2] * fa, fb[:, 0:1] * fa, z], axis=1)
    return np.stack([r0, r1, r2], axis=1).reshape(3 * n, 9)


def collinear(f):
    """Three of the four unit bearings f (4, 3) lie in one plane."""
    return min(abs(np.linalg.det(f[[i, j, k]]))
               for i, j, k in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))) <= COLLINEAR


def fit(fa, fb, minimal_check=True):
    """Unit bearings (n, 3), n >= 4 -> (H, s, Vt): H with middle singular
    value 1 and f_b . (H f_a) > 0 for the majority, its singular values and
    right singular vectors; None without a model."""
    if len(fa) < 4 or not (np.isfinite(fa).all() and np.isfinite(fb).all()):
        return None
    if minimal_check and len(fa) == 4 and (collinear(fa) or collinear(fb)):
        return None
    _, _, Vt = np.linalg.svd(rows(fa, fb), full_matrices=True)
    H = Vt[8].reshape(3, 3)
    _, s, Wt = np.linalg.svd(H)
    if not (np.isfinite(s).all() and s[2] ** 2 > SINGULAR * s[0] ** 2):
        return None
    H = H / s[1]
    d = ((fa @ H.T) * fb).sum(axis=1)
    if (d < 0).sum() > (d > 0).sum():
        H = -H
    return H, s / s[1], Wt


def decompose(H, s, Wt, fa):
    """dict(count, R (2, 3, 3), t (2, 3), planes (2, 4), tau, n_front (2,)):
    the slots beyond count are NaN."""
    tau = float(s[0] - s[2])
    R = np.full((2, 3, 3), np.nan)
    t = np.full((2, 3), np.nan)
    planes = np.full((2, 4), np.nan)
    if tau <= ROTATION_FLOOR:
        U, _, Vt = np.linalg.svd(H)
        R[0] = U @ Vt
        t[0] = 0.0
        planes[0] = 0.0
        return dict(count=1, R=R, t=t, planes=planes, tau=tau, n_front=np.array([len(fa), 0]))
    v1, v2, v3 = Wt[0], Wt[1], Wt[2]
    l1, l3 = s[0] ** 2, s[2] ** 2
    a, b = math.sqrt(max(1.0 - l3, 0.0)), math.sqrt(max(l1 - 1.0, 0.0))
    nr = math.hypot(a, b)
    cand = []
    for sign in (1.0, -1.0):
        u = (a * v1 + sign * b * v3) / nr
        n = np.cross(v2, u)
        U = np.column_stack([v2, u, n])
        W = np.column_stack([H @ v2, H @ u, np.cross(H @ v2, H @ u)])
        Rm = W @ U.T
        td = (H - Rm) @ n
        side = fa @ n
        pos, neg = int((side > 0).sum()), int((side < 0).sum())
        sg = 1.0 if pos >= neg else -1.0
        cand.append((max(pos, neg), sg * float(side.sum()), Rm, sg * td, sg * n))
    if (cand[1][0], cand[1][1]) > (cand[0][0], cand[0][1]):
        cand.reverse()
    for k, (nf, _, Rm, td, n) in enumerate(cand):
        ln = np.linalg.norm(td)
        R[k], t[k], planes[k] = Rm, td / ln, np.r_[n, 1.0 / ln]
    return dict(count=2, R=R, t=t, planes=planes, tau=tau,
                n_front=np.array([cand[0][0], cand[1][0]]))


def solve(fa, fb):
    """fa, fb (n, 3), n >= 4, any length.  decompose's dict with H, or None."""
    fa = np.asarray(fa, dtype=np.float64)
    fb = np.asarray(fb, dtype=np.float64)
    with np.errstate(all="ignore"):
        fa = fa / np.linalg.norm(fa, axis=1)[:, None]
        fb = fb / np.linalg.norm(fb, axis=1)[:, None]
    got = fit(fa, fb)
    if got is None:
        return None
    return dict(decompose(*got, fa), H=got[0])


def true_h(Rm, t, n, d):
    """R + (t / d) n^T: its middle singular value is 1 already."""
    return Rm + np.outer(t / d, n)


def solution_error(sol, R0, t0, n0, d0):
    """The smaller of the two slots' max-abs errors in (R, t^, n, d / |t|
    relative); for a pure rotation (t0 = 0) the error in R of slot 0."""
    if not np.any(t0):
        return float(np.abs(sol["R"][0] - R0).max())
    lt = np.linalg.norm(t0)
    best = math.inf
    for k in range(sol["count"]):
        e = max(np.abs(sol["R"][k] - R0).max(), np.abs(sol["t"][k] - t0 / lt).max(),
                np.abs(sol["planes"][k, :3] - n0).max(),
                abs(sol["planes"][k, 3] - d0 / lt) / (d0 / lt))
        best = min(best, float(e))
    return best


# ------------------------------------------------------------------- tuples
N_FAMILY = 4096
N_SPECIAL = 200
SPECIAL = ("rotation", "small_baseline", "oblique")


def planar_scene(rng, Rm, t, nrm, d, n_rows, min_cos=0.2):
    """n_rows matches per problem on the plane nrm . X = d (camera A's frame)
    seen through (R[i], t[i]): unit bearings (n, n_rows, 3) in A and in B.
    Directions N(0, I) with z replaced by |z| + 0.2, drawn again until
    nrm . dir >= min_cos, so a depth is at most d / min_cos."""
    n = len(Rm)
    dirs = np.empty((n, n_rows, 3))
    for i in range(n):
        k = 0
        while k < n_rows:
            v = rng.normal(size=3)
            v[2] = abs(v[2]) + 0.2
            v /= np.linalg.norm(v)
            if v @ nrm[i] >= min_cos:
                dirs[i, k] = v
                k += 1
    X = dirs * (d[:, None] / np.einsum("nki,ni->nk", dirs, nrm))[..., None]
    pb = np.einsum("nij,nkj->nki", Rm, X) + t[:, None, :]
    return dirs, pb / np.linalg.norm(pb, axis=2)[..., None]


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def random_tuples(n, n_rows=4, seed=20261020):
    """The family of the accuracy tests: plane normals (0.5 N, 0.5 N, 1)
    normalised, plane distances d in [2, 8), R = Exp(0.3 N(0, I)), |t| = tau d
    with tau in [0.05, 0.5) in a random direction.  Returns (fa (n, n_rows,
    3), fb, R, t, normal, d)."""
    rng = np.random.default_rng(seed)
    Rm = np.stack([exp_so3(w) for w in 0.3 * rng.normal(size=(n, 3))])
    nrm = _unit(np.column_stack([0.5 * rng.normal(size=(n, 2)), np.ones(n)]))
    d = rng.uniform(2.0, 8.0, n)
    t = _unit(rng.normal(size=(n, 3))) * (rng.uniform(0.05, 0.5, n) * d)[:, None]
    fa, fb = planar_scene(rng, Rm, t, nrm, d, n_rows)
    return fa, fb, Rm, t, nrm, d


def special_tuples(kind, n=N_SPECIAL, seed=20261023):
    """rotation: t = 0; small_baseline: tau = 1e-3; oblique: the plane's
    normal 75 degrees off camera A's axis."""
    rng = np.random.default_rng(seed + SPECIAL.index(kind))
    Rm = np.stack([exp_so3(w) for w in 0.3 * rng.normal(size=(n, 3))])
    nrm = _unit(np.column_stack([0.5 * rng.normal(size=(n, 2)), np.ones(n)]))
    d = rng.uniform(2.0, 8.0, n)
    tau = rng.uniform(0.05, 0.5, n)
    min_cos = 0.2
    if kind == "rotation":
        tau = np.zeros(n)
    elif kind == "small_baseline":
        tau = np.full(n, 1e-3)
    else:
        phi = rng.uniform(0.0, 2.0 * math.pi, n)
        a = math.radians(75.0)
        nrm = np.column_stack([math.sin(a) * np.cos(phi), math.sin(a) * np.sin(phi),
                               np.full(n, math.cos(a))])
        min_cos = 0.1
    t = _unit(rng.normal(size=(n, 3))) * (tau * d)[:, None]
    fa, fb = planar_scene(rng, Rm, t, nrm, d, 4, min_cos)
    return fa, fb, Rm, t, nrm, d


def _frozen(out):
    for arr in out:
        arr.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def family():
    """The N_FAMILY 4-tuples of the accuracy tests (read-only)."""
    return _frozen(random_tuples(N_FAMILY))


@functools.lru_cache(maxsize=None)
def special(kind):
    return _frozen(special_tuples(kind))


def reference_accuracy(fa, fb, R0, t0, n0, d0):
    """(errors (n,) of the matched slot, |H - H_true| (n,), count (n,)) of the
    reference over the tuples."""
    err, herr, cnt = np.empty(len(fa)), np.empty(len(fa)), np.empty(len(fa), dtype=int)
    for i in range(len(fa)):
        sol = solve(fa[i], fb[i])
        err[i] = solution_error(sol, R0[i], t0[i], n0[i], d0[i])
        herr[i] = np.abs(sol["H"] - true_h(R0[i], t0[i], n0[i], d0[i])).max()
        cnt[i] = sol["count"]
    return err, herr, cnt


@functools.lru_cache(maxsize=None)
def family_accuracy():
    return _frozen(reference_accuracy(*family()))


@functools.lru_cache(maxsize=None)
def special_accuracy(kind):
    return _frozen(reference_accuracy(*special(kind)))


def unpack(res):
    """A solver's raw output rows (n, 45) -- count, H (9), poses (24), planes
    (8), tau, n_front (2) -- as a list of solve()-like dicts."""
    out = []
    for r in res:
        poses = r[10:34].reshape(2, 12)
        out.append(dict(count=int(r[0]), H=r[1:10].reshape(3, 3), R=poses[:, :9].reshape(2, 3, 3),
                        t=poses[:, 9:], planes=r[34:42].reshape(2, 4), tau=float(r[42]),
                        n_front=r[43:45].astype(int)))
    return out


def check_solutions(sols, fa, fb, R0, t0, n0, d0):
    """(errors (n,), |H - H_true| (n,), worst |R^T R - I|, worst |f_b x H f_a|)
    of a solver under test; asserts finiteness, det R > 0, |t| = |n| = 1, the
    middle singular value 1, H = R + (t / d) n^T per slot and the slots'
    order."""
    n = len(fa)
    err, herr = np.empty(n), np.empty(n)
    orth = resid = 0.0
    for i, sol in enumerate(sols):
        H = sol["H"]
        assert sol["count"] in (1, 2) and np.isfinite(H).all(), i
        assert abs(np.linalg.svd(H, compute_uv=False)[1] - 1.0) <= 1e-12, i
        ua, ub = _unit(fa[i]), _unit(fb[i])
        g = ua @ H.T
        assert ((g * ub).sum(axis=1) > 0).sum() * 2 >= len(ua), i
        resid = max(resid, float(np.abs(np.cross(ub, g)).max()))
        for k in range(sol["count"]):
            Rm, t, pl = sol["R"][k], sol["t"][k], sol["planes"][k]
            assert np.isfinite(Rm).all() and np.isfinite(t).all() and np.isfinite(pl).all(), (i, k)
            assert np.linalg.det(Rm) > 0, (i, k)
            orth = max(orth, float(np.abs(Rm.T @ Rm - np.eye(3)).max()))
            if sol["count"] == 2:
                assert abs(np.linalg.norm(t) - 1.0) <= 1e-12, (i, k)
                assert abs(np.linalg.norm(pl[:3]) - 1.0) <= 1e-12, (i, k)
                back = Rm + np.outer(t / pl[3], pl[:3])
                assert np.abs(back - H).max() <= 1e-9 / min(sol["tau"], 1.0), (i, k)
                assert sol["n_front"][k] == max(((ua @ pl[:3]) > 0).sum(), 0), (i, k)
        for k in range(sol["count"], 2):
            assert np.isnan(sol["R"][k]).all() and np.isnan(sol["planes"][k]).all(), (i, k)
        if sol["count"] == 2:
            assert sol["n_front"][0] >= sol["n_front"][1], i
            assert abs(sol["tau"] - 1.0 / sol["planes"][0, 3]) <= 1e-9, i
        err[i] = solution_error(sol, R0[i], t0[i], n0[i], d0[i])
        herr[i] = np.abs(H - true_h(R0[i], t0[i], n0[i], d0[i])).max()
    return err, herr, orth, resid


def failing_tuples():
    """(fa (6, 4, 3), fb): a NaN bearing, an Inf bearing, a zero bearing in A,
    a zero bearing in B, a repeated match, three collinear points."""
    fa, fb = random_tuples(6, seed=5)[:2]
    fa, fb = fa.copy(), fb.copy()
    fa[0, 3, 1] = np.nan
    fb[1, 2, 0] = np.inf
    fa[2, 0] = 0.0
    fb[3, 1] = 0.0
    fa[4, 2], fb[4, 2] = fa[4, 0], fb[4, 0]
    fa[5, 2] = _unit(fa[5, 0] + fa[5, 1])
    return fa, fb


# -------------------------------------------------------------------- RANSAC
def transfer(H, fa, fb):
    """(c . c / g . g, f_b . g) with g = H f_a, c = f_b x g."""
    g = fa @ H.T
    c = np.cross(fb, g)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (c * c).sum(axis=1) / (g * g).sum(axis=1), (fb * g).sum(axis=1)


def inliers(H, fa, fb, usable, sin2):
    """(mask, score): the header's rule over the usable matches, in order."""
    with np.errstate(invalid="ignore"):
        e, dot = transfer(H, fa, fb)
        ok = usable & (dot > 0) & (e <= sin2)
    score = float(np.cumsum(e[ok])[-1]) if ok.any() else 0.0
    return ok, score


def ransac(fa, fb, usable, n_hypotheses=256, seed=1, inlier_angle=5e-3, min_inliers=4,
           refit_rounds=3):
    """One pair.  fa, fb (cnt, 3) unit bearings, usable (cnt,) bool.  Returns
    dict(status, H, sol, n_inliers, mask, h, refits); sol is decompose's dict
    over the final inliers."""
    cnt = len(fa)
    usable = np.asarray(usable, dtype=bool)
    none = dict(H=None, sol=None, mask=np.zeros(cnt, dtype=bool), h=-1, refits=0)
    if usable.sum() < 4:
        return dict(none, status=1, n_inliers=0)
    fa = np.where(usable[:, None], fa, 0.0)
    fb = np.where(usable[:, None], fb, 0.0)
    sin2 = math.sin(inlier_angle) ** 2
    best = keep = None  # (-count, score, h)
    for h in range(n_hypotheses):
        idx = sample(seed, h, cnt, usable)
        if idx is None:
            continue
        got = fit(fa[idx], fb[idx])
        if got is None:
            continue
        ok, score = inliers(got[0], fa, fb, usable, sin2)
        key = (-int(ok.sum()), score, h)
        if best is None or key < best:
            best, keep = key, (got, ok)
    if best is None:
        return dict(none, status=2, n_inliers=0)
    if -best[0] < min_inliers:
        return dict(none, status=2, n_inliers=-best[0])
    refits = 0
    for _ in range(refit_rounds):
        got = fit(fa[keep[1]], fb[keep[1]], minimal_check=False)
        if got is None:
            break
        ok, score = inliers(got[0], fa, fb, usable, sin2)
        if (-int(ok.sum()), score) < best[:2]:
            best, keep = (-int(ok.sum()), score, best[2]), (got, ok)
            refits += 1
        else:
            break
    got, ok = keep
    return dict(status=0, H=got[0], sol=decompose(*got, fa[ok]), n_inliers=-best[0], mask=ok,
                h=best[2], refits=refits)
