"""Exact sums for the fused intrinsic normal equations (not a test).

Every function takes a camera key (camera_zoo.camera_of): a model id for the
sample camera of samples.SAMPLES, or the name of a zoo camera.

Points: the 246 finite rows of point_jacobian_ref.base_points(key) -- the 240
grid rays, the on-axis and near-axis points and the four finite edge rows
(centre, behind).  The NaN / Inf rows are dropped: the oracle projects them
"Ok" to NaN, as the reference does, and a sum over them has no reference.
Larger shapes tile the rows: point i = base[i mod 246]; 246 is no multiple of
64 or 256, so every wave / workgroup seam lands on different data.

Evaluation camera: off the optimum -- fx x 1.01, fy x 0.995, cx + 1.5,
cy - 2.0, the distortion parameters untouched, so that a zoo camera stays on
the branch it was chosen for (alpha = 0.5 exactly, ...).

Observations: the oracle's pixels at the UNPERTURBED camera (3.0 where it
fails) plus N(0, 0.5) noise from a fixed seed, one row per point index up to
4099.

Reference: per base row the 2 x P Jacobian (mp.diff of mp_models.project in
each parameter, 50 digits) and the 50-digit projection at the evaluation
camera, rounded to float64 and cached per camera.  exact() sums the per-point
terms with math.fsum; check() holds every entry of a result to

    |got - exact| <= max(1e-10 |exact|, 1e-13 sum |terms|),

the rule of the pose, pose-batch, triangulation and calibration sums.  A
relative error on each entry on its own, not on the block's largest one: the
entries of one J^T J span 1e5 to 1e11 (tests/test_normal_equations_ref.py).
terms_exact() is the same sum over any per-point r and J, for the tests whose
points are not the base set.

Callers must not modify the returned arrays.
"""
import functools
import math

import numpy as np

import mp_models
import oracle
import point_jacobian_ref as R
from camera_zoo import camera_of

N_BASE = 246
N_NOISE = 4099
REL, ABS = 1e-10, 1e-13
MIN_VALID = 240
# (fx, fy), (fx, cy), (fy, cx), (cx, cy): du/dfy = du/dcy = dv/dfx = dv/dcx = 0
STRUCTURAL_ZEROS = ((0, 1), (0, 3), (1, 2), (2, 3))


@functools.lru_cache(maxsize=None)
def base_points(key):
    """(246, 3) float64: the finite rows of point_jacobian_ref.base_points."""
    pts = R.base_points(key)
    pts = pts[np.isfinite(pts).all(axis=1)].copy()
    assert pts.shape == (N_BASE, 3)
    pts.setflags(write=False)
    return pts


def eval_params(key):
    """The evaluation camera's parameter list (off the optimum)."""
    _, params, _ = camera_of(key)
    p = [float(c) for c in params]
    p[0] *= 1.01
    p[1] *= 0.995
    p[2] += 1.5
    p[3] -= 2.0
    return p


def points(key, n):
    """(n, 3): point i = base[i mod 246]."""
    return R.tiled(base_points(key), n)


@functools.lru_cache(maxsize=None)
def _noise():
    z = np.random.default_rng(20261021).normal(0.0, 0.5, (N_NOISE, 2))
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def _base_observations(key):
    model, params, (w, h) = camera_of(key)
    uv, st, _ = oracle.project(model, params, w, h, base_points(key))
    uv = np.where((st != 0)[:, None], 3.0, uv)
    assert np.isfinite(uv).all()
    uv.setflags(write=False)
    return uv


def observations(key, n):
    """(n, 2): the unperturbed camera's pixels of the tiled points + noise."""
    assert n <= N_NOISE
    return _base_observations(key)[np.arange(n) % N_BASE] + _noise()[:n]


@functools.lru_cache(maxsize=None)
def base_terms(key):
    """At the evaluation camera, per base row: J (246, 2, P) and uv (246, 2)
    from 50 digits (0 in the rows that are not valid), and the valid rows:
    those the oracle projects Ok there."""
    model, _, (w, h) = camera_of(key)
    p = eval_params(key)
    pts = base_points(key)
    _, st, _ = oracle.project(model, p, w, h, pts)
    valid = st == 0
    assert int(valid.sum()) >= MIN_VALID, (key, int(valid.sum()))
    J = np.zeros((N_BASE, 2, len(p)))
    uv = np.zeros((N_BASE, 2))
    for i in np.nonzero(valid)[0]:
        pt = [float(c) for c in pts[i]]
        Ju, Jv = mp_models.jacobian(model, p, pt)
        u, v = mp_models.project(model, p, pt)
        J[i, 0] = [float(c) for c in Ju]
        J[i, 1] = [float(c) for c in Jv]
        uv[i] = float(u), float(v)
    for a in (J, uv, valid):
        a.setflags(write=False)
    return J, uv, valid


def _fsum(terms):
    """(exact sum, sum of magnitudes) of a float64 array, each rounded once."""
    t = terms[terms != 0.0]
    return math.fsum(t.tolist()), math.fsum(np.abs(t).tolist())


def terms_exact(J, r, sentinels=0):
    """want, mag over the slots [JtJ (P*P) | Jtr (P) | cost] of the points
    with Jacobians J (m, 2, P) and residuals r (m, 2): want = fsum(terms), mag
    = fsum(|terms|), the terms J[:,0,a] J[:,0,b] and J[:,1,a] J[:,1,b], then
    J r, then 0.5 r^2.  sentinels: the number of invalid points under
    ACM_INVALID_SENTINEL, one cost term of 1e12 each (the kernel adds 2e12 to
    r.r); their J is 0 under both policies (include/acm.h)."""
    P = J.shape[2]
    want = np.zeros(P * P + P + 1)
    mag = np.zeros(P * P + P + 1)
    for a in range(P):
        for b in range(a, P):
            s = _fsum(np.concatenate([J[:, 0, a] * J[:, 0, b], J[:, 1, a] * J[:, 1, b]]))
            want[a * P + b], mag[a * P + b] = s
            want[b * P + a], mag[b * P + a] = s
        want[P * P + a], mag[P * P + a] = _fsum(
            np.concatenate([J[:, 0, a] * r[:, 0], J[:, 1, a] * r[:, 1]]))
    cost = np.concatenate([0.5 * r[:, 0] ** 2, 0.5 * r[:, 1] ** 2, np.full(sentinels, 1e12)])
    want[P * P + P], mag[P * P + P] = _fsum(cost)
    return want, mag


def exact(key, n, policy, obs=None):
    """want, mag (P*P + P + 1 each) and n_valid of the n tiled points at the
    evaluation camera against observations(key, n) (or `obs`, (n, 2))."""
    if obs is None:
        return _exact_cached(key, n, policy)
    Jb, uvb, validb = base_terms(key)
    idx = np.arange(n) % N_BASE
    valid = validb[idx]
    r = (uvb[idx] - obs)[valid]
    n_valid = int(valid.sum())
    want, mag = terms_exact(Jb[idx][valid], r, (n - n_valid) if policy == 1 else 0)
    want.setflags(write=False)
    mag.setflags(write=False)
    return want, mag, n_valid


@functools.lru_cache(maxsize=None)
def _exact_cached(key, n, policy):
    return exact(key, n, policy, observations(key, n))


def oracle_terms_exact(model, params, w, h, xyz, obs, policy):
    """want, mag, n_valid from fsum of the oracle's own per-point terms
    (oracle.residual_jacobian's r and J, whose J the CPU suite pins to 50
    digits): for points that are not the base set.  Invalid points have
    J = 0 and r = 0 or the sentinel, so they fall out of the terms by
    themselves."""
    r, J, st = oracle.residual_jacobian(model, params, w, h, xyz, obs, policy)
    assert np.isfinite(r).all() and np.isfinite(J).all()
    want, mag = terms_exact(np.ascontiguousarray(J.transpose(1, 2, 0)), r)
    return want, mag, int((st == 0).sum())


def pack(JtJ, Jtr, cost, n_valid):
    """[JtJ (P*P) | Jtr (P) | cost | n_valid], acm_normal_equations' result."""
    return np.concatenate([np.asarray(JtJ, dtype=np.float64).ravel(),
                           np.asarray(Jtr, dtype=np.float64).ravel(),
                           [float(cost), float(n_valid)]])


def oracle_result(key, n, policy):
    """oracle.normal_equations on the same inputs, packed like the kernel's."""
    model, _, (w, h) = camera_of(key)
    return pack(*oracle.normal_equations(model, eval_params(key), w, h, points(key, n),
                                         observations(key, n), policy))


def num_params(want):
    P = int(round(math.sqrt(len(want) + 0.25) - 0.5))
    assert P * P + P + 1 == len(want)
    return P


def ratios(got, want, mag):
    """|got - want| / max(1e-10 |want|, 1e-13 mag) per slot (0 where exact)."""
    err = np.abs(np.asarray(got)[:len(want)] - want)
    bound = np.maximum(REL * np.abs(want), ABS * mag)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / bound)


def check(got, want, mag, n_valid):
    """Hold a result [JtJ | Jtr | cost | n_valid] to the exact sums; returns
    the worst |err| / bound."""
    got = np.asarray(got, dtype=np.float64)
    P = num_params(want)
    assert got.shape == (P * P + P + 2,)
    A = got[:P * P].reshape(P, P)
    for a, b in STRUCTURAL_ZEROS:
        assert A[a, b] == 0.0 and A[b, a] == 0.0, ("structural zero", a, b, A[a, b], A[b, a])
    assert A[2, 2] == n_valid and A[3, 3] == n_valid and got[-1] == n_valid, \
        ("n_valid", A[2, 2], A[3, 3], got[-1], n_valid)
    assert A.tobytes() == np.ascontiguousarray(A.T).tobytes(), "JtJ not symmetric bit for bit"
    ratio = ratios(got, want, mag)
    worst = int(np.argmax(ratio))
    assert not (ratio > 1.0).any() and not np.isnan(ratio).any(), \
        ("slot", worst, "got", got[worst], "exact", want[worst], "sum |terms|", mag[worst],
         "|err| / bound", float(ratio[worst]))
    return float(ratio.max())


def passes_largest_entry_rule(got, ref, P, tol=1e-10):
    """The older assertion of the parity tests: each block within 1e-10 of
    its largest entry, against another f64 result `ref`."""
    A, A0 = got[:P * P], ref[:P * P]
    b, b0 = got[P * P:P * P + P], ref[P * P:P * P + P]
    c, c0 = got[P * P + P], ref[P * P + P]
    return bool(np.abs(A - A0).max() <= tol * np.abs(A0).max()
                and np.abs(b - b0).max() <= tol * max(np.abs(b0).max(), 1.0)
                and abs(c - c0) <= tol * max(abs(c0), 1.0) and got[-1] == ref[-1])
