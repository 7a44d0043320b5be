"""The reference acm_project_f32 is held to (not a test).

The f32 kernel evaluates the model code of camera_models.hpp in float.  A
comparison with the f64 oracle at the f64 inputs mixes two things: the
rounding of the inputs to f32 (which the caller did, not the kernel) and the
kernel's own arithmetic.  Here the inputs are rounded first -- the camera
parameters and the points become f32 values, held as float64 -- and every
reference is evaluated at exactly those values, so what is left is the
kernel's arithmetic error: a few units of 2^-24 times a first-order
condition scale.

Per camera key (a model id or a camera_zoo name; camera_zoo.camera_of) and
point set, reference(key) gives:

  uv     the exact pixel: mp_models.project at 50 digits
  J0     the f64 oracle's Jacobian at the rounded values (pinned to 1e-10 of
         50 digits by tests/test_oracle.py and test_camera_zoo_ref.py: 1e3
         below what f32 resolves)
  S      the value scale, per row a of (u, v):
           S_a = |c_a| + sum_k |da/dx_k| |x_k| + sum_q |J0_aq| |theta_q|
         c_a = cx or cy, k over x, y, z (point_jacobian_ref.mp_point_jacobian),
         q over the parameters other than cx, cy: the first-order effect of
         one relative rounding in every input and parameter.  A scale only.
  st_exact, st24
         boundary_probes.emulate_status at 170 bits and at 24 bits, both
         against the thresholds the kernel uses (the f64 constants cast to
         float): the exact decision and the binary32 one, on status_rows:
         finite rows whose non-zero |coordinates| lie in [2^-60, 2^60] and
         whose RadTan r^6 stays finite in f32 (radtan_overflows).
  rows   the rows a value comparison uses: finite input, exact status Ok,
         every non-zero |coordinate| in [2^-30, 2^30] (no square over- or
         underflows in f32), and 2^-24 S <= 1 px.  A GPU test also requires
         the kernel's status to be Ok.

The Jacobian scale of entry (q, i, a) is max(|J0_aq(i)|, m_q), m_q the median
over the compared rows of max(|J0_uq|, |J0_vq|): an error in the k4 column is
measured against the k4 column, not against du/dcx = 1 as
test_gpu_parity.jac_err's per-point-largest-entry scale does.

The bounds, measured on the references alone and frozen (measure_uv24,
measure_oracle_jac; tests/test_f32_ref.py pins both at all 26 cameras):

  K_UV = 8 x 1.38: the worst |uv24 - uv*| / (2^-24 S) of mp_models.project
         under mp.workprec(24) against 50 digits over the compared rows of
         all 26 cameras is 1.371 (per camera 0.75 .. 1.371).
  K_J  = 8 x the worst |J_oracle - J_mp| / (2^-53 scale) of the f64 oracle's
         Jacobian against mp_models.jacobian (50-digit mp.diff, the
         difference taken at 50 digits) over every compared row, per camera
         (measure_oracle_jac(key); _J_BASE below, pinned from both sides).  It
         assumes the same formulas lose about as many units of 2^-24 in f32
         as they lose units of 2^-53 in f64.  The scale knows nothing of a
         row's conditioning, so the figure depends on the camera: 0.93 ..
         0.97 for Pinhole, 3 .. 12 for most, but 108.9 at ds_alpha_half,
         140.1 at eucm_alpha_lt_half (rows with z < 0 where alpha d2 + (1 -
         alpha) gamma cancels) and 111.1 at fov_narrow (w = 0.2: the dw column
         is the difference of two terms 1 / w times larger than itself).  One
         constant for all would be 8 x 140.1 = 1121 units, 6.7e-5 of the
         scale, and a relative error of 1e-5 (168 units) in any column of any
         camera would pass; so each camera is held to its own figure, never
         wider than that.  K_J_MODEL is the worst of a model's cameras, for
         point sets other than the measured one (the golden rows of
         test_gpu_parity.test_f32_path_tracks_f64).
         A first measurement on 32 evenly spaced rows per camera missed the
         worst rows (UCM 3.7 against 21.2 over all rows) and the kernel
         exceeded the bound made from it; a numpy float32 restatement of the
         formulas gave the kernel's value bit for bit at those entries, so
         the bound was at fault and was measured again on every row.

The factor 8 (three bits) pays for the device's f32 atan2 and sincos (a few
ulp, not correctly rounded), for an operation order that differs from the
restatement's, and for the Jacobian reusing rounded intermediates.  No
constant is taken from the kernel: a kernel over its bound is a finding to
explain, not a constant to raise.
"""
import collections
import functools

import mpmath as mp
import numpy as np

import boundary_probes as B
import mp_models
import oracle
import point_jacobian_ref as R
from apex_camera_models import samples
from camera_zoo import NAMES, camera_of

U24 = 2.0 ** -24
U53 = 2.0 ** -53
K_UV = 8 * 1.38
# measured per camera over every compared row, rounded up
_J_BASE = {0: 0.95, 1: 10.20, 2: 12.23, 3: 7.27, 4: 3.18, 5: 5.15, 6: 7.99,
           "pinhole_aniso": 0.93, "pinhole_short": 0.97, "radtan_k3_tangential": 30.64,
           "radtan_barrel_pos": 8.99, "kb_strong": 11.86, "kb_negative": 11.83,
           "ds_alpha_lt_half": 11.04, "ds_alpha_half": 108.87, "ds_alpha_one": 5.29,
           "ds_xi_pos": 5.95, "ucm_alpha_lt_half": 21.18, "ucm_alpha_half": 20.97,
           "ucm_alpha_mid": 3.99, "eucm_alpha_lt_half": 140.15, "eucm_alpha_half": 16.84,
           "eucm_alpha_mid": 5.75, "fov_narrow": 111.07, "fov_mid": 4.71, "fov_max": 5.60}
K_J = {key: 8 * base for key, base in _J_BASE.items()}
K_J_MODEL = {m: max(k for key, k in K_J.items() if camera_of(key)[0] == m) for m in range(7)}
KEYS = tuple(range(7)) + NAMES  # the 26 cameras
# J entries that camera_models.hpp writes as the literals 0 and 1 for every
# model: du/dfy, du/dcx, du/dcy, dv/dfx, dv/dcx, dv/dcy
STRUCTURAL = ((1, 0, 0.0), (2, 0, 1.0), (3, 0, 0.0), (0, 1, 0.0), (2, 1, 0.0), (3, 1, 1.0))

Ref = collections.namedtuple("Ref", "model params res pts uv J0 S st_exact st24 status_rows rows")


def round32(a):
    """The f32 values nearest to a, as float64 (inf where |a| overflows f32)."""
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def params32(key):
    """The camera's parameters rounded to f32, as a list of Python floats."""
    return round32(camera_of(key)[1]).tolist()


def points32(pts):
    """(n, 3) points rounded to f32, as float64."""
    return round32(pts).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def point_set(key):
    """(780, 3): test_gpu_camera_zoo._points(key) -- the base set, the edge
    points and the wide set -- rounded to f32 (read-only)."""
    rng = np.random.default_rng(20251205)
    wide = np.stack([rng.uniform(-3, 3, 500), rng.uniform(-3, 3, 500),
                     rng.uniform(-1.0, 2.0, 500)], 1)
    pts = points32(np.concatenate([R.base_points(key), samples.EDGE_POINTS, wide]))
    pts.setflags(write=False)
    return pts


def in_range(pts, lo=2.0 ** -30, hi=2.0 ** 30):
    """Rows whose coordinates are finite and, where not zero, lo <= |c| <= hi."""
    a = np.abs(pts)
    with np.errstate(invalid="ignore"):
        return (np.isfinite(pts) & ((a == 0) | ((a >= lo) & (a <= hi)))).all(axis=1)


def radtan_overflows(model, pts):
    """Rows whose status emulate_status cannot state: it rounds to 24 bits
    but keeps an unbounded exponent, and RadTan's r^6 = ((x / z)^2 +
    (y / z)^2)^3 passes FLT_MAX once |x / z| or |y / z| exceeds about 2^21.
    There the kernel's u, v are inf or NaN (0 inf with k3 = 0), every bounds
    comparison with NaN is false and the status is Ok with a NaN pixel -- what
    the f64 path and the reference do at |x / z| ~ 1e51.  Rows with z below
    the sqrt(EPS) test are decided before any of that and stay."""
    if model != 1:
        return np.zeros(len(pts), dtype=bool)
    with np.errstate(all="ignore"):
        z = pts[:, 2]
        return (z >= B.EPS_SQRT) & (np.abs(pts[:, :2]).max(axis=1) > z * 2.0 ** 20)


def statuses(model, p32, res, pts, rows):
    """(exact, binary32) statuses of the rows in `rows` (255 elsewhere)."""
    se = np.full(len(pts), 255, dtype=np.uint8)
    s24 = np.full(len(pts), 255, dtype=np.uint8)
    for i in np.nonzero(rows)[0]:
        se[i] = B.emulate_status(model, p32, res[0], res[1], "project", pts[i], prec=170,
                                 f32_thresholds=True)
        s24[i] = B.emulate_status(model, p32, res[0], res[1], "project", pts[i], prec=24,
                                  f32_thresholds=True)
    return se, s24


def project24(model, p32, pt):
    """mp_models.project with every operation rounded to 24 bits."""
    with mp.workprec(24):
        u, v = mp_models.project(model, p32, [float(c) for c in pt])
        return float(u), float(v)


def make_reference(key, pts, lo=2.0 ** -30):
    """Ref of the camera at the f32 points pts ((n, 3) float64 holding f32
    values); lo is the smallest non-zero |coordinate| of a compared row."""
    model, _, res = camera_of(key)
    p32 = params32(key)
    n = len(pts)
    status_rows = in_range(pts, 2.0 ** -60, 2.0 ** 60) & ~radtan_overflows(model, pts)
    se, s24 = statuses(model, p32, res, pts, status_rows)
    cand = status_rows & in_range(pts, lo) & (se == 0)
    _, _, J0 = oracle.project(model, p32, res[0], res[1], np.where(np.isfinite(pts), pts, 1.0),
                              want_jac=True)
    uv = np.full((n, 2), np.nan)
    S = np.full((n, 2), np.inf)
    theta = np.abs(np.array(p32))
    theta[2:4] = 0.0  # cx, cy enter through |c_a|
    for i in np.nonzero(cand)[0]:
        pt = [float(c) for c in pts[i]]
        u, v = mp_models.project(model, p32, pt)
        uv[i] = float(u), float(v)
        with mp.workdps(25):  # a scale: two digits would do
            Jp = R.mp_point_jacobian(model, p32, pt)
        S[i] = (np.abs(p32[2:4]) + np.abs(Jp) @ np.abs(pts[i])
                + np.abs(J0[:, i, :]).T @ theta)
    rows = cand & (U24 * S <= 1.0).all(axis=1)
    for a in (uv, J0, S, se, s24, status_rows, rows):
        a.setflags(write=False)
    return Ref(model, p32, res, pts, uv, J0, S, se, s24, status_rows, rows)


@functools.lru_cache(maxsize=None)
def reference(key):
    """Ref of the camera at point_set(key), computed once per process."""
    return make_reference(key, point_set(key))


def kb_axis_points():
    """KB's axis test r < EPS = 2^-52 shapes values, not statuses: points
    whose r steps over the f32 neighbours -32 .. +32 of 2^-52 along x, along
    y and along (0.6, 0.8) -- for the value comparison (make_reference with
    lo = 2^-60: r^2 ~ 2^-104 is a normal f32)."""
    t = B.f32_steps(B.EPS)
    z = np.zeros_like(t)
    return points32(np.concatenate([np.stack([t, z, z + 1.0], 1), np.stack([z, t, z + 2.0], 1),
                                    np.stack([0.6 * t, 0.8 * t, z + 1.0], 1)]))


# ----------------------------------------------------------------- the rules
def uv_ratio(uv, ref, rows):
    """Worst |uv - uv*| / (2^-24 S) over `rows` (must be <= K_UV), and where."""
    r = np.abs(np.asarray(uv, dtype=np.float64)[rows] - ref.uv[rows]) / (U24 * ref.S[rows])
    r = np.where(np.isnan(r), np.inf, r)
    i = int(np.argmax(r.max(axis=1)))
    return float(r.max()), int(np.nonzero(rows)[0][i])


def jac_scale(J0, rows):
    """(P, n, 2): max(|J0_aq(i)|, m_q), m_q the median over rows of
    max(|J0_uq|, |J0_vq|)."""
    m = np.median(np.abs(J0[:, rows, :]).max(axis=2), axis=1)
    return np.maximum(np.abs(J0), m[:, None, None])


def jac_ratio(J, J0, rows, unit=U24, floor=0.0):
    """Worst |J - J0| / (unit scale) over `rows` (must be <= K_J[key]), and the
    (parameter, row, u or v) it sits at.  floor: an absolute error forgiven
    first (f32 underflow, where a test says so); an entry that is exact
    counts 0 even where its scale is 0."""
    d = np.abs(np.asarray(J, dtype=np.float64)[:, rows, :] - J0[:, rows, :])
    nan = np.isnan(d)
    d = np.maximum(np.where(nan, 0.0, d) - floor, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / (unit * jac_scale(J0, rows)[:, rows, :]))
    r = np.where(nan, np.inf, r)
    q, i, a = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r.max()), (int(q), int(np.nonzero(rows)[0][i]), int(a))


def structural_exact(J, rows):
    """True when every entry camera_models.hpp writes as a literal is that
    literal on `rows`."""
    J = np.asarray(J)
    return all(np.array_equal(J[q][rows, a], np.full(int(rows.sum()), val, dtype=J.dtype))
               for q, a, val in STRUCTURAL)


# --------------------------------------------- the yardsticks' measurements
def measure_uv24(key):
    """Worst |uv24 - uv*| / (2^-24 S) over reference(key).rows."""
    ref = reference(key)
    uv = np.full((len(ref.pts), 2), np.nan)
    for i in np.nonzero(ref.rows)[0]:
        uv[i] = project24(ref.model, ref.params, ref.pts[i])
    return uv_ratio(uv, ref, ref.rows)[0]


def measure_oracle_jac(key):
    """Worst |J_oracle - J_mp| / (2^-53 scale) over every compared row of
    reference(key), and the number of rows."""
    ref = reference(key)
    scale = jac_scale(ref.J0, ref.rows)
    worst = 0.0
    for i in np.nonzero(ref.rows)[0]:
        jm = mp_models.jacobian(ref.model, ref.params, [float(c) for c in ref.pts[i]])
        for a in range(2):
            for q in range(len(ref.params)):
                # the difference at 50 digits: rounding the derivative to f64
                # first would hide up to half a unit of it
                d = float(abs(mp.mpf(float(ref.J0[q, i, a])) - jm[a][q]))
                worst = max(worst, d / (U53 * scale[q, i, a]))
    return worst, int(ref.rows.sum())
