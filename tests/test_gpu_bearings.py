"""pixel_bearing on the GPU, pixel by pixel over whole images: the usable bit
and the unit ray the three RANSAC solvers (acm_pose_estimate_batch,
acm_relative_pose_batch, acm_homography_batch) give a pixel, against
tests/bearing_ref.py, which tests/test_bearing_ref.py pins to the 50-digit
forward models.

No call returns the bearing, so it is observed through the solvers:
  (a) every pixel of bearing_ref.grid (61 x 41 over the image and a 25 %
      margin) is an item of its own -- a view of one observation, a pair of
      one match whose other pixel is the principal point.  Each kernel writes
      n_usable before it decides "too few", so n_usable is the pixel's usable
      bit.  The threshold pixels of tests/boundary_probes.py (+-8 ulps around
      every status threshold of the unprojections) ride along.
  (b) pose estimation at the identity pose with world points on the
      reference's bearings: the inlier mask at 1e-6 rad must equal the
      reference's usable bits, so a device bearing that is more than 1e-6 rad
      off at one pixel fails and names the pixel.
  (c) the zero-noise tests of the two-view solvers on matches from the whole
      image instead of a narrow cone.

Grid pixels at which a quantity that decides `usable` lies within 1e-9
(relative) of its threshold are left out (bearing_ref.near_threshold; at most
1 % per camera, in fact none); the threshold pixels of (a) are compared as
they are: the kernels' status decisions are the oracle's bit for bit
(-ffp-contract=off, tests/test_gpu_parity.py).

Measured on an MI355X (CHANGELOG.md): 94 tests in 7.2 s, the slowest 0.32 s.
(a) no pixel differs in any of the 5 calls of any of the 24 cameras; (b) no
pixel differs, pose within 1.9e-14 rad / 7.7e-14 of the identity; (c) relative
pose within 4.1e-15 / 1.5e-14 rad (reference 6.4e-15 / 1.5e-14), homography
|H - H_true| 8.9e-15, matched solution 4.5e-14 (reference 7.8e-15 / 4.1e-14).
With the kernels as they were before FOV's and KB's bearing became the
projection's inverse: (a) differs at 2148 pixels of fov_max and 2 of
kb_strong, (b) at 174 / 499 / 32 pixels of the short view of fov / fov_mid /
kannala_brandt and at kb_strong.  A build with 2 k3 for 3 k3 in RadTan's
polish and 1 - r^2 in UCM's inverse at alpha <= 0.5 fails (c) at
radtan_k3_tangential and (b), (c) at ucm_alpha_lt_half and ucm_alpha_half,
and passes the three RANSAC suites as they were before this file.
"""
import functools
import math

import numpy as np
import pytest

import bearing_ref as BR
import boundary_probes
import camera_zoo as Z
import homography_ref as G
import oracle
import relative_pose_ref as Q
import test_gpu_homography as H
import test_gpu_pose_batch as B
import test_gpu_pose_estimate as PE
import test_gpu_relative_pose as RP
from apex_camera_models import samples
from apex_camera_models.optimizer import Pose

pytestmark = pytest.mark.gpu

CAMERAS = tuple(sorted(samples.SAMPLES)) + Z.SOLVER_SUBSET + (
    "radtan_barrel_pos", "kb_strong", "ds_alpha_half", "ds_alpha_one", "ucm_alpha_half",
    "ucm_alpha_mid", "eucm_alpha_mid", "fov_narrow")
ANGLE = 1e-6          # the zero-noise tests' inlier angle
STAGE = 1024          # records of up to 1024 observations live in LDS
MIN_KEPT = 0.6        # (c): share of the matches whose pixel in B is usable


@functools.lru_cache(maxsize=None)
def grid_pixels(key):
    """(uv, inside) of bearing_ref.grid without the pixels near a threshold."""
    uv, inside = BR.grid(key)
    near = BR.near_threshold(key, uv)
    assert near.sum() <= 0.01 * len(uv), (key, int(near.sum()))
    uv, inside = uv[~near], inside[~near]
    uv.setflags(write=False)
    inside.setflags(write=False)
    return uv, inside


@functools.lru_cache(maxsize=None)
def threshold_pixels(key):
    """The unprojection probes of tests/boundary_probes.py written for this
    camera's model and parameters, (n, 2); empty for most cameras."""
    mid, params, _ = Z.camera_of(key)
    rows = [pts for model, p, _, kind, pts in boundary_probes.probes()
            if kind == "unproject" and model == mid and list(p) == list(params)]
    out = np.concatenate(rows) if rows else np.empty((0, 2))
    out.setflags(write=False)
    return out


def test_threshold_pixels_reach_the_cameras():
    have = {Z.label(k): len(threshold_pixels(k)) for k in CAMERAS if len(threshold_pixels(k))}
    print(f"threshold pixels per camera: {have}")
    assert set(have) >= {"kannala_brandt", "double_sphere", "ucm", "eucm", "ucm_alpha_lt_half",
                         "ucm_alpha_half"}


# ------------------------------------------------------- (a) the usable bit
def _check_too_few(what, key, got, want, uv, too_few):
    bits = got["n_usable"]
    wrong = np.nonzero(bits != want.astype(bits.dtype))[0]
    assert len(wrong) == 0, (what, Z.label(key), len(wrong), uv[wrong[:5]].tolist(),
                             bits[wrong[:5]].tolist())
    assert (got["status"] == too_few).all(), what
    assert np.isnan(got["poses"]).all() and (got["n_inliers"] == 0).all(), what
    assert (got["mask"] == 0).all(), what


@pytest.mark.parametrize("key", CAMERAS + ("fov_max",), ids=Z.label)
def test_usable_bit_of_every_pixel(key):
    mid, params, _ = Z.camera_of(key)
    uv = np.concatenate([grid_pixels(key)[0], threshold_pixels(key)])
    m = len(uv)
    offsets = np.arange(m + 1, dtype=np.int64)
    centre = np.tile(np.array(params[2:4]), (m, 1))
    assert BR.bearings(key, centre[:1], True)[1][0], "the principal point should be usable"
    # pose estimation: no polish, a finite world point per observation
    _, want = BR.bearings(key, uv, False)
    world = np.tile(np.array([0.1, -0.2, 2.0]), (m, 1))
    got = PE._run(key, world, offsets, np.arange(m, dtype=np.int32), uv, inlier_angle=ANGLE)
    _check_too_few("pose estimate", key, got, want, uv, PE.TOO_FEW)
    # the two-view solvers: the pixel in image A, then in image B
    _, want = BR.bearings(key, uv, True)
    for side, (a, b) in (("A", (uv, centre)), ("B", (centre, uv))):
        got = RP.run(key, offsets, a, b, inlier_angle=ANGLE)
        _check_too_few(f"relative pose, image {side}", key, got, want, uv, RP.TOO_FEW)
        got = H.run(key, offsets, a, b, inlier_angle=ANGLE)
        assert np.isnan(got["homography"]).all() and (got["n_solutions"] == 0).all()
        _check_too_few(f"homography, image {side}", key, got, want, uv, H.TOO_FEW)
    print(f"usable bit {Z.label(key)}: {int(want.sum())} usable of {m} pixels "
          f"({len(threshold_pixels(key))} on thresholds), equal in 5 calls")


# --------------------------------- (b) the bearing, through pose estimation
@pytest.mark.parametrize("key", CAMERAS, ids=Z.label)
def test_bearing_of_every_pixel(key):
    """Two views at the identity pose, world points d f_ref(uv) with d in 1 ..
    5 (for an unusable pixel a finite point): 1024 pixels of the grid, drawn
    at random (records in LDS), and all of them (records in the workspace)."""
    uv_all, _ = grid_pixels(key)
    rng = np.random.default_rng(20261101 + Z.camera_of(key)[0])
    pick = np.sort(rng.permutation(len(uv_all))[:STAGE])
    uv = np.concatenate([uv_all[pick], uv_all])
    assert len(uv_all) > STAGE
    offsets = np.array([0, STAGE, len(uv)], dtype=np.int64)
    f, usable = BR.bearings(key, uv, False)
    depth = rng.uniform(1.0, 5.0, len(uv))
    world = np.where(usable[:, None], f, [0.0, 0.0, 1.0]) * depth[:, None]
    got = PE._run(key, world, offsets, np.arange(len(uv), dtype=np.int32), uv, inlier_angle=ANGLE)
    for k in range(2):
        sl = slice(offsets[k], offsets[k + 1])
        nu = int(usable[sl].sum())
        ang, dt, orth = (B._pose_errors(got["poses"][k], Pose())
                         if np.isfinite(got["poses"][k]).all() else (math.nan,) * 3)
        wrong = np.nonzero((got["mask"][sl] != 0) != usable[sl])[0]
        print(f"bearings {Z.label(key)}, view of {offsets[k + 1] - offsets[k]}: status "
              f"{got['status'][k]}, {got['n_inliers'][k]} inliers of {got['n_usable'][k]} usable "
              f"(reference {nu}), rotation {ang:.3e} rad, translation {dt:.3e}, "
              f"{len(wrong)} pixels differ")
    for k in range(2):
        sl = slice(offsets[k], offsets[k + 1])
        nu = int(usable[sl].sum())
        assert nu >= 100
        assert got["n_usable"][k] == nu, (k, got["n_usable"][k], nu)
        assert got["status"][k] == PE.OK, (k, got["status"][k])
        ang, dt, orth = B._pose_errors(got["poses"][k], Pose())
        assert ang <= 1e-6 and dt <= 1e-6 and orth <= 1e-12, (k, ang, dt, orth)
        wrong = np.nonzero((got["mask"][sl] != 0) != usable[sl])[0]
        assert len(wrong) == 0, (Z.label(key), k, len(wrong), uv[sl][wrong[:5]].tolist(),
                                 f[sl][wrong[:5]].tolist())
        assert got["n_inliers"][k] == nu


# --------------------------- (c) whole-image zero noise, two-view solvers
def _image_pixels(key, dense):
    """The usable grid pixels inside the image; dense: with the same grid
    moved by half a step, for a pair of more than 1024 matches."""
    uv, inside = grid_pixels(key)
    uv = uv[inside]
    if dense:
        _, _, (w, h) = Z.camera_of(key)
        step = np.array([(1.0 + 2.0 * BR.MARGIN) * w / (BR.GRID[0] - 1),
                         (1.0 + 2.0 * BR.MARGIN) * h / (BR.GRID[1] - 1)])
        more = uv + 0.5 * step
        more = more[(more[:, 0] < w) & (more[:, 1] < h) & ~BR.near_threshold(key, more)]
        uv = np.concatenate([uv, more])
    else:
        uv = uv[::2]
    return uv[BR.bearings(key, uv, True)[1]]


def _second_view(key, k, uv_a, X):
    """uv_b: the oracle's projection of X through true_pose(key, k); the
    matches whose pixel in B does not exist or is not usable are dropped, and
    those whose pixel in B is the image of a second ray as well, which the
    bearing returns instead (more than 1e-9 rad from the point's direction):
    beyond the fold of radtan_k3_tangential's and kb_strong's distortion the
    projection has no inverse."""
    mid, params, (w, h) = Z.camera_of(key)
    Rm, t = RP.true_pose(key, k)
    p_b = X @ Rm.T + t
    uv_b, st, _ = oracle.project(mid, params, w, h, np.ascontiguousarray(p_b))
    f_b, keep = BR.bearings(key, np.where((st == 0)[:, None], uv_b, 0.0), True)
    keep &= st == 0
    keep &= ~BR.near_threshold(key, np.where(keep[:, None], uv_b, 0.0))
    with np.errstate(invalid="ignore"):
        keep &= np.linalg.norm(np.cross(f_b, p_b / np.linalg.norm(p_b, axis=1)[:, None]),
                               axis=1) <= 1e-9
    assert keep.sum() >= MIN_KEPT * len(uv_a), (Z.label(key), k, int(keep.sum()), len(uv_a))
    return uv_a[keep], uv_b[keep]


@functools.lru_cache(maxsize=None)
def whole_image_scene(key, planar):
    """(offsets, uv_a, uv_b): pair 0 has fewer than 1024 matches, pair 1 more.
    X = d f_ref(uv_a), d in 2.5 .. 6 -- or, planar, on the plane of
    test_gpu_homography by homography_ref.planar_scene's rule: pixels whose
    bearing meets the plane at less than n . f = 0.2 are left out."""
    rng = np.random.default_rng(20261102 + Z.camera_of(key)[0])
    parts = []
    for k, dense in enumerate((False, True)):
        uv_a = _image_pixels(key, dense)
        f, _ = BR.bearings(key, uv_a, True)
        if planar:
            cos = f @ H.PLANE_N
            uv_a, f, cos = uv_a[cos >= 0.2], f[cos >= 0.2], cos[cos >= 0.2]
            X = f * (H.PLANE_D / cos)[:, None]
        else:
            X = f * rng.uniform(2.5, 6.0, len(f))[:, None]
        parts.append(_second_view(key, k, uv_a, X))
    counts = [len(a) for a, _ in parts]
    assert 8 <= counts[0] < STAGE < counts[1], (Z.label(key), counts)
    offsets = np.array([0, counts[0], counts[0] + counts[1]], dtype=np.int64)
    uv_a, uv_b = np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts])
    for arr in (offsets, uv_a, uv_b):
        arr.setflags(write=False)
    return offsets, uv_a, uv_b


@pytest.mark.parametrize("key", CAMERAS, ids=Z.label)
def test_relative_pose_whole_image(key):
    """test_gpu_relative_pose.test_zero_noise_every_model's assertions and
    bounds on matches from the whole image."""
    offsets, uv_a, uv_b = whole_image_scene(key, False)
    got = RP.run(key, offsets, uv_a, uv_b, inlier_angle=ANGLE)
    fa, fb, usable = RP.records(key, uv_a, uv_b)
    assert usable.all()
    figures = []
    for k in range(2):
        sl = slice(offsets[k], offsets[k + 1])
        ref = Q.solve(fa[sl], fb[sl])
        R0, t0 = RP.true_pose(key, k)
        ref_rot, ref_dir = Q.angles(ref["R"], ref["t"], R0, t0)
        rot, dirn = (RP.pose_angles(got["poses"][k], key, k) if np.isfinite(got["poses"][k]).all()
                     else (math.nan, math.nan))
        figures.append((rot, dirn, ref_rot, ref_dir))
        print(f"relative pose {Z.label(key)} whole image, pair of {offsets[k + 1] - offsets[k]}: "
              f"status {got['status'][k]}, {got['n_inliers'][k]} inliers of {got['n_usable'][k]} "
              f"usable, rotation error {rot:.3e} rad (reference {ref_rot:.3e}), translation "
              f"direction {dirn:.3e} rad (reference {ref_dir:.3e})")
    for k in range(2):
        sl = slice(offsets[k], offsets[k + 1])
        nu = int(offsets[k + 1] - offsets[k])
        assert got["n_usable"][k] == nu, (k, got["n_usable"][k], nu)
        assert got["status"][k] == RP.OK, (k, got["status"][k], got["n_inliers"][k], nu)
        assert got["n_inliers"][k] == nu, (k, got["n_inliers"][k], nu)
        assert (got["mask"][sl] == 1).all()
        row = got["poses"][k]
        Rm = row[:9].reshape(3, 3)
        assert np.abs(Rm.T @ Rm - np.eye(3)).max() <= 1e-12 and np.linalg.det(Rm) > 0
        assert abs(np.linalg.norm(row[9:]) - 1.0) <= 1e-12
        rot, dirn, ref_rot, ref_dir = figures[k]
        assert rot <= max(1e-9, 10.0 * ref_rot), (k, rot, ref_rot)
        assert dirn <= max(1e-9, 10.0 * ref_dir), (k, dirn, ref_dir)


@pytest.mark.parametrize("key", CAMERAS, ids=Z.label)
def test_homography_whole_image(key):
    """test_gpu_homography.test_zero_noise_every_model's assertions and bounds
    on matches from the whole image."""
    offsets, uv_a, uv_b = whole_image_scene(key, True)
    got = H.run(key, offsets, uv_a, uv_b, inlier_angle=ANGLE)
    fa, fb, usable = RP.records(key, uv_a, uv_b)
    assert usable.all()
    figures = []
    for k in range(2):
        sl = slice(offsets[k], offsets[k + 1])
        R0, t0 = RP.true_pose(key, k)
        H0 = G.true_h(R0, t0, H.PLANE_N, H.PLANE_D)
        ref = G.solve(fa[sl], fb[sl])
        ref_h = np.abs(ref["H"] - H0).max()
        ref_e = G.solution_error(ref, R0, t0, H.PLANE_N, H.PLANE_D)
        sol = H.solution(got, k)
        ok = got["status"][k] == H.OK and sol["count"] == 2
        h = np.abs(sol["H"] - H0).max() if ok else math.nan
        e = G.solution_error(sol, R0, t0, H.PLANE_N, H.PLANE_D) if ok else math.nan
        figures.append((h, e, ref_h, ref_e))
        print(f"homography {Z.label(key)} whole image, pair of {offsets[k + 1] - offsets[k]}: "
              f"status {got['status'][k]}, {got['n_inliers'][k]} inliers of {got['n_usable'][k]} "
              f"usable, |H - H_true| {h:.3e} (reference {ref_h:.3e}), matched solution {e:.3e} "
              f"(reference {ref_e:.3e}), n_front {sol['n_front'].tolist()}")
    for k in range(2):
        sl = slice(offsets[k], offsets[k + 1])
        nu = int(offsets[k + 1] - offsets[k])
        assert got["n_usable"][k] == nu, (k, got["n_usable"][k], nu)
        assert got["status"][k] == H.OK, (k, got["status"][k], got["n_inliers"][k], nu)
        assert got["n_inliers"][k] == nu, (k, got["n_inliers"][k], nu)
        assert (got["mask"][sl] == 1).all()
        sol = H.solution(got, k)
        assert sol["count"] == 2 and sol["n_front"][0] == nu
        G.check_solutions([sol], fa[sl][None], fb[sl][None],
                          *[np.asarray(x)[None] for x in (*RP.true_pose(key, k), H.PLANE_N,
                                                           H.PLANE_D)])
        h, e, ref_h, ref_e = figures[k]
        assert h <= max(1e-9, 10.0 * ref_h), (k, h, ref_h)
        assert e <= max(1e-9, 10.0 * ref_e), (k, e, ref_e)
