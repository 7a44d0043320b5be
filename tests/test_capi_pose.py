"""C-ABI of the point Jacobian and the pose solver without a device: argument
checks, workspace sizes, and acm_pose_retract against a 50-digit Rodrigues
formula."""
import ctypes
import math

import mpmath as mp
import numpy as np
import pytest

from apex_camera_models import _lib, samples
from apex_camera_models.optimizer import Pose

mp.mp.dps = 50


def _cam(model=_lib.KANNALA_BRANDT):
    params, (w, h) = samples.SAMPLES[model]
    cam = _lib.AcmCamera()
    arr = (ctypes.c_double * len(params))(*params)
    assert _lib.load().acm_camera_init(ctypes.byref(cam), model, arr, len(params), w, h) == 0
    return cam


def _identity():
    p = _lib.AcmPose()
    for k in (0, 4, 8):
        p.r[k] = 1.0
    return p


def _cfg():
    cfg = _lib.LmConfig()
    _lib.load().acm_lm_default_config(ctypes.byref(cfg))
    return cfg


BAD = (_lib.ERR_INVALID_ARGUMENT, _lib.ERR_INVALID_MODEL)
# never dereferenced: every call below is rejected on its arguments
PTR = ctypes.c_void_p(4096)


def test_point_jacobian_argument_checks():
    L = _lib.load()
    cam = _cam()
    ok = (PTR, 0, PTR, PTR, PTR, None)
    assert L.acm_project_point_jacobian(None, 4, *ok) in BAD
    for k in (0, 2, 3, 4):  # points_3d, points_2d, status, jacobian_point
        a = list(ok)
        a[k] = None
        assert L.acm_project_point_jacobian(ctypes.byref(cam), 4, *a) == _lib.ERR_INVALID_ARGUMENT
    for lay in (2, 7, 0x400, _lib.EXACT_MATH | 2, _lib.REFERENCE_NEWTON):
        a = list(ok)
        a[1] = lay
        assert L.acm_project_point_jacobian(ctypes.byref(cam), 4, *a) == _lib.ERR_INVALID_ARGUMENT
    bad = _cam()
    bad.model = 7
    assert L.acm_project_point_jacobian(ctypes.byref(bad), 4, *ok) == _lib.ERR_INVALID_MODEL
    # n = 0 is valid and touches nothing
    assert L.acm_project_point_jacobian(ctypes.byref(cam), 0, None, 0, None, None, None, None) == 0
    assert L.acm_project_point_jacobian(ctypes.byref(cam), 0, None, 1 | _lib.EXACT_MATH, None,
                                        None, None, None) == 0


def test_pose_normal_equations_argument_checks():
    L = _lib.load()
    cam, pose = _cam(), _identity()
    ws = L.acm_pose_normal_equations_workspace_size(4)

    def call(cam_=cam, pose_=pose, pts=PTR, lay=0, obs=PTR, res=PTR, w=PTR, wb=ws):
        return L.acm_pose_normal_equations(ctypes.byref(cam_) if cam_ else None,
                                           ctypes.byref(pose_) if pose_ else None, 4, pts, lay,
                                           obs, res, w, wb, None)
    assert call(cam_=None) in BAD
    assert call(pose_=None) == _lib.ERR_INVALID_ARGUMENT
    for kw in ("pts", "obs", "res", "w"):
        assert call(**{kw: None}) == _lib.ERR_INVALID_ARGUMENT
    for lay in (2, _lib.EXACT_MATH, _lib.EXACT_MATH | 1, _lib.REFERENCE_NEWTON, -1):
        assert call(lay=lay) == _lib.ERR_INVALID_ARGUMENT
    bad = _cam()
    bad.model = -2
    assert call(cam_=bad) == _lib.ERR_INVALID_MODEL
    assert call(wb=ws - 1) == _lib.ERR_WORKSPACE_TOO_SMALL


def test_pose_optimize_argument_checks():
    L = _lib.load()
    cam, pose, cfg, summ = _cam(), _identity(), _cfg(), _lib.LmSummary()
    ws = L.acm_pose_optimize_workspace_size(4)
    nocb = _lib.ALLREDUCE_FN()

    def call(cam_=cam, pose_=pose, pts=PTR, lay=0, obs=PTR, cfg_=cfg, w=PTR, wb=ws):
        return L.acm_pose_optimize(ctypes.byref(cam_) if cam_ else None,
                                   ctypes.byref(pose_) if pose_ else None, 4, pts, lay, obs,
                                   ctypes.byref(cfg_) if cfg_ else None, nocb, None,
                                   ctypes.byref(summ), w, wb, None)
    assert call(cam_=None) in BAD
    assert call(pose_=None) == _lib.ERR_INVALID_ARGUMENT
    assert call(cfg_=None) == _lib.ERR_INVALID_ARGUMENT
    assert call(pts=None) == _lib.ERR_INVALID_ARGUMENT
    assert call(obs=None) == _lib.ERR_INVALID_ARGUMENT
    assert call(lay=3) == _lib.ERR_INVALID_ARGUMENT
    assert call(lay=_lib.EXACT_MATH) == _lib.ERR_INVALID_ARGUMENT
    bounded = _cfg()
    bounded.has_bounds = 1
    assert call(cfg_=bounded) == _lib.ERR_INVALID_ARGUMENT
    bad = _cam()
    bad.model = 9
    assert call(cam_=bad) == _lib.ERR_INVALID_MODEL
    assert call(w=None) == _lib.ERR_WORKSPACE_TOO_SMALL
    assert call(wb=ws - 8) == _lib.ERR_WORKSPACE_TOO_SMALL
    assert L.acm_pose_retract(None, (ctypes.c_double * 6)()) == _lib.ERR_INVALID_ARGUMENT
    assert L.acm_pose_retract(ctypes.byref(pose), None) == _lib.ERR_INVALID_ARGUMENT


def test_workspace_sizes_nonzero_and_monotone():
    L = _lib.load()
    ns = [0, 1, 255, 256, 257, 4099, 10 ** 5, 10 ** 6, 10 ** 7, 10 ** 9]
    for f in (L.acm_pose_normal_equations_workspace_size, L.acm_pose_optimize_workspace_size):
        sizes = [f(n) for n in ns]
        assert all(s > 0 for s in sizes)
        assert sizes == sorted(sizes)
    for n in ns:
        assert L.acm_pose_optimize_workspace_size(n) >= \
            L.acm_pose_normal_equations_workspace_size(n) + 44 * 8


# ---------------------------------------------------------------- retract
def _mp_exp(phi):
    """Rodrigues' formula at 50 digits."""
    p = [mp.mpf(v) for v in phi]
    th = mp.sqrt(sum(v * v for v in p))
    K = mp.matrix([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
    if th == 0:
        return mp.eye(3)
    return mp.eye(3) + (mp.sin(th) / th) * K + ((1 - mp.cos(th)) / th ** 2) * (K * K)


def _mp_retract(R, t, delta):
    E = _mp_exp(delta[3:])
    Rm = mp.matrix([[mp.mpf(v) for v in row] for row in R])
    tm = mp.matrix([mp.mpf(v) for v in t])
    Rn = E * Rm
    tn = E * tm + mp.matrix([mp.mpf(v) for v in delta[:3]])
    return Rn, tn


def _close(got, want):
    """within 4 ulp of the entry's magnitude, or 1e-16 absolute"""
    g = float(got)
    err = abs(mp.mpf(g) - want)
    return err <= max(4 * mp.mpf(math.ulp(float(want))), mp.mpf("1e-16"))


AXIS = np.array([0.48, -0.6, 0.64])  # unit: 0.2304 + 0.36 + 0.4096 = 1
START_R = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
START_T = [0.3, -0.1, 0.2]


@pytest.mark.parametrize("theta", [0.0, 1e-12, 1e-8, 1e-4, 0.3, 3.0])
def test_retract_matches_mp_rodrigues(theta):
    delta = [0.05, -0.02, 0.01] + list(theta * AXIS)
    got = Pose(START_R, START_T).retract(delta)
    Rn, tn = _mp_retract(START_R, START_T, delta)
    for i in range(3):
        for j in range(3):
            assert _close(got.rotation[i][j], Rn[i, j]), (theta, i, j, got.rotation[i][j],
                                                          mp.nstr(Rn[i, j], 25))
        assert _close(got.translation[i], tn[i]), (theta, i, got.translation[i],
                                                   mp.nstr(tn[i], 25))
    R = np.array(got.rotation)
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15


def test_retract_composes_and_stays_orthonormal():
    """100 composed steps: R R^T - I <= 1e-12 (100 x a few eps), and the
    composition follows the 50-digit product."""
    rng = np.random.default_rng(7)
    pose = Pose(START_R, START_T)
    Rm = mp.matrix(START_R)
    tm = mp.matrix(START_T)
    for _ in range(100):
        d = list(rng.uniform(-0.05, 0.05, 3)) + list(rng.uniform(-0.4, 0.4, 3))
        pose = pose.retract(d)
        Rm, tm = _mp_retract(Rm.tolist(), list(tm), d)
    R = np.array(pose.rotation)
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12
    want = np.array([[float(Rm[i, j]) for j in range(3)] for i in range(3)])
    assert np.abs(R - want).max() <= 1e-13
    assert np.abs(np.array(pose.translation) - [float(v) for v in tm]).max() <= 1e-13
