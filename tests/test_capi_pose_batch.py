"""C-ABI of acm_pose_optimize_batch without a device: argument checks (every
pointer below is rejected before it could be dereferenced), the default
config, the workspace size, the documented constants, and tracks_by_view on
CPU tensors against a numpy restatement."""
import ctypes
import os
import re

import numpy as np
import torch

from apex_camera_models import _lib, samples
from apex_camera_models.optimizer import tracks_by_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = (_lib.ERR_INVALID_ARGUMENT, _lib.ERR_INVALID_MODEL)
PTR = ctypes.c_void_p(4096)  # never dereferenced


def _cam(model=_lib.KANNALA_BRANDT):
    params, (w, h) = samples.SAMPLES[model]
    cam = _lib.AcmCamera()
    arr = (ctypes.c_double * len(params))(*params)
    assert _lib.load().acm_camera_init(ctypes.byref(cam), model, arr, len(params), w, h) == 0
    return cam


def _cfg():
    cfg = _lib.PoseBatchConfig()
    _lib.load().acm_pose_optimize_batch_default_config(ctypes.byref(cfg))
    return cfg


def _call(cam, cfg, n_views=4, n_points=5, n_obs=8, poses=PTR, pts=PTR, offs=PTR, point=PTR,
          uv=PTR, status=PTR, cost=None, n_valid=None, iters=None, info=None, w=PTR, wb=None):
    L = _lib.load()
    if wb is None:
        wb = L.acm_pose_optimize_batch_workspace_size(n_views, n_obs)
    return L.acm_pose_optimize_batch(ctypes.byref(cam) if cam else None, n_views, poses, n_points,
                                     pts, offs, n_obs, point, uv,
                                     ctypes.byref(cfg) if cfg else None, status, cost, n_valid,
                                     iters, info, w, wb, None)


def test_default_config():
    cfg = _cfg()
    assert cfg.max_iterations == 20 and cfg.flags == 0
    lm = _lib.LmConfig()
    _lib.load().acm_lm_default_config(ctypes.byref(lm))
    assert (cfg.cost_tolerance, cfg.parameter_tolerance, cfg.gradient_tolerance,
            cfg.initial_damping) == (lm.cost_tolerance, lm.parameter_tolerance,
                                     lm.gradient_tolerance, lm.initial_damping)
    assert (cfg.cost_tolerance, cfg.parameter_tolerance, cfg.gradient_tolerance,
            cfg.initial_damping) == (1e-6, 1e-8, 1e-6, 1e-4)


def test_null_buffers_are_invalid_arguments():
    cam, cfg = _cam(), _cfg()
    assert _call(None, cfg) in BAD
    assert _call(cam, None) == _lib.ERR_INVALID_ARGUMENT
    for kw in ("poses", "pts", "offs", "point", "uv", "status"):
        assert _call(cam, cfg, **{kw: None}) == _lib.ERR_INVALID_ARGUMENT, kw
    # no points / no observations: those arrays may be NULL, the rest may not
    assert _call(cam, cfg, n_points=0, pts=None, status=None) == _lib.ERR_INVALID_ARGUMENT
    assert _call(cam, cfg, n_obs=0, point=None, uv=None, poses=None) == _lib.ERR_INVALID_ARGUMENT
    assert _call(cam, cfg, n_obs=0, point=None, uv=None, offs=None) == _lib.ERR_INVALID_ARGUMENT


def test_bad_model_config_and_workspace():
    cam, cfg = _cam(), _cfg()
    bad = _cam()
    for model in (7, -1):
        bad.model = model
        assert _call(bad, cfg) == _lib.ERR_INVALID_MODEL
    neg = _cfg()
    neg.max_iterations = -1
    assert _call(cam, neg) == _lib.ERR_INVALID_ARGUMENT
    for flags in (1, 2, 3, -2, 0x100):
        f = _cfg()
        f.flags = flags
        assert _call(cam, f) == _lib.ERR_INVALID_ARGUMENT, flags
    ws = _lib.load().acm_pose_optimize_batch_workspace_size(4, 8)
    assert _call(cam, cfg, w=None) == _lib.ERR_WORKSPACE_TOO_SMALL
    assert _call(cam, cfg, wb=ws - 1) == _lib.ERR_WORKSPACE_TOO_SMALL
    assert _call(cam, cfg, wb=0) == _lib.ERR_WORKSPACE_TOO_SMALL


def test_zero_views_is_valid_and_touches_nothing():
    cam = _cam()
    assert _call(cam, _cfg(), n_views=0, n_points=0, n_obs=0, poses=None, pts=None, offs=None,
                 point=None, uv=None, status=None, w=None, wb=0) == 0
    assert _call(cam, _cfg(), n_views=0, n_points=7, n_obs=9, poses=None, pts=None, offs=None,
                 point=None, uv=None, status=None, w=None, wb=0) == 0


def test_workspace_size_positive_and_monotone():
    L = _lib.load()
    ns = [0, 1, 63, 64, 65, 4099, 10 ** 5, 10 ** 7, 10 ** 9]
    for m in ns:
        sizes = [L.acm_pose_optimize_batch_workspace_size(n, m) for n in ns]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    for n in ns:
        sizes = [L.acm_pose_optimize_batch_workspace_size(n, m) for m in ns]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes)


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "acm.h")).read()
    assert int(re.search(r"#define\s+ACM_POSE_BATCH_STAGE_OBSERVATIONS\s+(\d+)", text).group(1)) == \
        _lib.POSE_BATCH_STAGE_OBSERVATIONS == 1024
    for name, value in (("OK", _lib.POSE_OK),
                        ("TOO_FEW_OBSERVATIONS", _lib.POSE_TOO_FEW_OBSERVATIONS),
                        ("NOT_CONVERGED", _lib.POSE_NOT_CONVERGED)):
        assert int(re.search(r"ACM_POSE_%s\s*=\s*(\d+)" % name, text).group(1)) == value
    assert ctypes.sizeof(_lib.PoseBatchConfig) == 40


def _by_view_numpy(offsets, view, uv, k):
    """Observation j belongs to the point whose track holds it; per view in
    turn, the kept observations in their original order."""
    point = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    vo, pts, uvs = [0], [], []
    for v in range(k):
        for j in range(len(view)):
            if view[j] == v:
                pts.append(point[j])
                uvs.append(uv[j])
        vo.append(len(pts))
    return (np.array(vo, dtype=np.int64), np.array(pts, dtype=np.int32),
            np.array(uvs, dtype=np.float64).reshape(-1, 2))


def test_tracks_by_view_matches_numpy():
    rng = np.random.default_rng(7)
    k, n = 7, 40
    lengths = rng.integers(0, 6, n)           # empty tracks too
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(lengths)
    m = int(offsets[-1])
    # view 3 and view 6 stay empty; -1, 7 and 100 are out of range; repeated
    # views inside a track test the stability of the order
    view = rng.choice(np.array([-1, 0, 1, 2, 4, 5, 5, 7, 100]), m).astype(np.int32)
    uv = rng.normal(size=(m, 2))
    uv[3] = np.nan                              # values are carried, not inspected
    vo, pt, out = tracks_by_view(torch.as_tensor(offsets), torch.as_tensor(view),
                                 torch.as_tensor(uv), k)
    assert vo.device.type == "cpu" and vo.dtype == torch.int64 and pt.dtype == torch.int32
    assert out.dtype == torch.float64 and out.shape[1] == 2
    wvo, wpt, wuv = _by_view_numpy(offsets, view, uv, k)
    assert np.array_equal(vo.numpy(), wvo)
    assert np.array_equal(pt.numpy(), wpt)
    assert out.numpy().tobytes() == wuv.tobytes()
    assert wvo[4] == wvo[3] and wvo[7] == wvo[6]          # the empty views
    assert len(wpt) == int(((view >= 0) & (view < k)).sum()) < m
    for v in range(k):                                    # ascending point order per view
        seg = pt.numpy()[wvo[v]:wvo[v + 1]]
        assert (np.diff(seg) >= 0).all()


def test_tracks_by_view_empty_inputs():
    vo, pt, uv = tracks_by_view(torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
                                torch.zeros((0, 2), dtype=torch.float64), 3)
    assert vo.tolist() == [0, 0, 0, 0] and pt.shape == (0,) and uv.shape == (0, 2)
    vo, pt, uv = tracks_by_view(torch.tensor([0, 2]), torch.tensor([0, 1], dtype=torch.int32),
                                torch.zeros((2, 2), dtype=torch.float64), 0)
    assert vo.tolist() == [0] and pt.shape == (0,) and uv.shape == (0, 2)
