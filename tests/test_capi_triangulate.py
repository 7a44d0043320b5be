"""C-ABI of acm_triangulate without a device: argument checks (every pointer
below is rejected before it could be dereferenced), the default config, the
workspace size, and the documented staging constant."""
import ctypes
import os
import re

from apex_camera_models import _lib, samples

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
    cfg = _lib.TriangulateConfig()
    _lib.load().acm_triangulate_default_config(ctypes.byref(cfg))
    return cfg


def _call(cam, cfg, n_points=4, n_obs=8, poses=PTR, offs=PTR, view=PTR, uv=PTR, pts=PTR,
          status=PTR, cost=None, n_valid=None, info=None, w=PTR, wb=None):
    L = _lib.load()
    if wb is None:
        wb = L.acm_triangulate_workspace_size(n_points, n_obs)
    return L.acm_triangulate(ctypes.byref(cam) if cam else None, 6, poses, n_points, offs, n_obs,
                             view, uv, ctypes.byref(cfg) if cfg else None, pts, status, cost,
                             n_valid, info, w, wb, None)


def test_default_config():
    cfg = _cfg()
    assert cfg.max_iterations == 20 and cfg.flags == 0
    assert cfg.cost_tolerance == 1e-6
    assert cfg.parameter_tolerance == 1e-8
    assert cfg.gradient_tolerance == 1e-6
    assert cfg.initial_damping == 1e-4
    assert cfg.min_parallax_sin2 == 1e-8
    lm = _lib.LmConfig()
    _lib.load().acm_lm_default_config(ctypes.byref(lm))
    assert (cfg.cost_tolerance, cfg.parameter_tolerance, cfg.gradient_tolerance,
            cfg.initial_damping) == (lm.cost_tolerance, lm.parameter_tolerance,
                                     lm.gradient_tolerance, lm.initial_damping)


def test_null_buffers_are_invalid_arguments():
    cam, cfg = _cam(), _cfg()
    assert _call(None, cfg) in BAD
    assert _call(cam, None) == _lib.ERR_INVALID_ARGUMENT
    for kw in ("poses", "offs", "view", "uv", "pts", "status"):
        assert _call(cam, cfg, **{kw: None}) == _lib.ERR_INVALID_ARGUMENT, kw
    # no observations at all: the observation arrays may be NULL, the rest may not
    assert _call(cam, cfg, n_obs=0, view=None, uv=None, pts=None) == _lib.ERR_INVALID_ARGUMENT


def test_bad_model_config_and_workspace():
    cam, cfg = _cam(), _cfg()
    bad = _cam()
    for model in (7, -1):
        bad.model = model
        assert _call(bad, cfg) == _lib.ERR_INVALID_MODEL
    neg = _cfg()
    neg.max_iterations = -1
    assert _call(cam, neg) == _lib.ERR_INVALID_ARGUMENT
    for flags in (2, 4, 3, -2, 0x100):
        f = _cfg()
        f.flags = flags
        assert _call(cam, f) == _lib.ERR_INVALID_ARGUMENT, flags
    ws = _lib.load().acm_triangulate_workspace_size(4, 8)
    assert _call(cam, cfg, w=None) == _lib.ERR_WORKSPACE_TOO_SMALL
    assert _call(cam, cfg, wb=ws - 1) == _lib.ERR_WORKSPACE_TOO_SMALL
    assert _call(cam, cfg, wb=0) == _lib.ERR_WORKSPACE_TOO_SMALL


def test_zero_points_is_valid_and_touches_nothing():
    cam = _cam()
    assert _call(cam, _cfg(), n_points=0, n_obs=0, poses=None, offs=None, view=None, uv=None,
                 pts=None, status=None, w=None, wb=0) == 0
    initial = _cfg()
    initial.flags = _lib.TRI_USE_INITIAL
    initial.max_iterations = 0
    assert _call(cam, initial, n_points=0, n_obs=0, poses=None, offs=None, view=None, uv=None,
                 pts=None, status=None, w=None, wb=0) == 0


def test_workspace_size_positive_and_monotone():
    L = _lib.load()
    ns = [0, 1, 63, 64, 65, 4099, 10 ** 5, 10 ** 7, 10 ** 9]
    for m in ns:
        sizes = [L.acm_triangulate_workspace_size(n, m) for n in ns]
        assert all(s > 0 for s in sizes)
        assert sizes == sorted(sizes)
    for n in ns:
        sizes = [L.acm_triangulate_workspace_size(n, m) for m in ns]
        assert all(s > 0 for s in sizes)
        assert sizes == sorted(sizes)


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "acm.h")).read()
    assert int(re.search(r"#define\s+ACM_TRI_STAGE_OBSERVATIONS\s+(\d+)", text).group(1)) == \
        _lib.TRI_STAGE_OBSERVATIONS
    for name, value in (("OK", _lib.TRI_OK), ("TOO_FEW_OBSERVATIONS", _lib.TRI_TOO_FEW_OBSERVATIONS),
                        ("DEGENERATE", _lib.TRI_DEGENERATE), ("NOT_CONVERGED", _lib.TRI_NOT_CONVERGED),
                        ("USE_INITIAL", _lib.TRI_USE_INITIAL)):
        assert int(re.search(r"ACM_TRI_%s\s*=\s*(\d+)" % name, text).group(1)) == value
    assert ctypes.sizeof(_lib.TriangulateConfig) == 48
