"""C-ABI of acm_calibrate without a device: argument checks (every pointer
below is rejected before it could be dereferenced), the default config, the
workspace size and the struct layouts."""
import ctypes
import math

from apex_camera_models import _lib, samples

BAD = (_lib.ERR_INVALID_ARGUMENT, _lib.ERR_INVALID_MODEL)
PTR = ctypes.c_void_p(4096)  # never dereferenced


def _cam(model=_lib.KANNALA_BRANDT):
    params, (w, h) = samples.SAMPLES[model]
    cam = _lib.AcmCamera()
    arr = (ctypes.c_double * len(params))(*params)
    assert _lib.load().acm_camera_init(ctypes.byref(cam), model, arr, len(params), w, h) == 0
    return cam


def _cfg():
    cfg = _lib.CalibrateConfig()
    _lib.load().acm_calibrate_default_config(ctypes.byref(cfg))
    return cfg


def _call(cam, cfg, n_views=4, n_points=5, n_obs=8, poses=PTR, pts=PTR, offs=PTR, point=PTR,
          uv=PTR, summary=None, status=PTR, cost=None, n_valid=None, system=None, w=PTR, wb=None):
    L = _lib.load()
    if wb is None:
        wb = L.acm_calibrate_workspace_size(_lib.KANNALA_BRANDT, n_views, n_obs)
    return L.acm_calibrate(ctypes.byref(cam) if cam else None, n_views, poses, n_points, pts, offs,
                           n_obs, point, uv, ctypes.byref(cfg) if cfg else None, summary, status,
                           cost, n_valid, system, w, wb, None)


def test_default_config():
    cfg = _cfg()
    assert cfg.max_iterations == 50 and cfg.flags == 0
    assert cfg.fixed_mask == 0 and cfg.has_bounds == 0
    lm = _lib.LmConfig()
    _lib.load().acm_lm_default_config(ctypes.byref(lm))
    assert (cfg.cost_tolerance, cfg.parameter_tolerance, cfg.gradient_tolerance,
            cfg.initial_damping) == (lm.cost_tolerance, lm.parameter_tolerance,
                                     lm.gradient_tolerance, lm.initial_damping)
    assert (cfg.cost_tolerance, cfg.parameter_tolerance, cfg.gradient_tolerance,
            cfg.initial_damping) == (1e-6, 1e-8, 1e-6, 1e-4)
    assert all(v == -math.inf for v in cfg.lower) and all(v == math.inf for v in cfg.upper)
    _lib.load().acm_calibrate_default_config(None)  # a NULL config is ignored


def test_struct_layouts():
    assert ctypes.sizeof(_lib.CalibrateConfig) == 8 + 4 * 8 + 8 + 2 * 9 * 8
    assert ctypes.sizeof(_lib.CalibrateSummary) == 16 + 3 * 8 + 81 * 8
    assert _lib.CalibrateConfig.fixed_mask.offset == 40
    assert _lib.CalibrateConfig.lower.offset == 48
    assert _lib.CalibrateSummary.information.offset == 40


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


def test_bad_model_flags_and_iterations():
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


def test_bad_mask_and_inverted_bounds():
    for model in sorted(samples.SAMPLES):
        cam = _cam(model)
        p = cam.num_params
        ok = _cfg()
        ok.fixed_mask = (1 << p) - 1          # every parameter fixed is a valid mask:
        assert _call(cam, ok, w=None) == _lib.ERR_WORKSPACE_TOO_SMALL  # the next check is reached
        for mask in (1 << p, 1 << 31, (1 << p) | 1):
            c = _cfg()
            c.fixed_mask = mask
            assert _call(cam, c) == _lib.ERR_INVALID_ARGUMENT, (model, mask)
    cam = _cam()
    c = _cfg()
    c.has_bounds = 1
    c.lower[4], c.upper[4] = 0.5, 0.4
    assert _call(cam, c) == _lib.ERR_INVALID_ARGUMENT
    c.lower[4], c.upper[4] = 0.4, 0.4           # an empty interior is allowed
    assert _call(cam, c, w=None) == _lib.ERR_WORKSPACE_TOO_SMALL
    c.upper[4] = math.nan
    assert _call(cam, c) == _lib.ERR_INVALID_ARGUMENT
    c.has_bounds = 0                            # bounds are ignored without has_bounds
    assert _call(cam, c, w=None) == _lib.ERR_WORKSPACE_TOO_SMALL
    c = _cfg()
    c.has_bounds = 1
    c.lower[8], c.upper[8] = 1.0, 0.0           # beyond KB's 8 parameters: not looked at
    assert _call(cam, c, w=None) == _lib.ERR_WORKSPACE_TOO_SMALL


def test_short_workspace():
    cam, cfg = _cam(), _cfg()
    ws = _lib.load().acm_calibrate_workspace_size(_lib.KANNALA_BRANDT, 4, 8)
    assert _call(cam, cfg, w=None) == _lib.ERR_WORKSPACE_TOO_SMALL
    assert _call(cam, cfg, wb=ws - 1) == _lib.ERR_WORKSPACE_TOO_SMALL
    assert _call(cam, cfg, wb=0) == _lib.ERR_WORKSPACE_TOO_SMALL


def test_workspace_size():
    L = _lib.load()
    ns = [0, 1, 63, 64, 65, 4099, 10 ** 5, 10 ** 7]
    for model in sorted(samples.SAMPLES):
        sizes = [L.acm_calibrate_workspace_size(model, n, 1000) for n in ns]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
        # two pose slots, two system slots and the Schur blocks per view at least
        assert all(s >= n * 8 * (24 + 3 * 256) for s, n in zip(sizes, ns))
        assert L.acm_calibrate_workspace_size(model, 64, 0) == \
            L.acm_calibrate_workspace_size(model, 64, 10 ** 9)
    assert L.acm_calibrate_workspace_size(7, 4, 8) == 0
    assert L.acm_calibrate_workspace_size(-1, 4, 8) == 0


def test_zero_views_is_valid_and_touches_nothing():
    cam = _cam()
    before = bytes(cam)
    summ = _lib.CalibrateSummary()
    ctypes.memset(ctypes.byref(summ), 0x5A, ctypes.sizeof(summ))
    keep = bytes(summ)
    for n_points, n_obs in ((0, 0), (7, 9)):
        assert _call(cam, _cfg(), n_views=0, n_points=n_points, n_obs=n_obs, poses=None, pts=None,
                     offs=None, point=None, uv=None, summary=ctypes.byref(summ), status=None,
                     w=None, wb=0) == 0
    assert bytes(cam) == before and bytes(summ) == keep
    # the argument checks still come first
    c = _cfg()
    c.flags = 1
    assert _call(cam, c, n_views=0) == _lib.ERR_INVALID_ARGUMENT
