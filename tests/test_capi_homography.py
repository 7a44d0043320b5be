"""C-ABI of acm_homography_4pt and acm_homography_batch without a device:
argument checks (every pointer below is rejected before it could be
dereferenced), the default config and its ranges, the workspace size, the
documented constants."""
import ctypes
import math
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


def _cfg(**kw):
    cfg = _lib.HomographyConfig()
    _lib.load().acm_homography_batch_default_config(ctypes.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _call(cam, cfg, n_pairs=4, n_matches=20, offs=PTR, uv_a=PTR, uv_b=PTR, hom=PTR, status=PTR,
          n_inliers=PTR, poses=None, planes=None, n_solutions=None, n_front=None, translation=None,
          mask=None, n_usable=None, w=PTR, wb=None):
    L = _lib.load()
    if wb is None:
        wb = L.acm_homography_batch_workspace_size(n_pairs, n_matches)
    return L.acm_homography_batch(ctypes.byref(cam) if cam else None, n_pairs, offs, n_matches, uv_a,
                                  uv_b, ctypes.byref(cfg) if cfg else None, hom, status, n_inliers,
                                  poses, planes, n_solutions, n_front, translation, mask, n_usable,
                                  w, wb, None)


def test_default_config():
    cfg = _cfg()
    assert (cfg.n_hypotheses, cfg.flags, cfg.seed, cfg.inlier_angle, cfg.min_inliers,
            cfg.refit_rounds) == (256, 0, 1, 5e-3, 4, 3)
    _lib.load().acm_homography_batch_default_config(None)  # a NULL config is ignored


def test_null_buffers_are_invalid_arguments():
    cam, cfg = _cam(), _cfg()
    assert _call(None, cfg) in BAD
    assert _call(cam, None) == _lib.ERR_INVALID_ARGUMENT
    for kw in ("offs", "uv_a", "uv_b", "hom", "status", "n_inliers"):
        assert _call(cam, cfg, **{kw: None}) == _lib.ERR_INVALID_ARGUMENT, kw
    # no matches: the pixel arrays may be NULL, the rest may not
    for kw in ("offs", "hom", "status", "n_inliers"):
        assert _call(cam, cfg, n_matches=0, uv_a=None, uv_b=None, **{kw: None}) == \
            _lib.ERR_INVALID_ARGUMENT, kw


def test_bad_model_config_and_workspace():
    cam, cfg = _cam(), _cfg()
    bad = _cam()
    for model in (7, -1):
        bad.model = model
        assert _call(bad, cfg) == _lib.ERR_INVALID_MODEL
    for field, values in (("n_hypotheses", (0, -1, 65537, 1 << 30)),
                          ("flags", (1, 2, -2, 0x100)),
                          ("inlier_angle", (0.0, -1e-3, math.pi / 2, 2.0, math.nan, math.inf)),
                          ("min_inliers", (3, 0, -1)),
                          ("refit_rounds", (-1, 9, 1 << 20))):
        for v in values:
            assert _call(cam, _cfg(**{field: v})) == _lib.ERR_INVALID_ARGUMENT, (field, v)
    # a bad config is rejected even when there is nothing to do
    assert _call(cam, _cfg(n_hypotheses=0), n_pairs=0) == _lib.ERR_INVALID_ARGUMENT
    ws = _lib.load().acm_homography_batch_workspace_size(4, 20)
    assert _call(cam, cfg, w=None) == _lib.ERR_WORKSPACE_TOO_SMALL
    assert _call(cam, cfg, wb=ws - 1) == _lib.ERR_WORKSPACE_TOO_SMALL
    assert _call(cam, cfg, wb=0) == _lib.ERR_WORKSPACE_TOO_SMALL


def test_zero_pairs_is_valid_and_touches_nothing():
    cam = _cam()
    for n_matches in (0, 9):
        assert _call(cam, _cfg(), n_pairs=0, n_matches=n_matches, offs=None, uv_a=None, uv_b=None,
                     hom=None, status=None, n_inliers=None, w=None, wb=0) == 0
    # the extreme values of the ranges are accepted
    for kw in (dict(n_hypotheses=1), dict(n_hypotheses=65536), dict(min_inliers=4),
               dict(min_inliers=1 << 30), dict(inlier_angle=1e-12), dict(inlier_angle=1.5),
               dict(seed=(1 << 64) - 1), dict(refit_rounds=0), dict(refit_rounds=8)):
        assert _call(cam, _cfg(**kw), n_pairs=0) == 0, kw


def test_workspace_size_holds_every_record():
    L = _lib.load()
    ns = [0, 1, 63, 64, 65, 4099, 10 ** 5, 10 ** 7, 10 ** 9]
    for m in ns:
        sizes = [L.acm_homography_batch_workspace_size(n, m) for n in ns]
        assert all(s >= 48 * m and s > 0 for s in sizes) and sizes == sorted(sizes)
    for n in ns:
        sizes = [L.acm_homography_batch_workspace_size(n, m) for m in ns]
        assert sizes == sorted(sizes)


def test_4pt_arguments():
    L = _lib.load()
    assert L.acm_homography_4pt(0, *([None] * 8), None) == 0
    for k in (0, 1, 2, 3, 4, 6, 7):  # the translation (5) is nullable
        args = [PTR] * 8
        args[k] = None
        assert L.acm_homography_4pt(3, *args, None) == _lib.ERR_INVALID_ARGUMENT, k


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "acm.h")).read()
    assert int(re.search(r"#define\s+ACM_HOMOGRAPHY_STAGE_MATCHES\s+(\d+)", text).group(1)) == \
        _lib.HOMOGRAPHY_STAGE_MATCHES == 1024
    for name, value in (("OK", _lib.HOMOGRAPHY_OK),
                        ("TOO_FEW_MATCHES", _lib.HOMOGRAPHY_TOO_FEW_MATCHES),
                        ("NO_MODEL", _lib.HOMOGRAPHY_NO_MODEL)):
        assert int(re.search(r"ACM_HOMOGRAPHY_%s\s*=\s*(\d+)" % name, text).group(1)) == value
    assert ctypes.sizeof(_lib.HomographyConfig) == 32
    assert _lib.HomographyConfig.seed.offset == 8
    assert _lib.HomographyConfig.inlier_angle.offset == 16
    assert _lib.HomographyConfig.min_inliers.offset == 24
    assert _lib.HomographyConfig.refit_rounds.offset == 28
