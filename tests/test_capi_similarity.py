"""C-ABI of acm_similarity_3pt and acm_similarity_batch without a device:
argument checks (every pointer below is rejected before it could be
dereferenced), the default config and its ranges, the workspace size, the
documented constants."""
import ctypes
import math
import os
import re

from apex_camera_models import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = ctypes.c_void_p(4096)  # never dereferenced


def _cfg(**kw):
    cfg = _lib.SimilarityConfig()
    _lib.load().acm_similarity_batch_default_config(ctypes.byref(cfg))
    cfg.inlier_distance = 0.05  # the default holds 0: the caller sets it
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _call(cfg, n_sets=4, n_points=20, offs=PTR, pa=PTR, pb=PTR, sim=PTR, status=PTR, n_inliers=PTR,
          rms=None, mask=None, n_usable=None, w=PTR, wb=None):
    L = _lib.load()
    if wb is None:
        wb = L.acm_similarity_batch_workspace_size(n_sets, n_points)
    return L.acm_similarity_batch(n_sets, offs, n_points, pa, pb, ctypes.byref(cfg) if cfg else None,
                                  sim, status, n_inliers, rms, mask, n_usable, w, wb, None)


def test_default_config():
    cfg = _lib.SimilarityConfig()
    _lib.load().acm_similarity_batch_default_config(ctypes.byref(cfg))
    assert (cfg.n_hypotheses, cfg.flags, cfg.seed, cfg.inlier_distance, cfg.min_inliers,
            cfg.refit_rounds) == (256, 0, 1, 0.0, 3, 3)
    _lib.load().acm_similarity_batch_default_config(None)  # a NULL config is ignored
    # the default config as it stands is rejected: it has no inlier distance
    assert _call(cfg) == _lib.ERR_INVALID_ARGUMENT


def test_null_buffers_are_invalid_arguments():
    cfg = _cfg()
    assert _call(None) == _lib.ERR_INVALID_ARGUMENT
    for kw in ("offs", "pa", "pb", "sim", "status", "n_inliers"):
        assert _call(cfg, **{kw: None}) == _lib.ERR_INVALID_ARGUMENT, kw
    # no points: the point arrays may be NULL, the rest may not
    for kw in ("offs", "sim", "status", "n_inliers"):
        assert _call(cfg, n_points=0, pa=None, pb=None, **{kw: None}) == \
            _lib.ERR_INVALID_ARGUMENT, kw


def test_bad_config_and_workspace():
    cfg = _cfg()
    for field, values in (("n_hypotheses", (0, -1, 65537, 1 << 30)),
                          ("flags", (2, -1, 3, 0x100)),
                          ("inlier_distance", (0.0, -1.0, math.nan, math.inf, -math.inf)),
                          ("min_inliers", (2, 0, -1)),
                          ("refit_rounds", (-1, 9, 1 << 20))):
        for v in values:
            assert _call(_cfg(**{field: v})) == _lib.ERR_INVALID_ARGUMENT, (field, v)
    # a bad config is rejected even when there is nothing to do
    assert _call(_cfg(n_hypotheses=0), n_sets=0) == _lib.ERR_INVALID_ARGUMENT
    assert _call(_cfg(inlier_distance=0.0), n_sets=0) == _lib.ERR_INVALID_ARGUMENT
    ws = _lib.load().acm_similarity_batch_workspace_size(4, 20)
    assert _call(cfg, w=None) == _lib.ERR_WORKSPACE_TOO_SMALL
    assert _call(cfg, wb=ws - 1) == _lib.ERR_WORKSPACE_TOO_SMALL
    assert _call(cfg, wb=0) == _lib.ERR_WORKSPACE_TOO_SMALL


def test_zero_sets_is_valid_and_touches_nothing():
    for n_points in (0, 9):
        assert _call(_cfg(), n_sets=0, n_points=n_points, offs=None, pa=None, pb=None, sim=None,
                     status=None, n_inliers=None, w=None, wb=0) == 0
    # the extreme values of the ranges are accepted
    for kw in (dict(n_hypotheses=1), dict(n_hypotheses=65536), dict(min_inliers=3),
               dict(min_inliers=1 << 30), dict(inlier_distance=1e-12), dict(inlier_distance=1e12),
               dict(flags=_lib.SIMILARITY_RIGID), dict(seed=(1 << 64) - 1), dict(refit_rounds=0),
               dict(refit_rounds=8)):
        assert _call(_cfg(**kw), n_sets=0) == 0, kw


def test_workspace_size_holds_every_record():
    L = _lib.load()
    ns = [0, 1, 63, 64, 65, 1025, 4099, 10 ** 5, 10 ** 7, 10 ** 9]
    for m in ns:
        sizes = [L.acm_similarity_batch_workspace_size(n, m) for n in ns]
        assert all(s >= 48 * m and s > 0 for s in sizes) and sizes == sorted(sizes)
    for n in ns:
        sizes = [L.acm_similarity_batch_workspace_size(n, m) for m in ns]
        assert sizes == sorted(sizes)
    # a 1025-point set (one past the LDS budget) keeps six planes of doubles there
    assert L.acm_similarity_batch_workspace_size(1, _lib.SIMILARITY_STAGE_POINTS + 1) >= 6 * 8 * 1025


def test_3pt_arguments():
    L = _lib.load()
    assert L.acm_similarity_3pt(0, None, None, 0, None, None, None) == 0
    assert L.acm_similarity_3pt(0, None, None, _lib.SIMILARITY_RIGID, None, None, None) == 0
    for k in range(4):
        args = [PTR] * 4
        args[k] = None
        assert L.acm_similarity_3pt(3, args[0], args[1], 0, args[2], args[3], None) == \
            _lib.ERR_INVALID_ARGUMENT, k
    for flags in (2, -1, 0x100):
        assert L.acm_similarity_3pt(3, PTR, PTR, flags, PTR, PTR, None) == _lib.ERR_INVALID_ARGUMENT
        assert L.acm_similarity_3pt(0, None, None, flags, None, None, None) == \
            _lib.ERR_INVALID_ARGUMENT


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "acm.h")).read()
    for name, value in (("STAGE_POINTS", _lib.SIMILARITY_STAGE_POINTS), ("DOUBLES", _lib.SIMILARITY_DOUBLES),
                        ("RIGID", _lib.SIMILARITY_RIGID)):
        assert int(re.search(r"#define\s+ACM_SIMILARITY_%s\s+(\d+)" % name, text).group(1)) == value
    assert (_lib.SIMILARITY_STAGE_POINTS, _lib.SIMILARITY_DOUBLES, _lib.SIMILARITY_RIGID) == (1024, 13, 1)
    for name, value in (("OK", _lib.SIMILARITY_OK),
                        ("TOO_FEW_POINTS", _lib.SIMILARITY_TOO_FEW_POINTS),
                        ("NO_MODEL", _lib.SIMILARITY_NO_MODEL)):
        assert int(re.search(r"ACM_SIMILARITY_%s\s*=\s*(\d+)" % name, text).group(1)) == value
    assert ctypes.sizeof(_lib.SimilarityConfig) == 32
    assert _lib.SimilarityConfig.seed.offset == 8
    assert _lib.SimilarityConfig.inlier_distance.offset == 16
    assert _lib.SimilarityConfig.min_inliers.offset == 24
    assert _lib.SimilarityConfig.refit_rounds.offset == 28
