"""The image-quality kernels (src/util/image_quality.rs) on the GPU vs the
numpy restatement in tests/image_quality_ref.py fed with the oracle's pixels:
the fused dual-projection masks and n_kept (byte-identical), the raster of
given pixels, the overlay, PSNR (bit-equal) and SSIM (every term bit-equal,
the mean within the reordering bound), and the Python pipeline on top.

Masks quantise pixels with round() and compare them with the image bounds, so
the kernels project reference-exactly (camera_models.hpp EXACT).  The one
tolerated difference from the oracle is a last-bit disagreement with glibc's
atan2 (tests/test_gpu_exact.py); _expected() therefore asserts, on the
oracle's pixels, that no kept coordinate lies within 1e-6 of a rounding
boundary k + 1/2 or of an image bound, so such a difference cannot move a
pixel."""
import functools
import math

import numpy as np
import pytest

import image_quality_ref as R
import oracle as O
from test_oracle import SAMPLES

pytestmark = pytest.mark.gpu

KB, DS, UCM = 2, 3, 4
EDGE_POINTS = np.array([
    [0.1, 0.2, -1.0], [0.0, 0.0, 0.0], [1.0, 1.0, 0.0], [-0.3, 0.2, -1e-9],  # z <= 0
    [0.0, 0.0, 1.0], [0.0, 0.0, 2.5],  # r = 0
    [50.0, 0.0, 1.0], [0.0, -80.0, 1.0], [5.0, 5.0, 0.1], [-3.0, 2.0, 0.5],  # far off-axis
    [0.7, -0.4, 1.0], [-0.9, 0.8, 1.3], [1.7, 1.1, 0.9],
])


def _model(model, params=None, size=None):
    from _backends import GpuBackend
    p, (w, h) = SAMPLES[model]
    w, h = size or (w, h)
    return GpuBackend()._model(model, params or p, w, h)


@functools.lru_cache(maxsize=None)
def _points(model=KB, n=3000):
    """The input model's own grid sample (~n rays) plus the edge points."""
    params, (w, h) = SAMPLES[model]
    _, xyz, _ = O.sample_points(model, params, w, h, n)
    pts = np.concatenate([xyz, EDGE_POINTS])
    if len(pts) % 64 == 0:
        pts = pts[:-1]
    pts.setflags(write=False)
    return pts


def _away_from_boundaries(uv, bounds):
    frac = np.abs(uv - np.floor(uv) - 0.5)
    ok = (frac > 1e-6).all()
    for axis, size in enumerate(bounds):
        ok = ok and (np.abs(uv[:, axis]) > 1e-6).all() and (np.abs(uv[:, axis] - size) > 1e-6).all()
    return bool(ok)


def _expected(m_in, m_out, pts, size=None):
    """(input mask, output mask, n_kept) of the restatement on the oracle's
    pixels; (W, H) = size or the input model's resolution."""
    p_in, r_in = SAMPLES[m_in]
    p_out, r_out = SAMPLES[m_out]
    w, h = size or r_in
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    uv_i, st_i, _ = O.project(m_in, p_in, *r_in, pts)
    uv_o, st_o, _ = O.project(m_out, p_out, *r_out, pts)
    k = R.keep(uv_i, st_i, uv_o, st_o, w, h)
    # the input condition of the comparison (module docstring)
    assert _away_from_boundaries(uv_o[k], (w, h)) and _away_from_boundaries(uv_i[k], ())
    return R.raster(uv_i[k], w, h), R.raster(uv_o[k], w, h), int(k.sum())


@functools.lru_cache(maxsize=None)
def _expected_sample(m_in, m_out, size=None):
    return _expected(m_in, m_out, _points(m_in), size)


def _masks(m_in, m_out, pts, size=None, **kw):
    import torch
    from apex_camera_models import util
    w, h = size or SAMPLES[m_in][1]
    pts = np.array(pts, dtype=np.float64).reshape(-1, 3)
    if kw.get("layout") == "soa":
        pts = np.ascontiguousarray(pts.T)
    a, b, kept = util.projection_masks(_model(m_in), _model(m_out), torch.as_tensor(pts), w, h, **kw)
    return a.cpu().numpy(), b.cpu().numpy(), int(kept.item())


def _same(got, want):
    assert got[2] == want[2]
    for g, e, name in zip(got[:2], want[:2], ("input", "output")):
        assert g.dtype == np.uint8 and g.shape == e.shape
        assert set(np.unique(g).tolist()) <= {0, 1}
        diff = np.argwhere(g != e)
        assert len(diff) == 0, f"{name} mask: {len(diff)} pixels differ, first (y, x) {diff[:5].tolist()}"


# ------------------------------------------------------------------ a. masks
@pytest.mark.parametrize("m_in,m_out", [(KB, m) for m in range(7)] + [(DS, KB)])
def test_masks_and_count_vs_restatement(m_in, m_out):
    pts = _points(m_in)
    assert len(pts) % 64 != 0 and len(pts) > 2048  # more than one workgroup
    want = _expected_sample(m_in, m_out)
    assert want[2] > 50 and want[0].any() and want[1].any()
    _same(_masks(m_in, m_out, pts), want)
    # every point projected exactly instead of only those in the guard band
    _same(_masks(m_in, m_out, pts, exact_all=True), want)


def test_masks_of_one_point_and_of_none():
    one = _points(KB)[1234:1235]
    want = _expected(KB, DS, one)
    assert want[2] == 1 and want[0].sum() == 13
    _same(_masks(KB, DS, one), want)
    w, h = SAMPLES[KB][1]
    zero = np.zeros((h, w), dtype=np.uint8)
    _same(_masks(KB, DS, np.zeros((0, 3))), (zero, zero, 0))


# ----------------------------------------------------------------- b. shapes
def _pinhole(params, w, h):
    return _model(0, params, (w, h))


def test_small_image_clipped_on_all_borders():
    """33 x 5 (a second, partly used mask word per row): discs around pixels on
    and just inside every border, through two slightly different pinholes."""
    import torch
    from apex_camera_models import util
    w, h = 33, 5
    p_in, p_out = [20.0, 20.0, 16.0, 2.5], [20.5, 19.5, 16.3, 2.2]
    u = np.array([-1.77, 0.23, 1.31, 15.8, 30.9, 31.71, 32.27, 33.9])
    v = np.array([-0.8, 0.31, 2.2, 4.27, 4.73, 5.9])
    uu, vv = np.meshgrid(u, v)
    pts = np.stack([(uu.ravel() - p_in[2]) / p_in[0], (vv.ravel() - p_in[3]) / p_in[1],
                    np.ones(uu.size)], 1)
    uv_i, st_i, _ = O.project(0, p_in, w, h, pts)
    uv_o, st_o, _ = O.project(0, p_out, w, h, pts)
    k = R.keep(uv_i, st_i, uv_o, st_o, w, h)
    assert _away_from_boundaries(uv_o[k], (w, h)) and _away_from_boundaries(uv_i[k], ())
    want = (R.raster(uv_i[k], w, h), R.raster(uv_o[k], w, h), int(k.sum()))
    assert 0 < want[2] < len(pts)
    for m in want[:2]:  # every border carries drawn pixels
        assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any()
    a, b, kept = util.projection_masks(_pinhole(p_in, w, h), _pinhole(p_out, w, h),
                                       torch.as_tensor(pts), w, h)
    _same((a.cpu().numpy(), b.cpu().numpy(), int(kept.item())), want)


def test_pixels_inside_the_guard_band():
    """Pixels exactly on a rounding boundary k + 1/2 and on the bounds 0 and
    W: the lanes the default path projects a second time.  Pinhole arithmetic
    (one division, one multiply-add) is the same on both sides, so the
    oracle's pixels are the kernel's, bit for bit."""
    import torch
    from apex_camera_models import util
    w, h = 40, 24
    p_in, p_out = [2.0, 2.0, 0.5, 0.5], [4.0, 4.0, 0.0, 0.0]
    xs = np.array([0.0, 1.0, 2.0, 2.25, 5.0, 9.875, 10.0 - 2.0 ** -40, 3.0 + 2.0 ** -40])
    ys = np.array([0.0, 0.125, 1.0, 3.5, 5.875, 6.0])
    xx, yy = np.meshgrid(xs, ys)
    pts = np.stack([xx.ravel(), yy.ravel(), np.ones(xx.size)], 1)
    uv_i, st_i, _ = O.project(0, p_in, w, h, pts)
    uv_o, st_o, _ = O.project(0, p_out, w, h, pts)
    assert (uv_i[st_i == 0] - np.floor(uv_i[st_i == 0]) == 0.5).any()  # 2 x + 0.5
    assert (uv_o[st_o == 0] == 0.0).any() and (uv_o[st_o == 0][:, 0] == 40.0 - 2.0 ** -38).any()
    k = R.keep(uv_i, st_i, uv_o, st_o, w, h)
    want = (R.raster(uv_i[k], w, h), R.raster(uv_o[k], w, h), int(k.sum()))
    assert 0 < want[2] < len(pts)
    for exact_all in (False, True):
        a, b, kept = util.projection_masks(_pinhole(p_in, w, h), _pinhole(p_out, w, h),
                                           torch.as_tensor(pts), w, h, exact_all=exact_all)
        _same((a.cpu().numpy(), b.cpu().numpy(), int(kept.item())), want)


def test_row_that_ends_mid_word():
    """752 x 480: 23.5 mask words per row, the LDS form's largest image."""
    want = _expected_sample(DS, KB)
    assert want[0].shape == (480, 752) and want[0][:, 736:].any()
    _same(_masks(DS, KB, _points(DS)), want)


def test_reference_image_size_takes_the_global_path():
    """A 2048 x 1536 "reference image" with the 752 x 480 model: the masks no
    longer fit a workgroup's LDS, and the output bounds are the image's."""
    size = (2048, 1536)
    want = _expected_sample(DS, UCM, size)
    assert want[2] > 4 * _expected_sample(DS, UCM)[2]  # the bounds are not the model's
    assert want[1][480:, 752:].any()
    _same(_masks(DS, UCM, _points(DS), size), want)


# ------------------------------------------------------ c. layout, accumulate
def test_soa_equals_aos_and_two_halves_equal_one_call():
    import torch
    from apex_camera_models import util
    pts = np.array(_points(KB))  # a writable copy for torch
    want = _expected_sample(KB, DS)
    _same(_masks(KB, DS, pts, layout="soa"), want)
    w, h = SAMPLES[KB][1]
    half = len(pts) // 2 + 7
    first = util.projection_masks(_model(KB), _model(DS), torch.as_tensor(pts[:half]), w, h)
    a, b, kept = util.projection_masks(_model(KB), _model(DS), torch.as_tensor(pts[half:]), w, h,
                                       out=first)
    _same((a.cpu().numpy(), b.cpu().numpy(), int(kept.item())), want)
    # accumulating nothing changes nothing
    a, b, kept = util.projection_masks(_model(KB), _model(DS), torch.zeros((0, 3)), w, h,
                                       out=(a, b, kept))
    _same((a.cpu().numpy(), b.cpu().numpy(), int(kept.item())), want)


# ---------------------------------------------------------- d. given pixels
def test_raster_points_rounding_cases():
    import torch
    from apex_camera_models import util
    from test_image_quality_ref import ROUNDING
    for u, _, _ in ROUNDING:
        for p in ([u, 3.0], [3.0, u], [u, u]):
            got = util.raster_points(torch.tensor([p], dtype=torch.float64), 8, 8).cpu().numpy()
            assert np.array_equal(got, R.raster([p], 8, 8)), p
    allp = [[u, 3.0] for u, _, _ in ROUNDING] + [[5.0, u] for u, _, _ in ROUNDING]
    got = util.raster_points(torch.tensor(allp, dtype=torch.float64), 8, 8)
    assert np.array_equal(got.cpu().numpy(), R.raster(allp, 8, 8))
    # accumulate, and an image beyond the LDS form (one mask of 1600 x 1000 bits)
    rng = np.random.default_rng(11)
    uv = rng.uniform(-5, 1605, (5000, 2)) * [1.0, 1000 / 1600]
    want = R.raster(uv, 1600, 1000)
    m = util.raster_points(torch.as_tensor(uv[:2000]), 1600, 1000)
    m = util.raster_points(torch.as_tensor(uv[2000:]), 1600, 1000, out=m)
    assert np.array_equal(m.cpu().numpy(), want)
    img = util.create_projection_image(torch.as_tensor(uv), (9, 8, 7), 1600, 1000).cpu().numpy()
    assert np.array_equal(img, R.compose(want, None, color_in=(9, 8, 7)))


# ---------------------------------------------------------- e. PSNR / SSIM
def _random_pair(w, h, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8)
    black = rng.random((h, w)) < 0.2  # pairs black in both images: skipped by PSNR
    a[black] = 0
    b[black] = 0
    b[rng.random((h, w)) < 0.1] = 0  # black in one image only: counted
    return a, b


def test_image_quality_vs_restatement():
    import torch
    from apex_camera_models import util
    a, b = _random_pair(37, 23, 1)
    assert ((a == 0).all(2) & (b == 0).all(2)).sum() > 50
    sse, valid, ssum, count, smap = util.image_quality_sums(torch.as_tensor(a), torch.as_tensor(b),
                                                            ssim_map=True)
    assert (sse, valid) == R.psnr_sums(a, b)
    mean0, count0 = R.ssim(a, b)
    assert count == count0 == 35 * 21
    assert np.array_equal(smap.cpu().numpy().view(np.int64), R.ssim_map(a, b).view(np.int64))
    psnr, ssim = util.image_quality(torch.as_tensor(a), torch.as_tensor(b))
    assert psnr == R.psnr(a, b) and math.isfinite(psnr)
    assert ssim == ssum / count
    # every |term| <= 1: reordering `count` additions moves the sum by at most
    # count * 2^-53 * count, the mean by count * 2^-53
    assert abs(ssim - mean0) <= count * 2.0 ** -53
    again = util.image_quality_sums(torch.as_tensor(a), torch.as_tensor(b))
    assert again[:4] == (sse, valid, ssum, count)
    assert util.calculate_psnr(a, b) == psnr and util.calculate_ssim(a, b) == ssim


def test_image_quality_edge_cases():
    from apex_camera_models import util
    a, b = _random_pair(2, 9, 2)  # W < 3: no window
    assert util.image_quality_sums(a, b)[2:4] == (0.0, 0)
    assert util.calculate_ssim(a, b) == 1.0
    assert util.calculate_psnr(a, b) == R.psnr(a, b)
    a, _ = _random_pair(40, 3, 3)  # H = 3: one row of windows
    assert util.image_quality(a, a) == (math.inf, 1.0)
    z = np.zeros((5, 6, 3), dtype=np.uint8)
    assert util.image_quality(z, z) == (math.inf, 1.0)
    w = np.full((3, 3, 3), 255, dtype=np.uint8)
    c1 = (0.01 * 255.0) * (0.01 * 255.0)
    assert util.image_quality(w, z[:3, :3]) == (0.0, c1 / (65025.0 + c1))
    with pytest.raises(util.UtilError):
        util.calculate_psnr(a, z)


# ------------------------------------------------------------- f. compose
def test_compose_vs_restatement():
    import torch
    from apex_camera_models import util
    rng = np.random.default_rng(4)
    w, h = 45, 19
    m_in = (rng.random((h, w)) < 0.3).astype(np.uint8)
    m_out = (rng.random((h, w)) < 0.3).astype(np.uint8)
    bg = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    t_in, t_out = torch.as_tensor(m_in).cuda(), torch.as_tensor(m_out).cuda()
    assert (m_in & m_out).any()  # magenta over green somewhere
    got = util.compose_projection_image(w, h, t_in, t_out, background=bg).cpu().numpy()
    assert np.array_equal(got, R.compose(m_in, m_out, background=bg))
    got = util.compose_projection_image(w, h, t_in, t_out).cpu().numpy()
    assert np.array_equal(got, R.compose(m_in, m_out))
    got = util.compose_projection_image(w, h, None, t_out, background=bg).cpu().numpy()
    assert np.array_equal(got, R.compose(None, m_out, background=bg))
    uv_i = rng.uniform(-3, 48, (60, 2)) * [1.0, 19 / 45]
    uv_o = uv_i + rng.uniform(-2, 2, uv_i.shape)
    got = util.create_combined_projection_image_on_reference(uv_i, uv_o, bg).cpu().numpy()
    assert np.array_equal(got, R.compose(R.raster(uv_i, w, h), R.raster(uv_o, w, h), background=bg))
    got = util.create_combined_projection_image(uv_i, uv_o, w, h).cpu().numpy()
    assert np.array_equal(got, R.compose(R.raster(uv_i, w, h), R.raster(uv_o, w, h)))
    got = util.model_projection_visualization(uv_i, "KB", reference_image=bg).cpu().numpy()
    assert np.array_equal(got, R.compose(R.raster(uv_i, w, h), None, background=bg))


# ---------------------------------------------------------- g. end to end
def test_compute_image_quality_metrics_end_to_end(tmp_path):
    import os

    import torch
    from apex_camera_models import conversion, util
    kb = _model(KB)
    p_in, (w, h) = SAMPLES[KB]
    uv, xyz = util.sample_points(kb, 500)
    plain = conversion.convert(kb, "double_sphere", xyz, uv)
    assert plain.image_quality is None
    cm = conversion.convert(kb, "double_sphere", xyz, uv, image_quality=True)
    q = cm.image_quality
    assert isinstance(q, util.ImageQualityMetrics)
    q2 = util.compute_image_quality_metrics(kb, cm.model, xyz, "Double Sphere",
                                            output_dir=str(tmp_path))
    assert (q2.psnr, q2.ssim, q2.n_kept) == (q.psnr, q.ssim, q.n_kept)
    assert os.path.getsize(tmp_path / "double_sphere_projection.png") > 100
    # the restatement on the oracle's pixels of the converted model
    pts = xyz.cpu().numpy()
    p_out = [float(v) for v in cm.model.params()]
    uv_i, st_i, _ = O.project(KB, p_in, w, h, pts)
    uv_o, st_o, _ = O.project(DS, p_out, w, h, pts)
    k = R.keep(uv_i, st_i, uv_o, st_o, w, h)
    m_i, m_o = R.raster(uv_i[k], w, h), R.raster(uv_o[k], w, h)
    assert q.n_kept == int(k.sum()) > 400
    assert np.array_equal(q.overlay.cpu().numpy(), R.compose(m_i, m_o))
    assert q.psnr == R.psnr(R.white(m_i), R.white(m_o))
    mean0, count = R.ssim(R.white(m_i), R.white(m_o))
    assert abs(q.ssim - mean0) <= count * 2.0 ** -53
    # with a reference image: its size, and the overlay drawn on it
    ref = np.random.default_rng(6).integers(0, 256, (300, 400, 3), dtype=np.uint8)
    q3 = util.compute_image_quality_metrics(kb, cm.model, xyz, reference_image=ref)
    k3 = R.keep(uv_i, st_i, uv_o, st_o, 400, 300)
    assert q3.n_kept == int(k3.sum()) < q.n_kept
    assert np.array_equal(q3.overlay.cpu().numpy(),
                          R.compose(R.raster(uv_i[k3], 400, 300), R.raster(uv_o[k3], 400, 300),
                                    background=ref))
    behind = torch.tensor([[0.1, 0.2, -1.0], [0.0, 0.3, -2.0]], dtype=torch.float64)
    with pytest.raises(util.ZeroProjectionPoints):
        util.compute_image_quality_metrics(kb, cm.model, behind)


def test_image_quality_over_shards_is_not_implemented():
    from apex_camera_models import conversion

    class _C:
        world = 2

    class _Coll:
        c = _C()
    with pytest.raises(NotImplementedError):
        conversion.convert(_model(KB), "double_sphere", None, None, collective=_Coll(),
                           image_quality=True)
