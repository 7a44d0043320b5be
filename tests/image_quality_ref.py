"""numpy restatement of the reference's image-quality utilities
(src/util/image_quality.rs), written from their semantics: the keep filter
and radius-2 disc rasters of compute_image_quality_metrics, the overlay
picture, PSNR and SSIM.  TEST INFRASTRUCTURE ONLY (the expected values of
tests/test_image_quality_ref.py and tests/test_gpu_image_quality.py); pixels
come from oracle.project.

Every floating-point step is a separate numpy operation in the reference's
order (numpy never contracts a * b + c), so PSNR and every SSIM term carry the
reference's bits; ssim() adds the terms sequentially in row-major order, as
the reference's loop does."""
import math

import numpy as np

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
C1 = (0.01 * 255.0) * (0.01 * 255.0)
C2 = (0.03 * 255.0) * (0.03 * 255.0)
# the 13 offsets with dx^2 + dy^2 <= 4
DISC = [(dx, dy) for dy in range(-2, 3) for dx in range(-2, 3) if dx * dx + dy * dy <= 4]


def rust_round_i32(v):
    """f64::round (half away from zero) then `as i32` (saturating, NaN -> 0)."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        t = np.trunc(v)
        r = t + np.sign(v) * (np.abs(v - t) >= 0.5)  # v - trunc(v) is exact
        r = np.where(np.isnan(r), 0.0, np.clip(r, float(I32_MIN), float(I32_MAX)))
    return r.astype(np.int64)


def raster(points_2d, width, height):
    """(H, W) uint8 0 / 1: the union of the discs around the points."""
    mask = np.zeros((height, width), dtype=np.uint8)
    p = np.asarray(points_2d, dtype=np.float64).reshape(-1, 2)
    cx, cy = rust_round_i32(p[:, 0]), rust_round_i32(p[:, 1])
    for dx, dy in DISC:
        x, y = cx + dx, cy + dy  # int64: no wrap-around
        ok = (x >= 0) & (x < width) & (y >= 0) & (y < height)
        mask[y[ok], x[ok]] = 1
    return mask


def keep(uv_in, st_in, uv_out, st_out, width, height):
    """Both projections Ok and the OUTPUT pixel inside [0, W) x [0, H)."""
    with np.errstate(invalid="ignore"):
        return ((st_in == 0) & (st_out == 0) & (uv_out[:, 0] >= 0.0) &
                (uv_out[:, 0] < float(width)) & (uv_out[:, 1] >= 0.0) &
                (uv_out[:, 1] < float(height)))


def compose(mask_in, mask_out, color_in=(0, 255, 0), color_out=(255, 0, 255), background=None):
    """All input discs drawn first, then all output discs, on the background."""
    h, w = (mask_in if mask_in is not None else mask_out).shape
    img = np.zeros((h, w, 3), dtype=np.uint8) if background is None else background.copy()
    if mask_in is not None:
        img[mask_in != 0] = color_in
    if mask_out is not None:
        img[mask_out != 0] = color_out
    return img


def white(mask):
    return compose(mask, None, color_in=(255, 255, 255))


def psnr_sums(img1, img2):
    a, b = img1.astype(np.int64), img2.astype(np.int64)
    pairs = (a != 0).any(axis=2) | (b != 0).any(axis=2)
    d = (a - b)[pairs]
    return int((d * d).sum()), 3 * int(pairs.sum())


def psnr(img1, img2):
    sse, valid = psnr_sums(img1, img2)
    if valid == 0:
        return math.inf
    mse = float(sse) / float(valid)
    if mse <= 1e-10:
        return math.inf
    return 10.0 * math.log10(255.0 * 255.0 / mse)


def gray(img):
    f = img.astype(np.float64)
    return (0.299 * f[..., 0] + 0.587 * f[..., 1] + 0.114 * f[..., 2]).astype(np.uint8)


def ssim_map(img1, img2):
    """(H - 2, W - 2) per-pixel terms (NaN where the denominator is not > 0)."""
    g1, g2 = gray(img1).astype(np.float64), gray(img2).astype(np.float64)
    h, w = g1.shape
    if h < 3 or w < 3:
        return np.zeros((max(h - 2, 0), max(w - 2, 0)))
    win = [(slice(1 + dy, h - 1 + dy), slice(1 + dx, w - 1 + dx))
           for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    sum1 = np.zeros((h - 2, w - 2))
    sum2 = np.zeros((h - 2, w - 2))
    for s in win:
        sum1 = sum1 + g1[s]
        sum2 = sum2 + g2[s]
    mu1, mu2 = sum1 / 9.0, sum2 / 9.0
    s1 = np.zeros_like(mu1)
    s2 = np.zeros_like(mu1)
    s12 = np.zeros_like(mu1)
    for s in win:
        d1, d2 = g1[s] - mu1, g2[s] - mu2
        s1 = s1 + d1 * d1
        s2 = s2 + d2 * d2
        s12 = s12 + d1 * d2
    s1, s2, s12 = s1 / 8.0, s2 / 8.0, s12 / 8.0
    num = (2.0 * mu1 * mu2 + C1) * (2.0 * s12 + C2)
    den = (mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0.0, num / den, np.nan)


def ssim(img1, img2):
    """(mean, count): the terms added one by one in row-major order."""
    t = ssim_map(img1, img2).ravel()
    t = t[~np.isnan(t)]
    if t.size == 0:
        return 1.0, 0
    return float(np.cumsum(t)[-1]) / float(t.size), int(t.size)
