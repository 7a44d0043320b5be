"""CPU checks for the image-quality feature (src/util/image_quality.rs):
hand-derived answers pin the numpy restatement (tests/image_quality_ref.py)
that the GPU tests compare against, the PNG writer round-trips through a
decoder written here, and the new C-ABI entries reject bad arguments before
any HIP call."""
import ctypes
import math
import struct
import zlib

import numpy as np
import pytest

import image_quality_ref as R


# ---------------------------------------------------------------- restatement
def test_white_is_gray_255():
    img = np.full((2, 2, 3), 255, dtype=np.uint8)
    assert (R.gray(img) == 255).all()
    assert R.gray(np.zeros((1, 1, 3), dtype=np.uint8))[0, 0] == 0
    # truncation, not rounding: 0.299 * 2 = 0.598 -> 0
    assert R.gray(np.array([[[2, 0, 0]]], dtype=np.uint8))[0, 0] == 0


def test_disc_away_from_border_has_13_pixels():
    m = R.raster([[10.2, 7.4]], 33, 20)
    assert m.sum() == 13
    ys, xs = np.nonzero(m)
    assert {(x - 10, y - 7) for x, y in zip(xs, ys)} == set(R.DISC)
    assert len(R.DISC) == 13 and (2, 1) not in R.DISC and (0, 2) in R.DISC


def test_identical_images():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    assert R.psnr(img, img) == math.inf
    assert R.ssim(img, img) == (1.0, 7 * 9)
    assert (R.ssim_map(img, img) == 1.0).all()


def test_black_images():
    z = np.zeros((5, 6, 3), dtype=np.uint8)
    assert R.psnr_sums(z, z) == (0, 0)
    assert R.psnr(z, z) == math.inf
    assert R.ssim(z, z) == (1.0, 3 * 4)


def test_white_against_black_3x3():
    w = np.full((3, 3, 3), 255, dtype=np.uint8)
    z = np.zeros((3, 3, 3), dtype=np.uint8)
    assert R.psnr_sums(w, z) == (27 * 255 * 255, 27)
    assert R.psnr(w, z) == 0.0  # mse = 255^2 exactly: 10 log10(1)
    c1 = (0.01 * 255.0) * (0.01 * 255.0)
    # mu1 = 255, mu2 = 0, all variances 0: (c1 c2) / ((65025 + c1) c2)
    assert R.ssim(w, z) == (c1 / (65025.0 + c1), 1)


def test_small_images_have_no_ssim_window():
    a = np.full((2, 7, 3), 9, dtype=np.uint8)
    assert R.ssim(a, a) == (1.0, 0)
    assert R.ssim_map(a, a).shape == (0, 5)


ROUNDING = [  # u, centre, pixels of the dy = 0 row inside a W = 8 image (v = 3, H = 8)
    (2.5, 3, [1, 2, 3, 4, 5]),
    (-0.5, -1, [0, 1]),
    (-2.5, -3, []),
    (7.5, 8, [6, 7]),  # W - 0.5 -> W: partly visible
    (1e12, 2 ** 31 - 1, []),
    (-1e12, -2 ** 31, []),
    (float("nan"), 0, [0, 1, 2]),
    (0.49999999999999994, 0, [0, 1, 2]),
]


@pytest.mark.parametrize("u,centre,row", ROUNDING)
def test_rounding_cases(u, centre, row):
    assert int(R.rust_round_i32(u)) == centre
    m = R.raster([[u, 3.0]], 8, 8)
    assert np.nonzero(m[3])[0].tolist() == row
    # the same along y
    assert np.nonzero(R.raster([[3.0, u]], 8, 8)[:, 3])[0].tolist() == row
    if not row:
        assert m.sum() == 0


def test_keep_filter_checks_only_the_output_pixel():
    uv_in = np.array([[-50.0, 3.0], [1.0, 1.0], [1.0, 1.0], [1.0, 1.0], [1.0, 1.0]])
    uv_out = np.array([[1.0, 1.0], [8.0, 1.0], [7.999, 0.0], [1.0, np.nan], [1.0, 1.0]])
    st_in = np.array([0, 0, 0, 0, 2], dtype=np.uint8)
    st_out = np.zeros(5, dtype=np.uint8)
    assert R.keep(uv_in, st_in, uv_out, st_out, 8, 8).tolist() == [True, False, True, False, False]


def test_compose_order():
    a = np.zeros((2, 3), dtype=np.uint8)
    b = np.zeros((2, 3), dtype=np.uint8)
    a[0, 0] = a[0, 1] = 1
    b[0, 1] = b[1, 2] = 1
    bg = np.full((2, 3, 3), 7, dtype=np.uint8)
    img = R.compose(a, b, background=bg)
    assert img[0, 0].tolist() == [0, 255, 0]
    assert img[0, 1].tolist() == [255, 0, 255]  # magenta over green
    assert img[1, 2].tolist() == [255, 0, 255]
    assert img[1, 0].tolist() == [7, 7, 7]
    assert R.compose(a, b)[1, 0].tolist() == [0, 0, 0]


# ---------------------------------------------------------------------- PNG
def _decode_png(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        pos += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(chunks[1][1])
    assert len(raw) == h * (1 + 3 * w)
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all()  # filter type 0
    return rows[:, 1:].reshape(h, w, 3)


def test_png_round_trip(tmp_path):
    from apex_camera_models import util
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (7, 13, 3), dtype=np.uint8)
    assert np.array_equal(_decode_png(util._png_bytes(img)), img)
    path = util.save_model_projection_image(img, "Double Sphere", str(tmp_path / "out"))
    assert path.endswith("double_sphere_projection.png")
    assert np.array_equal(_decode_png(open(path, "rb").read()), img)
    with pytest.raises(util.UtilError):
        util._png_bytes(np.zeros((3, 3), dtype=np.uint8))


# -------------------------------------------------------------------- C-ABI
def _cam():
    from apex_camera_models import _lib
    cam = _lib.AcmCamera()
    p = (ctypes.c_double * 4)(500.0, 500.0, 320.0, 240.0)
    assert _lib.load().acm_camera_init(ctypes.byref(cam), 0, p, 4, 640, 480) == 0
    return cam


def test_c_entries_reject_bad_arguments_on_the_host():
    from apex_camera_models import _lib
    L = _lib.load()
    cam = _cam()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)  # never dereferenced: every call below fails its host checks
    c = ctypes.byref(cam)
    big = 1 << 40
    assert L.acm_projection_masks_workspace_size(0, 5) == 0
    assert L.acm_projection_masks_workspace_size(33, 5) == 2 * 12 * 4 + 2048 * 8
    assert L.acm_image_quality_workspace_size(5, 0) == 0
    assert L.acm_image_quality_workspace_size(37, 23) == 4 * 4 * 8

    def masks(ci=c, co=c, w=8, h=8, n=4, pts=p, layout=0, flags=0, mi=p, mo=p, nk=p, ws=p,
              wsb=big):
        return L.acm_projection_masks(ci, co, w, h, n, pts, layout, flags, mi, mo, nk, ws, wsb, None)
    bad = _lib.ERR_INVALID_ARGUMENT
    assert masks(ci=None) == bad and masks(co=None) == bad
    assert masks(w=0) == bad and masks(h=0) == bad and masks(w=2 ** 31) == bad
    assert masks(layout=2) == bad and masks(flags=4) == bad
    for k in ("pts", "mi", "mo", "nk", "ws"):
        assert masks(**{k: None}) == bad, k
    assert masks(wsb=2 * 8 * 4 + 2048 * 8 - 1) == _lib.ERR_WORKSPACE_TOO_SMALL
    cam2 = _cam()
    cam2.num_params = 3
    assert masks(co=ctypes.byref(cam2)) == _lib.ERR_INVALID_PARAMS

    def raster(w=8, h=8, n=4, pts=p, flags=0, m=p, ws=p, wsb=big):
        return L.acm_raster_points(w, h, n, pts, flags, m, ws, wsb, None)
    assert raster(w=0) == bad and raster(h=0) == bad and raster(flags=2) == bad
    assert raster(pts=None) == bad and raster(m=None) == bad and raster(ws=None) == bad
    assert raster(wsb=16) == _lib.ERR_WORKSPACE_TOO_SMALL

    rgb = (ctypes.c_uint8 * 3)(1, 2, 3)
    assert L.acm_compose_projection_image(0, 8, p, p, rgb, rgb, None, p, None) == bad
    assert L.acm_compose_projection_image(8, 0, p, p, rgb, rgb, None, p, None) == bad
    assert L.acm_compose_projection_image(8, 8, p, p, rgb, rgb, None, None, None) == bad
    assert L.acm_compose_projection_image(8, 8, p, p, None, rgb, None, p, None) == bad

    def quality(w=8, h=8, a=p, b=p, res=p, ws=p, wsb=big):
        return L.acm_image_quality(w, h, a, b, res, None, ws, wsb, None)
    assert quality(w=0) == bad and quality(h=0) == bad
    for k in ("a", "b", "res", "ws"):
        assert quality(**{k: None}) == bad, k
    assert quality(wsb=31) == _lib.ERR_WORKSPACE_TOO_SMALL


def test_image_quality_finish_is_the_reference_arithmetic():
    from apex_camera_models import _lib
    L = _lib.load()

    def finish(sse, valid, ssim_sum, count):
        raw = struct.pack("<QQdQ", sse, valid, ssim_sum, count)
        ps, ss = ctypes.c_double(), ctypes.c_double()
        assert L.acm_image_quality_finish(raw, ctypes.byref(ps), ctypes.byref(ss)) == 0
        return ps.value, ss.value
    assert finish(0, 0, 0.0, 0) == (math.inf, 1.0)
    assert finish(0, 27, 3.0, 4) == (math.inf, 0.75)
    assert finish(27 * 65025, 27, 0.5, 1) == (0.0, 0.5)
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (6, 5, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (6, 5, 3), dtype=np.uint8)
    sse, valid = R.psnr_sums(a, b)
    assert finish(sse, valid, 1.0, 1)[0] == R.psnr(a, b)
    ps, ss = ctypes.c_double(), ctypes.c_double()
    assert L.acm_image_quality_finish(None, ctypes.byref(ps), ctypes.byref(ss)) \
        == _lib.ERR_INVALID_ARGUMENT
