"""Mirror of the reference's hot-path utilities (src/util/).

`sample_points` (point_sampling.rs:46-120) and `compute_reprojection_error`
(error_metrics.rs:62-121), both evaluated by libacm.so kernels on device
tensors; `undistort_image` (undistort.rs), `validate_conversion_accuracy`
(validation.rs) and the projection rasters, overlay picture and PSNR / SSIM
of image_quality.rs (below: the fused dual-projection raster kernel, PNG
output with the standard library only).
"""
from __future__ import annotations

import ctypes
import dataclasses
from dataclasses import dataclass

import torch

from . import _lib
from .camera import CameraModel, InvalidParams, NumericalError, _as_device_f64, _stream_handle


class UtilError(Exception):
    pass


class ZeroProjectionPoints(UtilError):
    def __init__(self):
        super().__init__("Zero projection points")


@dataclass
class ProjectionError:
    rmse: float
    min: float
    max: float
    mean: float
    stddev: float
    median: float
    n_valid: int = 0


@dataclass
class CellSample:
    """The cell form of grid-sampled correspondences (r06): cells[k] = i * ncx
    + j is the grid cell of points_2d[k] (point_sampling.rs:56-78), a uint32
    instead of the 16-B pixel -- what conversion.convert(cells=...) hands the
    LM (acm_lm_optimize_cells: the same iterates, 12 B per point less read per
    evaluation)."""
    cells: torch.Tensor  # (M,) int32 device tensor holding the uint32 cell ids
    grid: object         # _lib.CellGrid


def sample_points(camera_model: CameraModel, n: int, reference_newton: bool = False,
                  cells: bool = False, cell_range=None):
    """Grid of ~n pixel-cell centres, unprojected; keeps Ok && z > 0, in order.

    Returns (points_2d (M,2), points_3d (M,3)) float64 device tensors, and
    with cells=True a third item, the CellSample of the same points.
    reference_newton=True: ACM_REFERENCE_NEWTON for this call.  cell_range:
    (begin, end) cells of the grid (a multi-GPU shard), default all.
    """
    L = _lib.load()
    cam = camera_model.acm_camera()
    ncx, ncy = ctypes.c_uint32(), ctypes.c_uint32()
    _lib.check(L.acm_sample_points_grid(cam.width, cam.height, n, ctypes.byref(ncx),
                                        ctypes.byref(ncy)))
    c0, c1 = cell_range if cell_range is not None else (0, ncx.value * ncy.value)
    cap = max(c1 - c0, 1)
    dev = torch.device("cuda")
    uv = torch.empty((cap, 2), dtype=torch.float64, device=dev)
    xyz = torch.empty((cap, 3), dtype=torch.float64, device=dev)
    counts = torch.zeros((2,), dtype=torch.int64, device=dev)
    ws_bytes = L.acm_sample_points_workspace_size(ctypes.byref(cam), n)
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device=dev)
    flags = _lib.REFERENCE_NEWTON if reference_newton else 0
    cl = None
    if cells:
        cl = torch.empty((cap,), dtype=torch.int32, device=dev)
        _lib.check(L.acm_sample_points_cells(ctypes.byref(cam), n, c0, c1, flags, uv.data_ptr(),
                                             xyz.data_ptr(), cl.data_ptr(), counts.data_ptr(),
                                             ws.data_ptr(), ws_bytes, _stream_handle()))
    else:
        _lib.check(L.acm_sample_points_ex(ctypes.byref(cam), n, c0, c1, flags, uv.data_ptr(),
                                          xyz.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                          ws_bytes, _stream_handle()))
    m = int(counts[0].item())
    if cells:
        grid = _lib.CellGrid(ncx.value, ncy.value, cam.width, cam.height)
        return uv[:m], xyz[:m], CellSample(cl[:m], grid)
    return uv[:m], xyz[:m]


def reprojection_stats(camera_model: CameraModel, points3d, points2d, errors=None):
    """Device result [rmse, min, max, mean, stddev, n_valid, sum, sumsq]."""
    L = _lib.load()
    p3 = _as_device_f64(points3d, 3)
    p2 = _as_device_f64(points2d, 2)
    n = p3.shape[0]
    if p2.shape[0] != n:
        raise ValueError("points3d and points2d must have the same number of columns")
    ws_bytes = L.acm_reprojection_stats_workspace_size(n)
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device=p3.device)
    out = torch.empty((8,), dtype=torch.float64, device=p3.device)
    cam = camera_model.acm_camera()
    _lib.check(L.acm_reprojection_stats(ctypes.byref(cam), n, p3.data_ptr(), _lib.LAYOUT_AOS,
                                        p2.data_ptr(), out.data_ptr(),
                                        errors.data_ptr() if errors is not None else None,
                                        ws.data_ptr(), ws_bytes, _stream_handle()))
    return out


def compute_reprojection_error(camera_model: CameraModel, points3d, points2d,
                               collective=None, cells=None) -> ProjectionError:
    """error_metrics.rs:62-121: one acm_reprojection_error call (the
    statistics and the median, whose first radix histogram the statistics
    pass counts) and one device -> host read of its 9 doubles.

    collective (distributed.RcclCollective / TorchCollective, r06): the
    points are this rank's shard, and the result is the union's
    (acm_reprojection_error_sharded), the same on every rank.  cells (r06):
    the CellSample of points2d -- the pass reads the 4-B cells (same bits)."""
    L = _lib.load()
    p3 = _as_device_f64(points3d, 3)
    p2 = _as_device_f64(points2d, 2)
    n = p3.shape[0]
    if p2.shape[0] != n:
        raise ValueError("points3d and points2d must have the same number of columns")
    res = torch.empty((9,), dtype=torch.float64, device=p3.device)
    cam = camera_model.acm_camera()
    cl, grid = _cell_args(cells, n)
    if collective is not None:
        ws_bytes = L.acm_reprojection_error_sharded_workspace_size(n, collective.c.world)
        ws = _workspace(ws_bytes, p3.device)
        _lib.check(L.acm_reprojection_error_sharded(
            ctypes.byref(cam), n, p3.data_ptr() if n else None, _lib.LAYOUT_AOS,
            p2.data_ptr() if n else None, cl, grid, res.data_ptr(), None,
            ctypes.byref(collective.c), ws.data_ptr(), ws_bytes, _stream_handle()))
    elif cells is not None:
        ws_bytes = L.acm_reprojection_error_workspace_size(n)
        ws = _workspace(ws_bytes, p3.device)
        _lib.check(L.acm_reprojection_error_cells(ctypes.byref(cam), n, p3.data_ptr(),
                                                  _lib.LAYOUT_AOS, cl, grid, res.data_ptr(), None,
                                                  ws.data_ptr(), ws_bytes, _stream_handle()))
    else:
        ws_bytes = L.acm_reprojection_error_workspace_size(n)
        ws = _workspace(ws_bytes, p3.device)
        _lib.check(L.acm_reprojection_error(ctypes.byref(cam), n, p3.data_ptr(), _lib.LAYOUT_AOS,
                                            p2.data_ptr(), res.data_ptr(), None, ws.data_ptr(),
                                            ws_bytes, _stream_handle()))
    out = res.cpu().tolist()
    n_valid = int(out[5])
    if n_valid == 0:
        raise ZeroProjectionPoints()
    return ProjectionError(rmse=out[0], min=out[1], max=out[2], mean=out[3], stddev=out[4],
                           median=out[8], n_valid=n_valid)


def _workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=device)


def _cell_args(cells, n):
    """(cells pointer, grid reference) for the C-ABI's nullable cell-form
    arguments (None, None without a CellSample)."""
    if cells is None:
        return None, None
    if cells.cells.shape[0] != n:
        raise ValueError("cells and points_3d must have the same number of points")
    return (cells.cells.data_ptr() if n else None), ctypes.byref(cells.grid)


def initial_error_and_linear_estimation(model: CameraModel, points3d, points2d,
                                        defer_median: bool = False, collective=None,
                                        cells=None):
    """convert_to_*'s opening (camera_converter.rs:371-375): the reprojection
    error of `model` as given, then `model.linear_estimation` -- for the TSQR
    models one pass over the correspondences (acm_linear_estimation_with_error_async).
    Raises like the two calls in that order: ZeroProjectionPoints first, then
    the estimation's InvalidParams / NumericalError.

    defer_median=True (conversion.convert, r05): returns (error, finish) at
    once, `error.median` NaN; the median is still running on the stream and
    finish() returns the completed ProjectionError -- call it after the next
    synchronising step (the LM), so no host round trip separates the opening
    from the LM's first evaluation.

    collective (r06): the points are this rank's shard and everything is
    over the union (acm_linear_estimation_with_error_sharded: one all-gather
    of each rank's factor and statistics, the distributed median); every
    rank gets the same model.  cells (r06): the CellSample of points2d --
    the fused pass reads the 4-B cells (same bits)."""
    L = _lib.load()
    p3 = _as_device_f64(points3d, 3)
    p2 = _as_device_f64(points2d, 2)
    n = p3.shape[0]
    if p2.shape[0] != n:  # as linear_estimation raises it (kannala_brandt.rs:168-172 & co)
        raise InvalidParams("Number of 2D and 3D points must match")
    if collective is not None:
        ws_bytes = L.acm_linear_estimation_with_error_sharded_workspace_size(
            model.MODEL_ID, n, collective.c.world)
    else:
        ws_bytes = L.acm_linear_estimation_with_error_workspace_size(model.MODEL_ID, n)
    if ws_bytes == 0:
        raise InvalidParams(f"{model.NAME} has no GPU linear_estimation")
    ws = _workspace(ws_bytes, p3.device)
    # NaN until written: an early error return of the C call leaves it so
    res = torch.full((9,), float("nan"), dtype=torch.float64, device=p3.device)
    host = (ctypes.c_double * 8)(*([float("nan")] * 8))
    cam = model.acm_camera()
    cl, grid = _cell_args(cells, n)
    if collective is not None:
        rc = L.acm_linear_estimation_with_error_sharded(
            ctypes.byref(cam), n, p3.data_ptr() if n else None, _lib.LAYOUT_AOS,
            p2.data_ptr() if n else None, cl, grid, res.data_ptr(), host,
            ctypes.byref(collective.c), ws.data_ptr(), ws_bytes, _stream_handle())
    elif cells is not None:
        rc = L.acm_linear_estimation_with_error_cells_async(
            ctypes.byref(cam), n, p3.data_ptr(), _lib.LAYOUT_AOS, p2.data_ptr(), cl, grid,
            res.data_ptr(), host, ws.data_ptr(), ws_bytes, _stream_handle())
    else:
        rc = L.acm_linear_estimation_with_error_async(ctypes.byref(cam), n, p3.data_ptr(),
                                                      _lib.LAYOUT_AOS, p2.data_ptr(),
                                                      res.data_ptr(), host, ws.data_ptr(),
                                                      ws_bytes, _stream_handle())
    if rc not in (_lib.ACM_SUCCESS, _lib.ERR_INVALID_PARAMS, _lib.ERR_NUMERICAL):
        _lib.check(rc)
    out = list(host)
    if out[5] != out[5]:  # the initial error was never computed: the call's own error
        if rc == _lib.ERR_NUMERICAL:
            raise NumericalError(_lib.last_error())
        raise InvalidParams(_lib.last_error())
    n_valid = int(out[5])
    if n_valid == 0:
        raise ZeroProjectionPoints()
    if rc == _lib.ERR_INVALID_PARAMS:
        raise InvalidParams(_lib.last_error())
    if rc == _lib.ERR_NUMERICAL:
        raise NumericalError(_lib.last_error())
    model._set_params(list(cam.params)[: model.NUM_PARAMS])
    err = ProjectionError(rmse=out[0], min=out[1], max=out[2], mean=out[3], stddev=out[4],
                          median=float("nan"), n_valid=n_valid)

    def finish(err=err, res=res, ws=ws):  # ws: the median reads it until the stream passes
        return dataclasses.replace(err, median=float(res[8].item()))
    if defer_median:
        return err, finish
    return finish()


def reprojection_median(errors: torch.Tensor, n_valid: int) -> float:
    """Median of the valid (non-NaN) errors (error_metrics.rs:104-111)."""
    L = _lib.load()
    out = torch.empty((1,), dtype=torch.float64, device=errors.device)
    ws_bytes = L.acm_median_workspace_size(errors.numel())
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device=errors.device)
    _lib.check(L.acm_median_valid(errors.numel(), errors.data_ptr(), None, n_valid, out.data_ptr(),
                                  ws.data_ptr(), ws_bytes, _stream_handle()))
    return float(out.item())


NEAREST, BILINEAR = 0, 1


def undistort_image(input_image, camera_model: CameraModel, target_intrinsics=None,
                    interpolation: int = BILINEAR):
    """`undistort_image` (src/util/undistort.rs:14-49): input_image (H, W, 3)
    uint8 (device or host), returns the (H, W, 3) uint8 device tensor."""
    res = camera_model.get_resolution()
    img = input_image if isinstance(input_image, torch.Tensor) else torch.as_tensor(input_image)
    img = img.to("cuda", torch.uint8).contiguous()
    if img.dim() != 3 or img.shape[2] != 3:
        raise UtilError("expected an (H, W, 3) RGB8 image")
    h, w = img.shape[0], img.shape[1]
    if w != res.width or h != res.height:  # :23-28
        raise UtilError(f"Image {w}x{h} doesn't match model {res.width}x{res.height}")
    out = torch.empty_like(img)
    cam = camera_model.acm_camera()
    t = None
    if target_intrinsics is not None:
        ti = target_intrinsics
        t = (ctypes.c_double * 4)(ti.fx, ti.fy, ti.cx, ti.cy)
    _lib.check(_lib.load().acm_undistort_image(ctypes.byref(cam), t, interpolation,
                                               img.data_ptr(), out.data_ptr(),
                                               _stream_handle()))
    return out


# ------------------------------------------------- validate_conversion_accuracy
@dataclass
class RegionValidation:
    name: str
    input_projection: object  # (u, v) or None
    output_projection: object
    error: float


@dataclass
class ValidationResults:
    center_error: float
    near_center_error: float
    mid_region_error: float
    edge_region_error: float
    far_edge_error: float
    average_error: float
    max_error: float
    status: str
    region_data: list


_REGIONS = (("Center", 0.5), ("Near Center", 0.55), ("Mid Region", 0.65),
            ("Edge Region", 0.8), ("Far Edge", 0.95))
_VALIDATION_CACHE = {}
_VALIDATION_CACHE_MAX = 64


def _validation_buffers(width: int, height: int):
    """The five test pixels of a resolution, resident on the device, and the
    device / pinned-host result buffers of validate_conversion_accuracy
    (cached per resolution, device, stream and thread: the call then launches
    three kernels and copies twice, without building tensors on the host).
    Two calls on one device from different threads or streams get different
    buffers, so neither overwrites the other's results between the copies
    and the synchronisation; the cache is bounded."""
    import threading
    key = (int(width), int(height), torch.cuda.current_device(),
           torch.cuda.current_stream().cuda_stream, threading.get_ident())
    if key not in _VALIDATION_CACHE:
        if len(_VALIDATION_CACHE) >= _VALIDATION_CACHE_MAX:
            _VALIDATION_CACHE.clear()
        w, h = float(width), float(height)
        k = len(_REGIONS)
        pix = torch.tensor([[w * f, h * f] for _, f in _REGIONS], dtype=torch.float64,
                           device="cuda")
        _VALIDATION_CACHE[key] = (
            pix, torch.empty((3 * k,), dtype=torch.uint8, device="cuda"),
            torch.empty((2 * k, 2), dtype=torch.float64, device="cuda"),
            torch.empty((3 * k,), dtype=torch.uint8).pin_memory(),
            torch.empty((2 * k, 2), dtype=torch.float64).pin_memory())
    return _VALIDATION_CACHE[key]


def validate_conversion_accuracy(output_model: CameraModel,
                                 input_model: CameraModel) -> ValidationResults:
    """`validate_conversion_accuracy` (validation.rs:92-213): the five
    diagonal test pixels (0.5 .. 0.95 of the input resolution) are
    unprojected with the input model and the rays projected with both models
    (one batched kernel call each); error = ||input_proj - output_proj||."""
    import math
    res = input_model.get_resolution()
    k = len(_REGIONS)
    pix, st_d, uv_d, st_h, uv_h = _validation_buffers(res.width, res.height)
    rays, _ = input_model.unproject_batch(pix, out=(None, st_d[:k]))
    input_model.project_batch(rays, out=(uv_d[:k], st_d[k:2 * k], None))
    output_model.project_batch(rays, out=(uv_d[k:], st_d[2 * k:], None))
    # two async copies into pinned host memory and one stream synchronisation
    st_h.copy_(st_d, non_blocking=True)
    uv_h.copy_(uv_d, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    st = st_h.tolist()
    uvl = uv_h.tolist()
    rays_ok, ok_in, ok_out = st[:k], st[k:2 * k], st[2 * k:]
    a, b = uvl[:k], uvl[k:]
    total, max_error, valid = 0.0, 0.0, 0
    errs, data = [], []
    for i, (name, _) in enumerate(_REGIONS):
        if rays_ok[i] == 0 and ok_in[i] == 0 and ok_out[i] == 0:  # :120-143
            du, dv = a[i][0] - b[i][0], a[i][1] - b[i][1]
            e = math.sqrt(du * du + dv * dv)
            total += e
            max_error = max(max_error, e)
            valid += 1
            errs.append(e)
            data.append(RegionValidation(name, tuple(a[i]), tuple(b[i]), e))
        else:  # :144-182: any failure -> NaN, no projections recorded
            errs.append(float("nan"))
            data.append(RegionValidation(name, None, None, float("nan")))
    avg = total / valid if valid > 0 else float("nan")
    if math.isnan(avg):  # :192-200
        status = "NEEDS IMPROVEMENT"
    elif avg < 0.001:
        status = "EXCELLENT"
    elif avg < 0.1:
        status = "GOOD"
    else:
        status = "NEEDS IMPROVEMENT"
    return ValidationResults(*errs, average_error=avg, max_error=max_error, status=status,
                             region_data=data)


# ------------------------------------------------------------- image quality
# Mirror of src/util/image_quality.rs.  Images are (H, W, 3) uint8 device
# tensors (RGB8, row-major); a projection raster is a set of pixels (every
# disc of one raster has one colour), built as a (H, W) uint8 0 / 1 mask.
GREEN, MAGENTA, WHITE = (0, 255, 0), (255, 0, 255), (255, 255, 255)


@dataclass
class ImageQualityMetrics:
    """image_quality.rs:14-24, plus the overlay picture the reference only
    writes to disk and the number of points that passed the filter."""
    psnr: float
    ssim: float
    overlay: object = None  # (H, W, 3) uint8 device tensor
    n_kept: int = 0


def _as_rgb8(image) -> torch.Tensor:
    img = image if isinstance(image, torch.Tensor) else torch.as_tensor(image)
    if img.dim() != 3 or img.shape[2] != 3 or img.shape[0] == 0 or img.shape[1] == 0:
        raise UtilError("expected a non-empty (H, W, 3) RGB8 image")
    return img.to("cuda", torch.uint8).contiguous()


def _rgb(color):
    c = [int(v) for v in color]
    if len(c) != 3 or any(v < 0 or v > 255 for v in c):
        raise UtilError("a colour is three bytes (r, g, b)")
    return (ctypes.c_uint8 * 3)(*c)


def _image_size(width, height):
    w, h = int(width), int(height)
    if w <= 0 or h <= 0:
        raise UtilError("width and height must be positive")
    return w, h


def image_quality_sums(img1, img2, ssim_map: bool = False):
    """acm_image_quality's raw result: (sse, valid, ssim_sum, ssim_count,
    per-pixel SSIM map or None) -- the two integer sums of PSNR, the sum and
    the number of the SSIM terms (include/acm.h)."""
    import struct
    L = _lib.load()
    a, b = _as_rgb8(img1), _as_rgb8(img2)
    if a.shape != b.shape:  # :46-50, :109-113
        raise UtilError("Images must have the same dimensions")
    h, w = a.shape[0], a.shape[1]
    res = torch.empty((4,), dtype=torch.int64, device=a.device)
    smap = None
    if ssim_map:
        smap = torch.empty((max(h - 2, 0), max(w - 2, 0)), dtype=torch.float64, device=a.device)
    ws_bytes = L.acm_image_quality_workspace_size(w, h)
    ws = _workspace(ws_bytes, a.device)
    _lib.check(L.acm_image_quality(w, h, a.data_ptr(), b.data_ptr(), res.data_ptr(),
                                   smap.data_ptr() if smap is not None and smap.numel() else None,
                                   ws.data_ptr(), ws_bytes, _stream_handle()))
    sse, valid, ssim_sum, count = struct.unpack("<QQdQ", struct.pack("<4q", *res.cpu().tolist()))
    return sse, valid, ssim_sum, count, smap


def image_quality(img1, img2):
    """(psnr, ssim) of two images: one acm_image_quality launch, one 32-B
    read, the reference's closing arithmetic on the host
    (acm_image_quality_finish)."""
    import struct
    sse, valid, ssim_sum, count, _ = image_quality_sums(img1, img2)
    psnr, ssim = ctypes.c_double(), ctypes.c_double()
    _lib.check(_lib.load().acm_image_quality_finish(
        struct.pack("<QQdQ", sse, valid, ssim_sum, count), ctypes.byref(psnr),
        ctypes.byref(ssim)))
    return psnr.value, ssim.value


def calculate_psnr(img1, img2) -> float:
    """`calculate_psnr` (:45-89): dB, +inf for a perfect match; pixel pairs
    that are black in both images are skipped."""
    return image_quality(img1, img2)[0]


def calculate_ssim(img1, img2) -> float:
    """`calculate_ssim` (:108-210): mean 3 x 3-window SSIM of the gray images
    over the interior pixels, 1.0 when there are none."""
    return image_quality(img1, img2)[1]


def raster_points(projections, width: int, height: int, out=None) -> torch.Tensor:
    """The (H, W) uint8 mask of radius-2 discs around `projections` (N, 2)
    (:353-369).  out: an existing mask to OR into (ACM_RASTER_ACCUMULATE)."""
    L = _lib.load()
    w, h = _image_size(width, height)
    p2 = _as_device_f64(projections, 2)
    n = p2.shape[0]
    mask = out if out is not None else torch.empty((h, w), dtype=torch.uint8, device=p2.device)
    ws_bytes = L.acm_projection_masks_workspace_size(w, h)
    ws = _workspace(ws_bytes, p2.device)
    _lib.check(L.acm_raster_points(w, h, n, p2.data_ptr() if n else None,
                                   _lib.RASTER_ACCUMULATE if out is not None else 0,
                                   mask.data_ptr(), ws.data_ptr(), ws_bytes, _stream_handle()))
    return mask


def projection_masks(input_model: CameraModel, output_model: CameraModel, points_3d,
                     width: int, height: int, layout: str = "aos", out=None,
                     exact_all: bool = False):
    """The fused per-point pass of compute_image_quality_metrics (:272-293 and
    the two comparison rasters, :314-317): (input_mask, output_mask, n_kept)
    -- two (H, W) uint8 device masks and a one-element int64 device tensor.
    layout "soa": points_3d is (3, N).  out: the triple of an earlier call to
    accumulate into (another chunk of the same point set).  exact_all:
    ACM_RASTER_EXACT_ALL (every point projected exactly instead of only those
    in the guard band of a decision; the same masks)."""
    L = _lib.load()
    w, h = _image_size(width, height)
    if layout == "soa":
        p3 = points_3d if isinstance(points_3d, torch.Tensor) else torch.as_tensor(points_3d)
        p3 = p3.to("cuda", torch.float64).reshape(3, -1).contiguous()
        n = p3.shape[1]
    else:
        p3 = _as_device_f64(points_3d, 3)
        n = p3.shape[0]
    if out is not None:
        m_in, m_out, kept = out
    else:
        m_in = torch.empty((h, w), dtype=torch.uint8, device=p3.device)
        m_out = torch.empty((h, w), dtype=torch.uint8, device=p3.device)
        kept = torch.empty((1,), dtype=torch.int64, device=p3.device)
    ws_bytes = L.acm_projection_masks_workspace_size(w, h)
    ws = _workspace(ws_bytes, p3.device)
    ci, co = input_model.acm_camera(), output_model.acm_camera()
    _lib.check(L.acm_projection_masks(
        ctypes.byref(ci), ctypes.byref(co), w, h, n, p3.data_ptr() if n else None,
        _lib.LAYOUT_SOA if layout == "soa" else _lib.LAYOUT_AOS,
        (_lib.RASTER_ACCUMULATE if out is not None else 0) |
        (_lib.RASTER_EXACT_ALL if exact_all else 0), m_in.data_ptr(), m_out.data_ptr(),
        kept.data_ptr(), ws.data_ptr(), ws_bytes, _stream_handle()))
    return m_in, m_out, kept


def compose_projection_image(width: int, height: int, input_mask=None, output_mask=None,
                             input_color=GREEN, output_color=MAGENTA,
                             background=None) -> torch.Tensor:
    """output_color where output_mask is set, else input_color where
    input_mask is set, else the background (None: black) -- the result of
    drawing all input discs and then all output discs (:388-510)."""
    w, h = _image_size(width, height)
    bg = None
    if background is not None:
        bg = _as_rgb8(background)
        if bg.shape[0] != h or bg.shape[1] != w:
            raise UtilError("the background must be (height, width, 3)")
    img = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.load().acm_compose_projection_image(
        w, h, input_mask.data_ptr() if input_mask is not None else None,
        output_mask.data_ptr() if output_mask is not None else None, _rgb(input_color),
        _rgb(output_color), bg.data_ptr() if bg is not None else None, img.data_ptr(),
        _stream_handle()))
    return img


def create_projection_image(projections, color, width: int, height: int) -> torch.Tensor:
    """`create_projection_image` (:338-373): discs of ONE colour on black.
    The reference takes a colour per point; every caller passes a uniform
    list, and per-point colours would make the picture depend on the order
    of the points, so this takes the one colour."""
    mask = raster_points(projections, width, height)
    return compose_projection_image(width, height, input_mask=mask, input_color=color)


def create_combined_projection_image(input_projections, output_projections, width: int,
                                     height: int) -> torch.Tensor:
    """`create_combined_projection_image` (:454-510): input discs green,
    then output discs magenta, on black."""
    return compose_projection_image(width, height,
                                    raster_points(input_projections, width, height),
                                    raster_points(output_projections, width, height))


def create_combined_projection_image_on_reference(input_projections, output_projections,
                                                  reference_image) -> torch.Tensor:
    """`create_combined_projection_image_on_reference` (:388-438): the same
    on a copy of the reference image."""
    ref = _as_rgb8(reference_image)
    h, w = ref.shape[0], ref.shape[1]
    return compose_projection_image(w, h, raster_points(input_projections, w, h),
                                    raster_points(output_projections, w, h), background=ref)


def _png_bytes(image) -> bytes:
    """8-bit RGB PNG of an (H, W, 3) uint8 array: filter type 0 on every row,
    one zlib stream (standard library only)."""
    import struct
    import zlib
    img = image.cpu().numpy() if isinstance(image, torch.Tensor) else image
    if img.ndim != 3 or img.shape[2] != 3 or str(img.dtype) != "uint8":
        raise UtilError("expected an (H, W, 3) uint8 image")
    h, w = int(img.shape[0]), int(img.shape[1])
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return (struct.pack(">I", len(data)) + tag + data +
                struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF))
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def write_png(path: str, image) -> None:
    with open(path, "wb") as f:
        f.write(_png_bytes(image))


def save_model_projection_image(image, model_name: str, output_dir: str = "output") -> str:
    """`save_model_projection_image` (:526-539): writes
    <output_dir>/<lowercased name, spaces as underscores>_projection.png and
    returns the path (the reference always writes under output/)."""
    import os
    try:
        os.makedirs(output_dir, exist_ok=True)
        path = os.path.join(output_dir,
                            model_name.lower().replace(" ", "_") + "_projection.png")
        write_png(path, image)
    except OSError as e:
        raise UtilError(f"Failed to save projection image: {e}") from e
    return path


def load_image(image_path: str) -> torch.Tensor:
    """`load_image` (:225-230): the file as an (H, W, 3) uint8 host tensor.
    Decoding uses Pillow when it is importable; UtilError otherwise."""
    try:
        from PIL import Image
    except ImportError as e:
        raise UtilError("load_image needs Pillow to decode image files") from e
    import numpy as np
    try:
        with Image.open(image_path) as im:
            arr = np.array(im.convert("RGB"), dtype=np.uint8)
    except Exception as e:  # noqa: BLE001  (:226-227: any failure is InvalidParams)
        raise UtilError(f"Failed to load image: {e}") from e
    return torch.from_numpy(arr)


def compute_image_quality_metrics(input_model: CameraModel, output_model: CameraModel,
                                  points_3d, output_model_name: str = None,
                                  reference_image=None,
                                  output_dir: str = None) -> ImageQualityMetrics:
    """`compute_image_quality_metrics` (:252-324).  The optimisation points go
    through both models in one fused kernel (acm_projection_masks) that keeps
    a point iff both projections are Ok and the output pixel lies in the
    image -- the reference image's size when one is given, else the input
    model's resolution -- and rasterises both pixel sets; PSNR / SSIM compare
    the two white-on-black rasters, and the overlay (input green, output
    magenta, on the reference image or black) is returned in the result.

    The reference always writes the overlay to output/<name>_projection.png;
    here a file is written only when output_dir is given (the name then
    follows :530-531; output_model_name defaults to the model's own name).
    Raises ZeroProjectionPoints when no point is kept (:295-297)."""
    ref = None
    if reference_image is not None:
        ref = _as_rgb8(reference_image)
        h, w = ref.shape[0], ref.shape[1]  # :260-261
    else:
        res = input_model.get_resolution()
        w, h = _image_size(res.width, res.height)  # :263-264
    m_in, m_out, kept = projection_masks(input_model, output_model, points_3d, w, h)
    white_in = compose_projection_image(w, h, input_mask=m_in, input_color=WHITE)
    white_out = compose_projection_image(w, h, input_mask=m_out, input_color=WHITE)
    overlay = compose_projection_image(w, h, m_in, m_out, background=ref)
    n_kept = int(kept.item())
    if n_kept == 0:
        raise ZeroProjectionPoints()
    if output_dir is not None:
        save_model_projection_image(overlay, output_model_name or output_model.get_model_name(),
                                    output_dir)
    psnr, ssim = image_quality(white_in, white_out)
    return ImageQualityMetrics(psnr=psnr, ssim=ssim, overlay=overlay, n_kept=n_kept)


def model_projection_visualization(points_2d, model_name: str, reference_image=None,
                                   camera_resolution=None, output_dir: str = None) -> torch.Tensor:
    """`model_projection_visualization` (:556-616): the pixels as green discs
    on the reference image, or on black at camera_resolution = (width,
    height).  Returns the picture; with output_dir it is also written to
    <output_dir>/<lowercased name>_projection.png (:609; the reference always
    writes under output/)."""
    if reference_image is not None:
        ref = _as_rgb8(reference_image)
        h, w = ref.shape[0], ref.shape[1]
        img = compose_projection_image(w, h, input_mask=raster_points(points_2d, w, h),
                                       background=ref)
    else:
        if camera_resolution is None:
            raise UtilError("camera_resolution is needed without a reference image")
        w, h = camera_resolution
        img = create_projection_image(points_2d, GREEN, w, h)
    if output_dir is not None:
        import os
        try:
            os.makedirs(output_dir, exist_ok=True)
            write_png(os.path.join(output_dir, model_name.lower() + "_projection.png"), img)
        except OSError as e:
            raise UtilError(f"Failed to save projection image: {e}") from e
    return img
