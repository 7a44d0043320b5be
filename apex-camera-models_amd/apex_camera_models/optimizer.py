"""Levenberg-Marquardt model conversion (the apex-solver call sites of
bin/camera_converter.rs:381-420, :516-557, :655-698, :797-832, :928-965),
driven by libacm.so's C++ LM (csrc/solver.hip) over the fused GPU normal
equations.

`LevenbergMarquardtConfig` keeps apex-solver's builder surface
(`with_max_iterations`, `with_cost_tolerance`, ...).  For multi-GPU runs pass
`collective=distributed.make_collective(group)`: each rank holds its shard of
the correspondences and the (<= 92-double) normal-equation vector is summed
across ranks before every host solve (RCCL from C under the nccl backend).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional, Sequence, Tuple

import torch

from . import _lib
from .camera import CameraModel, _as_device_f64, _stream_handle


@dataclass
class LevenbergMarquardtConfig:
    max_iterations: int = 100
    cost_tolerance: float = 1e-6
    parameter_tolerance: float = 1e-8
    gradient_tolerance: float = 1e-6
    initial_damping: float = 1e-4
    invalid_policy: int = _lib.INVALID_SKIP

    def with_max_iterations(self, v):
        self.max_iterations = int(v)
        return self

    def with_cost_tolerance(self, v):
        self.cost_tolerance = float(v)
        return self

    def with_parameter_tolerance(self, v):
        self.parameter_tolerance = float(v)
        return self

    def with_gradient_tolerance(self, v):
        self.gradient_tolerance = float(v)
        return self

    def with_verbose(self, _v):
        return self


@dataclass
class LmResult:
    parameters: list
    iterations: int
    termination: str
    evaluations: int
    initial_cost: float
    final_cost: float
    n_valid: int


# camera_converter.rs set_variable_bounds per target model (index -> (lo, hi))
_INTR = {0: (1.0, 2000.0), 1: (1.0, 2000.0), 2: (0.0, 2000.0), 3: (0.0, 2000.0)}
CONVERTER_BOUNDS: Dict[str, Dict[int, Tuple[float, float]]] = {
    "double_sphere": {**_INTR, 4: (1e-6, 1.0), 5: (-5.0, 5.0)},          # :395-400
    "kannala_brandt": {**_INTR, 4: (-5.0, 5.0), 5: (-5.0, 5.0), 6: (-5.0, 5.0),
                       7: (-5.0, 5.0)},                                     # :536-543
    "rad_tan": {**_INTR, 4: (-5.0, 5.0), 5: (-5.0, 5.0), 6: (-1.0, 1.0), 7: (-1.0, 1.0),
                8: (-5.0, 5.0)},                                            # :676-684
    "ucm": {**_INTR, 4: (1e-6, 10.0)},                                      # :813-817
    "eucm": {**_INTR, 4: (1e-6, 1.0), 5: (1e-6, 5.0)},                      # :945-950
    "fov": {**_INTR, 4: (1e-6, 3.0)},                                       # :1076-1080
}


class LevenbergMarquardt:
    def __init__(self, config: Optional[LevenbergMarquardtConfig] = None):
        self.config = config or LevenbergMarquardtConfig()

    @classmethod
    def with_config(cls, config):
        return cls(config)

    def optimize(self, model: CameraModel, points_3d, points_2d,
                 bounds: Optional[Dict[int, Tuple[float, float]]] = None,
                 allreduce: Optional[Callable] = None, collective=None,
                 cells=None) -> LmResult:
        """Optimise model's factor-order parameters in place over the
        (local shard of the) correspondences.  collective (r06; e.g.
        distributed.RcclCollective): its all-reduce sums the normal
        equations of every evaluation across the ranks, from C; allreduce:
        a bare Python callback (acm_allreduce_fn) instead.  cells (r06):
        the util.CellSample of points_2d (grid-sampled correspondences):
        every evaluation reads the 4-B cells instead of the pixels
        (acm_lm_optimize_cells; the same iterates)."""
        L = _lib.load()
        p3 = _as_device_f64(points_3d, 3)
        p2 = _as_device_f64(points_2d, 2)
        n = p3.shape[0]
        cfg = _lib.LmConfig()
        L.acm_lm_default_config(ctypes.byref(cfg))
        c = self.config
        cfg.max_iterations = c.max_iterations
        cfg.cost_tolerance = c.cost_tolerance
        cfg.parameter_tolerance = c.parameter_tolerance
        cfg.gradient_tolerance = c.gradient_tolerance
        cfg.initial_damping = c.initial_damping
        cfg.invalid_policy = c.invalid_policy
        if bounds:
            cfg.has_bounds = 1
            for k, (lo, hi) in bounds.items():
                cfg.lower[k] = lo
                cfg.upper[k] = hi
        ws_bytes = L.acm_lm_workspace_size(model.MODEL_ID, n)
        ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device=p3.device)
        cam = model.acm_camera()
        summ = _lib.LmSummary()
        ctx = None
        if collective is not None:
            cb, ctx = collective.c.allreduce, collective.c.ctx
        elif allreduce is not None:
            cb = _lib.ALLREDUCE_FN(allreduce)
        else:
            cb = _lib.ALLREDUCE_FN()
        if cells is not None:
            if cells.cells.shape[0] != n:
                raise ValueError("cells and points_3d must have the same number of points")
            _lib.check(L.acm_lm_optimize_cells(ctypes.byref(cam), n, p3.data_ptr() if n else None,
                                               _lib.LAYOUT_AOS,
                                               cells.cells.data_ptr() if n else None,
                                               ctypes.byref(cells.grid), ctypes.byref(cfg), cb,
                                               ctx, ctypes.byref(summ), ws.data_ptr(), ws_bytes,
                                               _stream_handle()))
        else:
            _lib.check(L.acm_lm_optimize(ctypes.byref(cam), n, p3.data_ptr() if n else None,
                                         _lib.LAYOUT_AOS, p2.data_ptr() if n else None,
                                         ctypes.byref(cfg), cb, ctx,
                                         ctypes.byref(summ), ws.data_ptr(), ws_bytes,
                                         _stream_handle()))
        params = list(cam.params)[: model.NUM_PARAMS]
        model._set_params(params)
        return LmResult(parameters=params, iterations=summ.iterations,
                        termination=_lib.LM_TERMINATION.get(summ.termination, "?"),
                        evaluations=summ.evaluations, initial_cost=summ.initial_cost,
                        final_cost=summ.final_cost, n_valid=int(summ.n_valid))


class Pose:
    """World -> camera rigid transform, p_cam = R p_world + t (acm_pose):
    `rotation` a 3x3 nested list (row-major), `translation` a 3-list."""

    def __init__(self, rotation=None, translation=None):
        rot = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]] if rotation is None else rotation
        flat = [float(v) for row in rot for v in (row if hasattr(row, "__len__") else [row])]
        if len(flat) != 9:
            raise ValueError("rotation must be 3x3")
        tr = [0.0, 0.0, 0.0] if translation is None else [float(v) for v in translation]
        if len(tr) != 3:
            raise ValueError("translation must have 3 entries")
        self.rotation = [flat[0:3], flat[3:6], flat[6:9]]
        self.translation = tr

    def acm_pose(self) -> _lib.AcmPose:
        p = _lib.AcmPose()
        for k in range(9):
            p.r[k] = self.rotation[k // 3][k % 3]
        for k in range(3):
            p.t[k] = self.translation[k]
        return p

    @classmethod
    def _from_acm(cls, p: _lib.AcmPose) -> "Pose":
        return cls([list(p.r[0:3]), list(p.r[3:6]), list(p.r[6:9])], list(p.t))

    def retract(self, delta: Sequence[float]) -> "Pose":
        """The pose moved by the left perturbation delta = (rho, phi):
        R <- Exp(phi) R, t <- Exp(phi) t + rho (acm_pose_retract)."""
        if len(delta) != 6:
            raise ValueError("delta must have 6 entries (rho, phi)")
        p = self.acm_pose()
        d = (ctypes.c_double * 6)(*[float(v) for v in delta])
        _lib.check(_lib.load().acm_pose_retract(ctypes.byref(p), d))
        return Pose._from_acm(p)


def refine_pose(model: CameraModel, pose: Pose, points_world, points_2d,
                config: Optional[LevenbergMarquardtConfig] = None, collective=None,
                allreduce: Optional[Callable] = None,
                bounds: Optional[Dict[int, Tuple[float, float]]] = None) -> Tuple[Pose, LmResult]:
    """6-DoF pose refinement of a calibrated camera over the fused GPU pose
    normal equations (acm_pose_optimize): minimises sum ||project(R X + t) -
    obs||^2 from `pose`.  Points that do not project, or whose observation is
    NaN, are skipped.  collective / allreduce as LevenbergMarquardt.optimize
    (the 44-double vector of every evaluation is summed across the ranks).
    A local perturbation has no box: bounds raise."""
    L = _lib.load()
    p3 = _as_device_f64(points_world, 3)
    p2 = _as_device_f64(points_2d, 2)
    n = p3.shape[0]
    if p2.shape[0] != n:
        raise ValueError("points_world and points_2d must have the same number of points")
    cfg = _lib.LmConfig()
    L.acm_lm_default_config(ctypes.byref(cfg))
    c = config or LevenbergMarquardtConfig()
    cfg.max_iterations = c.max_iterations
    cfg.cost_tolerance = c.cost_tolerance
    cfg.parameter_tolerance = c.parameter_tolerance
    cfg.gradient_tolerance = c.gradient_tolerance
    cfg.initial_damping = c.initial_damping
    if bounds:
        cfg.has_bounds = 1  # rejected by the library (ACM_ERR_INVALID_ARGUMENT)
    ws_bytes = L.acm_pose_optimize_workspace_size(n)
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device=p3.device)
    cam = model.acm_camera()
    ap = pose.acm_pose()
    summ = _lib.LmSummary()
    ctx = None
    if collective is not None:
        cb, ctx = collective.c.allreduce, collective.c.ctx
    elif allreduce is not None:
        cb = _lib.ALLREDUCE_FN(allreduce)
    else:
        cb = _lib.ALLREDUCE_FN()
    _lib.check(L.acm_pose_optimize(ctypes.byref(cam), ctypes.byref(ap), n,
                                   p3.data_ptr() if n else None, _lib.LAYOUT_AOS,
                                   p2.data_ptr() if n else None, ctypes.byref(cfg), cb, ctx,
                                   ctypes.byref(summ), ws.data_ptr(), ws_bytes, _stream_handle()))
    return Pose._from_acm(ap), LmResult(
        parameters=list(ap.r) + list(ap.t), iterations=summ.iterations,
        termination=_lib.LM_TERMINATION.get(summ.termination, "?"),
        evaluations=summ.evaluations, initial_cost=summ.initial_cost,
        final_cost=summ.final_cost, n_valid=int(summ.n_valid))


# ------------------------------------------------------------ triangulation
@dataclass
class TriangulationConfig:
    """acm_triangulate_config; the defaults are acm_triangulate_default_config's."""
    max_iterations: int = 20
    cost_tolerance: float = 1e-6
    parameter_tolerance: float = 1e-8
    gradient_tolerance: float = 1e-6
    initial_damping: float = 1e-4
    min_parallax_sin2: float = 1e-8


@dataclass
class TriangulationResult:
    """Device tensors, one row per point: points (N, 3) f64, status (N,) u8
    (_lib.TRI_OK / TRI_TOO_FEW_OBSERVATIONS / TRI_DEGENERATE /
    TRI_NOT_CONVERGED), cost (N,) f64, n_valid (N,) i32, information (N, 6)
    f64 -- the upper triangle of J^T J, row by row -- or None."""
    points: torch.Tensor
    status: torch.Tensor
    cost: torch.Tensor
    n_valid: torch.Tensor
    information: Optional[torch.Tensor]


def _poses_tensor(poses) -> torch.Tensor:
    """(K, 12) device f64, acm_pose's layout: R row-major, then t."""
    if isinstance(poses, torch.Tensor):
        t = poses
        if t.device.type != "cuda":
            t = t.to("cuda")
        return t.to(torch.float64).reshape(-1, 12).contiguous()
    rows = [[v for row in p.rotation for v in row] + list(p.translation) for p in poses]
    return torch.tensor(rows, dtype=torch.float64, device="cuda").reshape(-1, 12)


def tracks_from_dense(observations):
    """CSR tracks of a dense observation tensor [K, N, 2] (view, point, uv):
    entries with a NaN coordinate are dropped.  Returns (track_offsets (N + 1,)
    int64, obs_view (M,) int32, obs_uv (M, 2) float64) on the device, each
    point's observations in view order."""
    obs = observations if isinstance(observations, torch.Tensor) else torch.as_tensor(observations)
    if obs.device.type != "cuda":
        obs = obs.to("cuda")
    obs = obs.to(torch.float64)
    if obs.dim() != 3 or obs.shape[2] != 2:
        raise ValueError("observations must be [K, N, 2]")
    per_point = obs.permute(1, 0, 2)                      # (N, K, 2)
    seen = ~torch.isnan(per_point).any(dim=2)             # (N, K)
    offsets = torch.zeros(per_point.shape[0] + 1, dtype=torch.int64, device=obs.device)
    offsets[1:] = torch.cumsum(seen.sum(dim=1), dim=0)
    idx = torch.nonzero(seen)                             # row-major: point, then view
    return offsets, idx[:, 1].to(torch.int32).contiguous(), per_point[seen].contiguous()


def triangulate(model: CameraModel, poses, track_offsets, obs_view, obs_uv, initial=None,
                config: Optional[TriangulationConfig] = None,
                want_information: bool = False) -> TriangulationResult:
    """Batched multi-view triangulation (acm_triangulate): one 3-D point per
    track from known world -> camera poses, by the midpoint of the unprojected
    rays refined with a per-point Levenberg-Marquardt on the reprojection
    error.  poses: a sequence of Pose or a (K, 12) tensor; track_offsets
    (N + 1,) int64, obs_view (M,) int32, obs_uv (M, 2) f64: the CSR tracks
    (tracks_from_dense builds them).  initial (N, 3): start the refinement
    there instead of at the midpoint (ACM_TRI_USE_INITIAL); the caller's
    tensor is not modified."""
    L = _lib.load()
    pt = _poses_tensor(poses)
    offs = torch.as_tensor(track_offsets).to(device="cuda", dtype=torch.int64).contiguous()
    view = torch.as_tensor(obs_view).to(device="cuda", dtype=torch.int32).contiguous()
    uv = _as_device_f64(obs_uv, 2)
    n = offs.shape[0] - 1
    m = view.shape[0]
    if n < 0 or uv.shape[0] != m:
        raise ValueError("track_offsets needs N + 1 entries; obs_view and obs_uv one row per observation")
    c = config or TriangulationConfig()
    cfg = _lib.TriangulateConfig()
    L.acm_triangulate_default_config(ctypes.byref(cfg))
    cfg.max_iterations = c.max_iterations
    cfg.cost_tolerance = c.cost_tolerance
    cfg.parameter_tolerance = c.parameter_tolerance
    cfg.gradient_tolerance = c.gradient_tolerance
    cfg.initial_damping = c.initial_damping
    cfg.min_parallax_sin2 = c.min_parallax_sin2
    if initial is not None:
        cfg.flags = _lib.TRI_USE_INITIAL
        points = _as_device_f64(initial, 3).clone()
        if points.shape[0] != n:
            raise ValueError("initial must have one row per point")
    else:
        points = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    status = torch.empty((n,), dtype=torch.uint8, device="cuda")
    cost = torch.empty((n,), dtype=torch.float64, device="cuda")
    n_valid = torch.empty((n,), dtype=torch.int32, device="cuda")
    info = torch.empty((n, 6), dtype=torch.float64, device="cuda") if want_information else None
    ws_bytes = L.acm_triangulate_workspace_size(n, m)
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device="cuda")
    cam = model.acm_camera()
    _lib.check(L.acm_triangulate(ctypes.byref(cam), pt.shape[0], pt.data_ptr(), n, offs.data_ptr(),
                                 m, view.data_ptr() if m else None, uv.data_ptr() if m else None,
                                 ctypes.byref(cfg), points.data_ptr() if n else None,
                                 status.data_ptr() if n else None, cost.data_ptr() if n else None,
                                 n_valid.data_ptr() if n else None,
                                 info.data_ptr() if info is not None and n else None,
                                 ws.data_ptr(), ws_bytes, _stream_handle()))
    return TriangulationResult(points, status, cost, n_valid, info)


# ------------------------------------------------- batched pose refinement
@dataclass
class PoseBatchConfig:
    """acm_pose_batch_config; the defaults are acm_pose_optimize_batch_default_config's."""
    max_iterations: int = 20
    cost_tolerance: float = 1e-6
    parameter_tolerance: float = 1e-8
    gradient_tolerance: float = 1e-6
    initial_damping: float = 1e-4


@dataclass
class PoseBatchResult:
    """Device tensors, one row per view: poses (K, 12) f64 (R row-major, then
    t), status (K,) u8 (_lib.POSE_OK / POSE_TOO_FEW_OBSERVATIONS /
    POSE_NOT_CONVERGED), cost (K,) f64, n_valid (K,) i32, iterations (K,) i32,
    information (K, 21) f64 -- the upper triangle of J^T J, row by row -- or
    None."""
    poses: torch.Tensor
    status: torch.Tensor
    cost: torch.Tensor
    n_valid: torch.Tensor
    iterations: torch.Tensor
    information: Optional[torch.Tensor]


def tracks_by_view(track_offsets, obs_view, obs_uv, n_views):
    """The view-major CSR of point-major tracks (track_offsets (N + 1,),
    obs_view (M,), obs_uv (M, 2), as acm_triangulate takes them): returns
    (view_offsets (K + 1,) int64, obs_point (M',) int32, obs_uv (M', 2) f64) on
    the inputs' device.  A stable sort on the view index, so each view's
    observations are in ascending point order (and in track order within a
    point); observations whose view index is outside [0, n_views) are
    dropped."""
    offs = torch.as_tensor(track_offsets).to(torch.int64)
    dev = offs.device
    view = torch.as_tensor(obs_view).to(device=dev, dtype=torch.int64)
    uv = torch.as_tensor(obs_uv).to(device=dev, dtype=torch.float64).reshape(-1, 2)
    m = view.shape[0]
    n = offs.shape[0] - 1
    if n < 0 or uv.shape[0] != m:
        raise ValueError("track_offsets needs N + 1 entries; obs_view and obs_uv one row per observation")
    k = int(n_views)
    # the point of observation j: the track whose [begin, end) holds j
    j = torch.arange(m, dtype=torch.int64, device=dev)
    point = torch.searchsorted(offs[1:].contiguous(), j, right=True)
    keep = (view >= 0) & (view < k) & (point < n) & (j >= offs[0])
    view, point, uv = view[keep], point[keep], uv[keep]
    order = torch.sort(view, stable=True).indices
    view_offsets = torch.zeros(k + 1, dtype=torch.int64, device=dev)
    if k:
        view_offsets[1:] = torch.cumsum(torch.bincount(view, minlength=k)[:k], dim=0)
    return view_offsets, point[order].to(torch.int32).contiguous(), uv[order].contiguous()


def refine_poses(model: CameraModel, poses, points_world, view_offsets, obs_point, obs_uv,
                 config: Optional[PoseBatchConfig] = None,
                 want_information: bool = False) -> PoseBatchResult:
    """Batched 6-DoF pose refinement (acm_pose_optimize_batch): every view's
    pose from known world points, one Levenberg-Marquardt per view, all in one
    launch.  poses: a sequence of Pose or a (K, 12) tensor (not modified);
    points_world (N, 3); view_offsets (K + 1,) int64, obs_point (M,) int32,
    obs_uv (M, 2) f64: the observations by view (tracks_by_view builds them
    from tracks).  Non-finite points (triangulate's failures) are skipped."""
    L = _lib.load()
    pt = _poses_tensor(poses).clone()
    pw = _as_device_f64(points_world, 3)
    offs = torch.as_tensor(view_offsets).to(device="cuda", dtype=torch.int64).contiguous()
    idx = torch.as_tensor(obs_point).to(device="cuda", dtype=torch.int32).contiguous()
    uv = _as_device_f64(obs_uv, 2)
    k, n, m = pt.shape[0], pw.shape[0], idx.shape[0]
    if offs.shape[0] != k + 1 or uv.shape[0] != m:
        raise ValueError("view_offsets needs K + 1 entries; obs_point and obs_uv one row per observation")
    c = config or PoseBatchConfig()
    cfg = _lib.PoseBatchConfig()
    L.acm_pose_optimize_batch_default_config(ctypes.byref(cfg))
    cfg.max_iterations = c.max_iterations
    cfg.cost_tolerance = c.cost_tolerance
    cfg.parameter_tolerance = c.parameter_tolerance
    cfg.gradient_tolerance = c.gradient_tolerance
    cfg.initial_damping = c.initial_damping
    status = torch.empty((k,), dtype=torch.uint8, device="cuda")
    cost = torch.empty((k,), dtype=torch.float64, device="cuda")
    n_valid = torch.empty((k,), dtype=torch.int32, device="cuda")
    iters = torch.empty((k,), dtype=torch.int32, device="cuda")
    info = torch.empty((k, 21), dtype=torch.float64, device="cuda") if want_information else None
    ws_bytes = L.acm_pose_optimize_batch_workspace_size(k, m)
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device="cuda")
    cam = model.acm_camera()
    _lib.check(L.acm_pose_optimize_batch(
        ctypes.byref(cam), k, pt.data_ptr() if k else None, n, pw.data_ptr() if n else None,
        offs.data_ptr(), m, idx.data_ptr() if m else None, uv.data_ptr() if m else None,
        ctypes.byref(cfg), status.data_ptr() if k else None, cost.data_ptr() if k else None,
        n_valid.data_ptr() if k else None, iters.data_ptr() if k else None,
        info.data_ptr() if info is not None and k else None, ws.data_ptr(), ws_bytes,
        _stream_handle()))
    return PoseBatchResult(pt, status, cost, n_valid, iters, info)


def alternate_bundle_adjustment(model: CameraModel, poses, track_offsets, obs_view, obs_uv,
                                sweeps: int, fixed_views: Sequence[int] = (0,),
                                initial_points=None):
    """Alternating bundle adjustment from the two batched launches:
    triangulate, then `sweeps` x (refine_poses, triangulate from the previous
    points), all on the device with no per-view Python.  The poses of
    fixed_views (the gauge) are restored after every pose step, and the cost
    of that step is evaluated at the restored poses (max_iterations = 0).  A
    point that triangulate could not solve stays NaN and is skipped by both
    halves.  Returns (poses (K, 12), the last TriangulationResult, costs) with
    costs the total cost (0-d device tensors; the NaN costs of unsolved points
    / views left out) after every half step: 1 + 2 sweeps entries."""
    pt = _poses_tensor(poses).clone()
    start = pt.clone()
    fixed = torch.as_tensor(list(fixed_views), dtype=torch.int64, device=pt.device)
    offs = torch.as_tensor(track_offsets).to(device="cuda", dtype=torch.int64)
    view = torch.as_tensor(obs_view).to(device="cuda", dtype=torch.int32)
    uv = _as_device_f64(obs_uv, 2)
    view_offsets, obs_point, view_uv = tracks_by_view(offs, view, uv, pt.shape[0])
    evaluate = PoseBatchConfig(max_iterations=0)
    tri = triangulate(model, pt, offs, view, uv, initial=initial_points)
    costs = [torch.nansum(tri.cost)]
    for _ in range(int(sweeps)):
        pt = refine_poses(model, pt, tri.points, view_offsets, obs_point, view_uv).poses
        pt[fixed] = start[fixed]
        at = refine_poses(model, pt, tri.points, view_offsets, obs_point, view_uv, evaluate)
        costs.append(torch.nansum(at.cost))
        tri = triangulate(model, pt, offs, view, uv, initial=tri.points)
        costs.append(torch.nansum(tri.cost))
    return pt, tri, costs


# ------------------------------------------------ absolute pose from scratch
def p3p(bearings, points_world):
    """The minimal absolute-pose solver (acm_p3p), batched: bearings (N, 3, 3)
    -- f1, f2, f3 per triplet, any length -- and points_world (N, 3, 3).
    Returns (poses (N, 4, 12) f64 -- R row-major, then t; NaN beyond the count
    --, count (N,) u8) on the device."""
    L = _lib.load()
    f = _as_device_f64(torch.as_tensor(bearings).reshape(-1, 3), 3)
    x = _as_device_f64(torch.as_tensor(points_world).reshape(-1, 3), 3)
    if f.shape[0] % 3 or f.shape[0] != x.shape[0]:
        raise ValueError("bearings and points_world must both be (N, 3, 3)")
    n = f.shape[0] // 3
    poses = torch.empty((n, 4, 12), dtype=torch.float64, device="cuda")
    count = torch.empty((n,), dtype=torch.uint8, device="cuda")
    _lib.check(L.acm_p3p(n, f.data_ptr() if n else None, x.data_ptr() if n else None,
                         poses.data_ptr() if n else None, count.data_ptr() if n else None,
                         _stream_handle()))
    return poses, count


@dataclass
class PoseEstimateConfig:
    """acm_pose_estimate_config; the defaults are
    acm_pose_estimate_batch_default_config's, except inlier_angle: None takes
    the angle of estimate_poses' threshold_px."""
    n_hypotheses: int = 256
    seed: int = 1
    inlier_angle: Optional[float] = None
    min_inliers: int = 4


@dataclass
class PoseEstimateResult:
    """Device tensors: poses (K, 12) f64 (R row-major, then t; NaN where
    status is not POSE_EST_OK), status (K,) u8 (_lib.POSE_EST_OK /
    POSE_EST_TOO_FEW_OBSERVATIONS / POSE_EST_NO_MODEL), n_inliers (K,) i32,
    n_usable (K,) i32, inlier_mask (M,) u8, one byte per observation."""
    poses: torch.Tensor
    status: torch.Tensor
    n_inliers: torch.Tensor
    n_usable: torch.Tensor
    inlier_mask: torch.Tensor


def estimate_poses(model: CameraModel, points_world, view_offsets, obs_point, obs_uv,
                   config: Optional[PoseEstimateConfig] = None, threshold_px: float = 3.0,
                   refine: bool = False,
                   refine_config: Optional[PoseBatchConfig] = None) -> PoseEstimateResult:
    """Every view's pose from 2-D / 3-D correspondences with no prior
    (acm_pose_estimate_batch): P3P on the unprojected rays inside RANSAC, one
    workgroup per view, all views in one launch.  Inputs as refine_poses
    without start poses (tracks_by_view's output feeds the call unchanged).
    Without config.inlier_angle the threshold is atan(threshold_px / min(fx,
    fy)).  refine: refine_poses from the estimated poses over the inliers only
    (the other observations get point index -1, one torch.where on the
    device); the views whose status is not POSE_EST_OK stay as they are."""
    import math
    L = _lib.load()
    pw = _as_device_f64(points_world, 3)
    offs = torch.as_tensor(view_offsets).to(device="cuda", dtype=torch.int64).contiguous()
    idx = torch.as_tensor(obs_point).to(device="cuda", dtype=torch.int32).contiguous()
    uv = _as_device_f64(obs_uv, 2)
    k, n, m = offs.shape[0] - 1, pw.shape[0], idx.shape[0]
    if k < 0 or uv.shape[0] != m:
        raise ValueError("view_offsets needs K + 1 entries; obs_point and obs_uv one row per observation")
    cam = model.acm_camera()
    c = config or PoseEstimateConfig()
    cfg = _lib.PoseEstimateConfig()
    L.acm_pose_estimate_batch_default_config(ctypes.byref(cfg))
    cfg.n_hypotheses = c.n_hypotheses
    cfg.seed = c.seed
    cfg.min_inliers = c.min_inliers
    cfg.inlier_angle = (c.inlier_angle if c.inlier_angle is not None
                        else math.atan(threshold_px / min(cam.params[0], cam.params[1])))
    poses = torch.empty((k, 12), dtype=torch.float64, device="cuda")
    status = torch.empty((k,), dtype=torch.uint8, device="cuda")
    n_inliers = torch.empty((k,), dtype=torch.int32, device="cuda")
    n_usable = torch.empty((k,), dtype=torch.int32, device="cuda")
    mask = torch.zeros((m,), dtype=torch.uint8, device="cuda")  # entries no view owns stay 0
    ws_bytes = L.acm_pose_estimate_batch_workspace_size(k, m)
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device="cuda")
    _lib.check(L.acm_pose_estimate_batch(
        ctypes.byref(cam), k, poses.data_ptr() if k else None, n, pw.data_ptr() if n else None,
        offs.data_ptr(), m, idx.data_ptr() if m else None, uv.data_ptr() if m else None,
        ctypes.byref(cfg), status.data_ptr() if k else None, n_inliers.data_ptr() if k else None,
        mask.data_ptr() if m else None, n_usable.data_ptr() if k else None, ws.data_ptr(),
        ws_bytes, _stream_handle()))
    if refine and k:
        kept = torch.where(mask != 0, idx, torch.full_like(idx, -1))
        poses = refine_poses(model, poses, pw, offs, kept, uv, refine_config).poses
    return PoseEstimateResult(poses, status, n_inliers, n_usable, mask)


# --------------------------------------------------- two-view relative pose
def relative_pose_8pt(bearings_a, bearings_b):
    """The 8-point relative-pose solver (acm_relative_pose_8pt), batched:
    bearings_a, bearings_b (N, 8, 3), the rays of eight matches in image A and
    in image B, any length.  Returns (poses (N, 12) f64 -- p_b = R p_a + t, R
    row-major, then the unit t --, essential (N, 9) f64 -- unit norm, signed
    as [t]x R --, n_front (N,) u8) on the device; NaN and 0 where it fails."""
    L = _lib.load()
    fa = _as_device_f64(torch.as_tensor(bearings_a).reshape(-1, 3), 3)
    fb = _as_device_f64(torch.as_tensor(bearings_b).reshape(-1, 3), 3)
    if fa.shape[0] % 8 or fa.shape[0] != fb.shape[0]:
        raise ValueError("bearings_a and bearings_b must both be (N, 8, 3)")
    n = fa.shape[0] // 8
    poses = torch.empty((n, 12), dtype=torch.float64, device="cuda")
    ess = torch.empty((n, 9), dtype=torch.float64, device="cuda")
    front = torch.empty((n,), dtype=torch.uint8, device="cuda")
    _lib.check(L.acm_relative_pose_8pt(n, fa.data_ptr() if n else None, fb.data_ptr() if n else None,
                                       poses.data_ptr() if n else None, ess.data_ptr() if n else None,
                                       front.data_ptr() if n else None, _stream_handle()))
    return poses, ess, front


@dataclass
class RelativePoseConfig:
    """acm_relative_pose_config; the defaults are
    acm_relative_pose_batch_default_config's, except inlier_angle: None takes
    the angle of estimate_relative_poses' threshold_px."""
    n_hypotheses: int = 512
    seed: int = 1
    inlier_angle: Optional[float] = None
    min_inliers: int = 8
    refit_rounds: int = 3


@dataclass
class RelativePoseResult:
    """Device tensors: poses (K, 12) f64 (camera A -> camera B, R row-major,
    then the unit t; NaN where status is not RELPOSE_OK), status (K,) u8
    (_lib.RELPOSE_OK / RELPOSE_TOO_FEW_MATCHES / RELPOSE_NO_MODEL), n_inliers
    (K,) i32, n_usable (K,) i32, inlier_mask (M,) u8, one byte per match."""
    poses: torch.Tensor
    status: torch.Tensor
    n_inliers: torch.Tensor
    n_usable: torch.Tensor
    inlier_mask: torch.Tensor


def estimate_relative_poses(model: CameraModel, pair_offsets, uv_a, uv_b,
                            config: Optional[RelativePoseConfig] = None,
                            threshold_px: float = 3.0) -> RelativePoseResult:
    """Every view pair's relative pose from 2-D / 2-D matches alone
    (acm_relative_pose_batch): the 8-point solver on the unprojected rays
    inside RANSAC with a refit over the inliers, one workgroup per pair, all
    pairs in one launch.  pair_offsets (K + 1,) int64: pair k owns the matches
    pair_offsets[k] .. pair_offsets[k + 1] - 1; uv_a, uv_b (M, 2): their pixels
    in image A and in image B of the pair.  Without config.inlier_angle the
    threshold is atan(threshold_px / min(fx, fy))."""
    import math
    L = _lib.load()
    offs = torch.as_tensor(pair_offsets).to(device="cuda", dtype=torch.int64).contiguous()
    ua = _as_device_f64(uv_a, 2)
    ub = _as_device_f64(uv_b, 2)
    k, m = offs.shape[0] - 1, ua.shape[0]
    if k < 0 or ub.shape[0] != m:
        raise ValueError("pair_offsets needs K + 1 entries; uv_a and uv_b one row per match")
    cam = model.acm_camera()
    c = config or RelativePoseConfig()
    cfg = _lib.RelativePoseConfig()
    L.acm_relative_pose_batch_default_config(ctypes.byref(cfg))
    cfg.n_hypotheses = c.n_hypotheses
    cfg.seed = c.seed
    cfg.min_inliers = c.min_inliers
    cfg.refit_rounds = c.refit_rounds
    cfg.inlier_angle = (c.inlier_angle if c.inlier_angle is not None
                        else math.atan(threshold_px / min(cam.params[0], cam.params[1])))
    poses = torch.empty((k, 12), dtype=torch.float64, device="cuda")
    status = torch.empty((k,), dtype=torch.uint8, device="cuda")
    n_inliers = torch.empty((k,), dtype=torch.int32, device="cuda")
    n_usable = torch.empty((k,), dtype=torch.int32, device="cuda")
    mask = torch.zeros((m,), dtype=torch.uint8, device="cuda")  # entries no pair owns stay 0
    ws_bytes = L.acm_relative_pose_batch_workspace_size(k, m)
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device="cuda")
    _lib.check(L.acm_relative_pose_batch(
        ctypes.byref(cam), k, poses.data_ptr() if k else None, offs.data_ptr(), m,
        ua.data_ptr() if m else None, ub.data_ptr() if m else None, ctypes.byref(cfg),
        status.data_ptr() if k else None, n_inliers.data_ptr() if k else None,
        mask.data_ptr() if m else None, n_usable.data_ptr() if k else None, ws.data_ptr(),
        ws_bytes, _stream_handle()))
    return RelativePoseResult(poses, status, n_inliers, n_usable, mask)


def two_view_tracks(pair_offsets, uv_a, uv_b, inlier_mask, poses=None):
    """estimate_relative_poses' inliers as triangulate's input, built on the
    device without a loop over the pairs.  Pair k becomes the views 2 k (pose
    [I | 0]) and 2 k + 1 (pose [R | t], row k of poses), and every inlier match
    one track of two observations.  Returns (view_poses (2 K, 12) -- None
    without poses --, track_offsets (N + 1,) int64, obs_view (2 N,) int32,
    obs_uv (2 N, 2) f64, match (N,) int64: the match each track came from).
    The points triangulate returns are in camera A's frame of their pair, in
    units of the baseline."""
    offs = torch.as_tensor(pair_offsets).to(device="cuda", dtype=torch.int64).contiguous()
    ua = _as_device_f64(uv_a, 2)
    ub = _as_device_f64(uv_b, 2)
    mask = torch.as_tensor(inlier_mask).to(device="cuda")
    if offs.shape[0] < 1 or ub.shape[0] != ua.shape[0] or mask.shape[0] != ua.shape[0]:
        raise ValueError("pair_offsets needs K + 1 entries; uv_a, uv_b and inlier_mask one row per match")
    k = offs.shape[0] - 1
    match = torch.nonzero(mask != 0).reshape(-1)
    n = match.shape[0]
    pair = torch.bucketize(match, offs[1:].contiguous(), right=True)  # offs[p] <= match < offs[p + 1]
    obs_view = torch.stack([2 * pair, 2 * pair + 1], dim=1).reshape(-1).to(torch.int32)
    obs_uv = torch.stack([ua[match], ub[match]], dim=1).reshape(-1, 2).contiguous()
    track_offsets = 2 * torch.arange(n + 1, dtype=torch.int64, device="cuda")
    view_poses = None
    if poses is not None:
        rel = _poses_tensor(poses)
        if rel.shape[0] != k:
            raise ValueError("poses must have one row per pair")
        eye = torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=torch.float64, device="cuda")
        view_poses = torch.stack([eye.expand(k, 12), rel], dim=1).reshape(2 * k, 12).contiguous()
    return view_poses, track_offsets, obs_view, obs_uv, match


# ------------------------------------------------------- two-view homography
def homography_4pt(bearings_a, bearings_b):
    """The 4-point homography solver (acm_homography_4pt), batched:
    bearings_a, bearings_b (N, 4, 3), the rays of four matches in image A and
    in image B, any length.  Returns (homography (N, 9) f64 -- f_b ~ H f_a,
    row-major, middle singular value 1 --, poses (N, 2, 12) f64 -- the two
    motions p_b = R p_a + t, unit t --, planes (N, 2, 4) f64 -- (n, d / |t|)
    --, translation (N,) f64 -- tau = |t| / d --, count (N,) u8 -- 0, 1
    (rotation only) or 2 --, n_front (N, 2) u8) on the device; NaN and 0 where
    it fails and in the slots beyond count."""
    L = _lib.load()
    fa = _as_device_f64(torch.as_tensor(bearings_a).reshape(-1, 3), 3)
    fb = _as_device_f64(torch.as_tensor(bearings_b).reshape(-1, 3), 3)
    if fa.shape[0] % 4 or fa.shape[0] != fb.shape[0]:
        raise ValueError("bearings_a and bearings_b must both be (N, 4, 3)")
    n = fa.shape[0] // 4
    hom = torch.empty((n, 9), dtype=torch.float64, device="cuda")
    poses = torch.empty((n, 2, 12), dtype=torch.float64, device="cuda")
    planes = torch.empty((n, 2, 4), dtype=torch.float64, device="cuda")
    tau = torch.empty((n,), dtype=torch.float64, device="cuda")
    count = torch.empty((n,), dtype=torch.uint8, device="cuda")
    front = torch.empty((n, 2), dtype=torch.uint8, device="cuda")
    ptr = [x.data_ptr() if n else None for x in (fa, fb, hom, poses, planes, tau, count, front)]
    _lib.check(L.acm_homography_4pt(n, *ptr, _stream_handle()))
    return hom, poses, planes, tau, count, front


@dataclass
class HomographyConfig:
    """acm_homography_config; the defaults are
    acm_homography_batch_default_config's, except inlier_angle: None takes the
    angle of estimate_homographies' threshold_px."""
    n_hypotheses: int = 256
    seed: int = 1
    inlier_angle: Optional[float] = None
    min_inliers: int = 4
    refit_rounds: int = 3


@dataclass
class HomographyResult:
    """Device tensors, K pairs: homography (K, 9) f64 (f_b ~ H f_a, row-major,
    middle singular value 1; NaN where status is not HOMOGRAPHY_OK), status
    (K,) u8 (_lib.HOMOGRAPHY_OK / HOMOGRAPHY_TOO_FEW_MATCHES /
    HOMOGRAPHY_NO_MODEL), n_inliers (K,) i32, poses (K, 2, 12) f64 (the two
    motions camera A -> camera B, R row-major, then the unit t; NaN beyond
    n_solutions), planes (K, 2, 4) f64 ((n, d / |t|) in camera A's frame),
    n_solutions (K,) u8 (1: rotation only, t = 0), n_front (K, 2) i32,
    translation (K,) f64 (tau = |t| / d), inlier_mask (M,) u8, n_usable (K,)
    i32."""
    homography: torch.Tensor
    status: torch.Tensor
    n_inliers: torch.Tensor
    poses: torch.Tensor
    planes: torch.Tensor
    n_solutions: torch.Tensor
    n_front: torch.Tensor
    translation: torch.Tensor
    inlier_mask: torch.Tensor
    n_usable: torch.Tensor

    def pose_slot(self, slot):
        """(K, 12): one solution per pair as two_view_tracks' poses.  slot: an
        int for all pairs, or (K,) integers (0 or 1) choosing per pair."""
        if isinstance(slot, int):
            return self.poses[:, slot].contiguous()
        idx = torch.as_tensor(slot).to(device=self.poses.device, dtype=torch.int64).reshape(-1, 1, 1)
        return torch.gather(self.poses, 1, idx.expand(-1, 1, 12)).reshape(-1, 12).contiguous()


def estimate_homographies(model: CameraModel, pair_offsets, uv_a, uv_b,
                          config: Optional[HomographyConfig] = None,
                          threshold_px: float = 3.0) -> HomographyResult:
    """Every view pair's homography from 2-D / 2-D matches
    (acm_homography_batch): the model of a planar scene or a rotating camera,
    where estimate_relative_poses' 8-point system loses rank.  The 4-point
    solver on the unprojected rays inside RANSAC with a refit over the
    inliers, one workgroup per pair, all pairs in one launch; the final H is
    decomposed into its two (R, t, plane).  Inputs as estimate_relative_poses.
    Without config.inlier_angle the threshold is atan(threshold_px / min(fx,
    fy))."""
    import math
    L = _lib.load()
    offs = torch.as_tensor(pair_offsets).to(device="cuda", dtype=torch.int64).contiguous()
    ua = _as_device_f64(uv_a, 2)
    ub = _as_device_f64(uv_b, 2)
    k, m = offs.shape[0] - 1, ua.shape[0]
    if k < 0 or ub.shape[0] != m:
        raise ValueError("pair_offsets needs K + 1 entries; uv_a and uv_b one row per match")
    cam = model.acm_camera()
    c = config or HomographyConfig()
    cfg = _lib.HomographyConfig()
    L.acm_homography_batch_default_config(ctypes.byref(cfg))
    cfg.n_hypotheses = c.n_hypotheses
    cfg.seed = c.seed
    cfg.min_inliers = c.min_inliers
    cfg.refit_rounds = c.refit_rounds
    cfg.inlier_angle = (c.inlier_angle if c.inlier_angle is not None
                        else math.atan(threshold_px / min(cam.params[0], cam.params[1])))
    hom = torch.empty((k, 9), dtype=torch.float64, device="cuda")
    status = torch.empty((k,), dtype=torch.uint8, device="cuda")
    n_inliers = torch.empty((k,), dtype=torch.int32, device="cuda")
    poses = torch.empty((k, 2, 12), dtype=torch.float64, device="cuda")
    planes = torch.empty((k, 2, 4), dtype=torch.float64, device="cuda")
    n_solutions = torch.empty((k,), dtype=torch.uint8, device="cuda")
    n_front = torch.empty((k, 2), dtype=torch.int32, device="cuda")
    tau = torch.empty((k,), dtype=torch.float64, device="cuda")
    n_usable = torch.empty((k,), dtype=torch.int32, device="cuda")
    mask = torch.zeros((m,), dtype=torch.uint8, device="cuda")  # entries no pair owns stay 0
    ws_bytes = L.acm_homography_batch_workspace_size(k, m)
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device="cuda")
    per_pair = [x.data_ptr() if k else None
                for x in (hom, status, n_inliers, poses, planes, n_solutions, n_front, tau)]
    _lib.check(L.acm_homography_batch(
        ctypes.byref(cam), k, offs.data_ptr(), m, ua.data_ptr() if m else None,
        ub.data_ptr() if m else None, ctypes.byref(cfg), *per_pair,
        mask.data_ptr() if m else None, n_usable.data_ptr() if k else None, ws.data_ptr(),
        ws_bytes, _stream_handle()))
    return HomographyResult(hom, status, n_inliers, poses, planes, n_solutions, n_front, tau, mask,
                            n_usable)


# ------------------------------------------------- 3-D similarity alignment
def similarity_3pt(points_a, points_b, rigid: bool = False):
    """The 3-point similarity solver (acm_similarity_3pt), batched: points_a,
    points_b (N, 3, 3), three corresponding 3-D points in frame A and in frame
    B.  Returns (similarity (N, 13) f64 -- b = s R a + t: R row-major, t, s --,
    count (N,) u8) on the device; NaN and 0 where the triple is void
    (collinear, coincident, not finite).  rigid: s fixed to 1."""
    L = _lib.load()
    pa = _as_device_f64(torch.as_tensor(points_a).reshape(-1, 3), 3)
    pb = _as_device_f64(torch.as_tensor(points_b).reshape(-1, 3), 3)
    if pa.shape[0] % 3 or pa.shape[0] != pb.shape[0]:
        raise ValueError("points_a and points_b must both be (N, 3, 3)")
    n = pa.shape[0] // 3
    sim = torch.empty((n, _lib.SIMILARITY_DOUBLES), dtype=torch.float64, device="cuda")
    count = torch.empty((n,), dtype=torch.uint8, device="cuda")
    _lib.check(L.acm_similarity_3pt(n, pa.data_ptr() if n else None, pb.data_ptr() if n else None,
                                    _lib.SIMILARITY_RIGID if rigid else 0,
                                    sim.data_ptr() if n else None, count.data_ptr() if n else None,
                                    _stream_handle()))
    return sim, count


@dataclass
class SimilarityConfig:
    """acm_similarity_config; the defaults are
    acm_similarity_batch_default_config's.  The inlier distance is
    estimate_similarities' own argument: it has no default."""
    n_hypotheses: int = 256
    seed: int = 1
    min_inliers: int = 3
    refit_rounds: int = 3
    rigid: bool = False


@dataclass
class SimilarityResult:
    """Device tensors, K sets: similarity (K, 13) f64 (b = s R a + t: R
    row-major, t, s; NaN where status is not SIMILARITY_OK), status (K,) u8
    (_lib.SIMILARITY_OK / SIMILARITY_TOO_FEW_POINTS / SIMILARITY_NO_MODEL),
    n_inliers (K,) i32, rms (K,) f64 (over the inliers, in B's units),
    n_usable (K,) i32, inlier_mask (M,) u8, one byte per correspondence."""
    similarity: torch.Tensor
    status: torch.Tensor
    n_inliers: torch.Tensor
    rms: torch.Tensor
    n_usable: torch.Tensor
    inlier_mask: torch.Tensor


def estimate_similarities(set_offsets, points_a, points_b, inlier_distance: float,
                          config: Optional[SimilarityConfig] = None) -> SimilarityResult:
    """Every correspondence set's similarity b ~ s R a + t between two 3-D
    frames (acm_similarity_batch): the 3-point absolute-orientation solver
    inside RANSAC with a least-squares refit over the inliers, one workgroup
    per set, all sets in one launch.  set_offsets (K + 1,) int64: set k owns
    the rows set_offsets[k] .. set_offsets[k + 1] - 1 of points_a, points_b (M,
    3).  inlier_distance: the largest |b - (s R a + t)| of an inlier, in frame
    B's units."""
    L = _lib.load()
    offs = torch.as_tensor(set_offsets).to(device="cuda", dtype=torch.int64).contiguous()
    pa = _as_device_f64(points_a, 3)
    pb = _as_device_f64(points_b, 3)
    k, m = offs.shape[0] - 1, pa.shape[0]
    if k < 0 or pb.shape[0] != m:
        raise ValueError("set_offsets needs K + 1 entries; points_a and points_b one row per correspondence")
    c = config or SimilarityConfig()
    cfg = _lib.SimilarityConfig()
    L.acm_similarity_batch_default_config(ctypes.byref(cfg))
    cfg.n_hypotheses = c.n_hypotheses
    cfg.flags = _lib.SIMILARITY_RIGID if c.rigid else 0
    cfg.seed = c.seed
    cfg.inlier_distance = inlier_distance
    cfg.min_inliers = c.min_inliers
    cfg.refit_rounds = c.refit_rounds
    sim = torch.empty((k, _lib.SIMILARITY_DOUBLES), dtype=torch.float64, device="cuda")
    status = torch.empty((k,), dtype=torch.uint8, device="cuda")
    n_inliers = torch.empty((k,), dtype=torch.int32, device="cuda")
    rms = torch.empty((k,), dtype=torch.float64, device="cuda")
    n_usable = torch.empty((k,), dtype=torch.int32, device="cuda")
    mask = torch.zeros((m,), dtype=torch.uint8, device="cuda")  # entries no set owns stay 0
    ws_bytes = L.acm_similarity_batch_workspace_size(k, m)
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device="cuda")
    per_set = [x.data_ptr() if k else None for x in (sim, status, n_inliers, rms)]
    _lib.check(L.acm_similarity_batch(
        k, offs.data_ptr(), m, pa.data_ptr() if m else None, pb.data_ptr() if m else None,
        ctypes.byref(cfg), *per_set, mask.data_ptr() if m else None,
        n_usable.data_ptr() if k else None, ws.data_ptr(), ws_bytes, _stream_handle()))
    return SimilarityResult(sim, status, n_inliers, rms, n_usable, mask)


def _similarity_parts(similarity):
    """(R (..., 3, 3), t (..., 3), s (...,)) of (..., 13) on the device."""
    sim = torch.as_tensor(similarity).to(device="cuda", dtype=torch.float64)
    if sim.shape[-1] != _lib.SIMILARITY_DOUBLES:
        raise ValueError("a similarity has 13 entries: R row-major, t, s")
    return sim[..., :9].reshape(*sim.shape[:-1], 3, 3), sim[..., 9:12], sim[..., 12]


def _similarity_pack(R, t, s):
    return torch.cat([R.reshape(*R.shape[:-2], 9), t, s.unsqueeze(-1)], dim=-1).contiguous()


def apply_similarity(similarity, points, set_index=None):
    """s R X + t on the device.  similarity (13,) or (K, 13); points (N, 3);
    set_index (N,) integers: the row of `similarity` each point takes (None:
    the one similarity given).  Returns (N, 3) f64."""
    R, t, s = _similarity_parts(similarity)
    X = _as_device_f64(points, 3)
    if set_index is None:
        if R.dim() == 3 and R.shape[0] != 1:
            raise ValueError("several similarities need set_index")
        R, t, s = R.reshape(1, 3, 3), t.reshape(1, 3), s.reshape(1)
    else:
        idx = torch.as_tensor(set_index).to(device="cuda", dtype=torch.int64).reshape(-1)
        if idx.shape[0] != X.shape[0]:
            raise ValueError("set_index needs one entry per point")
        R, t, s = R.reshape(-1, 3, 3)[idx], t.reshape(-1, 3)[idx], s.reshape(-1)[idx]
    return s.unsqueeze(-1) * torch.matmul(R, X.unsqueeze(-1)).squeeze(-1) + t


def similarity_transform_poses(similarity, poses):
    """View poses [R_c | t_c] given in frame A carried into frame B by the
    similarity X_B = s R X_A + t (13,): [R_c R^T | s t_c - R_c R^T t], (V, 12).
    From p_c = R_c X_A + t_c and X_A = R^T (X_B - t) / s: s p_c = R_c R^T X_B -
    R_c R^T t + s t_c, so camera coordinates then come in B's unit."""
    R, t, s = _similarity_parts(similarity)
    if R.dim() != 2:
        raise ValueError("similarity_transform_poses takes one similarity (13,)")
    P = _poses_tensor(poses)
    Rc, tc = P[:, :9].reshape(-1, 3, 3), P[:, 9:]
    Rn = torch.matmul(Rc, R.t())
    tn = s * tc - torch.matmul(Rn, t)
    return torch.cat([Rn.reshape(-1, 9), tn], dim=1).contiguous()


def similarity_compose(second, first):
    """The similarity that applies `first`, then `second` ((..., 13) each,
    broadcast): R = R2 R1, t = s2 R2 t1 + t2, s = s2 s1."""
    R2, t2, s2 = _similarity_parts(second)
    R1, t1, s1 = _similarity_parts(first)
    R = torch.matmul(R2, R1)
    t = s2.unsqueeze(-1) * torch.matmul(R2, t1.unsqueeze(-1)).squeeze(-1) + t2
    return _similarity_pack(R, t, s2 * s1)


def similarity_inverse(similarity):
    """a = R^T (b - t) / s as a similarity: (R^T, -R^T t / s, 1 / s)."""
    R, t, s = _similarity_parts(similarity)
    Rt = R.transpose(-1, -2)
    ti = -torch.matmul(Rt, t.unsqueeze(-1)).squeeze(-1) / s.unsqueeze(-1)
    return _similarity_pack(Rt, ti, 1.0 / s)


# ------------------------------------------------------ multi-view calibration
@dataclass
class CalibrationConfig:
    """acm_calibrate_config; the defaults are acm_calibrate_default_config's.
    bounds: parameter index -> (lower, upper), on the intrinsics only."""
    max_iterations: int = 50
    cost_tolerance: float = 1e-6
    parameter_tolerance: float = 1e-8
    gradient_tolerance: float = 1e-6
    initial_damping: float = 1e-4
    bounds: Optional[Dict[int, Tuple[float, float]]] = None


@dataclass
class CalibrationResult:
    """model: a new camera model with the calibrated intrinsics; poses (K, 12)
    f64, status (K,) u8 (_lib.POSE_*), cost (K,) f64 (NaN for a view that did
    not take part), n_valid (K,) i32: device tensors, one row per view;
    summary: an LmResult over the whole problem (its parameters the
    intrinsics) with n_views_used added; information (P, P) f64 host tensor,
    the reduced (Schur) normal matrix of the intrinsics; view_system (K, 16,
    16) device f64 or None."""
    model: CameraModel
    poses: torch.Tensor
    status: torch.Tensor
    cost: torch.Tensor
    n_valid: torch.Tensor
    summary: LmResult
    information: torch.Tensor
    view_system: Optional[torch.Tensor] = None
    n_views_used: int = 0


def calibrate(model: CameraModel, poses, points_world, view_offsets, obs_point, obs_uv,
              config: Optional[CalibrationConfig] = None, fixed: Optional[Sequence[int]] = None,
              want_view_system: bool = False) -> CalibrationResult:
    """Multi-view calibration (acm_calibrate): the model's intrinsics and
    every view's pose from known world points, one Levenberg-Marquardt on the
    joint problem through the Schur complement.  Inputs as refine_poses
    (tracks_by_view's output feeds the call unchanged); neither `model` nor
    the caller's pose tensor is modified.  fixed: indices of intrinsics held
    at their start value."""
    L = _lib.load()
    pt = _poses_tensor(poses).clone()
    pw = _as_device_f64(points_world, 3)
    offs = torch.as_tensor(view_offsets).to(device="cuda", dtype=torch.int64).contiguous()
    idx = torch.as_tensor(obs_point).to(device="cuda", dtype=torch.int32).contiguous()
    uv = _as_device_f64(obs_uv, 2)
    k, n, m = pt.shape[0], pw.shape[0], idx.shape[0]
    if offs.shape[0] != k + 1 or uv.shape[0] != m:
        raise ValueError("view_offsets needs K + 1 entries; obs_point and obs_uv one row per observation")
    c = config or CalibrationConfig()
    cfg = _lib.CalibrateConfig()
    L.acm_calibrate_default_config(ctypes.byref(cfg))
    cfg.max_iterations = c.max_iterations
    cfg.cost_tolerance = c.cost_tolerance
    cfg.parameter_tolerance = c.parameter_tolerance
    cfg.gradient_tolerance = c.gradient_tolerance
    cfg.initial_damping = c.initial_damping
    if c.bounds:
        cfg.has_bounds = 1
        for j, (lo, hi) in c.bounds.items():
            cfg.lower[j] = lo
            cfg.upper[j] = hi
    for j in fixed or ():
        if not 0 <= int(j) < 32:
            raise ValueError("fixed takes parameter indices")
        cfg.fixed_mask |= 1 << int(j)
    p = model.NUM_PARAMS
    status = torch.empty((k,), dtype=torch.uint8, device="cuda")
    cost = torch.empty((k,), dtype=torch.float64, device="cuda")
    n_valid = torch.empty((k,), dtype=torch.int32, device="cuda")
    vsys = torch.empty((k, 16, 16), dtype=torch.float64, device="cuda") if want_view_system else None
    ws_bytes = L.acm_calibrate_workspace_size(model.MODEL_ID, k, m)
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device="cuda")
    cam = model.acm_camera()
    summ = _lib.CalibrateSummary()
    _lib.check(L.acm_calibrate(
        ctypes.byref(cam), k, pt.data_ptr() if k else None, n, pw.data_ptr() if n else None,
        offs.data_ptr(), m, idx.data_ptr() if m else None, uv.data_ptr() if m else None,
        ctypes.byref(cfg), ctypes.byref(summ), status.data_ptr() if k else None,
        cost.data_ptr() if k else None, n_valid.data_ptr() if k else None,
        vsys.data_ptr() if vsys is not None and k else None, ws.data_ptr(), ws_bytes,
        _stream_handle()))
    params = list(cam.params)[:p]
    res = type(model.resolution)(model.resolution.width, model.resolution.height)
    out = type(model)._from_params(params, res)
    info = torch.tensor(list(summ.information)[: p * p], dtype=torch.float64).reshape(p, p)
    summary = LmResult(parameters=params, iterations=summ.iterations,
                       termination=_lib.LM_TERMINATION.get(summ.termination, "?"),
                       evaluations=summ.evaluations, initial_cost=summ.initial_cost,
                       final_cost=summ.final_cost, n_valid=int(summ.n_valid))
    return CalibrationResult(out, pt, status, cost, n_valid, summary, info, vsys,
                             summ.n_views_used)
