"""Batched multi-view triangulation on the GPU (acm_triangulate).

References (tests/triangulation_ref.py): the numpy midpoint from oracle rays,
scipy's TRF on oracle residuals, and 50-digit point Jacobians / projections
(tests/point_jacobian_ref.py) for information and cost.  Every test asserts
its input condition on the CPU before calling the GPU.  The midpoint start and
the information / cost sums run for all seven models at their sample cameras
(each on triangulation_ref.rig_kind's rig: Pinhole and RadTan reject pixels
outside the image and take the medium rig); the sums also run, at a given
start with max_iterations = 0, on the solver subset of tests/camera_zoo.py.

Measured on an MI355X: start vs numpy midpoint, worst error / bound Pinhole
2.4e-6, RadTan 5.3e-6 (medium rig, cond(A) <= 645), KB 3.9e-6, DS 2.6e-6, UCM
2.3e-6, EUCM 2.3e-6, FOV 5.0e-6 (cond(A) <= 445); zero noise from the
displaced start (bound 1e-6): Pinhole 4.4e-9, RadTan 3.4e-8, KB 3.7e-8, DS 3.3e-8, UCM
3.7e-9, EUCM 3.6e-8, FOV 3.9e-8; noisy cost / scipy cost KB 1 + 1.8e-10, DS
1 + 1.1e-10; information and cost, worst |gpu - exact| / bound Pinhole
5.0e-3, RadTan 1.4e-2, KB 1.3e-2, DS 3.8e-2, UCM 7.5e-2, EUCM 2.5e-2, FOV
2.2e-2; at a given start on the zoo cameras 2.1e-4 (pinhole_aniso) ... 7.7e-3
(kb_negative).
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import camera_zoo as Z
import oracle
import point_jacobian_ref as PJ
import triangulation_ref as T
from apex_camera_models import _lib, samples, tracks_from_dense, triangulate
from apex_camera_models.optimizer import Pose, TriangulationConfig

pytestmark = pytest.mark.gpu

KB, DS = _lib.KANNALA_BRANDT, _lib.DOUBLE_SPHERE
ALL_MODELS = tuple(range(7))
START_SIZES = (1, 63, 64, 65, 257, 1000)


def _model(mid):
    """mid: a model id (its sample camera) or a zoo camera's name, here and below"""
    return Z.device_model(mid)


def _dev(a, dtype):
    return torch.as_tensor(np.array(a), dtype=dtype, device="cuda")  # a copy: inputs are read-only


def _c_triangulate(mid, poses, offsets, view, uv, max_iterations=None, initial=None,
                   n_views=None):
    """The C call; returns host arrays (X, status, cost, n_valid, information)."""
    L = _lib.load()
    n, m = len(offsets) - 1, len(view)
    cfg = _lib.TriangulateConfig()
    L.acm_triangulate_default_config(ctypes.byref(cfg))
    if max_iterations is not None:
        cfg.max_iterations = max_iterations
    poses_t = _dev(poses, torch.float64)
    offs_t, view_t, uv_t = _dev(offsets, torch.int64), _dev(view, torch.int32), _dev(uv, torch.float64)
    if initial is not None:
        cfg.flags = _lib.TRI_USE_INITIAL
        X = _dev(initial, torch.float64)
    else:
        X = torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda")
    status = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    cost = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    nv = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    info = torch.full((n, 6), 7.0, dtype=torch.float64, device="cuda")
    ws_bytes = L.acm_triangulate_workspace_size(n, m)
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device="cuda")
    cam = _model(mid).acm_camera()
    _lib.check(L.acm_triangulate(
        ctypes.byref(cam), len(poses) if n_views is None else n_views, poses_t.data_ptr(), n,
        offs_t.data_ptr(), m, view_t.data_ptr() if m else None, uv_t.data_ptr() if m else None,
        ctypes.byref(cfg), X.data_ptr(), status.data_ptr(), cost.data_ptr(), nv.data_ptr(),
        info.data_ptr(), ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream))
    return (X.cpu().numpy(), status.cpu().numpy(), cost.cpu().numpy(), nv.cpu().numpy(),
            info.cpu().numpy())


def _prefix(kind, mid, n, noise_px=0.0):
    """The first n points of the scene: (X, offsets, view, uv)."""
    X, offsets, view = T.scene(kind)
    uv = T.observations(kind, mid, noise_px)
    m = offsets[n]
    return X[:n], offsets[: n + 1], view[:m], uv[:m]


# ------------------------------------------------------------ 1. start only
@functools.lru_cache(maxsize=None)
def _midpoint_reference(mid, noise_px=0.0):
    """The numpy midpoint of the first 1000 points of the camera's rig (shared)."""
    kind = T.rig_kind(mid)
    _, offsets, view, uv = _prefix(kind, mid, 1000, noise_px)
    return T.midpoint(kind, mid, offsets, view, uv)


@pytest.mark.parametrize("mid", ALL_MODELS)
def test_midpoint_start_matches_numpy(mid):
    kind = T.rig_kind(mid)
    X_ref, cond, usable = _midpoint_reference(mid)
    _, _, centres = T.rig(kind)
    params, (w, h) = samples.SAMPLES[mid]
    _, offsets, view, uv = _prefix(kind, mid, 1000)
    _, st = oracle.unproject(mid, params, w, h, uv)
    assert (st == 0).all() and (usable == np.diff(offsets)).all()
    assert cond.max() <= 2000.0, cond.max()
    cmax = np.linalg.norm(centres, axis=1).max()
    worst = 0.0
    for n in START_SIZES:
        _, offs, vw, obs = _prefix(kind, mid, n)
        X, status, cost, nv, info = _c_triangulate(mid, T.poses12(kind), offs, vw, obs,
                                                   max_iterations=0)
        assert (status == _lib.TRI_OK).all(), (n, status)
        assert (nv == np.diff(offs)).all()
        bound = cond[:n] * 1e-10 * np.maximum(np.linalg.norm(X_ref[:n], axis=1), cmax)
        err = np.linalg.norm(X - X_ref[:n], axis=1)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (n, int(np.argmax(err / bound)), float((err / bound).max()))
    print(f"midpoint {samples.MODEL_NAMES[mid]}: worst |X - X_ref| / bound = {worst:.3e}, "
          f"cond(A) <= {cond.max():.0f}")


# ----------------------------------------- 2. zero noise, displaced start
@pytest.mark.parametrize("mid", ALL_MODELS)
def test_zero_noise_from_displaced_start(mid):
    params, (w, h) = samples.SAMPLES[mid]
    truth, offsets, view, uv = _prefix("narrow", mid, 500)
    _, st = oracle.unproject(mid, params, w, h, uv)
    assert (st == 0).all(), "an oracle unprojection of the narrow rig is not Ok"
    start = truth + np.array([0.05, -0.05, 0.05])
    X, status, cost, nv, _ = _c_triangulate(mid, T.poses12("narrow"), offsets, view, uv,
                                            initial=start)
    err = np.linalg.norm(X - truth, axis=1)
    print(f"zero noise {samples.MODEL_NAMES[mid]}: worst |X - truth| = {err.max():.3e}, "
          f"worst cost {cost.max():.3e}")
    assert (status == _lib.TRI_OK).all(), np.unique(status, return_counts=True)
    assert (nv == np.diff(offsets)).all()
    assert (err <= 1e-6).all(), float(err.max())


# ------------------------------------------------------- 3. noise 0.5 px
N_NOISY = 4099


@functools.lru_cache(maxsize=None)
def _noisy_run(mid):
    """The default call on the camera's noisy rig (the wide one for KB and
    DS; shared by tests 3 and 4)."""
    kind = T.rig_kind(mid)
    params, (w, h) = samples.SAMPLES[mid]
    _, offsets, view, uv = _prefix(kind, mid, N_NOISY, 0.5)
    _, st = oracle.unproject(mid, params, w, h, uv)
    assert (st == 0).all(), "a noisy pixel does not unproject on the oracle"
    return _c_triangulate(mid, T.poses12(kind), offsets, view, uv)


@pytest.mark.parametrize("mid", [KB, DS])
def test_noisy_optimum_matches_scipy(mid):
    X, status, cost, nv, _ = _noisy_run(mid)
    _, offsets, view, uv = _prefix("wide", mid, N_NOISY, 0.5)
    assert (status == _lib.TRI_OK).all(), np.unique(status, return_counts=True)
    X0, cond, _ = _midpoint_reference(mid, 0.5)
    assert cond[:200].max() <= 2000.0
    worst = 0.0
    for i in range(200):
        sl = slice(offsets[i], offsets[i + 1])
        ref = T.scipy_cost("wide", mid, view[sl], uv[sl], X0[i])
        worst = max(worst, cost[i] / ref if ref > 0 else 1.0)
        assert cost[i] <= ref * (1.0 + 1e-6) + 1e-9, (i, cost[i], ref)
    print(f"noisy {samples.MODEL_NAMES[mid]}: worst gpu cost / scipy cost = {worst:.12f}")


# ------------------------------------- 4. information, cost, n_valid
@pytest.mark.parametrize("mid", ALL_MODELS)
def test_information_cost_and_n_valid(mid):
    n = 250
    kind = T.rig_kind(mid)
    X, status, cost, nv, info = _noisy_run(mid)
    _, offsets, view, uv = _prefix(kind, mid, n, 0.5)
    R, t, _ = T.rig(kind)
    p = T.camera_points(kind, X[:n], offsets, view)
    have = PJ.reference_rows(mid, p)
    assert have.all(), "a projection at the returned X is not Ok on the oracle"
    Jp = PJ.mp_jacobians(mid, p)                       # (M, 2, 3)
    uv_exact = PJ.mp_project(mid, p, have)
    J = np.einsum("mab,mbc->mac", Jp, R[view])         # J = Jpoint(p) R
    r = uv_exact - uv
    worst = 0.0
    for i in range(n):
        sl = slice(offsets[i], offsets[i + 1])
        assert nv[i] == offsets[i + 1] - offsets[i]
        Ji, ri = J[sl], r[sl]
        k = 0
        checks = []
        for a in range(3):
            for b in range(a, 3):
                terms = np.concatenate([Ji[:, 0, a] * Ji[:, 0, b], Ji[:, 1, a] * Ji[:, 1, b]])
                checks.append((info[i, k], terms))
                k += 1
        checks.append((cost[i], 0.5 * np.concatenate([ri[:, 0] ** 2, ri[:, 1] ** 2])))
        for got, terms in checks:
            exact, mag = math.fsum(terms), math.fsum(np.abs(terms))
            bound = max(1e-10 * abs(exact), 1e-13 * mag)
            err = abs(got - exact)
            worst = max(worst, err / bound)
            assert err <= bound, (i, got, exact, err / bound)
    print(f"information / cost {samples.MODEL_NAMES[mid]}: worst |gpu - exact| / bound = {worst:.3e}")


ZOO_N, ZOO_N_REFERENCE = 1000, 300


@pytest.mark.parametrize("name", Z.SOLVER_SUBSET)
def test_information_cost_and_n_valid_at_a_given_start(name):
    """ACM_TRI_USE_INITIAL with max_iterations = 0 on a zoo camera: one
    evaluation at the given points (the truth moved by (0.01, -0.01, 0.02)),
    0.5 px noise, NaN / Inf pixels and out-of-range view indices put in at
    fixed places.  1000 points in one call (across the wave and the workgroup
    seams); n_valid and the status of every point, information and cost of
    the first 300 against the 50-digit terms; the first 257 alone give the
    same bits."""
    kind = T.rig_kind(name)
    truth, offsets, view, uv = _prefix(kind, name, ZOO_N, 0.5)
    view, uv = np.array(view), np.array(uv)
    j = np.arange(len(view))
    uv[j % 37 == 5, 0] = np.nan
    uv[j % 53 == 7, 1] = np.inf
    view[j % 41 == 11] = -1
    view[j % 43 == 13] = T.K_VIEWS
    usable = np.isfinite(uv).all(axis=1) & (view >= 0) & (view < T.K_VIEWS)
    start = truth + np.array([0.01, -0.01, 0.02])
    poses = T.poses12(kind)
    X, status, cost, nv, info = _c_triangulate(name, poses, offsets, view, uv, max_iterations=0,
                                               initial=start)
    m257 = offsets[257]
    alone = _c_triangulate(name, poses, offsets[:258], view[:m257], uv[:m257], max_iterations=0,
                           initial=start[:257])
    for x, y in zip((X, status, cost, nv, info), alone):
        assert x[:257].tobytes() == y.tobytes(), "the first 257 points differ when run alone"
    want_nv = np.add.reduceat(usable.astype(np.int64), offsets[:-1])
    assert (nv == want_nv).all(), np.nonzero(nv != want_nv)[0][:5]
    few = want_nv < 2
    assert few.any() and (status[few] == _lib.TRI_TOO_FEW_OBSERVATIONS).all()
    assert (status[~few] == _lib.TRI_OK).all(), np.unique(status, return_counts=True)
    assert np.isnan(cost[few]).all() and (info[few] == 0.0).all()
    assert X[~few].tobytes() == start[~few].tobytes(), "max_iterations = 0 moved a point"
    n = ZOO_N_REFERENCE
    mref = offsets[n]
    R, t, _ = T.rig(kind)
    safe_view = np.where(usable, view, 0)[:mref]
    p = np.einsum("mij,mj->mi", R[safe_view], start[T.point_of(offsets[: n + 1])]) + t[safe_view]
    have = PJ.reference_rows(name, p)
    assert have[usable[:mref]].all(), "a projection at the start is not Ok on the oracle"
    Jp = PJ.mp_jacobians(name, p)
    uv_exact = PJ.mp_project(name, p, have)
    J = np.einsum("mab,mbc->mac", Jp, R[safe_view])
    r = uv_exact - uv[:mref]
    worst = 0.0
    for i in np.nonzero(~few[:n])[0]:
        rows = np.arange(offsets[i], offsets[i + 1])
        rows = rows[usable[rows]]
        Ji, ri = J[rows], r[rows]
        k = 0
        checks = []
        for a in range(3):
            for b in range(a, 3):
                terms = np.concatenate([Ji[:, 0, a] * Ji[:, 0, b], Ji[:, 1, a] * Ji[:, 1, b]])
                checks.append((info[i, k], terms))
                k += 1
        checks.append((cost[i], 0.5 * np.concatenate([ri[:, 0] ** 2, ri[:, 1] ** 2])))
        for got, terms in checks:
            exact, mag = math.fsum(terms), math.fsum(np.abs(terms))
            bound = max(1e-10 * abs(exact), 1e-13 * mag)
            err = abs(got - exact)
            worst = max(worst, err / bound)
            assert err <= bound, (i, got, exact, err / bound)
    print(f"information / cost at a given start {name}: worst |gpu - exact| / bound = {worst:.3e}")


# ------------------------------------------------------------ 5. statuses
def test_statuses_and_skipped_observations():
    mid = KB
    _, offsets, view, uv = _prefix("wide", mid, 8, 0.5)
    # a two-view track (a, b) from the scene
    i2 = int(np.nonzero(np.diff(offsets) >= 2)[0][0])
    a, b = offsets[i2], offsets[i2] + 1
    va, vb, pa, pb = int(view[a]), int(view[b]), uv[a], uv[b]
    nan2 = [np.nan, np.nan]
    tracks = [
        ([], []),                                              # 0: empty
        ([va], [pa]),                                          # 1: one observation
        ([va, va], [pa, pa]),                                  # 2: the same pixel and pose twice
        ([va, vb], [pa, pb]),                                  # 3: the plain two-view track
        ([va, 3, vb], [pa, [np.nan, 5.0], pb]),                # 4: + a NaN pixel
        ([va, T.K_VIEWS, vb], [pa, pb, pb]),                   # 5: + view index = n_views
        ([-1, va, vb], [pa, pa, pb]),                          # 6: + view index = -1
        ([va, vb, 0], [nan2, nan2, nan2]),                     # 7: every pixel NaN
        ([va, vb, 2 ** 31 - 1], [pa, pb, pa]),                 # 8: + a huge view index
    ]
    offs = np.cumsum([0] + [len(v) for v, _ in tracks]).astype(np.int64)
    vw = np.array([x for v, _ in tracks for x in v], dtype=np.int32)
    obs = np.array([x for _, p in tracks for x in p], dtype=np.float64).reshape(-1, 2)
    X, status, cost, nv, info = _c_triangulate(mid, T.poses12("wide"), offs, vw, obs)
    TF, DG = _lib.TRI_TOO_FEW_OBSERVATIONS, _lib.TRI_DEGENERATE
    assert list(status[[0, 1, 2, 7]]) == [TF, TF, DG, TF], status
    assert list(nv[[0, 1, 2, 7]]) == [0, 1, 2, 0], nv
    for i in (0, 1, 2, 7):
        assert np.isnan(X[i]).all() and np.isnan(cost[i]) and (info[i] == 0).all()
    assert status[3] == _lib.TRI_OK and nv[3] == 2 and np.isfinite(X[3]).all()
    for i in (4, 5, 6, 8):
        assert status[i] == status[3] and nv[i] == 2
        assert X[i].tobytes() == X[3].tobytes(), i
        assert cost[i].tobytes() == cost[3].tobytes(), i
        assert info[i].tobytes() == info[3].tobytes(), i


# -------------------------------------------------------- 6. independence
LONG_TRACK = 3000


@functools.lru_cache(maxsize=None)
def _independence_problem():
    """1000 wide-rig KB tracks (0.5 px noise) + one point with LONG_TRACK
    observations cycling the 6 views with fresh noise, as a list of tracks."""
    mid = KB
    params, (w, h) = samples.SAMPLES[mid]
    X, offsets, view, uv = _prefix("wide", mid, 1000, 0.5)
    tracks = [(view[offsets[i]:offsets[i + 1]], uv[offsets[i]:offsets[i + 1]]) for i in range(1000)]
    R, t, _ = T.rig("wide")
    lv = (np.arange(LONG_TRACK) % T.K_VIEWS).astype(np.int32)
    clean, st, _ = oracle.project(mid, params, w, h, R[lv] @ X[0] + t[lv])
    assert (st == 0).all()
    noise = np.random.default_rng(T.SEED + 2).normal(0.0, 0.5, clean.shape)
    tracks.insert(500, (lv, clean + noise))
    return tracks


def _csr(tracks):
    offs = np.cumsum([0] + [len(v) for v, _ in tracks]).astype(np.int64)
    return offs, np.concatenate([v for v, _ in tracks]).astype(np.int32), \
        np.concatenate([p for _, p in tracks]).reshape(-1, 2)


def test_outputs_do_not_depend_on_the_batch():
    assert LONG_TRACK > _lib.TRI_STAGE_OBSERVATIONS  # the long track's wave cannot stage its run
    tracks = _independence_problem()
    poses = T.poses12("wide")
    base = _c_triangulate(KB, poses, *_csr(tracks))
    again = _c_triangulate(KB, poses, *_csr(tracks))
    for x, y in zip(base, again):
        assert x.tobytes() == y.tobytes(), "two calls differ"
    assert (base[1] == _lib.TRI_OK).all()
    assert base[3][500] == LONG_TRACK
    perm = np.random.default_rng(3).permutation(len(tracks))
    shuffled = _c_triangulate(KB, poses, *_csr([tracks[k] for k in perm]))
    for x, y in zip(base, shuffled):
        assert x[perm].tobytes() == y.tobytes(), "a point's outputs depend on its place"
    for k in [500, 0, 1000, 436, 437, 499, 501, 563, 564] + list(range(63, 1000, 90)):
        alone = _c_triangulate(KB, poses, *_csr([tracks[k]]))
        for x, y in zip(base, alone):
            assert x[k:k + 1].tobytes() == y.tobytes(), (k, "differs when run alone")


def test_many_views_give_the_same_bits():
    """Up to 64 views the kernel keeps the poses in LDS, beyond that it reads
    them through the cache: 6 views padded to 64 and to 70 (the extra ones
    never referenced) must not change a bit."""
    _, offsets, view, uv = _prefix("wide", KB, 300, 0.5)
    poses = T.poses12("wide")
    base = _c_triangulate(KB, poses, offsets, view, uv)
    for k in (64, 70):
        padded = np.concatenate([poses, np.tile(poses[:1], (k - T.K_VIEWS, 1))])
        many = _c_triangulate(KB, padded, offsets, view, uv)
        for x, y in zip(base, many):
            assert x.tobytes() == y.tobytes(), k


# ------------------------------------------------------ 7. Python surface
def test_python_surface_matches_the_c_call():
    mid = DS
    offsets, view, uv = (np.array(a) for a in _prefix("wide", mid, 300, 0.5)[1:])
    X, status, cost, nv, info = _c_triangulate(mid, T.poses12("wide"), offsets, view, uv)
    R, t, _ = T.rig("wide")
    poses = [Pose(R[k].tolist(), t[k].tolist()) for k in range(T.K_VIEWS)]
    for given in (poses, _dev(T.poses12("wide"), torch.float64)):
        res = triangulate(_model(mid), given, offsets, view, uv, want_information=True)
        assert res.points.cpu().numpy().tobytes() == X.tobytes()
        assert res.status.cpu().numpy().tobytes() == status.tobytes()
        assert res.cost.cpu().numpy().tobytes() == cost.tobytes()
        assert res.n_valid.cpu().numpy().tobytes() == nv.tobytes()
        assert res.information.cpu().numpy().tobytes() == info.tobytes()
    assert triangulate(_model(mid), poses, offsets, view, uv).information is None
    # initial= sets ACM_TRI_USE_INITIAL and leaves the caller's tensor alone
    start = _dev(X + 0.01, torch.float64)
    keep = start.clone()
    Xi, sti, costi, nvi, infoi = _c_triangulate(mid, T.poses12("wide"), offsets, view, uv,
                                                initial=X + 0.01)
    res = triangulate(_model(mid), poses, offsets, view, uv, initial=start,
                      config=TriangulationConfig(), want_information=True)
    assert torch.equal(start, keep)
    assert res.points.cpu().numpy().tobytes() == Xi.tobytes()
    assert res.cost.cpu().numpy().tobytes() == costi.tobytes()
    only_start = triangulate(_model(mid), poses, offsets, view, uv, initial=start,
                             config=TriangulationConfig(max_iterations=0))
    assert torch.equal(only_start.points, start)


def test_tracks_from_dense():
    nan = float("nan")
    dense = np.full((3, 4, 2), nan)            # [K, N, 2]
    dense[0, 0] = [1.0, 2.0]
    dense[2, 0] = [3.0, 4.0]
    dense[1, 1] = [5.0, 6.0]
    dense[0, 3] = [7.0, 8.0]
    dense[1, 3] = [9.0, nan]                   # half a pixel: dropped
    dense[2, 3] = [11.0, 12.0]
    offs, view, uv = tracks_from_dense(torch.as_tensor(dense, device="cuda"))
    assert offs.dtype == torch.int64 and view.dtype == torch.int32 and uv.dtype == torch.float64
    assert offs.is_cuda and view.is_cuda and uv.is_cuda
    assert offs.cpu().tolist() == [0, 2, 3, 3, 5]
    assert view.cpu().tolist() == [0, 2, 1, 0, 2]
    assert uv.cpu().tolist() == [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0], [11.0, 12.0]]
