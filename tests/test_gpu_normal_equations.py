"""Every entry of the fused intrinsic normal equations (k_normal_eq: the
structured accumulator of NeAccum, KB's 37 sums of powers of theta, the
ne_out_src index map and the FAST projection form) against exactly summed
50-digit terms.

Reference: tests/normal_equations_ref.py.  Per output entry,

    |gpu - exact| <= max(1e-10 |exact|, 1e-13 sum |terms|),

at all seven sample cameras and the 19 cameras of tests/camera_zoo.py, both
point layouts, both invalid-point policies, and the sizes 0, 1 and either side
of the wave (64) and workgroup (256) seams.  The structural zeros are exactly
0, (cx, cx) = (cy, cy) = the last slot = n_valid, J^T J is symmetric bit for
bit, and a second call returns the same bytes.  The cell form is held to the
same reference and to the pixel form's bits, and the valid count of the FAST
form to the oracle's on every threshold probe of tests/boundary_probes.py.

Measured on an MI355X: see CHANGELOG.md (worst |gpu - exact| / bound per
camera).
"""
import ctypes

import numpy as np
import pytest
import torch

import camera_zoo as Z
import normal_equations_ref as N
import oracle
from apex_camera_models import _lib, samples

pytestmark = pytest.mark.gpu

ALL_MODELS = tuple(sorted(samples.SAMPLES))
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1000, 4099)
ZOO_SIZES = (257, 1000)  # across a wave and a workgroup seam
CELL_GRID = (94, 60)     # num_cells_x, num_cells_y


def _layout_tensor(pts, layout):
    """Device points in the layout: (n, 3) rows, or the three planes."""
    return torch.as_tensor(pts if layout == "aos" else np.ascontiguousarray(pts.T), device="cuda")


def _ne_call(cam, n, pts_t, layout, obs_t, policy, cells_t=None, grid=None):
    """acm_normal_equations (or _cells when cells_t is given) -> host f64
    [JtJ | Jtr | cost | n_valid]; the result buffer starts as NaN."""
    L = _lib.load()
    P = cam.num_params
    assert pts_t.numel() == 3 * n and pts_t.dtype == torch.float64
    ws_bytes = L.acm_normal_equations_workspace_size(cam.model, n)
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device="cuda")
    res = torch.full((P * P + P + 2,), float("nan"), dtype=torch.float64, device="cuda")
    lay = _lib.LAYOUT_SOA if layout == "soa" else _lib.LAYOUT_AOS
    stream = torch.cuda.current_stream().cuda_stream
    if cells_t is None:
        assert obs_t.numel() == 2 * n and obs_t.dtype == torch.float64
        _lib.check(L.acm_normal_equations(ctypes.byref(cam), n, pts_t.data_ptr(), lay,
                                          obs_t.data_ptr(), policy, res.data_ptr(),
                                          ws.data_ptr(), ws_bytes, stream))
    else:
        assert cells_t.numel() == n and cells_t.dtype == torch.int32
        _lib.check(L.acm_normal_equations_cells(ctypes.byref(cam), n, pts_t.data_ptr(), lay,
                                                cells_t.data_ptr(), ctypes.byref(grid), policy,
                                                res.data_ptr(), ws.data_ptr(), ws_bytes, stream))
    return res.cpu().numpy()


def _eval_camera(key):
    return Z.device_model(key, N.eval_params(key)).acm_camera()


@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("key", ALL_MODELS + Z.NAMES, ids=Z.label)
def test_every_entry(key, layout, policy):
    cam = _eval_camera(key)
    worst = 0.0
    for n in (SIZES if key in ALL_MODELS else ZOO_SIZES):
        pts_t = _layout_tensor(N.points(key, n), layout)
        obs_t = torch.as_tensor(N.observations(key, n), device="cuda")
        got = _ne_call(cam, n, pts_t, layout, obs_t, policy)
        again = _ne_call(cam, n, pts_t, layout, obs_t, policy)
        assert got.tobytes() == again.tobytes(), (n, "two calls differ")
        want, mag, n_valid = N.exact(key, n, policy)
        if n == 0:
            assert not got.any(), got  # every slot written, and with 0
        try:
            worst = max(worst, N.check(got, want, mag, n_valid))
        except AssertionError as e:
            raise AssertionError(f"n = {n}: {e}") from None
    print(f"NE {Z.label(key)} {layout} policy {policy}: worst |gpu - exact| / bound = {worst:.3e}")


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("key", ALL_MODELS + Z.NAMES, ids=Z.label)
def test_policies_share_every_sum_but_the_cost(key, layout):
    """An invalid point adds only the sentinel to r.r (J = 0 under both
    policies, include/acm.h; NeAccum::add touches one accumulator for it), so
    JtJ, Jtr and n_valid have the same bits under both, and cost(1) - cost(0)
    is 1e12 per invalid point."""
    cam = _eval_camera(key)
    P = cam.num_params
    n = 1000
    pts_t = _layout_tensor(N.points(key, n), layout)
    obs_t = torch.as_tensor(N.observations(key, n), device="cuda")
    skip = _ne_call(cam, n, pts_t, layout, obs_t, _lib.INVALID_SKIP)
    sent = _ne_call(cam, n, pts_t, layout, obs_t, _lib.INVALID_SENTINEL)
    c = P * P + P
    assert skip[:c].tobytes() == sent[:c].tobytes() and skip[c + 1] == sent[c + 1]
    n_invalid = n - int(skip[c + 1])
    assert n_invalid == n - N.exact(key, n, 0)[2] and n_invalid >= 2
    off = (sent[c] - skip[c]) - 1e12 * n_invalid
    print(f"NE {Z.label(key)} {layout}: {n_invalid} invalid, cost(1) - cost(0) - 1e12 n_invalid = "
          f"{off:.3e} = {off / np.spacing(sent[c]):+.2f} ulp of cost(1)")
    assert abs(off) <= np.spacing(sent[c])


def _cell_observations(key, n):
    """Per point the cell of the 94 x 60 grid over the image that holds the
    oracle's pixel (cell 0 where the projection fails), and the cell centres
    ((j + 0.5) * (width / num_cells_x), (i + 0.5) * (height / num_cells_y)),
    c = i * num_cells_x + j (include/acm.h, acm_cell_grid)."""
    model, params, (w, h) = Z.camera_of(key)
    ncx, ncy = CELL_GRID
    uv, st, _ = oracle.project(model, params, w, h, N.points(key, n))
    cw, ch = float(w) / float(ncx), float(h) / float(ncy)
    ok = st == 0
    j = np.where(ok, np.clip(np.floor(np.where(ok, uv[:, 0], 0.0) / cw), 0, ncx - 1), 0).astype(np.int64)
    i = np.where(ok, np.clip(np.floor(np.where(ok, uv[:, 1], 0.0) / ch), 0, ncy - 1), 0).astype(np.int64)
    cells = (i * ncx + j).astype(np.uint32)
    centres = np.stack([(j.astype(np.float64) + 0.5) * cw, (i.astype(np.float64) + 0.5) * ch], axis=1)
    return cells, centres, _lib.CellGrid(ncx, ncy, w, h)


@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("key", ALL_MODELS, ids=Z.label)
def test_cell_form_every_entry(key, policy):
    cam = _eval_camera(key)
    worst = 0.0
    for n in ZOO_SIZES:
        cells, centres, grid = _cell_observations(key, n)
        assert len(np.unique(cells)) >= 100  # the observations spread over the grid
        pts_t = _layout_tensor(N.points(key, n), "aos")
        obs_t = torch.as_tensor(centres, device="cuda")
        cells_t = torch.as_tensor(cells.view(np.int32), device="cuda")
        pix = _ne_call(cam, n, pts_t, "aos", obs_t, policy)
        cel = _ne_call(cam, n, pts_t, "aos", None, policy, cells_t=cells_t, grid=grid)
        want, mag, n_valid = N.exact(key, n, policy, obs=centres)
        worst = max(worst, N.check(pix, want, mag, n_valid), N.check(cel, want, mag, n_valid))
        assert pix.tobytes() == cel.tobytes(), (n, "the cell form differs from the pixel form")
    print(f"NE cells {Z.label(key)} policy {policy}: worst |gpu - exact| / bound = {worst:.3e}")


@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_fast_form_valid_count_on_thresholds(layout):
    """The FAST projection form (used by the fused normal equations alone)
    takes every status decision of the threshold probes as the oracle does:
    n_valid over each family, and over each run of 17 rows -- one +-8 ulp
    window, so a single flipped decision shows and is located.  Only n_valid
    is read (some probes lie at |p| ~ 1e13); the observations are zeros."""
    import boundary_probes as B
    from apex_camera_models import Resolution
    from apex_camera_models.camera import MODEL_CLASSES
    families = [f for f in B.probes() if f[3] == "project"]
    assert len(families) >= 11
    windows = 0
    for model, params, (w, h), _, pts in families:
        assert len(pts) % 17 == 0 and len(pts) >= 51
        cam = MODEL_CLASSES[samples.MODEL_NAMES[model]]._from_params(
            list(params), Resolution(w, h)).acm_camera()
        _, st, _ = oracle.project(model, params, w, h, pts)
        ok = st == 0
        assert 0 < int(ok.sum()) < len(pts)
        obs_t = torch.zeros((len(pts), 2), dtype=torch.float64, device="cuda")
        for lo, hi in [(0, len(pts))] + [(k, k + 17) for k in range(0, len(pts), 17)]:
            rows = np.ascontiguousarray(pts[lo:hi])
            got = _ne_call(cam, hi - lo, _layout_tensor(rows, layout), layout, obs_t[:hi - lo], 0)
            assert got[-1] == float(ok[lo:hi].sum()), \
                (samples.MODEL_NAMES[model], list(params), lo, hi, got[-1], int(ok[lo:hi].sum()),
                 rows[(hi - lo) // 2].tolist())
            windows += 1
    print(f"FAST form on thresholds, {layout}: {len(families)} families, {windows} counts equal")
