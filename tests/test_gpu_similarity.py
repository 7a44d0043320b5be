"""acm_similarity_3pt and acm_similarity_batch on the GPU: the 3-point
similarity solver (absolute orientation) and RANSAC with a least-squares refit
over it, one workgroup per correspondence set.

The solver's accuracy tests run the triples of similarity_ref (4096 general
triples, 200 of each special family) under the bounds of
tests/test_similarity_ref.py: median error <= 10 x the numpy reference's median
on the same triples, worst <= 100 x its worst; the error of a similarity is
max( max|R - R_true|, max|t - t_true| / max(1, max|t_true|), |s / s_true - 1|).
The sets of the RANSAC tests are similarity_ref.scene's: points in the box
[+-4, +-3, 6 +- 2], s = 2.5, a motion of their own per set; with noise 0.01 per
axis, 40 % of b moved by N(0, I), "far" being more than 0.2 from the true
transform.

Measured on an MI355X (profiles/similarity_perf.log).
acm_similarity_3pt returns the bits of the host build of similarity.hpp for
every n compared; on the 4096 triples worst error 4.0e-13 (reference 4.8e-13),
median 1.6e-15 (1.4e-15).  Zero noise: error 9.7e-16 .. 7.1e-15 (reference
2.0e-15 .. 2.7e-14), rms 2.2e-15 .. 3.3e-15.  Noise and outliers, seed 1: 24 /
60 / 180 / 615 inliers, the numpy RANSAC's counts, no far point in a mask, no
borderline correspondence, errors equal to the reference's to four digits
(4.6e-3 .. 7.1e-4), |R - R_true| 6.2e-4 .. 1.8e-5; rigid 24 / 60 / 180 / 614;
without the refit 24 / 60 / 180 / 612.  Three views end to end: 300 common
tracks, all inliers, |S - S_reference| 1.8e-15, view 2's pose error 1.0e-13
(with the reference alignment 9.9e-14).
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import similarity_ref as G
from apex_camera_models import _lib
from apex_camera_models.optimizer import (RelativePoseConfig, SimilarityConfig, apply_similarity,
                                          estimate_relative_poses, estimate_similarities,
                                          similarity_3pt, similarity_compose, similarity_inverse,
                                          similarity_transform_poses, triangulate,
                                          two_view_tracks)
from test_similarity_ref import CSRC, DRIVER, check_against_reference

pytestmark = pytest.mark.gpu

OK, TOO_FEW, NO_MODEL = _lib.SIMILARITY_OK, _lib.SIMILARITY_TOO_FEW_POINTS, _lib.SIMILARITY_NO_MODEL
# too few points, the minimal sample, lanes with and without a hypothesis'
# worth of points, both sides of the LDS / workspace boundary
COUNTS = (0, 2, 3, 4, 64, 257, 1024, 1025, 2000)
NOISY_COUNTS = (40, 100, 300, 1025)
NOISY_DISTANCE = 0.04


# ------------------------------------------------------- acm_similarity_3pt
def _rows(out):
    """similarity_3pt's two tensors as the host driver's rows (n, 14)."""
    sim, count = [x.cpu().numpy() for x in out]
    return np.concatenate([count.reshape(-1, 1).astype(np.float64), sim], axis=1)


def _on_device(a, b, rigid=False):
    return _rows(similarity_3pt(torch.as_tensor(np.array(a), device="cuda"),
                                torch.as_tensor(np.array(b), device="cuda"), rigid))


@functools.lru_cache(maxsize=None)
def _family_on_device():
    res = _on_device(*G.family()[:2])
    res.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def _family_on_host():
    """The first 257 triples through the host build of similarity.hpp."""
    import tempfile
    a, b = G.family()[:2]
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "similarity_host_driver")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, DRIVER, "-o",
                        exe], check=True)
        inp, out = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        np.concatenate([a[:257].reshape(257, 9), b[:257].reshape(257, 9)], axis=1).tofile(inp)
        subprocess.run([exe, inp, out, "3", "0", "3pt"], check=True)
        return np.fromfile(out).reshape(257, 14)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_3pt_sizes(n):
    """The same bits as the host build of similarity.hpp for every n, nothing
    written past n."""
    a, b = G.family()[:2]
    a_t = torch.as_tensor(a[:n].copy(), device="cuda")
    b_t = torch.as_tensor(b[:n].copy(), device="cuda")
    sim = torch.full((n + 1, 13), -7.0, dtype=torch.float64, device="cuda")
    count = torch.full((n + 1,), 99, dtype=torch.uint8, device="cuda")
    rc = _lib.load().acm_similarity_3pt(n, a_t.data_ptr() if n else None,
                                        b_t.data_ptr() if n else None, 0, sim.data_ptr(),
                                        count.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.last_error()
    got = _rows((sim, count))
    assert (got[n, 1:] == -7.0).all() and got[n, 0] == 99, "wrote past n"
    assert got[:n].tobytes() == _family_on_device()[:n].tobytes(), "a problem's result depends on n"
    assert got[:n].tobytes() == _family_on_host()[:n].tobytes(), "not the host build's bits"


def test_3pt_accuracy():
    check_against_reference("acm_similarity_3pt", _family_on_device(), G.family(),
                            G.family_accuracy())


@pytest.mark.parametrize("kind", G.SPECIAL)
def test_3pt_special_families(kind):
    a, b = G.special(kind)[:2]
    check_against_reference(f"acm_similarity_3pt, {kind}", _on_device(a, b), G.special(kind),
                            G.special_accuracy(kind))


def test_3pt_failures_and_rigid():
    a, b = G.failing_triples()
    for rigid in (False, True):
        res = _on_device(a, b, rigid)
        assert (res[:, 0] == 0).all() and np.isnan(res[:, 1:]).all()
    a, _, R0, t0, _ = G.family()
    a, R0, t0 = a[:512], R0[:512], t0[:512]
    s0 = np.ones(len(a))
    b = np.einsum("nij,nkj->nki", R0, a) + t0[:, None, :]
    res = _on_device(a, b, True)
    assert (res[:, 13] == 1.0).all()
    check_against_reference("acm_similarity_3pt, rigid", res, (a, b, R0, t0, s0),
                            G.reference_accuracy(a, b, R0, t0, s0, rigid=True))


# ------------------------------------------------------ acm_similarity_batch
def run(offsets, a, b, distance, want_rms=True, want_mask=True, want_usable=True, **kw):
    """The C call; numpy outputs, every output prefilled with a sentinel and a
    guard row behind it."""
    L = _lib.load()
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    a = np.array(a, dtype=np.float64).reshape(-1, 3)  # a copy: the scenes are read-only
    b = np.array(b, dtype=np.float64).reshape(-1, 3)
    k, m = len(offsets) - 1, len(a)
    cfg = _lib.SimilarityConfig()
    L.acm_similarity_batch_default_config(ctypes.byref(cfg))
    cfg.inlier_distance = distance
    for key, v in kw.items():
        setattr(cfg, key, v)
    dev = "cuda"
    offs_t = torch.as_tensor(offsets, device=dev)
    a_t, b_t = torch.as_tensor(a, device=dev), torch.as_tensor(b, device=dev)
    sim = torch.full((k + 1, 13), -7.0, dtype=torch.float64, device=dev)
    status = torch.full((k + 1,), 99, dtype=torch.uint8, device=dev)
    n_inliers = torch.full((k + 1,), -5, dtype=torch.int32, device=dev)
    rms = torch.full((k + 1,), -7.0, dtype=torch.float64, device=dev)
    n_usable = torch.full((k + 1,), -5, dtype=torch.int32, device=dev)
    mask = torch.full((m + 1,), 99, dtype=torch.uint8, device=dev)
    ws_bytes = L.acm_similarity_batch_workspace_size(k, m)
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.float64, device=dev)
    rc = L.acm_similarity_batch(
        k, offs_t.data_ptr(), m, a_t.data_ptr() if m else None, b_t.data_ptr() if m else None,
        ctypes.byref(cfg), sim.data_ptr(), status.data_ptr(), n_inliers.data_ptr(),
        rms.data_ptr() if want_rms else None, mask.data_ptr() if want_mask else None,
        n_usable.data_ptr() if want_usable else None, ws.data_ptr(), ws_bytes,
        torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.last_error()
    out = dict(sim=sim, status=status, n_inliers=n_inliers, rms=rms, n_usable=n_usable, mask=mask)
    out = {key: v.cpu().numpy() for key, v in out.items()}
    assert (out["sim"][k] == -7.0).all() and out["status"][k] == 99 and out["n_inliers"][k] == -5
    assert out["rms"][k] == -7.0 and out["n_usable"][k] == -5 and out["mask"][m] == 99
    if not want_rms:
        assert (out["rms"] == -7.0).all()
    if not want_mask:
        assert (out["mask"] == 99).all()
    if not want_usable:
        assert (out["n_usable"] == -5).all()
    return {key: v[:-1] for key, v in out.items()}


def kernel_rule(row, a, b, distance):
    """The inlier rule at the similarity `row` in the kernel's operation order
    (similarity.hpp's residual2: numpy's elementwise arithmetic does not
    contract either): the mask over the usable rows."""
    S = row
    with np.errstate(invalid="ignore"):
        px = S[0] * a[:, 0] + S[1] * a[:, 1] + S[2] * a[:, 2]
        py = S[3] * a[:, 0] + S[4] * a[:, 1] + S[5] * a[:, 2]
        pz = S[6] * a[:, 0] + S[7] * a[:, 1] + S[8] * a[:, 2]
        ex, ey, ez = b[:, 0] - (S[12] * px + S[9]), b[:, 1] - (S[12] * py + S[10]), b[:, 2] - (S[12] * pz + S[11])
        e = ex * ex + ey * ey + ez * ez
        return G.usable_rows(a, b) & (e <= distance * distance), e


def _offsets(counts):
    offsets = np.zeros(len(counts) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(counts)
    return offsets


@functools.lru_cache(maxsize=None)
def scenes(counts, noise, rigid=False, seed=20261021):
    """(offsets, a, b, truths, far): one scene per set, concatenated."""
    rng = np.random.default_rng(seed)
    parts = [G.scene(rng, n, noise=noise, moved=0.4 if noise else 0.0, rigid=rigid) for n in counts]
    a = np.concatenate([p[0] for p in parts])
    b = np.concatenate([p[1] for p in parts])
    far = np.concatenate([p[5] for p in parts])
    truths = tuple((p[2], p[3], p[4]) for p in parts)
    for arr in (a, b, far):
        arr.setflags(write=False)
    return _offsets(counts), a, b, truths, far


def test_zero_noise():
    offsets, a, b, truths, _ = scenes(COUNTS, 0.0)
    got = run(offsets, a, b, 1e-6)
    for k, n in enumerate(COUNTS):
        sl = slice(offsets[k], offsets[k + 1])
        assert got["n_usable"][k] == n
        if n < 3:
            assert got["status"][k] == TOO_FEW and got["n_inliers"][k] == 0
            assert np.isnan(got["sim"][k]).all() and np.isnan(got["rms"][k])
            assert (got["mask"][sl] == 0).all()
            continue
        assert got["status"][k] == OK, n
        assert got["n_inliers"][k] == n and (got["mask"][sl] == 1).all()
        err = G.model_error(G.unpack(got["sim"][k]), *truths[k])
        ref = G.model_error(G.fit(a[sl], b[sl]), *truths[k])
        print(f"zero noise, {n} points: error {err:.3e} (reference {ref:.3e}), rms "
              f"{got['rms'][k]:.3e}")
        assert err <= max(1e-9, 10.0 * ref)
        assert got["rms"][k] <= 1e-9


@functools.lru_cache(maxsize=None)
def noisy_reference(k, rigid=False, refit_rounds=3):
    offsets, a, b, _, _ = scenes(NOISY_COUNTS, 0.01, rigid)
    sl = slice(offsets[k], offsets[k + 1])
    return G.ransac(a[sl], b[sl], NOISY_DISTANCE, rigid=rigid, refit_rounds=refit_rounds)


@functools.lru_cache(maxsize=None)
def noisy_on_device(rigid=False, refit_rounds=3):
    offsets, a, b, _, _ = scenes(NOISY_COUNTS, 0.01, rigid)
    return run(offsets, a, b, NOISY_DISTANCE, refit_rounds=refit_rounds,
               flags=_lib.SIMILARITY_RIGID if rigid else 0)


def _check_noisy(rigid):
    offsets, a, b, truths, far = scenes(NOISY_COUNTS, 0.01, rigid)
    got = noisy_on_device(rigid)
    for k, n in enumerate(NOISY_COUNTS):
        sl = slice(offsets[k], offsets[k + 1])
        ref = noisy_reference(k, rigid)
        assert got["status"][k] == OK and ref["status"] == G.OK
        mask = got["mask"][sl] != 0
        assert not mask[far[sl]].any(), "a far point is in the mask"
        want, e = kernel_rule(got["sim"][k], a[sl], b[sl], NOISY_DISTANCE)
        assert np.array_equal(mask, want) and got["n_inliers"][k] == mask.sum()
        assert abs(got["rms"][k] - np.sqrt(e[mask].sum() / mask.sum())) <= 1e-12
        e_ref = G.residual2(ref["model"], a[sl], b[sl])
        d2 = NOISY_DISTANCE ** 2
        borderline = int((np.abs(e_ref - d2) <= 1e-9 * d2).sum())
        err = G.model_error(G.unpack(got["sim"][k]), *truths[k])
        err_ref = G.model_error(ref["model"], *truths[k])
        print(f"noise and outliers{', rigid' if rigid else ''}, {n} points: {got['n_inliers'][k]} "
              f"inliers (reference {ref['n_inliers']}, {borderline} borderline, "
              f"{int((~far[sl]).sum())} not far), error {err:.3e} (reference {err_ref:.3e}), |R - "
              f"R_true| {np.abs(got['sim'][k][:9].reshape(3, 3) - truths[k][0]).max():.3e}, rms "
              f"{got['rms'][k]:.3e}")
        assert got["n_inliers"][k] >= ref["n_inliers"] - borderline
        assert err <= 2.0 * err_ref
        if rigid:
            assert got["sim"][k][12] == 1.0


def test_noise_and_outliers():
    _check_noisy(False)


def test_rigid():
    _check_noisy(True)


def test_refit_rounds():
    """Without the refit the count is the RANSAC winner's: not above the
    default's, and the reference's without it."""
    raw, fit = noisy_on_device(False, 0), noisy_on_device(False, 3)
    assert (raw["status"] == OK).all()
    assert (raw["n_inliers"] <= fit["n_inliers"]).all()
    for k in range(len(NOISY_COUNTS)):
        ref = noisy_reference(k, False, 0)
        print(f"no refit, {NOISY_COUNTS[k]} points: {raw['n_inliers'][k]} inliers (reference "
              f"{ref['n_inliers']}; with the refit {fit['n_inliers'][k]})")


def test_degenerate_sets():
    rng = np.random.default_rng(3)
    # collinear throughout: no sample has a model
    line = np.outer(np.linspace(-2.0, 2.0, 64), [1.0, 2.0, -1.0]) + np.array([3.0, 1.0, 5.0])
    # planar: a proper rotation, not the reflection that fits as well
    plane = np.column_stack([rng.uniform(-4, 4, 64), rng.uniform(-3, 3, 64), np.full(64, 6.0)])
    R0, t0, s0 = G.exp_so3(np.array([0.3, -0.5, 0.8])), np.array([1.0, -2.0, 0.5]), 2.5
    a = np.concatenate([line, plane])
    b = s0 * (a @ R0.T) + t0
    offsets = _offsets((64, 64))
    got = run(offsets, a, b, 1e-6)
    assert got["status"][0] == NO_MODEL and got["n_inliers"][0] == 0
    assert np.isnan(got["sim"][0]).all() and (got["mask"][:64] == 0).all()
    assert got["status"][1] == OK and got["n_inliers"][1] == 64
    R = got["sim"][1][:9].reshape(3, 3)
    err = G.model_error(G.unpack(got["sim"][1]), R0, t0, s0)
    print(f"planar set: det R {np.linalg.det(R):.6f}, error {err:.3e}")
    assert np.linalg.det(R) > 0 and err <= 1e-9
    # min_inliers out of reach: the best count, no model
    n_off, n_a, n_b, _, _ = scenes(NOISY_COUNTS, 0.01)
    raw = noisy_on_device(False, 0)
    high = run(n_off, n_a, n_b, NOISY_DISTANCE, min_inliers=2000)
    assert (high["status"] == NO_MODEL).all() and np.isnan(high["sim"]).all()
    assert np.isnan(high["rms"]).all() and (high["mask"] == 0).all()
    assert np.array_equal(high["n_inliers"], raw["n_inliers"])


def _per_set(got, offsets, k):
    lo, hi = (int(min(max(offsets[i], 0), len(got["mask"]))) for i in (k, k + 1))
    hi = max(lo, hi)
    return b"".join([got["sim"][k].tobytes(), got["status"][k].tobytes(), got["n_inliers"][k].tobytes(),
                     got["rms"][k].tobytes(), got["n_usable"][k].tobytes(),
                     got["mask"][lo:hi].tobytes()])


def test_independence_and_reproducibility():
    counts = (100, 1025, 40, 300)
    offsets, a, b, _, _ = scenes(counts, 0.01, seed=7)
    a, b = np.array(a), np.array(b)
    # spoiled entries: NaN or Inf in a or b
    a[3, 1], b[17, 0], a[150, 2], b[1100, 1], a[1120, 0] = np.nan, np.inf, -np.inf, np.nan, np.inf
    got = run(offsets, a, b, NOISY_DISTANCE)
    again = run(offsets, a, b, NOISY_DISTANCE)
    for key in got:
        assert got[key].tobytes() == again[key].tobytes(), key
    assert (got["status"] == OK).all()
    assert got["n_usable"].tolist() == [98, 1022, 40, 300]
    assert not got["mask"][[3, 17, 150, 1100, 1120]].any()
    # every set alone, and in another place of another batch
    for k in range(len(counts)):
        sl = slice(offsets[k], offsets[k + 1])
        alone = run(_offsets((counts[k],)), a[sl], b[sl], NOISY_DISTANCE)
        assert _per_set(alone, [0, counts[k]], 0) == _per_set(got, offsets, k), k
    order = (2, 0, 3, 1)
    p_off = _offsets([counts[k] for k in order])
    p_a = np.concatenate([a[offsets[k]:offsets[k + 1]] for k in order])
    p_b = np.concatenate([b[offsets[k]:offsets[k + 1]] for k in order])
    perm = run(p_off, p_a, p_b, NOISY_DISTANCE)
    for i, k in enumerate(order):
        assert _per_set(perm, p_off, i) == _per_set(got, offsets, k), k
    # decreasing and out-of-range offsets are clamped; the nullable outputs
    # do not change the others
    m = len(a)
    odd = np.array([-5, 100, 60, 1125, 10 ** 12, 3], dtype=np.int64)
    wild = run(odd, a, b, NOISY_DISTANCE, want_rms=False, want_usable=False)
    ranges = [(0, 100), (100, 100), (60, 1125), (1125, m), (m, m)]
    for k, (lo, hi) in enumerate(ranges):
        alone = run(np.array([0, hi - lo]), a[lo:hi], b[lo:hi], NOISY_DISTANCE)
        for key in ("sim", "status", "n_inliers"):
            assert wild[key][k].tobytes() == alone[key][0].tobytes(), (k, key)
    assert wild["mask"][1125:m].tobytes() == run(np.array([0, m - 1125]), a[1125:], b[1125:],
                                                 NOISY_DISTANCE)["mask"].tobytes()
    assert wild["status"].tolist() == [OK, TOO_FEW, OK, OK, TOO_FEW]


def test_hypothesis_count():
    """One hypothesis (255 lanes bring no model), a full round of lanes, a
    round and a part.  Hypothesis h does not depend on how many there are, so
    without the refit 300 of them cannot do worse than their first 256; one
    hypothesis is void or not as the reference's is."""
    offsets, a, b, _, far = scenes(NOISY_COUNTS, 0.01)
    h1 = run(offsets, a, b, NOISY_DISTANCE, n_hypotheses=1)
    h256 = noisy_on_device(False, 0)
    h300 = run(offsets, a, b, NOISY_DISTANCE, n_hypotheses=300, refit_rounds=0)
    for k in range(len(NOISY_COUNTS)):
        sl = slice(offsets[k], offsets[k + 1])
        ref1 = G.ransac(a[sl], b[sl], NOISY_DISTANCE, n_hypotheses=1)
        assert h1["status"][k] == ref1["status"]
        for got in (h1, h300):
            if got["status"][k] == OK:
                want, _ = kernel_rule(got["sim"][k], a[sl], b[sl], NOISY_DISTANCE)
                assert np.array_equal(got["mask"][sl] != 0, want)
        assert h300["status"][k] == OK and h300["n_inliers"][k] >= h256["n_inliers"][k]
        assert not (h300["mask"][sl] != 0)[far[sl]].any()


# ------------------------------------------------------------------ helpers
def _np_pose_transform(S, poses):
    R, t, s = G.unpack(S)
    out = []
    for p in poses:
        Rc, tc = p[:9].reshape(3, 3), p[9:]
        Rn = Rc @ R.T
        out.append(np.r_[Rn.ravel(), s * tc - Rn @ t])
    return np.array(out)


def _np_compose(S2, S1):
    R2, t2, s2 = G.unpack(S2)
    R1, t1, s1 = G.unpack(S1)
    return G.pack((R2 @ R1, s2 * (R2 @ t1) + t2, s2 * s1))


def _np_inverse(S):
    R, t, s = G.unpack(S)
    return G.pack((R.T, -(R.T @ t) / s, 1.0 / s))


def test_helpers():
    rng = np.random.default_rng(9)
    S = np.array([G.pack((G.exp_so3(rng.normal(size=3)), rng.normal(size=3), rng.uniform(0.3, 3.0)))
                  for _ in range(5)])
    X = rng.normal(size=(40, 3)) * 3.0
    idx = rng.integers(0, 5, 40)
    got = apply_similarity(torch.as_tensor(S), torch.as_tensor(X), torch.as_tensor(idx)).cpu().numpy()
    want = np.array([G.apply(G.unpack(S[i]), X[j]) for j, i in enumerate(idx)])
    assert np.abs(got - want).max() <= 1e-12
    one = apply_similarity(S[2], X).cpu().numpy()
    assert np.abs(one - G.apply(G.unpack(S[2]), X)).max() <= 1e-12
    poses = np.array([np.r_[G.exp_so3(rng.normal(size=3)).ravel(), rng.normal(size=3)]
                      for _ in range(7)])
    got = similarity_transform_poses(S[1], torch.as_tensor(poses)).cpu().numpy()
    assert np.abs(got - _np_pose_transform(S[1], poses)).max() <= 1e-12
    # what the transform means: a point's camera coordinates, in B's unit
    Xb = G.apply(G.unpack(S[1]), X[0])
    for p, q in zip(poses, got):
        cam_a = p[:9].reshape(3, 3) @ X[0] + p[9:]
        cam_b = q[:9].reshape(3, 3) @ Xb + q[9:]
        assert np.abs(cam_b - S[1][12] * cam_a).max() <= 1e-12
    comp = similarity_compose(torch.as_tensor(S[3]), torch.as_tensor(S[4])).cpu().numpy()
    assert np.abs(comp - _np_compose(S[3], S[4])).max() <= 1e-12
    inv = similarity_inverse(torch.as_tensor(S)).cpu().numpy()
    assert np.abs(inv - np.array([_np_inverse(s) for s in S])).max() <= 1e-12
    ident = similarity_compose(similarity_inverse(torch.as_tensor(S)), torch.as_tensor(S)).cpu().numpy()
    assert np.abs(ident - G.pack((np.eye(3), np.zeros(3), 1.0))).max() <= 1e-12


# ------------------------------------------------------ three views, end to end
def test_three_views_end_to_end():
    """Pixels alone -> the pairs (0, 1) and (1, 2), each reconstructed in its
    own frame and unit -> one similarity puts view 2 into frame 0 in units of
    the baseline 01.  KB sample camera, 300 points, zero pixel noise."""
    from test_gpu_relative_pose import KB, _model, project, true_pose
    rng = np.random.default_rng(20261021)
    n = 300
    X0 = np.column_stack([rng.uniform(-4.0, 4.0, n), rng.uniform(-4.0, 4.0, n),
                          rng.uniform(1.5, 6.0, n)])
    R01, t01 = true_pose(KB, 0)
    R12, t12 = true_pose(KB, 1)
    X1 = X0 @ R01.T + t01
    X2 = X1 @ R12.T + t12
    uv = [project(KB, X) for X in (X0, X1, X2)]
    model = _model(KB)
    offs = np.array([0, n, 2 * n], dtype=np.int64)
    a_t = torch.as_tensor(np.concatenate([uv[0], uv[1]]), device="cuda")
    b_t = torch.as_tensor(np.concatenate([uv[1], uv[2]]), device="cuda")
    rel = estimate_relative_poses(model, offs, a_t, b_t, RelativePoseConfig(), threshold_px=1.0)
    assert (rel.status.cpu().numpy() == _lib.RELPOSE_OK).all()
    view_poses, t_off, t_view, t_uv, match = two_view_tracks(offs, a_t, b_t, rel.inlier_mask, rel.poses)
    tri = triangulate(model, view_poses, t_off, t_view, t_uv)
    match = match.cpu().numpy()
    good = tri.status.cpu().numpy() == _lib.TRI_OK
    # the common tracks of the two pairs, through `match`: point j is match j
    # of pair (0, 1) and match n + j of pair (1, 2)
    track_of = np.full(2 * n, -1)
    track_of[match[good]] = np.nonzero(good)[0]
    common = np.nonzero((track_of[:n] >= 0) & (track_of[n:] >= 0))[0]
    assert len(common) >= 250
    i01 = torch.as_tensor(track_of[:n][common], device="cuda")
    i12 = torch.as_tensor(track_of[n:][common], device="cuda")
    poses = rel.poses  # (2, 12): view 1 in frame 0, view 2 in frame 1, unit baselines
    one = torch.ones((1,), dtype=torch.float64, device="cuda")
    S01 = torch.cat([poses[0], one])  # frame 0 -> frame 1 as a similarity, s = 1
    in_1_from_01 = apply_similarity(S01, tri.points[i01])  # frame 1, units of baseline 01
    in_1_from_12 = tri.points[i12].contiguous()            # frame 1, units of baseline 12
    res = estimate_similarities(np.array([0, len(common)]), in_1_from_12, in_1_from_01, 1e-6)
    assert res.status.cpu().numpy()[0] == OK
    S = res.similarity[0]
    a_np, b_np = in_1_from_12.cpu().numpy(), in_1_from_01.cpu().numpy()
    mask = res.inlier_mask.cpu().numpy() != 0
    assert mask.sum() == res.n_inliers.cpu().numpy()[0] >= 250
    S_ref = G.pack(G.fit(a_np[mask], b_np[mask]))
    diff = np.abs(S.cpu().numpy() - S_ref).max()
    # view 2 in frame 0: its pose in frame 1 (units 12), carried by S into
    # frame 1 (units 01), then by S01's inverse into frame 0
    total = similarity_compose(similarity_inverse(S01), S)
    pose2 = similarity_transform_poses(total, poses[1:2]).cpu().numpy()[0]
    S01_np = S01.cpu().numpy()
    pose2_ref = _np_pose_transform(_np_compose(_np_inverse(S01_np), S_ref),
                                   poses[1:2].cpu().numpy())[0]
    base = np.linalg.norm(t01)
    truth = np.r_[(R12 @ R01).ravel(), (R12 @ t01 + t12) / base]
    err, err_ref = np.abs(pose2 - truth).max(), np.abs(pose2_ref - truth).max()
    print(f"three views end to end: {len(common)} common tracks, {int(mask.sum())} inliers, s = "
          f"{float(S[12]):.9f} (true {np.linalg.norm(t12) / base:.9f}), rms "
          f"{float(res.rms[0]):.3e}, |S - S_reference| {diff:.3e}, view 2's pose error {err:.3e} "
          f"(with the reference alignment {err_ref:.3e})")
    assert diff <= 1e-9
    assert err <= max(1e-7, 10.0 * err_ref)
