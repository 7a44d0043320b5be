"""tests/bearing_ref.py against the 50-digit forward models: the bearing the
RANSAC solvers' reference gives a pixel is the ray that projects to it.

For each of the 7 sample and 19 zoo cameras, every usable pixel of
bearing_ref.grid (61 x 41 pixels over the image and a 25 % margin) is mapped
forward by mp_models.project -- the model's formula itself, also where the
library's projection answers "behind the camera" (KB, DS and FOV beyond 90
degrees) -- and must return to the pixel: within 1e-9 px with RadTan's polish
(and for every other model, which has none), within 2 x the worst error
measured on the CPU without it (NO_POLISH_PX; include/acm.h documents 1e-6
rad for that case).

Measured with the f64 oracle (CHANGELOG.md has the table): worst 8.2e-12 px
(the UCM sample) with the polish; without it 4.58e-4 px (RadTan sample),
4.43e-4 (radtan_k3_tangential), 5.86e-4 (radtan_barrel_pos).  fov_max keeps
353 usable pixels of the 1080 inside its image (rd w >= pi on the rest), every
other camera at least 918 (ds_alpha_one).

Without the FOV and KB rules of bearing_ref.bearings (the oracle's own rays)
the round trip fails at fov, fov_mid, fov_max, kannala_brandt and kb_strong
and nowhere else: the FOV sample's pixel (10, 10) comes back at (915.2,
923.4), the KB sample's (0, 6.4) 58 px away.
"""
import functools
import math

import mpmath as mp
import numpy as np
import pytest

import bearing_ref as BR
import camera_zoo as Z
import mp_models as M
from apex_camera_models import samples

CAMERAS = tuple(sorted(samples.SAMPLES)) + Z.NAMES
POLISHED_PX = 1e-9
# worst round-trip error (px) of the unpolished RadTan bearing over the grid,
# measured on the CPU; the test asserts 2 x
NO_POLISH_PX = {BR.RADTAN: 4.582e-4, "radtan_k3_tangential": 4.427e-4, "radtan_barrel_pos": 5.860e-4}
SINGULAR_RAD = 1e-6    # FOV pixels this close to rd w = pi are left out
# usable grid pixels inside the image, of 1080.  fov_max: rd w >= pi on two
# thirds of its image, where no ray projects to the pixel; the rest is 353
MIN_USABLE_INSIDE = {"fov_max": 300}
MIN_USABLE_INSIDE_DEFAULT = 800


@functools.lru_cache(maxsize=None)
def round_trip(key, polish):
    """dict: uv, inside, f, usable, left_out (usable but singular), err (px;
    NaN where not measured)."""
    mid, params, _ = Z.camera_of(key)
    uv, inside = BR.grid(key)
    f, usable = BR.bearings(key, uv, polish)
    left_out = np.zeros(len(uv), dtype=bool)
    if mid == BR.FOV:
        left_out = usable & (np.abs(BR.fov_psi(params, uv)[4] - math.pi) <= SINGULAR_RAD)
    err = np.full(len(uv), np.nan)
    for j in np.nonzero(usable & ~left_out)[0]:
        u, v = M.project(mid, params, f[j])
        err[j] = float(mp.sqrt((u - mp.mpf(uv[j, 0])) ** 2 + (v - mp.mpf(uv[j, 1])) ** 2))
    out = dict(uv=uv, inside=inside, f=f, usable=usable, left_out=left_out, err=err)
    for a in out.values():
        a.setflags(write=False)
    return out


def _check(key, polish, bound):
    r = round_trip(key, polish)
    measured = np.isfinite(r["err"])
    worst = int(np.nanargmax(r["err"]))
    print(f"bearing round trip {Z.label(key)}{' polished' if polish else ''}: "
          f"{int(r['usable'].sum())} usable of {len(r['uv'])} ({int((r['usable'] & r['inside']).sum())}"
          f" of {int(r['inside'].sum())} inside), {int(r['left_out'].sum())} left out, worst "
          f"{r['err'][worst]:.3e} px at ({r['uv'][worst, 0]:.1f}, {r['uv'][worst, 1]:.1f}), bound "
          f"{bound:.3e}")
    assert (measured == (r["usable"] & ~r["left_out"])).all()
    assert r["left_out"].sum() <= 0.01 * len(r["uv"]), int(r["left_out"].sum())
    assert (r["usable"] & r["inside"]).sum() >= MIN_USABLE_INSIDE.get(key, MIN_USABLE_INSIDE_DEFAULT)
    bad = np.nonzero(measured & ~(r["err"] <= bound))[0]
    assert len(bad) == 0, (Z.label(key), len(bad), r["uv"][bad[:5]].tolist(),
                           r["err"][bad[:5]].tolist())


@pytest.mark.parametrize("key", CAMERAS, ids=Z.label)
def test_round_trip_polished(key):
    """The two-view solvers' bearing."""
    _check(key, True, POLISHED_PX)


@pytest.mark.parametrize("key", sorted(NO_POLISH_PX, key=str), ids=Z.label)
def test_round_trip_without_polish(key):
    """Pose estimation's bearing differs from the polished one for RadTan
    only; there the unprojection's Newton iteration stops at 1e-6."""
    _check(key, False, 2.0 * NO_POLISH_PX[key])


@pytest.mark.parametrize("key", [k for k in CAMERAS if Z.camera_of(k)[0] != BR.RADTAN], ids=Z.label)
def test_polish_changes_radtan_only(key):
    uv, _ = BR.grid(key)
    f0, u0 = BR.bearings(key, uv, False)
    f1, u1 = BR.bearings(key, uv, True)
    assert f0.tobytes() == f1.tobytes() and u0.tobytes() == u1.tobytes()


def test_only_fov_max_has_singular_pixels():
    for key in CAMERAS:
        if Z.camera_of(key)[0] == BR.FOV and key != "fov_max":
            assert not round_trip(key, True)["left_out"].any(), key


def test_branch_witnesses():
    """The pixels each camera is in the zoo for are in its grid."""
    for key in ("fov_mid", BR.FOV):
        r = round_trip(key, True)
        behind = r["usable"] & (r["f"][:, 2] < 0)
        print(f"{Z.label(key)}: {int(behind.sum())} usable pixels with z < 0")
        assert behind.sum() >= 10
    r = round_trip("radtan_k3_tangential", True)
    k3 = Z.camera_of("radtan_k3_tangential")[1][8]
    r2 = (r["f"][:, 0] ** 2 + r["f"][:, 1] ** 2) / r["f"][:, 2] ** 2
    strong = r["usable"] & (np.abs(k3 * r2 ** 3) > 1e-4)
    print(f"radtan_k3_tangential: {int(strong.sum())} usable pixels with |k3 r^6| > 1e-4")
    assert strong.sum() >= 100
    r = round_trip("ucm_alpha_lt_half", True)
    refused = ~r["usable"]
    print(f"ucm_alpha_lt_half: {int(refused.sum())} pixels the unprojection refuses")
    assert refused.sum() >= 10
    # fov_max: most of the image is no image of any ray
    r = round_trip("fov_max", True)
    assert (~r["usable"] & r["inside"]).sum() > 0.5 * r["inside"].sum()


def test_without_the_kb_rule_the_round_trip_fails():
    """The oracle's own KB ray (the reference's, |m| clamped to pi / 2): its
    forward image is off by more than a pixel wherever |m| > 1.6, and that
    happens in the sample camera's and kb_strong's image only."""
    import oracle
    for key in CAMERAS:
        mid, params, (w, h) = Z.camera_of(key)
        if mid != BR.KB:
            continue
        uv, _ = BR.grid(key)
        rays, st = oracle.unproject(mid, params, w, h, uv)
        ru = np.hypot((uv[:, 0] - params[2]) / params[0], (uv[:, 1] - params[3]) / params[1])
        beyond = np.nonzero((st == 0) & (ru > 1.6))[0]
        assert (len(beyond) >= 10) == (key in (BR.KB, "kb_strong")), (key, len(beyond))
        for j in beyond[:: max(1, len(beyond) // 20)]:
            u, v = M.project(mid, params, rays[j])
            assert math.hypot(float(u) - uv[j, 0], float(v) - uv[j, 1]) > 1.0, (key, uv[j])


def test_without_the_fov_rule_the_round_trip_fails():
    """The oracle's own FOV ray (the reference's, divided by cos(rd w)): its
    forward image is off by hundreds of pixels wherever rd w > pi / 2."""
    import oracle
    for key in CAMERAS:
        mid, params, (w, h) = Z.camera_of(key)
        if mid != BR.FOV:
            continue
        uv, _ = BR.grid(key)
        psi = BR.fov_psi(params, uv)[4]
        rays, st = oracle.unproject(mid, params, w, h, uv)
        assert (st == 0).all()
        beyond = np.nonzero((psi > math.pi / 2 + 1e-3) & (psi < math.pi - 1e-3))[0]
        if key in (BR.FOV, "fov_mid", "fov_max"):
            assert len(beyond) >= 10, (key, len(beyond))
        else:
            assert len(beyond) == 0, (key, len(beyond))
        for j in beyond[:: max(1, len(beyond) // 20)]:
            u, v = M.project(mid, params, rays[j])
            assert math.hypot(float(u) - uv[j, 0], float(v) - uv[j, 1]) > 100.0, (key, uv[j])
