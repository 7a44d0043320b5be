"""The numpy restatement of acm_homography_4pt / acm_homography_batch
(homography_ref.py) against ground truth, the pinned sampler, and a host build
of csrc/homography.hpp -- the code the kernels run -- against that reference.
CPU only.

The error of a solution is the max-abs error in (R, t^, n, d / |t| relative)
of the slot that matches the truth best.  The reference's own bound against
the truth is 1e6 eps / tau_min of the family: eps / tau is the decomposition's
error growth and 1e6 the headroom for the conditioning of the
worst 4-tuple among thousands (measured: 4e5 for the family).  The bounds on
the solver under test come from the reference on the same tuples: median
error <= 10 x the reference's median, worst <= 100 x its worst.

Measured over the 4096 4-tuples (tau in [0.05, 0.5)): the reference worst
1.9e-10, median 9.7e-15, |H - H_true| worst 3.1e-11; the host build of
homography.hpp (bearings scaled by 0.5 .. 3) worst 2.6e-10, median 7.2e-15,
|H - H_true| worst 4.3e-11, |R^T R - I| 8.9e-16, |f_b x H f_a| 7.8e-16.  Special families (200 tuples
each, reference worst / median, host worst / median): pure rotation 4.9e-14 /
8.5e-16, 2.8e-14 / 3.9e-16 (count 1, t = 0 throughout); tau = 1e-3 2.3e-10 /
2.2e-12, 3.6e-10 / 1.6e-12; plane at 75 degrees 2.8e-11 / 1.0e-14, 1.7e-11 /
8.7e-15.
"""
import math
import os
import subprocess

import numpy as np
import pytest

import homography_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "apex-camera-models_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "homography_host_driver.cpp")
EPS = 2.0 ** -52
TAU_MIN = {"family": 0.05, "rotation": 1.0, "small_baseline": 1e-3, "oblique": 0.05}


def _tuples(kind):
    return G.family() if kind == "family" else G.special(kind)


def _accuracy(kind):
    return G.family_accuracy() if kind == "family" else G.special_accuracy(kind)


@pytest.mark.parametrize("kind", ("family",) + G.SPECIAL)
def test_reference_recovers_the_truth(kind):
    err, herr, cnt = _accuracy(kind)
    print(f"reference homography, {kind}: worst error {err.max():.3e}, median "
          f"{np.median(err):.3e}, |H - H_true| worst {herr.max():.3e}")
    assert (cnt == (1 if kind == "rotation" else 2)).all()
    assert err.max() <= 1e6 * EPS / TAU_MIN[kind]
    assert herr.max() <= 1e6 * EPS
    if kind == "rotation":
        fa, fb = G.special(kind)[:2]
        for i in range(len(fa)):
            sol = G.solve(fa[i], fb[i])
            assert (sol["t"][0] == 0.0).all() and (sol["planes"][0] == 0.0).all()
            assert np.isnan(sol["R"][1]).all() and sol["tau"] <= G.ROTATION_FLOOR
            assert sol["n_front"].tolist() == [4, 0]


def test_reference_failures():
    fa, fb = G.failing_tuples()
    for i in range(len(fa)):
        assert G.solve(fa[i], fb[i]) is None, i
    good = G.family()
    assert G.solve(good[0][0, :3], good[1][0, :3]) is None  # fewer than four matches


# literal values of the reference sampler (seed 1, cnt 12)
PINNED_DRAWS = [[6, 8, 11, 5, 5, 9, 10, 6], [3, 9, 4, 7, 5, 6, 5, 2], [7, 9, 8, 10, 0, 0, 5, 1]]
PINNED_SAMPLES = [[6, 8, 11, 5], [3, 9, 4, 7], [7, 9, 8, 10], [3, 0, 6, 8], [4, 5, 3, 6],
                  [10, 8, 2, 7]]
PINNED_WITH_HOLE = [6, 11, 5, 9]


def test_sampler_is_pinned():
    assert G.splitmix64(1 + G.GOLDEN) == 0x910A2DEC89025CC1
    draws = [[G.draw(1, h, d, 12) for d in range(8)] for h in range(3)]
    assert draws == PINNED_DRAWS
    every = [True] * 12
    assert [G.sample(1, h, 12, every) for h in range(6)] == PINNED_SAMPLES
    # an unusable draw is passed over
    holes = list(every)
    holes[PINNED_SAMPLES[0][1]] = False
    got = G.sample(1, 0, 12, holes)
    assert got == PINNED_WITH_HOLE and PINNED_SAMPLES[0][1] not in got
    # eight draws without four distinct usable ones: void
    assert G.sample(1, 0, 4, [True] * 4) is None
    assert G.sample(1, 1, 4, [True] * 4) == [1, 3, 2, 0]
    assert G.sample(1, 0, 12, [True] * 3 + [False] * 9) is None


# the issue's scene: one plane, one motion
PLANE_N = np.array([0.1, -0.2, 1.0]) / np.linalg.norm([0.1, -0.2, 1.0])
PLANE_D = 3.0
MOTION_R = G.exp_so3(np.array([0.2, -0.3, 0.1]))
MOTION_T = np.array([0.3, -0.2, 0.5])


def _pair(rng, n, n_bad, angle):
    """n matches on the plane through the true motion, zero noise; every third
    of the first 3 n_bad an outlier: a bearing uniform on the sphere, drawn
    again until its transfer sine at the true H exceeds 10 sin(angle)."""
    fa, fb = G.planar_scene(rng, MOTION_R[None], MOTION_T[None], PLANE_N[None],
                            np.array([PLANE_D]), n)
    fa, fb = fa[0], fb[0].copy()
    H0 = G.true_h(MOTION_R, MOTION_T, PLANE_N, PLANE_D)
    bad = np.zeros(n, dtype=bool)
    bad[:3 * n_bad:3] = True
    for j in np.nonzero(bad)[0]:
        while True:
            g = rng.normal(size=3)
            g /= np.linalg.norm(g)
            e, _ = G.transfer(H0, fa[j:j + 1], g[None])
            if e[0] > (10.0 * math.sin(angle)) ** 2:
                fb[j] = g
                break
    return fa, fb, bad


def _truth_error(sol):
    return G.solution_error(sol, MOTION_R, MOTION_T, PLANE_N, PLANE_D)


def test_reference_ransac_rejects_outliers():
    rng = np.random.default_rng(11)
    n, angle = 60, 1e-6
    fa, fb, bad = _pair(rng, n, 20, angle)
    assert bad.sum() == 20
    usable = np.ones(n, dtype=bool)
    usable[5] = False
    got = G.ransac(fa, fb, usable, n_hypotheses=64, inlier_angle=angle)
    assert got["status"] == 0
    assert np.array_equal(got["mask"], ~bad & usable)
    assert got["n_inliers"] == int((~bad & usable).sum())
    err = _truth_error(got["sol"])
    herr = np.abs(got["H"] - G.true_h(MOTION_R, MOTION_T, PLANE_N, PLANE_D)).max()
    print(f"reference homography RANSAC: error {err:.3e}, |H - H_true| {herr:.3e}, winner h = "
          f"{got['h']}, refits {got['refits']}, n_front {got['sol']['n_front']}")
    assert err <= 1e-9 and herr <= 1e-9
    assert got["sol"]["count"] == 2 and got["sol"]["n_front"][0] == got["n_inliers"]
    assert G.ransac(fa[:3], fb[:3], usable[:3])["status"] == 1
    few = usable.copy()
    few[3:] = False
    assert G.ransac(fa, fb, few)["status"] == 1
    high = G.ransac(fa, fb, usable, n_hypotheses=64, inlier_angle=angle, min_inliers=n)
    assert high["status"] == 2 and high["n_inliers"] == got["n_inliers"] and high["H"] is None
    # four usable matches, three of them collinear in A: every sample is degenerate
    deg_a = np.stack([fa[1], fa[2], G._unit(fa[1] + fa[2]), fa[4]])
    none = G.ransac(deg_a, fb[[1, 2, 3, 4]], np.ones(4, dtype=bool), n_hypotheses=64)
    assert none["status"] == 2 and none["n_inliers"] == 0


def test_reference_refit_improves_a_noisy_pair():
    """With noise the minimal sample is a weak estimate: the refit must not
    lose inliers and must tighten the model."""
    rng = np.random.default_rng(12)
    n, angle, noise = 200, 4e-3, 1e-3
    fa, fb, bad = _pair(rng, n, 25, angle)
    fb = fb + noise * rng.normal(size=fb.shape) * (~bad)[:, None]
    fb /= np.linalg.norm(fb, axis=1)[:, None]
    usable = np.ones(n, dtype=bool)
    raw = G.ransac(fa, fb, usable, n_hypotheses=128, inlier_angle=angle, refit_rounds=0)
    fit = G.ransac(fa, fb, usable, n_hypotheses=128, inlier_angle=angle)
    H0 = G.true_h(MOTION_R, MOTION_T, PLANE_N, PLANE_D)
    e0, e1 = np.abs(raw["H"] - H0).max(), np.abs(fit["H"] - H0).max()
    print(f"reference homography refit: inliers {raw['n_inliers']} -> {fit['n_inliers']}, "
          f"|H - H_true| {e0:.3e} -> {e1:.3e}, {fit['refits']} rounds taken, solution error "
          f"{_truth_error(fit['sol']):.3e}")
    assert fit["n_inliers"] >= raw["n_inliers"] and fit["refits"] >= 1
    assert not fit["mask"][bad].any()
    assert e1 <= e0


# ----------------------------------------------------------- the host build
def _build(d, *flags):
    exe = str(d / ("homography_host_driver" + ("_san" if flags else "")))
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *flags, "-I", CSRC, DRIVER,
                    "-o", exe], check=True)
    return exe


def _runner(d, exe):
    def run(fa, fb):
        n, rows = fa.shape[0], fa.shape[1]
        inp, out = str(d / "in.bin"), str(d / "out.bin")
        np.concatenate([fa.reshape(n, 3 * rows), fb.reshape(n, 3 * rows)], axis=1).tofile(inp)
        subprocess.run([exe, inp, out, str(rows)], check=True)
        return np.fromfile(out).reshape(n, 45)
    return run


@pytest.fixture(scope="module")
def host_4pt(tmp_path_factory):
    d = tmp_path_factory.mktemp("homography")
    return _runner(d, _build(d))


def check_against_reference(name, res, tuples, ref, count):
    """The bounds of the module docstring for a solver under test (its raw
    rows, homography_ref.unpack's layout); prints what it measured."""
    ref_err, ref_herr, _ = ref
    assert (res[:, 0] == count).all()
    err, herr, orth, resid = G.check_solutions(G.unpack(res), *tuples)
    print(f"{name}: worst error {err.max():.3e} (reference {ref_err.max():.3e}), median "
          f"{np.median(err):.3e} (reference {np.median(ref_err):.3e}), |H - H_true| worst "
          f"{herr.max():.3e} (reference {ref_herr.max():.3e}), |R^T R - I| {orth:.1e}, "
          f"|f_b x H f_a| {resid:.1e}")
    assert orth <= 1e-12
    assert resid <= 1e-12
    assert np.median(err) <= 10.0 * np.median(ref_err)
    assert err.max() <= 100.0 * ref_err.max()
    assert np.median(herr) <= 10.0 * np.median(ref_herr)
    assert herr.max() <= 100.0 * ref_herr.max()


def test_host_build_of_the_device_solver(host_4pt):
    fa, fb = G.family()[:2]
    scale = np.linspace(0.5, 3.0, len(fa))[:, None, None]  # bearings need not be unit
    res = host_4pt(fa * scale, fb / scale)
    check_against_reference("homography.hpp on the host", res, G.family(), G.family_accuracy(), 2)


@pytest.mark.parametrize("kind", G.SPECIAL)
def test_host_build_special_families(host_4pt, kind):
    fa, fb = G.special(kind)[:2]
    res = host_4pt(np.array(fa), np.array(fb))
    check_against_reference(f"homography.hpp on the host, {kind}", res, G.special(kind),
                            G.special_accuracy(kind), 1 if kind == "rotation" else 2)
    if kind == "rotation":
        assert (res[:, 19:22] == 0.0).all() and (res[:, 34:38] == 0.0).all()  # t, the plane
        assert (res[:, 43] == 4).all() and (res[:, 44] == 0).all()


def test_host_build_failures(host_4pt):
    fa, fb = G.failing_tuples()
    res = host_4pt(fa, fb)
    assert (res[:, 0] == 0).all() and np.isnan(res[:, 1:43]).all() and (res[:, 43:] == 0).all()


def test_host_build_takes_any_row_count(host_4pt):
    """The refit feeds every inlier's rows: 5, 37 and 300 exact matches."""
    for n_rows in (5, 37, 300):
        tuples = G.random_tuples(32, n_rows=n_rows, seed=3)
        res = host_4pt(tuples[0], tuples[1])
        err, herr, _, _ = G.check_solutions(G.unpack(res), *tuples)
        print(f"homography.hpp on the host, {n_rows} rows: worst error {err.max():.3e}, "
              f"|H - H_true| {herr.max():.3e}")
        assert (res[:, 0] == 2).all() and (res[:, 43] == n_rows).all()
        assert err.max() <= 1e-11 and herr.max() <= 1e-12


def test_rotation_floor_error_curve(host_4pt):
    """The floor of homography.hpp against the error curve: above
    it the decomposition's error in (t^, n) grows like eps / tau while R stays
    at the rounding level; at and below it the motion is returned as a
    rotation, which costs an error of tau in R.  The two cross near sqrt(eps) =
    1.5e-8, the floor 2^-24 = 6e-8 sits just above."""
    rng = np.random.default_rng(7)
    n = 300
    print("tau: matched-slot error median / worst, error in R median / worst, count")
    for tau in (0.5, 3e-3, 3e-5, 3e-7, 1e-7, 3e-8, 1e-8):
        Rm = np.stack([G.exp_so3(w) for w in 0.3 * rng.normal(size=(n, 3))])
        nrm = G._unit(np.column_stack([0.5 * rng.normal(size=(n, 2)), np.ones(n)]))
        d = rng.uniform(2.0, 8.0, n)
        t = G._unit(rng.normal(size=(n, 3))) * (tau * d)[:, None]
        fa, fb = G.planar_scene(rng, Rm, t, nrm, d, 4)
        res = host_4pt(fa, fb)
        sols = G.unpack(res)
        e_r = np.array([min(np.abs(s["R"][k] - Rm[i]).max() for k in range(s["count"]))
                        for i, s in enumerate(sols)])
        above = tau > G.ROTATION_FLOOR
        assert (res[:, 0] == (2 if above else 1)).all(), tau
        if above:
            e = np.array([G.solution_error(s, Rm[i], t[i], nrm[i], d[i])
                          for i, s in enumerate(sols)])
            print(f"{tau:.0e}: {np.median(e):.1e} / {e.max():.1e}, {np.median(e_r):.1e} / "
                  f"{e_r.max():.1e}, 2")
            assert np.median(e) <= 1e3 * EPS / tau and e_r.max() <= 1e-9
            assert np.median(np.abs(res[:, 42] / tau - 1.0)) <= 1e3 * EPS / tau
        else:
            print(f"{tau:.0e}: - / -, {np.median(e_r):.1e} / {e_r.max():.1e}, 1")
            assert e_r.max() <= 2.0 * tau  # |H - R| <= tau


def test_host_build_under_sanitizers(tmp_path):
    """The stand-alone driver once more with the address and undefined-
    behaviour sanitizers: the same bits, and no report."""
    exe = _build(tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    fa, fb = G.family()[:2]
    bad_a, bad_b = G.failing_tuples()
    rot_a, rot_b = G.special("rotation")[:2]
    fa, fb = np.concatenate([fa[:256], bad_a, rot_a[:8]]), np.concatenate([fb[:256], bad_b, rot_b[:8]])
    san = _runner(tmp_path, exe)(fa, fb)
    plain = _runner(tmp_path, _build(tmp_path))(fa, fb)
    assert san.tobytes() == plain.tobytes()
