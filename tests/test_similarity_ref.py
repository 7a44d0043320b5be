"""The numpy restatement of acm_similarity_3pt / acm_similarity_batch
(similarity_ref.py) against ground truth, the pinned sampler, and a host build
of csrc/similarity.hpp -- the code the kernels run -- against that reference.
CPU only.

The error of a similarity is max( max|R - R_true|, max|t - t_true| / max(1,
max|t_true|), |s / s_true - 1| ).  The reference is Umeyama's SVD form, the
code under test Horn's quaternion through a cyclic Jacobi: a different
algorithm on the same conditioning.  The bounds on the solver under test come
from the reference on the same triples: median error <= 10 x the reference's
median, worst <= 100 x its worst (the factors of test_homography_ref.py).

Measured over the 4096 triples (a = 2 N + 10 N per triple, sin^2 >= 0.01 at the
first vertex, s in [0.1, 10], t = 10 N): the reference worst 4.8e-13, median
1.4e-15; the host build of similarity.hpp worst 4.0e-13, median 1.6e-15,
|R^T R - I| 1.3e-15.  Special families (200 triples each, reference worst /
median, host worst / median): s = 1e-3 1.8e-12 / 1.8e-13, 1.8e-12 / 1.8e-13;
s = 1e3 1.3e-11 / 6.9e-13, 5.0e-11 / 7.9e-13; rotation by pi - 1e-6 3.7e-14 /
1.5e-15, 6.1e-14 / 1.6e-15; identity 8.2e-14 / 4.4e-15, 7.1e-15 / 0; sin^2 =
1e-6 1.8e-9 / 5.1e-11, 3.5e-9 / 9.6e-11.  Jacobi sweeps: four miss the bounds
(worst 7.5e-6 on the family), five meet them and return the figures of eight;
similarity.hpp runs six.
"""
import os
import subprocess

import numpy as np
import pytest

import similarity_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "apex-camera-models_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "similarity_host_driver.cpp")
EPS = 2.0 ** -52


def _triples(kind):
    return G.family() if kind == "family" else G.special(kind)


def _accuracy(kind):
    return G.family_accuracy() if kind == "family" else G.special_accuracy(kind)


@pytest.mark.parametrize("kind", ("family",) + G.SPECIAL)
def test_reference_recovers_the_truth(kind):
    """The reference's own bound: 1e5 eps, times 1e3 for the thin triangle
    (its gap is 1e-4 of the family's smallest) and for s = 1e+-3 (t is then
    measured against max(1, |t|) while its error scales with s |a|)."""
    err = _accuracy(kind)
    print(f"reference similarity, {kind}: worst error {err.max():.3e}, median "
          f"{np.median(err):.3e}")
    assert np.isfinite(err).all()
    assert err.max() <= (1e8 if kind in ("thin", "scale_small", "scale_large") else 1e5) * EPS


def test_reference_failures():
    a, b = G.failing_triples()
    for i in range(len(a)):
        assert G.fit(a[i], b[i]) is None, i
    good = G.family()
    assert G.fit(good[0][0, :2], good[1][0, :2]) is None  # fewer than three points
    assert G.fit(good[0][0], good[1][0]) is not None
    # a mirrored set: a proper rotation all the same
    R, t, s = G.fit(good[0][0], good[0][0] * np.array([1.0, 1.0, -1.0]))
    assert np.linalg.det(R) > 0


# literal values of the reference sampler (seed 1, cnt 12)
PINNED_DRAWS = [[6, 8, 11, 5, 5, 9], [10, 6, 3, 9, 4, 7], [5, 6, 5, 2, 7, 9]]
PINNED_SAMPLES = [[6, 8, 11], [10, 6, 3], [5, 6, 2]]


def test_sampler_is_pinned():
    """ctr = 6 h + d + 1: the draws are homography_ref's stream (ctr = 8 h + d
    + 1, pinned in test_homography_ref.py) cut into sixes."""
    draws = [[G.draw(1, h, d, 12) for d in range(6)] for h in range(3)]
    assert draws == PINNED_DRAWS
    every = [True] * 12
    assert [G.sample(1, h, 12, every) for h in range(3)] == PINNED_SAMPLES
    holes = list(every)
    holes[8] = False  # an unusable draw is passed over
    assert G.sample(1, 0, 12, holes) == [6, 11, 5]
    # six draws without three distinct usable ones: void
    assert G.sample(1, 0, 12, [False] * 5 + [True] * 2 + [False] * 5) is None


def test_reference_ransac_rejects_outliers():
    rng = np.random.default_rng(11)
    a, b, R0, t0, s0, far = G.scene(rng, 60, noise=0.0)
    b[5] = np.nan
    got = G.ransac(a, b, 1e-6, n_hypotheses=64)
    clean = ~far & G.usable_rows(a, b)
    assert got["status"] == G.OK and got["n_usable"] == 59
    assert np.array_equal(got["mask"], clean) and got["n_inliers"] == int(clean.sum())
    err = G.model_error(got["model"], R0, t0, s0)
    print(f"reference similarity RANSAC: error {err:.3e}, rms {got['rms']:.3e}, winner h = "
          f"{got['h']}, refits {got['refits']}")
    assert err <= 1e-12 and got["rms"] <= 1e-12
    assert G.ransac(a[:2], b[:2], 1e-6)["status"] == G.TOO_FEW_POINTS
    high = G.ransac(a, b, 1e-6, n_hypotheses=64, min_inliers=60)
    assert high["status"] == G.NO_MODEL and high["n_inliers"] == got["n_inliers"]
    line = np.outer(np.linspace(-1.0, 1.0, 20), [1.0, 2.0, -1.0]) + 5.0
    none = G.ransac(line, 2.0 * line, 1e-6, n_hypotheses=64)
    assert none["status"] == G.NO_MODEL and none["n_inliers"] == 0


def test_reference_refit_improves_a_noisy_set():
    rng = np.random.default_rng(12)
    a, b, R0, t0, s0, far = G.scene(rng, 200)
    raw = G.ransac(a, b, 0.04, refit_rounds=0)
    fit = G.ransac(a, b, 0.04)
    e0, e1 = G.model_error(raw["model"], R0, t0, s0), G.model_error(fit["model"], R0, t0, s0)
    print(f"reference similarity refit: inliers {raw['n_inliers']} -> {fit['n_inliers']}, error "
          f"{e0:.3e} -> {e1:.3e}, {fit['refits']} rounds taken")
    assert fit["n_inliers"] >= raw["n_inliers"] and fit["refits"] >= 1
    assert not fit["mask"][far].any()
    assert e1 <= e0


# ----------------------------------------------------------- the host build
def _build(d, *flags):
    exe = str(d / ("similarity_host_driver" + ("_san" if flags else "")))
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *flags, "-I", CSRC, DRIVER,
                    "-o", exe], check=True)
    return exe


def _runner(d, exe):
    def run(a, b, rigid=False, mode="3pt"):
        """a, b (n, rows, 3) -> (n, 14): count, then the similarity"""
        n, rows = a.shape[0], a.shape[1]
        inp, out = str(d / "in.bin"), str(d / "out.bin")
        np.concatenate([a.reshape(n, 3 * rows), b.reshape(n, 3 * rows)], axis=1).tofile(inp)
        subprocess.run([exe, inp, out, str(rows), "1" if rigid else "0", mode], check=True)
        return np.fromfile(out).reshape(n, 14)
    return run


@pytest.fixture(scope="module")
def host_3pt(tmp_path_factory):
    d = tmp_path_factory.mktemp("similarity")
    return _runner(d, _build(d))


def solver_errors(res, a, b, R0, t0, s0):
    """(error (n,), |R^T R - I| worst, the smallest det R, the worst |b - (s R
    a + t)| / max(1, |b|) over the points) of a solver's rows (n, 14)."""
    err = np.empty(len(res))
    orth, det, resid = 0.0, np.inf, 0.0
    for i, row in enumerate(res):
        m = G.unpack(row[1:])
        err[i] = G.model_error(m, R0[i], t0[i], s0[i])
        orth = max(orth, np.abs(m[0].T @ m[0] - np.eye(3)).max())
        det = min(det, np.linalg.det(m[0]))
        e = np.linalg.norm(b[i] - G.apply(m, a[i]), axis=1) / np.maximum(1.0, np.linalg.norm(b[i], axis=1))
        resid = max(resid, e.max())
    return err, orth, det, resid


def check_against_reference(name, res, triples, ref_err):
    """The bounds of the module docstring for a solver under test (rows of
    count, similarity); prints what it measured."""
    assert (res[:, 0] == 1).all()
    err, orth, det, resid = solver_errors(res, *triples)
    print(f"{name}: worst error {err.max():.3e} (reference {ref_err.max():.3e}), median "
          f"{np.median(err):.3e} (reference {np.median(ref_err):.3e}), |R^T R - I| {orth:.1e}, "
          f"det R >= {det:.6f}, |b - (s R a + t)| / max(1, |b|) {resid:.1e}")
    assert orth <= 1e-12
    assert det > 0
    assert resid <= 1e-10
    assert np.median(err) <= 10.0 * np.median(ref_err)
    assert err.max() <= 100.0 * ref_err.max()


def test_host_build_of_the_device_solver(host_3pt):
    a, b = G.family()[:2]
    check_against_reference("similarity.hpp on the host", host_3pt(a, b), G.family(),
                            G.family_accuracy())


@pytest.mark.parametrize("kind", G.SPECIAL)
def test_host_build_special_families(host_3pt, kind):
    a, b = G.special(kind)[:2]
    check_against_reference(f"similarity.hpp on the host, {kind}", host_3pt(a, b), G.special(kind),
                            G.special_accuracy(kind))


def test_host_build_failures(host_3pt):
    a, b = G.failing_triples()
    for rigid in (False, True):
        res = host_3pt(a, b, rigid=rigid)
        assert (res[:, 0] == 0).all() and np.isnan(res[:, 1:]).all()


def test_host_build_rigid(host_3pt):
    """The rigid flag: s == 1.0 exactly, R and t the reference's rigid fit to
    the same factors.  The scene is rigid (s_true = 1)."""
    a, _, R0, t0, _ = G.family()
    a, R0, t0 = a[:512], R0[:512], t0[:512]
    s0 = np.ones(len(a))
    b = np.einsum("nij,nkj->nki", R0, a) + t0[:, None, :]
    res = host_3pt(a, b, rigid=True)
    assert (res[:, 13] == 1.0).all()
    check_against_reference("similarity.hpp on the host, rigid", res, (a, b, R0, t0, s0),
                            G.reference_accuracy(a, b, R0, t0, s0, rigid=True))
    # a scaled scene under the flag still returns s = 1
    assert (host_3pt(a[:8], 2.0 * b[:8], rigid=True)[:, 13] == 1.0).all()


def test_host_build_refit_arithmetic_far_from_the_origin(host_3pt):
    """similarity_fit from two-pass centred sums, 1e6 added to every coordinate
    of a: within 100 x the reference's worst over the four sets.  A raw-moment
    one-pass form loses |a|^2 / spread^2 = 1e11 here and fails."""
    ref, got = [], []
    for n in (3, 4, 257, 1025):
        a, b, R0, t0, s0 = G.offset_set(n)
        ref.append(G.model_error(G.fit(a, b), R0, t0, s0))
        res = host_3pt(a[None], b[None], mode="fit")
        assert res[0, 0] == 1, n
        got.append(G.model_error(G.unpack(res[0, 1:]), R0, t0, s0))
        print(f"similarity.hpp fit, {n} points at 1e6: error {got[-1]:.3e}, reference {ref[-1]:.3e}")
    assert max(got) <= 100.0 * max(ref)
    # the reference itself stays meaningful: R is off by eps |a| / spread from
    # b's rounding, t = bm - s R am by |a| times that, about 2e-4 absolute
    assert max(ref) <= 1e-3


def test_host_build_under_sanitizers(tmp_path):
    """The stand-alone driver once more with the address and undefined-
    behaviour sanitizers: the same bits, and no report."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    if subprocess.run(["g++", *flags, str(probe), "-o", str(tmp_path / "probe")],
                      capture_output=True).returncode != 0:
        pytest.skip("the compiler has no address / undefined-behaviour sanitizer runtime")
    exe = _build(tmp_path, *flags)
    a, b = G.family()[:2]
    bad_a, bad_b = G.failing_triples()
    a, b = np.concatenate([a, bad_a]), np.concatenate([b, bad_b])
    san = _runner(tmp_path, exe)(a, b)
    plain = _runner(tmp_path, _build(tmp_path))(a, b)
    assert san.tobytes() == plain.tobytes()
    off_a, off_b = G.offset_set(1025)[:2]
    san = _runner(tmp_path, exe)(off_a[None], off_b[None], mode="fit")
    plain = _runner(tmp_path, _build(tmp_path))(off_a[None], off_b[None], mode="fit")
    assert san.tobytes() == plain.tobytes()
