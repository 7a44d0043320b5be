"""Pins tests/normal_equations_ref.py before it judges a kernel: the CPU
oracle's normal equations (f64 terms, summed in point order) pass its check
at every camera with room to spare, and the check sees what the older
largest-entry rule lets through.

Measured (worst |oracle - exact| / bound over n = 246 and 1000, both
policies): see CHANGELOG.md; the worst camera is ds_alpha_half.
"""
import numpy as np
import pytest

import camera_zoo as Z
import normal_equations_ref as N
from apex_camera_models import samples

ALL_MODELS = tuple(sorted(samples.SAMPLES))
CAMERAS = ALL_MODELS + Z.NAMES
SIZES = (246, 1000)
# The oracle is the plain-f64 evaluation of the same formulas: what any
# correct f64 kernel can reach.  Measured <= 4.5e-2 (ds_alpha_half); the cap
# keeps a later edit of the helper from silently loosening what it proves.
ORACLE_CAP = 0.1


def test_there_are_26_cameras():
    assert len(CAMERAS) == 26 and len(set(CAMERAS)) == 26


@pytest.mark.parametrize("key", CAMERAS, ids=Z.label)
def test_oracle_passes_the_entrywise_bound(key):
    pts = N.base_points(key)
    assert pts.shape == (246, 3) and np.isfinite(pts).all()
    assert np.array_equal(N.points(key, 257)[246:], pts[:11])
    _, _, validb = N.base_terms(key)
    assert int(validb.sum()) >= 240
    worst = 0.0
    for n in SIZES:
        for policy in (0, 1):
            want, mag, n_valid = N.exact(key, n, policy)
            got = N.oracle_result(key, n, policy)
            assert got[-1] == n_valid == int(validb[np.arange(n) % 246].sum())
            worst = max(worst, N.check(got, want, mag, n_valid))
    print(f"oracle NE {Z.label(key)}: {int(validb.sum())} of 246 base rows valid, "
          f"worst |oracle - exact| / bound = {worst:.3e}")
    assert worst <= ORACLE_CAP


def test_sentinel_adds_1e12_per_invalid_point_to_the_cost_only():
    key, n = 3, 1000
    w0, m0, nv = N.exact(key, n, 0)
    w1, m1, nv1 = N.exact(key, n, 1)
    assert nv == nv1 < n
    assert np.array_equal(w0[:-1], w1[:-1]) and np.array_equal(m0[:-1], m1[:-1])
    assert abs((w1[-1] - w0[-1]) - 1e12 * (n - nv)) <= np.spacing(w1[-1])


def test_empty_problem_is_all_zero():
    want, mag, n_valid = N.exact(2, 0, 1)
    assert n_valid == 0 and not want.any() and not mag.any()
    assert N.check(np.zeros(8 * 8 + 8 + 2), want, mag, 0) == 0.0
    bad = np.zeros(8 * 8 + 8 + 2)
    bad[7 * 8 + 7] = 1e-300
    with pytest.raises(AssertionError):
        N.check(bad, want, mag, 0)


# model, the entry: KB (k4, k4), RadTan (k3, k3), DS (alpha, alpha)
@pytest.mark.parametrize("key,entry", [(2, 7), (1, 8), (3, 4)])
def test_check_sees_what_the_largest_entry_rule_lets_through(key, entry):
    """One well-conditioned entry of the oracle's own result off by 1e-7
    relative fails the entrywise bound, whichever entry it is; the older rule
    (1e-10 of the block's largest entry) passes it on the small entries."""
    n = 1000
    want, mag, n_valid = N.exact(key, n, 0)
    P = N.num_params(want)
    ref = N.oracle_result(key, n, 0)
    assert N.check(ref, want, mag, n_valid) <= ORACLE_CAP
    A = np.abs(want[:P * P])
    # the named distortion entry, and the smallest entry that does not cancel
    # (structural zeros and the n_valid entries aside): on this point set the
    # named entries are among the largest of their J^T J (KB's (k4, k4) IS the
    # largest: theta reaches 1.3 rad, theta^18 ~ 100), so the older rule
    # already holds them to 1e-10 ... 1e-8 and it is the small entries, (fx, fx)
    # and its like, that it leaves unpinned
    cand = [s for s in range(P * P) if A[s] >= 0.1 * mag[s] > 0 and s not in (2 * P + 2, 3 * P + 3)]
    small = min(cand, key=lambda s: A[s])
    named = entry * P + entry
    assert named in cand, "the named entry cancels: not a fair probe"
    for slot in (named, small):
        bad = ref.copy()
        bad[slot] *= 1 + 1e-7
        r, c = divmod(slot, P)
        bad[c * P + r] = bad[slot]  # keep it symmetric: only the value is wrong
        old = N.passes_largest_entry_rule(bad, ref, P)
        print(f"{Z.label(key)} entry ({r}, {c}) = {want[slot]:.3e} (largest {A.max():.3e}) x (1 + 1e-7): "
              f"largest-entry rule {'passes' if old else 'fails'} it, entrywise ratio "
              f"{float(N.ratios(bad, want, mag)[slot]):.1f}")
        with pytest.raises(AssertionError):
            N.check(bad, want, mag, n_valid)
        # 1e-7 / 1e-10, less the oracle's own error
        assert float(N.ratios(bad, want, mag)[slot]) >= 900.0
        if slot == small:
            assert A[small] <= 1e-4 * A.max()
            assert old, "the older rule should let a 1e-7 error on the smallest entry through"


def test_check_rejects_each_structural_fault():
    key, n = 5, 246
    want, mag, n_valid = N.exact(key, n, 0)
    P = N.num_params(want)
    ref = N.oracle_result(key, n, 0)
    N.check(ref, want, mag, n_valid)
    for slot, value in ((0 * P + 1, 1e-30),              # a structural zero
                        (2 * P + 2, n_valid - 1.0),      # (cx, cx)
                        (P * P + P + 1, n_valid + 1.0),  # the last slot
                        (4 * P + 5, np.nextafter(ref[4 * P + 5], np.inf))):  # symmetry
        bad = ref.copy()
        bad[slot] = value
        with pytest.raises(AssertionError):
            N.check(bad, want, mag, n_valid)
