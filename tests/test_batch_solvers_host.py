"""csrc/batch_solvers.hpp on the host (no GPU): the pieces the batched solvers'
kernels share, built with g++ -ffp-contract=off as the library is, against
what they claim to restate.

* chol_ut<P> against lm::cholesky_solve, byte for byte: the kernels' comments
  have long said "lm::cholesky_solve's operation order"; this is the check.
* the LM pieces (predicted_reduction, gain_ratio / gain_update,
  accepted_terminates, next_step), assembled into the loop k_triangulate and
  k_pose_batch run, against lm_core.hpp's start / consume / advance without
  bounds: the same evaluation points, final x, iteration count and class of
  stop reason.
* ransac::better: a strict order, total on keys that carry a model, and a
  pairwise tree finds the scan's winner whatever the order of the leaves.
* ransac::draw against the Python restatements' samplers.
"""
import os
import subprocess

import numpy as np
import pytest

import pose_estimation_ref as PE
import relative_pose_ref as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "apex-camera-models_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
DRIVER = os.path.join(ROOT, "tests", "batch_solvers_host_driver.cpp")
K_MAX_EVAL = 64
K_REC = 5 + 9 + 9 * K_MAX_EVAL


def _build(d, *flags):
    exe = str(d / ("batch_solvers_host_driver" + ("_san" if flags else "")))
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *flags, "-I", CSRC, "-I", INCLUDE,
                    DRIVER, "-o", exe], check=True)
    return exe


class Driver:
    def __init__(self, d, exe):
        self.d, self.exe = d, exe

    def _run(self, mode, args, data, dtype=np.float64):
        inp, out = str(self.d / "in.bin"), str(self.d / "out.bin")
        np.ascontiguousarray(data, dtype=np.float64).tofile(inp)
        subprocess.run([self.exe, mode, *args, inp, out], check=True)
        return np.fromfile(out, dtype=dtype)

    def chol(self, P, A, b):
        n = len(A)
        res = self._run("chol", [str(P)], np.concatenate([A.reshape(n, P * P), b], axis=1))
        return res.reshape(n, 2, 1 + P)  # [:, 0]: chol_ut, [:, 1]: lm::cholesky_solve

    def lm(self, problems):
        res = self._run("lm", [], np.concatenate(problems))
        return res.reshape(len(problems), 2, K_REC)  # [:, 0]: the pieces, [:, 1]: lm_core.hpp

    def gain(self, rows):
        return self._run("gain", [], rows).reshape(len(rows), 4)  # rho, result, mu, nu

    def order(self, keys):
        return self._run("order", [], keys, np.uint8).reshape(len(keys), len(keys)).astype(bool)

    def tree(self, arrangements):
        return self._run("tree", [], arrangements).reshape(len(arrangements), 2, 4)

    def draw(self, seed, draws, cnt, H):
        out = str(self.d / "draw.bin")
        subprocess.run([self.exe, "draw", str(seed), str(draws), str(cnt), str(H), out], check=True)
        return np.fromfile(out, dtype=np.int64).reshape(H, draws)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_solvers")
    return Driver(d, _build(d))


# ------------------------------------------------------------------ Cholesky
def chol_systems(P, n=10000, seed=0):
    """n random SPD systems over twelve decades of conditioning; then, for each
    pivot position, a system whose pivot there is exactly zero and one where it
    is negative; then a NaN entry in A (each position of row 0) and in b."""
    rng = np.random.default_rng(seed + P)
    G = rng.standard_normal((n, P, P + 2))
    G *= 10.0 ** rng.uniform(-6, 6, (n, P, 1))
    A = G @ G.transpose(0, 2, 1)
    b = rng.standard_normal((n, P)) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    bad_A, bad_b = [], []
    for pos in range(P):
        for kind in ("zero", "negative"):
            # L D L^T with small integers: exact in double, so the pivot at
            # `pos` is exactly 0 or -2 after the earlier columns are removed
            L = np.tril(rng.integers(-3, 4, (P, P)).astype(float), -1) + np.eye(P)
            D = rng.integers(1, 5, P).astype(float) ** 2
            D[pos] = 0.0 if kind == "zero" else -2.0
            bad_A.append(L @ np.diag(D) @ L.T)
            bad_b.append(rng.standard_normal(P))
    for q in range(P):
        M = A[q].copy()
        M[0, q] = M[q, 0] = np.nan
        bad_A.append(M)
        bad_b.append(b[q])
    bad_A.append(A[0])
    bad_b.append(np.full(P, np.nan))
    return np.concatenate([A, np.array(bad_A)]), np.concatenate([b, np.array(bad_b)]), n


@pytest.mark.parametrize("P", [3, 6, 9])
def test_chol_ut_is_cholesky_solve_bit_for_bit(host, P):
    A, b, n = chol_systems(P)
    res = host.chol(P, A, b)
    ok = res[:, 1, 0] == 1.0
    print(f"P = {P}: {len(A)} systems, {int(ok.sum())} solved, {int((~ok).sum())} refused")
    assert res[:, 0].tobytes() == res[:, 1].tobytes()
    # the cases are what they say: the SPD ones solve (and solve A x = b), the
    # zero / negative pivots are refused, a NaN in b solves to NaN
    assert ok[:n].all()
    assert not ok[n:n + 2 * P].any()
    assert ok[-1] and np.isnan(res[-1, 0, 1:]).all()
    x = res[:n, 0, 1:]
    resid = np.abs(np.einsum("nij,nj->ni", A[:n], x) - b[:n]).max(axis=1)
    scale = np.abs(A[:n]).max(axis=(1, 2)) * np.abs(x).max(axis=1) + np.abs(b[:n]).max(axis=1)
    assert (resid <= 1e-9 * scale).all()


# ------------------------------------------------------------------------ LM
def lm_problem(P, kind, T, y, x0, max_it, ctol=1e-6, ptol=1e-8, gtol=1e-6, mu0=1e-4):
    T = np.asarray(T, dtype=float)
    return np.concatenate([[P, kind, len(y), max_it, ctol, ptol, gtol, mu0], x0, T.ravel(), y])


def lm_problems():
    """(name, problem, what must have happened) for P = 3 and 6."""
    rng = np.random.default_rng(5)
    out = []
    for P in (3, 6):
        M = 4 * P
        T = rng.uniform(-1.0, 1.0, (M, P))
        xt = rng.uniform(-0.5, 0.5, P)
        y = np.exp(T @ xt)
        # a clean fit from a near start, at several iteration limits; one
        # step from 0.1 away cannot meet a tolerance, so the limit of 1 ends it
        for max_it in (1, 2, 5, 40):
            out.append((f"P{P} fit max_it {max_it}", lm_problem(P, 0, T, y, xt + 0.1, max_it),
                        {"stop": 0} if max_it == 1 else {}))
        # all tolerances zero: runs on until the step is exactly zero or the limit
        out.append((f"P{P} no tolerance", lm_problem(P, 0, T, y, xt + 0.1, 12, 0.0, 0.0, 0.0), {}))
        # already at the optimum: the gradient test ends it at the first evaluation
        out.append((f"P{P} at optimum", lm_problem(P, 0, T, y, xt, 40), {"stop": 1, "evals": 1}))
        # a start far below the optimum of a fit with positive exponents and
        # almost no damping: the Jacobian exp(T x) T is tiny there, the
        # Gauss-Newton step is huge, the trial cost overflows: rejected
        Tp = rng.uniform(0.5, 1.0, (M, P))
        xp = np.full(P, 0.5)
        out.append((f"P{P} far start", lm_problem(P, 0, Tp, np.exp(Tp @ xp), xp - 2.0, 60, mu0=1e-12),
                    {"rejected": 1}))
        # a parameter no residual depends on, and a damping so small that
        # mu * 1e-12 max(dmax, 1) underflows to zero (dmax < 4e8): that pivot is
        # exactly zero, the factorization fails and is retried with mu times
        # 2, 4, 8, ... until the product is a positive number
        T0 = T.copy()
        T0[:, 1] = 0.0
        out.append((f"P{P} dead parameter", lm_problem(P, 0, T0, np.exp(T0 @ xt), xt + 0.1, 60,
                                                       mu0=1e-320), {"retries": 1}))
        # both at once: the retries, then the far start's rejected steps
        Tp0 = Tp.copy()
        Tp0[:, 1] = 0.0
        out.append((f"P{P} dead parameter far", lm_problem(P, 0, Tp0, np.exp(Tp0 @ xp), xp - 2.0, 60,
                                                           mu0=1e-320), {"retries": 1, "rejected": 1}))
        # every trial point evaluates to NaN: the damping grows past 1e32 (x0 =
        # 0 and no parameter tolerance, so no step is ever small against x)
        out.append((f"P{P} diverges", lm_problem(P, 1, T, y, np.zeros(P), 60, ptol=0.0),
                    {"stop": 2, "rejected": 10}))
    return out


def test_lm_pieces_walk_lm_core_s_path(host):
    cases = lm_problems()
    res = host.lm([c[1] for c in cases])
    for (name, prob, want), (pieces, core) in zip(cases, res):
        P = int(prob[0])
        evals, it, stop, rejected, retries = (int(v) for v in pieces[:5])
        print(f"{name}: {evals} evaluations, {it} iterations, stop class {stop}, "
              f"{rejected} rejected, {retries} Cholesky retries")
        assert evals <= K_MAX_EVAL
        assert pieces[:3].tobytes() == core[:3].tobytes(), name  # evaluations, iterations, class
        assert pieces[5:].tobytes() == core[5:].tobytes(), name  # final x, every evaluation point
        assert np.isfinite(pieces[5:5 + P]).all()
        if "stop" in want:
            assert stop == want["stop"], name
        if "evals" in want:
            assert evals == want["evals"], name
        assert rejected >= want.get("rejected", 0), name
        assert retries >= want.get("retries", 0), name


def test_gain_ratio_and_update_by_value(host):
    """lm_core.hpp's consume calls these two itself, so the comparison above
    cannot see an error in them: here they meet Nielsen's rule written out in
    Python floats (IEEE doubles, the same operations in the same order)."""
    GAIN_ACCEPT, GAIN_REJECT, GAIN_FAILED = 0.0, 1.0, 2.0
    inf, nan = float("inf"), float("nan")
    rows = [  # F, Fn, pred, comparable, mu, nu
        (10.0, 4.0, 8.0, 1, 1e-4, 2.0),      # rho 0.75: mu shrinks by 1 - 0.5^3
        (10.0, 4.0, 6.0, 1, 3.0, 8.0),       # rho 1: the factor is floored at 1/3
        (10.0, 9.0, 100.0, 1, 1e-4, 4.0),    # rho 0.01: t = -0.98, mu nearly doubles
        (10.0, 5.0, 10.0, 1, 7.0, 16.0),     # rho 0.5: factor exactly 1
        (10.0, 11.0, 8.0, 1, 1e-4, 2.0),     # cost went up: rho < 0, reject
        (10.0, 10.0, 8.0, 1, 1e-4, 2.0),     # no decrease: rho = 0 is a reject
        (10.0, 4.0, 0.0, 1, 1e-4, 2.0),      # the model predicts nothing
        (10.0, 4.0, -1.0, 1, 1e-4, 2.0),     # ... or an increase
        (10.0, inf, 8.0, 1, 1e-4, 2.0),      # trial cost not finite
        (10.0, nan, 8.0, 1, 1e-4, 2.0),
        (10.0, 4.0, nan, 1, 1e-4, 2.0),
        (10.0, 4.0, 8.0, 0, 1e-4, 2.0),      # not comparable: rejected whatever the cost
        (10.0, 11.0, 8.0, 1, 5e31, 2.0),     # mu -> 1e32 exactly: not above, goes on
        (10.0, 11.0, 8.0, 1, 5e31, 2.5),     # mu -> 1.25e32: failed
        (10.0, 11.0, 8.0, 1, 1e200, 1e200),  # mu -> inf: failed
    ]
    got = host.gain(np.array(rows, dtype=float))
    for (F, Fn, pred, comparable, mu, nu), (rho, res, mu2, nu2) in zip(rows, got):
        ok = np.isfinite(Fn) and pred > 0.0 and comparable
        want_rho = (F - Fn) / pred if ok else -1.0
        assert rho == want_rho, (F, Fn, pred, comparable)
        if want_rho > 0.0:
            t = 2.0 * want_rho - 1.0
            want = (GAIN_ACCEPT, mu * max(1.0 / 3.0, 1.0 - t * t * t), 2.0)
        else:
            m = mu * nu
            want = (GAIN_FAILED if (not np.isfinite(m) or m > 1e32) else GAIN_REJECT, m, nu * 2.0)
        assert (res, mu2, nu2) == want, (F, Fn, pred, comparable, mu, nu)
    # the cases are what their comments say
    assert [r[1] for r in got] == [0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2]
    assert got[0][2] == 1e-4 * 0.875 and got[1][2] == 1.0 and got[3][2] == 7.0 and got[12][2] == 1e32


# -------------------------------------------------------------------- RANSAC
def random_keys(n, rng):
    """Keys with many ties in count and score and some without a model; the
    (h, k) of the keys with a model are all different, as in the kernels."""
    count = rng.integers(-1, 4, n)
    score = rng.integers(0, 3, n) * 0.25
    hk = rng.permutation(4 * n)[:n]
    keys = np.stack([count, score, hk // 4, hk % 4], axis=1).astype(float)
    keys[count < 0, 1:] = 0.0  # what a lane without a model holds
    return keys


def test_better_is_a_strict_order(host):
    rng = np.random.default_rng(11)
    keys = random_keys(160, rng)
    B = host.order(keys)
    model = keys[:, 0] >= 0
    assert not B.diagonal().any()                      # irreflexive
    assert not (B & B.T).any()                         # asymmetric
    Bi = B.astype(np.int64)
    assert not ((Bi @ Bi > 0) & ~B).any()              # transitive
    # total on the keys with a model; a key without one loses to each of them
    # and ties with its like (there is nothing to choose between two of those)
    either = B | B.T | np.eye(len(keys), dtype=bool)
    assert either[np.ix_(model, model)].all()
    assert B[np.ix_(model, ~model)].all()
    assert (~model).sum() > 1 and not (B | B.T)[np.ix_(~model, ~model)].any()
    # the order is the documented one: count down, score up, h up, k up
    idx = np.flatnonzero(model)
    by_rule = idx[np.lexsort((keys[idx, 3], keys[idx, 2], keys[idx, 1], -keys[idx, 0]))]
    wins = B[np.ix_(idx, idx)].sum(axis=1)
    assert (idx[np.argsort(-wins, kind="stable")] == by_rule).all()


def test_tree_and_scan_agree_in_any_leaf_order(host):
    rng = np.random.default_rng(12)
    sets = [random_keys(256, rng) for _ in range(4)]
    none = np.zeros((256, 4))
    none[:, 0] = -1.0
    one = none.copy()
    one[200] = [0.0, 0.0, 7.0, 1.0]
    sets += [none, one]
    for keys in sets:
        arr = np.stack([keys] + [keys[rng.permutation(256)] for _ in range(15)] + [keys[::-1]])
        win = host.tree(arr)
        assert win[:, 0].tobytes() == win[:, 1].tobytes()          # tree == scan
        assert (win[:, 0] == win[0, 0]).all()                      # in every order
        model = keys[keys[:, 0] >= 0]
        if len(model):
            best = model[np.lexsort((model[:, 3], model[:, 2], model[:, 1], -model[:, 0]))[0]]
            assert (win[0, 0] == best).all()
        else:
            assert win[0, 0, 0] == -1.0


@pytest.mark.parametrize("ref,draws,size", [(PE, 8, 3), (RP, 16, 8)])
def test_draw_reproduces_the_python_samplers(host, ref, draws, size):
    assert ref.N_DRAWS == draws
    rng = np.random.default_rng(13)
    for seed, cnt in [(1, 5), (1, 977), (0xDEADBEEFCAFEF00D, 64), (2 ** 64 - 1, 100000), (12345, 17)]:
        H = 300
        got = host.draw(seed, draws, cnt, H)
        want = np.array([[ref.draw(seed, h, d, cnt) for d in range(draws)] for h in range(H)])
        assert (got == want).all()
        assert got.min() >= 0 and got.max() < cnt
        # the sample the kernels take from those draws (skip unusable and
        # repeated indices) is the restatement's
        usable = rng.random(cnt) < 0.8
        voids = 0
        for h in range(H):
            mine = []
            for j in got[h]:
                if usable[j] and j not in mine and len(mine) < size:
                    mine.append(int(j))
            theirs = ref.sample(seed, h, cnt, usable)
            voids += theirs is None
            assert theirs == (mine if len(mine) == size else None)
        print(f"{ref.__name__}: seed {seed:#x}, cnt {cnt}: {H - voids} of {H} samples complete")


# ---------------------------------------------------------------- sanitizers
def test_host_build_under_sanitizers(tmp_path, host):
    """The stand-alone driver once more with the address and undefined-
    behaviour sanitizers: the same bytes, and no report."""
    san = Driver(tmp_path, _build(tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for P in (3, 6, 9):
        A, b, n = chol_systems(P, n=500)
        assert san.chol(P, A, b).tobytes() == host.chol(P, A, b).tobytes()
    probs = [c[1] for c in lm_problems()]
    assert san.lm(probs).tobytes() == host.lm(probs).tobytes()
    rows = np.array([(10.0, 4.0, 8.0, 1, 1e-4, 2.0), (10.0, np.nan, 8.0, 0, 1e200, 1e200)])
    assert san.gain(rows).tobytes() == host.gain(rows).tobytes()
    rng = np.random.default_rng(14)
    keys = random_keys(256, rng)
    assert (san.order(keys[:64]) == host.order(keys[:64])).all()
    arr = np.stack([keys, keys[::-1]])
    assert san.tree(arr).tobytes() == host.tree(arr).tobytes()
    assert (san.draw(2 ** 64 - 1, 16, 100000, 64) == host.draw(2 ** 64 - 1, 16, 100000, 64)).all()
