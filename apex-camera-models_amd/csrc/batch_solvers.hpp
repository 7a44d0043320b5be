// batch_solvers.hpp -- what the batched geometry solvers of acm.hip share
// (k_pose_normal_eq, k_triangulate, k_pose_batch, k_calib_*, k_pose_estimate,
// k_relative_pose): the upper-triangle Cholesky solve, the pose transform and
// Jacobian rows, the normal-equation sums, the Levenberg-Marquardt step as
// pure functions over caller-owned arrays, the clamped CSR range, and
// RANSAC's sample draw and key order.  One definition of each; the kernels
// keep their state where they need it (registers, LDS) and call in.
//
// Self-contained and host-callable, as p3p.hpp and essential.hpp are
// (tests/batch_solvers_host_driver.cpp builds it with g++).  The library is
// built with -ffp-contract=off, so the same operation order gives the same
// bits on the host and on the device; the host driver pins chol_ut and the LM
// pieces against lm_core.hpp's cholesky_solve / consume / advance that way.
#pragma once

#include <math.h>
#include <stdint.h>

#include "acm.h"

#if defined(__HIPCC__)
#define ACM_BS_FN __host__ __device__ __forceinline__
#else
#define ACM_BS_FN inline
#endif

namespace acm {

// index of (r, q) in the row-by-row upper triangle of a symmetric P x P
template <int P>
ACM_BS_FN constexpr int ut(int r, int q) {
    return r <= q ? r * P - r * (r - 1) / 2 + (q - r) : q * P - q * (q - 1) / 2 + (r - q);
}

// A x = b for the symmetric P x P A (upper triangle, P (P + 1) / 2) by
// Cholesky, in lm::cholesky_solve's operation order, every index a
// compile-time constant after unrolling; false when A is not positive
// definite (x is then untouched).  For P = 3 the layout is [00 01 02 11 12 22].
template <int P>
ACM_BS_FN bool chol_ut(const double* A, const double* b, double* x) {
    double L[P * (P + 1) / 2];  // lower triangle, (i, j) at ut(j, i)
#pragma unroll
    for (int i = 0; i < P; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = A[ut<P>(j, i)];
#pragma unroll
            for (int q = 0; q < j; ++q) s -= L[ut<P>(q, i)] * L[ut<P>(q, j)];
            if (i == j) {
                if (!(s > 0.0)) return false;
                L[ut<P>(i, i)] = sqrt(s);
            } else {
                L[ut<P>(j, i)] = s / L[ut<P>(j, j)];
            }
        }
    }
    double y[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
        double s = b[i];
#pragma unroll
        for (int q = 0; q < i; ++q) s -= L[ut<P>(q, i)] * y[q];
        y[i] = s / L[ut<P>(i, i)];
    }
#pragma unroll
    for (int i = P - 1; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int q = i + 1; q < P; ++q) s -= L[ut<P>(i, q)] * x[q];
        x[i] = s / L[ut<P>(i, i)];
    }
    return true;
}

// p = R X + t for the 12 doubles of a pose (R row-major, then t)
ACM_BS_FN void transform_point(const double* P12, double X, double Y, double Z, double& px,
                               double& py, double& pz) {
    px = P12[0] * X + P12[1] * Y + P12[2] * Z + P12[9];
    py = P12[3] * X + P12[4] * Y + P12[5] * Z + P12[10];
    pz = P12[6] * X + P12[7] * Y + P12[8] * Z + P12[11];
}

// The pose Jacobian's two rows for a left perturbation (rho, phi): with
// ju = du/dp, jv = dv/dp at p, row j of Jp gives (j, p x j).
ACM_BS_FN void pose_rows(const double* ju, const double* jv, double px, double py, double pz,
                         double* a, double* b) {
    a[0] = ju[0];
    a[1] = ju[1];
    a[2] = ju[2];
    a[3] = py * ju[2] - pz * ju[1];
    a[4] = pz * ju[0] - px * ju[2];
    a[5] = px * ju[1] - py * ju[0];
    b[0] = jv[0];
    b[1] = jv[1];
    b[2] = jv[2];
    b[3] = py * jv[2] - pz * jv[1];
    b[4] = pz * jv[0] - px * jv[2];
    b[5] = px * jv[1] - py * jv[0];
}

// One observation's rows a, b (of u and v) and residuals r0, r1 into
// acc = [J^T J upper triangle | J^T r (P) | r.r | n]
template <int P>
ACM_BS_FN void normal_eq_accumulate(double* acc, const double* a, const double* b, double r0,
                                    double r1) {
    constexpr int T = P * (P + 1) / 2;
    int k = 0;
#pragma unroll
    for (int r = 0; r < P; ++r) {
#pragma unroll
        for (int q = r; q < P; ++q, ++k) acc[k] = fma(a[r], a[q], fma(b[r], b[q], acc[k]));
    }
#pragma unroll
    for (int r = 0; r < P; ++r) acc[T + r] = fma(a[r], r0, fma(b[r], r1, acc[T + r]));
    acc[T + P] = fma(r0, r0, fma(r1, r1, acc[T + P]));
    acc[T + P + 1] += 1.0;
}

// Entries i, i + 1 of a CSR offset array as a range inside [0, n], whatever
// they hold: nothing indexed through it reads out of bounds.
ACM_BS_FN void clamped_range(const int64_t* offs, size_t i, size_t n, long long& begin,
                             long long& count) {
    const long long nn = (long long)n;
    long long b = offs[i], e = offs[i + 1];
    b = b < 0 ? 0 : (b > nn ? nn : b);
    e = e < b ? b : (e > nn ? nn : e);
    begin = b;
    count = e - b;
}

// ---------------------------------------------------- Levenberg-Marquardt
// The arithmetic of lm_core.hpp's consume / advance without bounds, for a
// compile-time P and A = J^T J held as its upper triangle.  No state of its
// own: the caller owns x, A, g, F, mu, nu, dmax and the iteration count.
namespace lm {

enum : int { GAIN_ACCEPT = 0, GAIN_REJECT = 1, GAIN_FAILED = 2 };
enum : int { STEP_EVALUATE = 0, STEP_CONVERGED = 1, STEP_EXHAUSTED = 2 };

// predicted reduction L(0) - L(h) = -(g.h + 0.5 h.A.h)
template <int P>
ACM_BS_FN double predicted_reduction(const double* A_ut, const double* g, const double* h) {
    double gh = 0.0, hAh = 0.0;
#pragma unroll
    for (int i = 0; i < P; ++i) {
        gh += g[i] * h[i];
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < P; ++j) t += A_ut[ut<P>(i, j)] * h[j];
        hAh += h[i] * t;
    }
    return -(gh + 0.5 * hAh);
}

// The gain ratio of a trial with cost Fn against the accepted cost F; -1
// (reject) when the trial's cost is not finite, the model predicts no
// reduction, or the caller's own rule says the two costs do not compare
// (`comparable` false: the trial lost valid observations).
ACM_BS_FN double gain_ratio(double F, double Fn, double pred, bool comparable) {
    return (__builtin_isfinite(Fn) && pred > 0.0 && comparable) ? (F - Fn) / pred : -1.0;
}

// Nielsen's damping update on the gain ratio: accept (rho > 0) shrinks mu,
// reject grows it, and a damping that leaves 1e32 or the finite numbers fails.
ACM_BS_FN int gain_update(double rho, double& mu, double& nu) {
    if (rho > 0.0) {
        const double t = 2.0 * rho - 1.0;
        mu *= fmax(1.0 / 3.0, 1.0 - t * t * t);
        nu = 2.0;
        return GAIN_ACCEPT;
    }
    mu *= nu;
    nu *= 2.0;
    return (!__builtin_isfinite(mu) || mu > 1e32) ? GAIN_FAILED : GAIN_REJECT;
}

// After a point is accepted (g its gradient): does a tolerance end the run?
// The cost test applies to an accepted trial step only, not to the start.
template <int P>
ACM_BS_FN bool accepted_terminates(const double* g, double gtol, bool trial, double dF, double Fold,
                                   double ctol) {
    // max |g_k| folded from the last entry (k_triangulate's order): fmax skips
    // a NaN entry, and a gradient that is NaN throughout stays NaN and meets
    // no tolerance (lm_core.hpp's ginf starts at 0 and would let it pass)
    double gi = fabs(g[P - 1]);
#pragma unroll
    for (int k = P - 2; k >= 0; --k) gi = fmax(fabs(g[k]), gi);
    if (gi <= gtol) return true;
    return trial && dF <= ctol * Fold;
}

// From the accepted point x (A, g there) to the next point to evaluate:
// (A + mu max(diag A, 1e-12 max(dmax, 1))) h = -g, a failed factorization
// raising the damping and trying again, each try one iteration.
// STEP_EVALUATE: xn = x + h is to be evaluated; STEP_CONVERGED: the step is
// below the parameter tolerance; STEP_EXHAUSTED: no iteration is left.
template <int P>
ACM_BS_FN int next_step(const double* A_ut, const double* g, const double* x, double& mu, double& nu,
                        double dmax, double ptol, int& it, int max_it, double* xn, double* h) {
    constexpr int T = P * (P + 1) / 2;
    while (it < max_it) {
        ++it;
        double Ad[T], mg[P], hs[P];
#pragma unroll
        for (int k = 0; k < T; ++k) Ad[k] = A_ut[k];
        const double floor_d = 1e-12 * fmax(dmax, 1.0);
#pragma unroll
        for (int k = 0; k < P; ++k) {
            Ad[ut<P>(k, k)] += mu * fmax(Ad[ut<P>(k, k)], floor_d);
            mg[k] = -g[k];
        }
        if (!chol_ut<P>(Ad, mg, hs)) {
            mu *= nu;
            nu *= 2.0;
            continue;
        }
        double hn = 0.0, xnorm = 0.0;
#pragma unroll
        for (int k = 0; k < P; ++k) {
            xn[k] = x[k] + hs[k];
            h[k] = xn[k] - x[k];
            hn += h[k] * h[k];
            xnorm += x[k] * x[k];
        }
        hn = sqrt(hn);
        xnorm = sqrt(xnorm);
        return hn <= ptol * (xnorm + ptol) ? STEP_CONVERGED : STEP_EVALUATE;
    }
    return STEP_EXHAUSTED;
}

}  // namespace lm

// ------------------------------------------------------------------ RANSAC
namespace ransac {

ACM_BS_FN unsigned long long mix(unsigned long long z) {  // splitmix64's finalizer
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

ACM_BS_FN unsigned long long mul_hi(unsigned long long a, unsigned long long b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (unsigned long long)(((unsigned __int128)a * b) >> 64);
#endif
}

// Draw d of hypothesis h, a local index in [0, cnt): counter-based, so a
// hypothesis' sample depends on (seed, h) alone, not on which lane runs it.
ACM_BS_FN long long draw(unsigned long long seed, int h, int d, int draws_per_hypothesis,
                         long long cnt) {
    const unsigned long long ctr = (unsigned long long)draws_per_hypothesis * (unsigned long long)h +
                                   (unsigned long long)d + 1ull;
    return (long long)mul_hi(mix(seed + ctr * 0x9E3779B97F4A7C15ull), (unsigned long long)cnt);
}

// What a hypothesis is judged by: more inliers, then the smaller score, then
// the earlier hypothesis h, then the earlier solution k of that hypothesis
// (0 where a hypothesis has one solution).  count = -1: no model.
struct Key {
    int count;
    double score;
    int h, k;
};

// a wins over b.  Strict; total over keys with a model, which differ in
// (h, k); keys without a model (count -1) are all alike and lose to the rest.
ACM_BS_FN bool better(const Key& a, const Key& b) {
    return a.count > b.count ||
           (a.count == b.count && a.count >= 0 &&
            (a.score < b.score || (a.score == b.score && (a.h < b.h || (a.h == b.h && a.k < b.k)))));
}

}  // namespace ransac
}  // namespace acm

#undef ACM_BS_FN
