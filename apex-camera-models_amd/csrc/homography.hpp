// homography.hpp -- the two-view homography solver shared by k_homography_4pt
// and k_homography (acm.hip), f64; host-callable so that a CPU driver can run
// the same code.
//
// The route (include/acm.h, acm_homography_4pt): every match gives the three
// rows [f_b]x (x) f_a of the linear system f_b x (H f_a) = 0 (H row-major);
// the rows go through essential.hpp's streaming Givens factor R9 and its
// inverse-iteration null vector.  H is scaled so that its middle singular
// value is 1 -- the eigenpairs of the symmetric H^T H come from a cyclic Jacobi
// with a fixed number of sweeps -- and decomposed in closed form (Ma, Soatto,
// Kosecka, Sastry, An Invitation to 3-D Vision, 5.3) into two (R, t / d, n)
// with H = R + (t / d) n^T.
//
// Every array index is a compile-time constant, as in essential.hpp.
#pragma once

#include "essential.hpp"

namespace acm {
namespace homography {

using essential::kTri;

// Jacobi sweeps over the three off-diagonal entries of H^T H.  The iteration
// converges quadratically; for a 3 x 3 matrix four sweeps reach the rounding
// level and the rest cost 3 x 20 flops each.
constexpr int kJacobiSweeps = 6;
// H counts as singular when sigma_3^2 <= 2^-40 sigma_1^2: camera B would sit
// within 1e-6 of the plane's distance from the plane.
constexpr double kSingular = 0x1p-40;
// Below this baseline over plane distance the motion is returned as a
// rotation (the decomposition's error eps / tau crosses the
// error tau of calling it a rotation near sqrt(eps) = 1.5e-8; 2^-24 = 6e-8).
constexpr double kRotationFloor = 0x1p-24;
// Three of a minimal sample's four bearings within this volume of one plane
// through the centre (the points are collinear in the image, repeated matches
// included): the four matches do not determine H.
constexpr double kCollinear = 0x1p-40;

// the three rows of match (fa, fb) into the factor
ACM_ESS_FN void feed_match(double (&T)[kTri], const double (&fa)[3], const double (&fb)[3]) {
    {
        double a[9] = {0.0, 0.0, 0.0, -fb[2] * fa[0], -fb[2] * fa[1], -fb[2] * fa[2],
                       fb[1] * fa[0], fb[1] * fa[1], fb[1] * fa[2]};
        essential::feed<3>(T, a);
    }
    {
        double a[9] = {fb[2] * fa[0], fb[2] * fa[1], fb[2] * fa[2], 0.0, 0.0, 0.0,
                       -fb[0] * fa[0], -fb[0] * fa[1], -fb[0] * fa[2]};
        essential::feed<0>(T, a);
    }
    {
        double a[9] = {-fb[1] * fa[0], -fb[1] * fa[1], -fb[1] * fa[2], fb[0] * fa[0], fb[0] * fa[1],
                       fb[0] * fa[2], 0.0, 0.0, 0.0};
        essential::feed<0>(T, a);
    }
}

ACM_ESS_FN double det3(const double (&a)[3], const double (&b)[3], const double (&c)[3]) {
    return a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) +
           a[2] * (b[0] * c[1] - b[1] * c[0]);
}

// a minimal sample of unit bearings with three of them in one plane
ACM_ESS_FN bool collinear4(const double (&f0)[3], const double (&f1)[3], const double (&f2)[3],
                           const double (&f3)[3]) {
    return !(fabs(det3(f0, f1, f2)) > kCollinear && fabs(det3(f0, f1, f3)) > kCollinear &&
             fabs(det3(f0, f2, f3)) > kCollinear && fabs(det3(f1, f2, f3)) > kCollinear);
}

// g = H f
ACM_ESS_FN void apply(const double (&H)[9], double x, double y, double z, double& g0, double& g1,
                      double& g2) {
    g0 = H[0] * x + H[1] * y + H[2] * z;
    g1 = H[3] * x + H[4] * y + H[5] * z;
    g2 = H[6] * x + H[7] * y + H[8] * z;
}

// one Jacobi rotation of the symmetric A (a[0..5] = a00 a01 a02 a11 a12 a22)
// in the plane (P, Q), R the third index; V's columns follow
template <int P, int Q, int R>
ACM_ESS_FN void jacobi_rotate(double (&a)[6], double (&V)[9]) {
    constexpr int ipp = P == 0 ? 0 : (P == 1 ? 3 : 5);
    constexpr int iqq = Q == 0 ? 0 : (Q == 1 ? 3 : 5);
    constexpr int ipq = P + Q == 1 ? 1 : (P + Q == 2 ? 2 : 4);
    constexpr int irp = R + P == 1 ? 1 : (R + P == 2 ? 2 : 4);
    constexpr int irq = R + Q == 1 ? 1 : (R + Q == 2 ? 2 : 4);
    const double apq = a[ipq];
    if (apq == 0.0) return;
    const double theta = (a[iqq] - a[ipp]) / (2.0 * apq);
    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[ipp] -= t * apq;
    a[iqq] += t * apq;
    a[ipq] = 0.0;
    const double arp = a[irp], arq = a[irq];
    a[irp] = c * arp - s * arq;
    a[irq] = s * arp + c * arq;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double vp = V[3 * r + P], vq = V[3 * r + Q];
        V[3 * r + P] = c * vp - s * vq;
        V[3 * r + Q] = s * vp + c * vq;
    }
}

// lam[I] >= lam[J] afterwards, V's columns with them
template <int I, int J>
ACM_ESS_FN void order(double (&lam)[3], double (&V)[9]) {
    const bool sw = lam[J] > lam[I];
    const double l = lam[I];
    lam[I] = sw ? lam[J] : l;
    lam[J] = sw ? l : lam[J];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double v = V[3 * r + I];
        V[3 * r + I] = sw ? V[3 * r + J] : v;
        V[3 * r + J] = sw ? v : V[3 * r + J];
    }
}

// The eigenvalues of H^T H, lam[0] >= lam[1] >= lam[2], and their
// eigenvectors, V's columns: cyclic Jacobi, kJacobiSweeps sweeps.
ACM_ESS_FN void eigen(const double (&H)[9], double (&lam)[3], double (&V)[9]) {
    double a[6] = {H[0] * H[0] + H[3] * H[3] + H[6] * H[6], H[0] * H[1] + H[3] * H[4] + H[6] * H[7],
                   H[0] * H[2] + H[3] * H[5] + H[6] * H[8], H[1] * H[1] + H[4] * H[4] + H[7] * H[7],
                   H[1] * H[2] + H[4] * H[5] + H[7] * H[8], H[2] * H[2] + H[5] * H[5] + H[8] * H[8]};
#pragma unroll
    for (int i = 0; i < 9; ++i) V[i] = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        jacobi_rotate<0, 1, 2>(a, V);
        jacobi_rotate<0, 2, 1>(a, V);
        jacobi_rotate<1, 2, 0>(a, V);
    }
    lam[0] = a[0];
    lam[1] = a[3];
    lam[2] = a[5];
    order<0, 1>(lam, V);
    order<1, 2>(lam, V);
    order<0, 1>(lam, V);
}

// eigen() of an H whose middle singular value is 1 up to rounding, as
// decompose takes it: lam[1] = 1 exactly, H untouched
ACM_ESS_FN void spectrum(const double (&H)[9], double (&lam)[3], double (&V)[9]) {
    eigen(H, lam, V);
    lam[0] /= lam[1];
    lam[2] /= lam[1];
    lam[1] = 1.0;
}

// H (any scale, any sign) -> H with the middle singular value 1.  false: H is
// singular or not finite.
ACM_ESS_FN bool normalize(double (&H)[9]) {
    double lam[3], V[9];
    eigen(H, lam, V);
    if (!(lam[2] > kSingular * lam[0] && __builtin_isfinite(lam[0]))) return false;
    const double s = 1.0 / sqrt(lam[1]);
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        H[i] *= s;
        ok = ok && __builtin_isfinite(H[i]);
    }
    return ok;
}

// pos - neg over the rows decides H's sign: f_b . (H f_a) > 0 for the majority
ACM_ESS_FN int side(const double (&H)[9], const double (&fa)[3], const double (&fb)[3]) {
    double g0, g1, g2;
    apply(H, fa[0], fa[1], fa[2], g0, g1, g2);
    const double d = fb[0] * g0 + fb[1] * g1 + fb[2] * g2;
    return d > 0.0 ? 1 : (d < 0.0 ? -1 : 0);
}

ACM_ESS_FN void negate(double (&H)[9]) {
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = -H[i];
}

// The inlier rule of acm_homography_batch at H for the unit bearings: with
// g = H f_a and c = f_b x g, f_b . g > 0 and c . c <= sin2 g . g; e = the
// squared sine c . c / g . g.
ACM_ESS_FN bool inlier(const double (&H)[9], double ax, double ay, double az, double bx, double by,
                       double bz, double sin2, double& e) {
    double g0, g1, g2;
    apply(H, ax, ay, az, g0, g1, g2);
    const double c0 = by * g2 - bz * g1, c1 = bz * g0 - bx * g2, c2 = bx * g1 - by * g0;
    const double cc = c0 * c0 + c1 * c1 + c2 * c2, gg = g0 * g0 + g1 * g1 + g2 * g2;
    if (!(bx * g0 + by * g1 + bz * g2 > 0.0 && cc <= sin2 * gg)) return false;
    e = cc / gg;
    return true;
}

// one (R, t / d, n) of the decomposition, n's sign still open
struct Motion {
    double R[9], td[3], n[3];
};

// Motion M from u = a v1 + b v3 (unit), see the file comment
ACM_ESS_FN void motion_from(const double (&H)[9], const double (&V)[9], double a, double b,
                            Motion& M) {
    const double v2[3] = {V[1], V[4], V[7]};
    const double u[3] = {a * V[0] + b * V[2], a * V[3] + b * V[5], a * V[6] + b * V[8]};
    const double w[3] = {v2[1] * u[2] - v2[2] * u[1], v2[2] * u[0] - v2[0] * u[2],
                         v2[0] * u[1] - v2[1] * u[0]};  // v2 x u = n
    double p[3], q[3];
    apply(H, v2[0], v2[1], v2[2], p[0], p[1], p[2]);
    apply(H, u[0], u[1], u[2], q[0], q[1], q[2]);
    const double r[3] = {p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2],
                         p[0] * q[1] - p[1] * q[0]};
    // R = W U^T = p v2^T + q u^T + r w^T
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) M.R[3 * i + j] = p[i] * v2[j] + q[i] * u[j] + r[i] * w[j];
    }
    essential::orthonormalize(M.R);
    double hn[3], rn[3];
    apply(H, w[0], w[1], w[2], hn[0], hn[1], hn[2]);
    apply(M.R, w[0], w[1], w[2], rn[0], rn[1], rn[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        M.td[i] = hn[i] - rn[i];
        M.n[i] = w[i];
    }
}

// The normalised H with its eigenpairs -> tau = sigma_1 - sigma_3 and either
// two motions (returns 2) or, at tau <= kRotationFloor, the rotation alone in
// A (returns 1: A.td = A.n = 0).  0: not finite.
ACM_ESS_FN int decompose(const double (&H)[9], const double (&lam)[3], const double (&V)[9],
                         Motion& A, Motion& B, double& tau) {
    tau = (lam[0] - lam[2]) / (sqrt(lam[0]) + sqrt(lam[2]));
    if (!__builtin_isfinite(tau)) return 0;
    int count;
    if (tau <= kRotationFloor) {
#pragma unroll
        for (int i = 0; i < 9; ++i) A.R[i] = H[i];
        essential::orthonormalize(A.R);
#pragma unroll
        for (int i = 0; i < 3; ++i) A.td[i] = A.n[i] = 0.0;
        B = A;
        count = 1;
    } else {
        double a = sqrt(fmax(1.0 - lam[2], 0.0)), b = sqrt(fmax(lam[0] - 1.0, 0.0));
        const double nr = sqrt(a * a + b * b);
        a /= nr;
        b /= nr;
        motion_from(H, V, a, b, A);
        motion_from(H, V, a, -b, B);
        count = 2;
    }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) ok = ok && __builtin_isfinite(A.R[i]) && __builtin_isfinite(B.R[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
        ok = ok && __builtin_isfinite(A.td[i]) && __builtin_isfinite(B.td[i]) &&
             __builtin_isfinite(A.n[i]) && __builtin_isfinite(B.n[i]);
    return ok ? count : 0;
}

// what the rows say about the plane's side: per motion the rows with
// n . f_a > 0, those with n . f_a < 0, and the sum of n . f_a
struct Front {
    int pos0 = 0, neg0 = 0, pos1 = 0, neg1 = 0;
    double sum0 = 0.0, sum1 = 0.0;
};

ACM_ESS_FN void front_add(const Motion& A, const Motion& B, const double (&fa)[3], Front& f) {
    const double d0 = A.n[0] * fa[0] + A.n[1] * fa[1] + A.n[2] * fa[2];
    const double d1 = B.n[0] * fa[0] + B.n[1] * fa[1] + B.n[2] * fa[2];
    f.pos0 += d0 > 0.0 ? 1 : 0;
    f.neg0 += d0 < 0.0 ? 1 : 0;
    f.pos1 += d1 > 0.0 ? 1 : 0;
    f.neg1 += d1 < 0.0 ? 1 : 0;
    f.sum0 += d0;
    f.sum1 += d1;
}

// motion M signed by s as output slot: the pose (R, t^), the plane (n, d / |t|)
ACM_ESS_FN void slot(const Motion& M, double s, double* pose12, double* plane4) {
    const double len = sqrt(M.td[0] * M.td[0] + M.td[1] * M.td[1] + M.td[2] * M.td[2]);
#pragma unroll
    for (int i = 0; i < 9; ++i) pose12[i] = M.R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        pose12[9 + i] = s * M.td[i] / len;
        plane4[i] = s * M.n[i];
    }
    plane4[3] = 1.0 / len;
}

// The outputs of a decomposition (count from decompose, f over `rows` rows):
// poses 24 doubles, planes 8, n_front 2.  (t, n)'s sign per motion: the one
// with more rows in front, a tie takes +; the motions ordered by n_front
// descending, then by the signed sum descending.  Returns the count, 0 when a
// slot is not finite (everything NaN then).
ACM_ESS_FN int finish(int count, const Motion& A, const Motion& B, const Front& f, long long rows,
                      double* poses24, double* planes8, unsigned (&n_front)[2]) {
    const double qnan = __builtin_nan("");
#pragma unroll
    for (int i = 0; i < 24; ++i) poses24[i] = qnan;
#pragma unroll
    for (int i = 0; i < 8; ++i) planes8[i] = qnan;
    n_front[0] = n_front[1] = 0u;
    if (count == 1) {
#pragma unroll
        for (int i = 0; i < 9; ++i) poses24[i] = A.R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) poses24[9 + i] = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) planes8[i] = 0.0;
        n_front[0] = (unsigned)rows;
    } else if (count == 2) {
        const double s0 = f.pos0 >= f.neg0 ? 1.0 : -1.0, s1 = f.pos1 >= f.neg1 ? 1.0 : -1.0;
        const int c0 = f.pos0 >= f.neg0 ? f.pos0 : f.neg0, c1 = f.pos1 >= f.neg1 ? f.pos1 : f.neg1;
        const double m0 = s0 * f.sum0, m1 = s1 * f.sum1;
        const bool swap = c1 > c0 || (c1 == c0 && m1 > m0);
        double pa[12], pb[12], qa[4], qb[4];
        slot(A, s0, pa, qa);
        slot(B, s1, pb, qb);
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            poses24[i] = swap ? pb[i] : pa[i];
            poses24[12 + i] = swap ? pa[i] : pb[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            planes8[i] = swap ? qb[i] : qa[i];
            planes8[4 + i] = swap ? qa[i] : qb[i];
        }
        n_front[0] = (unsigned)(swap ? c1 : c0);
        n_front[1] = (unsigned)(swap ? c0 : c1);
    }
    bool ok = count > 0;
    if (count == 2) {
#pragma unroll
        for (int i = 0; i < 24; ++i) ok = ok && __builtin_isfinite(poses24[i]);
#pragma unroll
        for (int i = 0; i < 8; ++i) ok = ok && __builtin_isfinite(planes8[i]);
    }
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 24; ++i) poses24[i] = qnan;
#pragma unroll
        for (int i = 0; i < 8; ++i) planes8[i] = qnan;
        n_front[0] = n_front[1] = 0u;
        return 0;
    }
    return count;
}

// From a finished factor: the normalised H, unsigned.  false: no finite,
// non-singular result.
ACM_ESS_FN bool factor_to_h(double (&T)[kTri], double (&H)[9]) {
    return essential::null_vector(T, H) && normalize(H);
}

// The model of n >= 4 matches: H normalised and signed.  fetch(i, fa, fb) ->
// bool delivers match i's unit bearings (false: the match has none; the fit
// then fails).  With n = 4 a sample with three bearings in one plane fails.
template <class Fetch>
ACM_ESS_FN bool fit_rows(long long n, Fetch fetch, double (&H)[9]) {
    double T[kTri];
    essential::clear(T);
    bool ok = n >= 4;
#pragma unroll 1
    for (long long i = 0; i < n; ++i) {
        double fa[3], fb[3];
        ok = fetch(i, fa, fb) && ok;
        feed_match(T, fa, fb);
    }
    if (ok && n == 4) {
        double a0[3], a1[3], a2[3], a3[3], b0[3], b1[3], b2[3], b3[3];
        fetch(0, a0, b0);
        fetch(1, a1, b1);
        fetch(2, a2, b2);
        fetch(3, a3, b3);
        ok = !collinear4(a0, a1, a2, a3) && !collinear4(b0, b1, b2, b3);
    }
    ok = ok && factor_to_h(T, H);
    if (!ok) return false;
    int sgn = 0;
#pragma unroll 1
    for (long long i = 0; i < n; ++i) {
        double fa[3], fb[3];
        fetch(i, fa, fb);
        sgn += side(H, fa, fb);
    }
    if (sgn < 0) negate(H);
    return true;
}

// The solver over n >= 4 matches: fit_rows, then the decomposition with the
// cheirality counts over the same matches.  Returns the count of solutions
// (0, 1, 2); on failure everything is NaN and 0.
template <class Fetch>
ACM_ESS_FN int solve_rows(long long n, Fetch fetch, double (&H)[9], double* poses24, double* planes8,
                          double& tau, unsigned (&n_front)[2]) {
    Motion A, B;
    int count = 0;
    if (fit_rows(n, fetch, H)) {
        double lam[3], V[9];
        spectrum(H, lam, V);
        count = decompose(H, lam, V, A, B, tau);
    }
    Front f;
    if (count == 2) {
#pragma unroll 1
        for (long long i = 0; i < n; ++i) {
            double fa[3], fb[3];
            fetch(i, fa, fb);
            front_add(A, B, fa, f);
        }
    }
    count = finish(count, A, B, f, n, poses24, planes8, n_front);
    if (count == 0) {
        const double qnan = __builtin_nan("");
#pragma unroll
        for (int i = 0; i < 9; ++i) H[i] = qnan;
        tau = qnan;
    }
    return count;
}

// acm_homography_4pt for one problem of n matches: bearings 3 n doubles each,
// any length (normalised here)
ACM_ESS_FN int solve(long long n, const double* bearings_a, const double* bearings_b, double* h9,
                     double* poses24, double* planes8, double* tau_out, unsigned (&n_front)[2]) {
    double H[9], tau;
    const int count = solve_rows(
        n,
        [=](long long i, double(&fa)[3], double(&fb)[3]) {
            bool ok = true;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const double* src = (s ? bearings_b : bearings_a) + 3 * i;
                double(&f)[3] = s ? fb : fa;
                const double nr = sqrt(src[0] * src[0] + src[1] * src[1] + src[2] * src[2]);
#pragma unroll
                for (int k = 0; k < 3; ++k) f[k] = src[k] / nr;
                ok = ok && nr > 0.0 && __builtin_isfinite(nr);
            }
            return ok;
        },
        H, poses24, planes8, tau, n_front);
#pragma unroll
    for (int i = 0; i < 9; ++i) h9[i] = H[i];
    if (tau_out) *tau_out = tau;
    return count;
}

}  // namespace homography
}  // namespace acm
