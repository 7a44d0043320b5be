// similarity.hpp -- the least-squares 3-D similarity b ~ s R a + t (absolute
// orientation: Horn 1987, Umeyama 1991) shared by k_similarity_3pt and
// k_similarity (acm.hip), f64; host-callable so that a CPU driver can run the
// same code (tests/similarity_host_driver.cpp builds it with g++).
//
// The route (include/acm.h, acm_similarity_3pt): from the centred sums M = sum
// (b - bm)(a - am)^T and Saa = sum |a - am|^2 build Horn's symmetric 4 x 4
// matrix N, whose largest eigenvalue's eigenvector is the unit quaternion of
// the rotation that maximises sum (b - bm) . R (a - am).  The eigenpairs come
// from a cyclic Jacobi with a fixed number of sweeps.  One code path serves
// the minimal sample of three and the refit over any number of inliers.
//
// No libm beyond sqrt and fabs; a fixed operation order, so that under
// -ffp-contract=off the host build and the device return the same bits; every
// array index is a compile-time constant after unrolling.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ACM_SIM_FN __host__ __device__ __forceinline__
#else
#define ACM_SIM_FN inline
#endif

namespace acm {
namespace similarity {

// Jacobi sweeps over the six off-diagonal entries of N, no early exit.  The
// iteration converges quadratically: on the test families four sweeps miss
// the accuracy bounds (worst error 7.5e-6), five meet them and return what
// eight return, and six are run -- one to spare.
constexpr int kJacobiSweeps = 6;
// The rotation about the line of a collinear (or coincident) configuration is
// free: N's two largest eigenvalues then coincide.  The fit is void unless
// lambda_1 - lambda_2 > kGap lambda_1 (5e-16 for three collinear points, >=
// 2e-4 for a triangle with sin^2 >= 0.01 of the angle at its first vertex).
constexpr double kGap = 1e-9;
// 13 doubles per similarity: R row-major (9), t (3), s
constexpr int kDoubles = 13;
// the centred sums of a fit: M row-major (9), M[3 r + c] = sum (b - bm)_r (a - am)_c, then Saa
constexpr int kSums = 10;

// index of (i, j), i <= j, in the row-by-row upper triangle of the 4 x 4 N
ACM_SIM_FN constexpr int ut4(int i, int j) {
    return i <= j ? 4 * i - i * (i - 1) / 2 + (j - i) : 4 * j - j * (j - 1) / 2 + (i - j);
}

// one Jacobi rotation of the symmetric 4 x 4 A (upper triangle) in the plane
// (P, Q), P < Q; V's columns follow
template <int P, int Q>
ACM_SIM_FN void jacobi_rotate(double (&A)[10], double (&V)[16]) {
    const double apq = A[ut4(P, Q)];
    if (apq == 0.0) return;  // nothing to rotate (and theta would be 0 / 0)
    const double theta = (A[ut4(Q, Q)] - A[ut4(P, P)]) / (2.0 * apq);
    const double sg = theta < 0.0 ? -1.0 : 1.0;
    const double t = sg / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[ut4(P, P)] -= t * apq;
    A[ut4(Q, Q)] += t * apq;
    A[ut4(P, Q)] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r == P || r == Q) continue;
        const double arp = A[ut4(r, P)], arq = A[ut4(r, Q)];
        A[ut4(r, P)] = c * arp - s * arq;
        A[ut4(r, Q)] = s * arp + c * arq;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double vp = V[4 * r + P], vq = V[4 * r + Q];
        V[4 * r + P] = c * vp - s * vq;
        V[4 * r + Q] = s * vp + c * vq;
    }
}

// p = R a for the similarity's first nine doubles
ACM_SIM_FN void rotate(const double (&S)[kDoubles], double ax, double ay, double az, double& px,
                       double& py, double& pz) {
    px = S[0] * ax + S[1] * ay + S[2] * az;
    py = S[3] * ax + S[4] * ay + S[5] * az;
    pz = S[6] * ax + S[7] * ay + S[8] * az;
}

// e . e for the residual e = b - (s R a + t)
ACM_SIM_FN double residual2(const double (&S)[kDoubles], double ax, double ay, double az, double bx,
                            double by, double bz) {
    double px, py, pz;
    rotate(S, ax, ay, az, px, py, pz);
    const double ex = bx - (S[12] * px + S[9]), ey = by - (S[12] * py + S[10]),
                 ez = bz - (S[12] * pz + S[11]);
    return ex * ex + ey * ey + ez * ez;
}

// one correspondence into the centred sums, about the centroids am and bm
ACM_SIM_FN void add_centred(double (&c)[kSums], const double (&am)[3], const double (&bm)[3],
                            double ax, double ay, double az, double bx, double by, double bz) {
    const double da[3] = {ax - am[0], ay - am[1], az - am[2]};
    const double db[3] = {bx - bm[0], by - bm[1], bz - bm[2]};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int q = 0; q < 3; ++q) c[3 * r + q] += db[r] * da[q];
    }
    c[9] += da[0] * da[0] + da[1] * da[1] + da[2] * da[2];
}

// The similarity of n >= 3 correspondences from their centroids and centred
// sums; rigid: s = 1.  false (S all NaN): void -- n < 3, an input or output
// that is not finite, Saa <= 0, s <= 0, or N's largest eigenvalue not
// positive or not separated from the second by kGap.
ACM_SIM_FN bool fit(long long n, const double (&am)[3], const double (&bm)[3],
                    const double (&c)[kSums], bool rigid, double (&S)[kDoubles]) {
    const double qnan = __builtin_nan("");
#pragma unroll
    for (int i = 0; i < kDoubles; ++i) S[i] = qnan;
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) fin = fin && __builtin_isfinite(am[i]) && __builtin_isfinite(bm[i]);
#pragma unroll
    for (int i = 0; i < kSums; ++i) fin = fin && __builtin_isfinite(c[i]);
    const double Saa = c[9];
    if (!(n >= 3 && fin && Saa > 0.0)) return false;
    // Horn's N with S_xy = sum a_x b_y = M[y][x]
    const double Sxx = c[0], Sxy = c[3], Sxz = c[6], Syx = c[1], Syy = c[4], Syz = c[7], Szx = c[2],
                 Szy = c[5], Szz = c[8];
    double A[10] = {(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz,         Sxy - Syx,
                    (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz,
                    (Syy - Sxx) - Szz, Syz + Szy,
                    (Szz - Sxx) - Syy};
    double V[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        jacobi_rotate<0, 1>(A, V);
        jacobi_rotate<0, 2>(A, V);
        jacobi_rotate<0, 3>(A, V);
        jacobi_rotate<1, 2>(A, V);
        jacobi_rotate<1, 3>(A, V);
        jacobi_rotate<2, 3>(A, V);
    }
    // the two largest eigenvalues and the first's eigenvector (V's column)
    double l1 = A[ut4(0, 0)], l2 = -__builtin_inf();
    double q0 = V[0], q1 = V[4], q2 = V[8], q3 = V[12];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const double d = A[ut4(k, k)];
        const bool top = d > l1;
        l2 = top ? l1 : (d > l2 ? d : l2);
        l1 = top ? d : l1;
        q0 = top ? V[k] : q0;
        q1 = top ? V[4 + k] : q1;
        q2 = top ? V[8 + k] : q2;
        q3 = top ? V[12 + k] : q3;
    }
    if (!(l1 > 0.0 && l1 - l2 > kGap * l1)) return false;
    // unit quaternion, signed: q0 >= 0, at q0 = 0 the first non-zero component positive
    const bool neg = q0 < 0.0 || (q0 == 0.0 && (q1 < 0.0 || (q1 == 0.0 && (q2 < 0.0 || (q2 == 0.0 && q3 < 0.0)))));
    const double nrm = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    const double inv = (neg ? -1.0 : 1.0) / nrm;
    q0 *= inv;
    q1 *= inv;
    q2 *= inv;
    q3 *= inv;
    double R[9];
    R[0] = (q0 * q0 + q1 * q1) - (q2 * q2 + q3 * q3);
    R[1] = 2.0 * (q1 * q2 - q0 * q3);
    R[2] = 2.0 * (q1 * q3 + q0 * q2);
    R[3] = 2.0 * (q1 * q2 + q0 * q3);
    R[4] = (q0 * q0 + q2 * q2) - (q1 * q1 + q3 * q3);
    R[5] = 2.0 * (q2 * q3 - q0 * q1);
    R[6] = 2.0 * (q1 * q3 - q0 * q2);
    R[7] = 2.0 * (q2 * q3 + q0 * q1);
    R[8] = (q0 * q0 + q3 * q3) - (q1 * q1 + q2 * q2);
    // s = sum (b - bm) . R (a - am) / Saa = sum_rc R[r][c] M[r][c] / Saa
    double dot = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) dot += R[i] * c[i];
    const double s = rigid ? 1.0 : dot / Saa;
    if (!(s > 0.0)) return false;
    double out[kDoubles];
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] = R[i];
    out[9] = bm[0] - s * (R[0] * am[0] + R[1] * am[1] + R[2] * am[2]);
    out[10] = bm[1] - s * (R[3] * am[0] + R[4] * am[1] + R[5] * am[2]);
    out[11] = bm[2] - s * (R[6] * am[0] + R[7] * am[1] + R[8] * am[2]);
    out[12] = s;
    fin = true;
#pragma unroll
    for (int i = 0; i < kDoubles; ++i) fin = fin && __builtin_isfinite(out[i]);
    if (!fin) return false;
#pragma unroll
    for (int i = 0; i < kDoubles; ++i) S[i] = out[i];
    return true;
}

// The similarity of three correspondences (a_i, b_i): the centroids, the
// centred sums in index order, then fit -- the same path as the refit, and no
// dependence on a triad built from the points' order.
ACM_SIM_FN bool solve3(const double (&a0)[3], const double (&a1)[3], const double (&a2)[3],
                       const double (&b0)[3], const double (&b1)[3], const double (&b2)[3],
                       bool rigid, double (&S)[kDoubles]) {
    double am[3], bm[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        am[k] = ((a0[k] + a1[k]) + a2[k]) / 3.0;
        bm[k] = ((b0[k] + b1[k]) + b2[k]) / 3.0;
    }
    double c[kSums];
#pragma unroll
    for (int i = 0; i < kSums; ++i) c[i] = 0.0;
    add_centred(c, am, bm, a0[0], a0[1], a0[2], b0[0], b0[1], b0[2]);
    add_centred(c, am, bm, a1[0], a1[1], a1[2], b1[0], b1[1], b1[2]);
    add_centred(c, am, bm, a2[0], a2[1], a2[2], b2[0], b2[1], b2[2]);
    return fit(3, am, bm, c, rigid, S);
}

// similarity_3pt on packed arrays: a, b hold three points of three doubles
ACM_SIM_FN bool similarity_3pt(const double* a, const double* b, bool rigid, double (&S)[kDoubles]) {
    const double a0[3] = {a[0], a[1], a[2]}, a1[3] = {a[3], a[4], a[5]}, a2[3] = {a[6], a[7], a[8]};
    const double b0[3] = {b[0], b[1], b[2]}, b1[3] = {b[3], b[4], b[5]}, b2[3] = {b[6], b[7], b[8]};
    return solve3(a0, a1, a2, b0, b1, b2, rigid, S);
}

}  // namespace similarity
}  // namespace acm

#undef ACM_SIM_FN
