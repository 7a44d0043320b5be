// essential.hpp -- the two-view relative-pose solver shared by
// k_relative_pose_8pt and k_relative_pose (acm.hip), f64; host-callable so
// that a CPU driver can run the same code.
//
// The route (include/acm.h, acm_relative_pose_8pt): every match gives the row
// a = f_b (x) f_a of the linear system a . vec(E) = 0 (E row-major); the rows
// are streamed through Givens rotations into a 9 x 9 upper-triangular factor
// (45 doubles, no normal equations), whose smallest right singular vector
// comes from three rounds of inverse iteration on R9^T R9.  E is decomposed in
// closed form (Horn 1990, no SVD) into two rotations and the baseline's
// direction, and the candidate with the most matches in front of both cameras
// wins.
//
// Every array index is a compile-time constant (the loops over the factor are
// fully unrolled), so on the device the factor stays in registers.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define ACM_ESS_FN __host__ __device__ __forceinline__
#else
#define ACM_ESS_FN inline
#endif

namespace acm {
namespace essential {

// the factor: the upper triangle of R9, row by row
constexpr int kTri = 45;
constexpr int tri(int i, int j) { return i * 9 - i * (i - 1) / 2 + (j - i); }
// A diagonal entry below this times max |R9| is replaced by it, so that the
// triangular solves never divide by zero.  Flooring the last entry perturbs
// R9^T R9 only in second order (the last row is then the only one changed and
// it was zero), but a motion with zeros in E (forward, sideways) puts the
// vanishing entry inside the diagonal, where the floor is a first-order
// perturbation of the null vector: 2^-44 cost 4e-12 there (median over 200
// 8-tuples, against 5e-15 for a general motion), 2^-60 costs nothing
// measurable, and nine such entries in a row still cannot overflow.
constexpr double kDiagFloor = 0x1p-60;
constexpr int kInverseIterations = 3;

ACM_ESS_FN void clear(double (&T)[kTri]) {
#pragma unroll
    for (int i = 0; i < kTri; ++i) T[i] = 0.0;
}

// a = f_b (x) f_a: a . vec(E) = f_b^T E f_a
ACM_ESS_FN void row(const double (&fa)[3], const double (&fb)[3], double (&a)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) a[3 * i + j] = fb[i] * fa[j];
    }
}

// One more row a (entries before K0 are zero) into the factor: Givens
// rotations against rows K0 .. 8, no pivoting.  a is destroyed.
template <int K0 = 0>
ACM_ESS_FN void feed(double (&T)[kTri], double (&a)[9]) {
#pragma unroll
    for (int k = K0; k < 9; ++k) {
        const double x = T[tri(k, k)], y = a[k];
        if (y == 0.0) continue;
        const double r = sqrt(x * x + y * y);
        if (r == 0.0) continue;  // y * y underflowed
        const double c = x / r, s = y / r;
        T[tri(k, k)] = r;
#pragma unroll
        for (int j = k + 1; j < 9; ++j) {
            const double p = T[tri(k, j)], q = a[j];
            T[tri(k, j)] = c * p + s * q;
            a[j] = c * q - s * p;
        }
    }
}

// T <- the factor of both row sets: U's rows are fed into T, first to last
ACM_ESS_FN void merge(double (&T)[kTri], const double (&U)[kTri]) {
#define ACM_ESS_MERGE_ROW(I)                                    \
    {                                                           \
        double a[9];                                            \
        _Pragma("unroll") for (int j = 0; j < 9; ++j)           \
            a[j] = j >= I ? U[tri(I, j >= I ? j : I)] : 0.0;    \
        feed<I>(T, a);                                          \
    }
    ACM_ESS_MERGE_ROW(0)
    ACM_ESS_MERGE_ROW(1)
    ACM_ESS_MERGE_ROW(2)
    ACM_ESS_MERGE_ROW(3)
    ACM_ESS_MERGE_ROW(4)
    ACM_ESS_MERGE_ROW(5)
    ACM_ESS_MERGE_ROW(6)
    ACM_ESS_MERGE_ROW(7)
    ACM_ESS_MERGE_ROW(8)
#undef ACM_ESS_MERGE_ROW
}

ACM_ESS_FN bool normalize9(double (&x)[9]) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) s += x[i] * x[i];
    const double n = sqrt(s);
#pragma unroll
    for (int i = 0; i < 9; ++i) x[i] /= n;
    return n > 0.0 && __builtin_isfinite(n);
}

// The unit right singular vector of the factor's smallest singular value, by
// inverse iteration on R9^T R9 from x0 ~ (1, 2, ..., 9).  The small diagonal
// entries of T are floored (with 8 rows the last one is exactly 0).  false:
// an empty or non-finite factor.
ACM_ESS_FN bool null_vector(double (&T)[kTri], double (&x)[9]) {
    double big = 0.0;
#pragma unroll
    for (int i = 0; i < kTri; ++i) big = fmax(big, fabs(T[i]));
    if (!(big > 0.0 && __builtin_isfinite(big))) return false;
    const double floor_ = kDiagFloor * big;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double d = T[tri(k, k)];
        if (fabs(d) < floor_) T[tri(k, k)] = copysign(floor_, d);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) x[i] = (double)(i + 1);
    bool ok = normalize9(x);
#pragma unroll 1
    for (int it = 0; it < kInverseIterations; ++it) {
        double z[9];
        // R9^T z = x
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            double s = x[i];
#pragma unroll
            for (int k = 0; k < i; ++k) s -= T[tri(k, i)] * z[k];
            z[i] = s / T[tri(i, i)];
        }
        ok = normalize9(z) && ok;
        // R9 x = z
#pragma unroll
        for (int i = 8; i >= 0; --i) {
            double s = z[i];
#pragma unroll
            for (int j = i + 1; j < 9; ++j) s -= T[tri(i, j)] * x[j];
            x[i] = s / T[tri(i, i)];
        }
        ok = normalize9(x) && ok;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) ok = ok && __builtin_isfinite(x[i]);
    return ok;
}

// rows 0 and 1 by Gram-Schmidt, row 2 their cross product: a rotation
ACM_ESS_FN void orthonormalize(double (&R)[9]) {
    const double n0 = sqrt(R[0] * R[0] + R[1] * R[1] + R[2] * R[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) R[i] /= n0;
    const double d = R[0] * R[3] + R[1] * R[4] + R[2] * R[5];
#pragma unroll
    for (int i = 0; i < 3; ++i) R[3 + i] -= d * R[i];
    const double n1 = sqrt(R[3] * R[3] + R[4] * R[4] + R[5] * R[5]);
#pragma unroll
    for (int i = 0; i < 3; ++i) R[3 + i] /= n1;
    R[6] = R[1] * R[5] - R[2] * R[4];
    R[7] = R[2] * R[3] - R[0] * R[5];
    R[8] = R[0] * R[4] - R[1] * R[3];
}

// E (row-major, any scale) = [t]x R up to sign: the two rotations Rp, Rm and
// the unit baseline b with E ~ [b]x Rp ~ [-b]x Rm.  B = tr(E E^T) / 2 I - E E^T
// = b b^T gives b from its column of the largest diagonal entry; with C the
// cofactor matrix of E, R+- = (C -+ [b]x E) / (b . b).  false: not finite.
ACM_ESS_FN bool decompose(const double (&E)[9], double (&Rp)[9], double (&Rm)[9], double (&b)[3]) {
    const double m00 = E[0] * E[0] + E[1] * E[1] + E[2] * E[2];
    const double m11 = E[3] * E[3] + E[4] * E[4] + E[5] * E[5];
    const double m22 = E[6] * E[6] + E[7] * E[7] + E[8] * E[8];
    const double m01 = E[0] * E[3] + E[1] * E[4] + E[2] * E[5];
    const double m02 = E[0] * E[6] + E[1] * E[7] + E[2] * E[8];
    const double m12 = E[3] * E[6] + E[4] * E[7] + E[5] * E[8];
    const double h = 0.5 * (m00 + m11 + m22);
    const double B00 = h - m00, B11 = h - m11, B22 = h - m22;
    double v0, v1, v2, dd;
    if (B00 >= B11 && B00 >= B22) {
        v0 = B00, v1 = -m01, v2 = -m02, dd = B00;
    } else if (B11 >= B22) {
        v0 = -m01, v1 = B11, v2 = -m12, dd = B11;
    } else {
        v0 = -m02, v1 = -m12, v2 = B22, dd = B22;
    }
    const double sd = sqrt(dd);
    const double t0 = v0 / sd, t1 = v1 / sd, t2 = v2 / sd;
    const double bb = t0 * t0 + t1 * t1 + t2 * t2;
    // C: rows e1 x e2, e2 x e0, e0 x e1 of E's rows e0, e1, e2
    const double C[9] = {E[4] * E[8] - E[5] * E[7], E[5] * E[6] - E[3] * E[8], E[3] * E[7] - E[4] * E[6],
                         E[7] * E[2] - E[8] * E[1], E[8] * E[0] - E[6] * E[2], E[6] * E[1] - E[7] * E[0],
                         E[1] * E[5] - E[2] * E[4], E[2] * E[3] - E[0] * E[5], E[0] * E[4] - E[1] * E[3]};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double x0 = t1 * E[6 + j] - t2 * E[3 + j];  // ([b]x E) row 0
        const double x1 = t2 * E[j] - t0 * E[6 + j];
        const double x2 = t0 * E[3 + j] - t1 * E[j];
        Rp[j] = (C[j] - x0) / bb;
        Rp[3 + j] = (C[3 + j] - x1) / bb;
        Rp[6 + j] = (C[6 + j] - x2) / bb;
        Rm[j] = (C[j] + x0) / bb;
        Rm[3 + j] = (C[3 + j] + x1) / bb;
        Rm[6 + j] = (C[6 + j] + x2) / bb;
    }
    orthonormalize(Rp);
    orthonormalize(Rm);
    const double nb = sqrt(bb);
    b[0] = t0 / nb;
    b[1] = t1 / nb;
    b[2] = t2 / nb;
    bool ok = __builtin_isfinite(b[0]) && __builtin_isfinite(b[1]) && __builtin_isfinite(b[2]);
#pragma unroll
    for (int i = 0; i < 9; ++i) ok = ok && __builtin_isfinite(Rp[i]) && __builtin_isfinite(Rm[i]);
    return ok;
}

// The match (fa, fb), unit bearings, is in front of both cameras of the pose
// (R, t) iff both depths of  lb fb = la R fa + t  are positive: with g = R fa
// and c = g . fb,  c (fb . t) - g . t > 0  and  fb . t - c (g . t) > 0 (the
// common divisor 1 - c^2 is positive).  The four candidates in order: (Rp, b),
// (Rp, -b), (Rm, -b), (Rm, b); cnt[k] grows by one where candidate k passes.
ACM_ESS_FN void front4(const double (&Rp)[9], const double (&Rm)[9], const double (&b)[3],
                       const double (&fa)[3], const double (&fb)[3], int (&cnt)[4]) {
    const double fbt = fb[0] * b[0] + fb[1] * b[1] + fb[2] * b[2];
    {
        const double g0 = Rp[0] * fa[0] + Rp[1] * fa[1] + Rp[2] * fa[2];
        const double g1 = Rp[3] * fa[0] + Rp[4] * fa[1] + Rp[5] * fa[2];
        const double g2 = Rp[6] * fa[0] + Rp[7] * fa[1] + Rp[8] * fa[2];
        const double c = g0 * fb[0] + g1 * fb[1] + g2 * fb[2];
        const double gt = g0 * b[0] + g1 * b[1] + g2 * b[2];
        const double la = c * fbt - gt, lb = fbt - c * gt;
        cnt[0] += (la > 0.0 && lb > 0.0) ? 1 : 0;
        cnt[1] += (la < 0.0 && lb < 0.0) ? 1 : 0;
    }
    {
        const double g0 = Rm[0] * fa[0] + Rm[1] * fa[1] + Rm[2] * fa[2];
        const double g1 = Rm[3] * fa[0] + Rm[4] * fa[1] + Rm[5] * fa[2];
        const double g2 = Rm[6] * fa[0] + Rm[7] * fa[1] + Rm[8] * fa[2];
        const double c = g0 * fb[0] + g1 * fb[1] + g2 * fb[2];
        const double gt = g0 * b[0] + g1 * b[1] + g2 * b[2];
        const double la = c * fbt - gt, lb = fbt - c * gt;
        cnt[2] += (la < 0.0 && lb < 0.0) ? 1 : 0;
        cnt[3] += (la > 0.0 && lb > 0.0) ? 1 : 0;
    }
}

// the candidate with the largest count, the first of equals
ACM_ESS_FN int best_of4(const int (&cnt)[4]) {
    int k = 0, c = cnt[0];
    if (cnt[1] > c) k = 1, c = cnt[1];
    if (cnt[2] > c) k = 2, c = cnt[2];
    if (cnt[3] > c) k = 3, c = cnt[3];
    return k;
}

// candidate k as a pose (R row-major, then t; acm_pose's layout)
ACM_ESS_FN void candidate(int k, const double (&Rp)[9], const double (&Rm)[9], const double (&b)[3],
                          double (&P)[12]) {
    const bool plus = k < 2;
    const double s = (k == 0 || k == 3) ? 1.0 : -1.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) P[i] = plus ? Rp[i] : Rm[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) P[9 + i] = s * b[i];
}

// The inlier rule of acm_relative_pose_batch at pose P for the unit bearings
// (fa, fb): with g = R fa, n = t x g and d = fb . n, the squared sine of the
// angle between fb and the epipolar plane, e = d^2 / (n . n), is at most sin2,
// and the match is in front of both cameras.  n = 0 (no parallax) is no inlier.
ACM_ESS_FN bool inlier(const double (&P)[12], double ax, double ay, double az, double bx, double by,
                       double bz, double sin2, double& e) {
    const double g0 = P[0] * ax + P[1] * ay + P[2] * az;
    const double g1 = P[3] * ax + P[4] * ay + P[5] * az;
    const double g2 = P[6] * ax + P[7] * ay + P[8] * az;
    const double n0 = P[10] * g2 - P[11] * g1;
    const double n1 = P[11] * g0 - P[9] * g2;
    const double n2 = P[9] * g1 - P[10] * g0;
    const double d = bx * n0 + by * n1 + bz * n2;
    const double nn = n0 * n0 + n1 * n1 + n2 * n2;
    if (!(nn > 0.0 && d * d <= sin2 * nn)) return false;
    const double c = g0 * bx + g1 * by + g2 * bz;
    const double fbt = bx * P[9] + by * P[10] + bz * P[11];
    const double gt = g0 * P[9] + g1 * P[10] + g2 * P[11];
    if (!(c * fbt - gt > 0.0 && fbt - c * gt > 0.0)) return false;
    e = d * d / nn;
    return true;
}

// From a finished factor: the essential matrix (unit Frobenius norm) and the
// decomposition.  false: no finite result.
ACM_ESS_FN bool factor_to_candidates(double (&T)[kTri], double (&E)[9], double (&Rp)[9],
                                     double (&Rm)[9], double (&b)[3]) {
    return null_vector(T, E) && decompose(E, Rp, Rm, b);
}

// The solver over n >= 8 matches.  fetch(i, fa, fb) -> bool delivers match i's
// unit bearings (false: the match has none; the solve then fails).  P: the
// pose, E: the unit-norm essential matrix signed as [t]x R; the return value
// is the number of matches in front of both cameras.  On failure everything
// is NaN and 0 is returned.
template <class Fetch>
ACM_ESS_FN int solve_rows(long long n, Fetch fetch, double (&P)[12], double (&E)[9]) {
    double T[kTri];
    clear(T);
    bool ok = n >= 8;
#pragma unroll 1
    for (long long i = 0; i < n; ++i) {
        double fa[3], fb[3], a[9];
        ok = fetch(i, fa, fb) && ok;
        row(fa, fb, a);
        feed(T, a);
    }
    double Rp[9], Rm[9], b[3];
    ok = ok && factor_to_candidates(T, E, Rp, Rm, b);
    int front = 0;
    if (ok) {
        int cnt[4] = {0, 0, 0, 0};
#pragma unroll 1
        for (long long i = 0; i < n; ++i) {
            double fa[3], fb[3];
            fetch(i, fa, fb);
            front4(Rp, Rm, b, fa, fb, cnt);
        }
        const int k = best_of4(cnt);
        front = k == 0 ? cnt[0] : (k == 1 ? cnt[1] : (k == 2 ? cnt[2] : cnt[3]));
        candidate(k, Rp, Rm, b, P);
        if (k == 1 || k == 3) {
#pragma unroll
            for (int i = 0; i < 9; ++i) E[i] = -E[i];
        }
    } else {
        const double qnan = __builtin_nan("");
#pragma unroll
        for (int i = 0; i < 12; ++i) P[i] = qnan;
#pragma unroll
        for (int i = 0; i < 9; ++i) E[i] = qnan;
    }
    return front;
}

// acm_relative_pose_8pt for one problem of n matches: bearings 3 n doubles
// each, any length (normalised here)
ACM_ESS_FN int solve(long long n, const double* bearings_a, const double* bearings_b, double* pose12,
                     double* essential9) {
    double P[12], E[9];
    const int front = solve_rows(
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
        P, E);
#pragma unroll
    for (int i = 0; i < 12; ++i) pose12[i] = P[i];
    if (essential9) {
#pragma unroll
        for (int i = 0; i < 9; ++i) essential9[i] = E[i];
    }
    return front;
}

}  // namespace essential
}  // namespace acm
