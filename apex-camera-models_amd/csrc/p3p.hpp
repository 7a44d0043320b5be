// p3p.hpp -- the minimal absolute-pose solver (three bearings, three world
// points) shared by k_p3p and k_pose_estimate (acm.hip), f64, closed form
// with a polish; host-callable so that a CPU driver can run the same code.
//
// Grunert's route (include/acm.h, acm_p3p): the quartic in v = s3 / s1 is
// factored into two real quadratics through the resolvent cubic (Ferrari),
// each real root takes two Newton steps on the quartic, u = s2 / s1 follows
// from the linear relation, s1 from the law of cosines, and the depths take
// three Gauss-Newton steps on the three law-of-cosines equations.  R, t align
// the orthonormal frame of (s_i f_i) to the frame of (X_i).
//
// Every array index is a compile-time constant: a solution stays in the slot
// of its quartic root (0, 1: the first quadratic, 2, 3: the second) and a
// 4-bit mask says which slots hold one, so nothing is indexed at run time.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define ACM_P3P_FN __host__ __device__ __forceinline__
#else
#define ACM_P3P_FN inline
#endif

namespace acm {
namespace p3p {

// a solution is kept when its law-of-cosines residuals are at most this times
// a^2 + b^2 + c^2 after the polish
constexpr double kResidualTol = 1e-12;
// a triplet is degenerate when the sine of an angle of the world triangle, or
// of the angle between two bearings, is at most this
constexpr double kDegenerateSin = 1e-10;

ACM_P3P_FN bool finite3(double a, double b, double c) {
    return __builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c);
}

// the largest real root of m^3 + p2 m^2 + p1 m + p0 (Cardano / the cosine
// form, then three Newton steps)
ACM_P3P_FN double cubic_largest(double p2, double p1, double p0) {
    const double sh = p2 / 3.0;
    const double P = p1 - p2 * sh;
    const double Q = 2.0 * sh * sh * sh - sh * p1 + p0;
    const double disc = 0.25 * Q * Q + P * P * P / 27.0;
    double t;
    if (disc >= 0.0) {
        const double sd = sqrt(disc);
        const double A = -0.5 * Q + (Q > 0.0 ? -sd : sd);  // the larger magnitude
        const double u = cbrt(A);
        t = u != 0.0 ? u - P / (3.0 * u) : 0.0;
    } else {
        const double rho = sqrt(-P / 3.0);
        double ca = 3.0 * Q / (2.0 * P * rho);
        ca = ca < -1.0 ? -1.0 : (ca > 1.0 ? 1.0 : ca);
        t = 2.0 * rho * cos(acos(ca) / 3.0);
    }
    double m = t - sh;
#pragma unroll
    for (int it = 0; it < 3; ++it) {
        const double g = ((m + p2) * m + p1) * m + p0;
        const double dg = (3.0 * m + 2.0 * p2) * m + p1;
        const double step = g / dg;
        if (__builtin_isfinite(step)) m -= step;
    }
    return m;
}

// the real roots of y^2 + B y + C into r0, r1; a slightly negative
// discriminant (a double root under rounding) counts as zero
ACM_P3P_FN bool quadratic(double B, double C, double& r0, double& r1) {
    const double disc = B * B - 4.0 * C;
    if (!(disc >= -1e-10 * (B * B + fabs(4.0 * C)))) return false;
    const double sq = sqrt(disc > 0.0 ? disc : 0.0);
    const double qq = -0.5 * (B + (B < 0.0 ? -sq : sq));
    r0 = qq;
    r1 = qq != 0.0 ? C / qq : 0.0;
    return true;
}

// the real roots of a4 x^4 + ... + a0, a4 != 0: mask of the slots of r that
// hold one
ACM_P3P_FN unsigned quartic(double a4, double a3, double a2, double a1, double a0,
                            double (&r)[4]) {
    const double b = a3 / a4, c = a2 / a4, d = a1 / a4, e = a0 / a4;
    const double bb = b * b;
    // x = y - b / 4: y^4 + p y^2 + q y + rr
    const double p = c - 0.375 * bb;
    const double q = d - 0.5 * b * c + 0.125 * bb * b;
    const double rr = e - 0.25 * b * d + 0.0625 * bb * c - (3.0 / 256.0) * bb * bb;
    // (y^2 + p / 2 + m)^2 = 2 m y^2 - q y + m^2 + p m + p^2 / 4 - rr is a
    // square in y for a root m of the resolvent cubic
    double m = cubic_largest(p, 0.25 * p * p - rr, -0.125 * q * q);
    unsigned mask = 0;
    const double big = fmax(fabs(p), fmax(sqrt(fabs(rr)), 1.0));
    if (m > 1e-13 * big) {
        const double s = sqrt(2.0 * m);
        const double h = 0.5 * p + m, k = q / (2.0 * s);
        if (quadratic(-s, h + k, r[0], r[1])) mask |= 3u;
        if (quadratic(s, h - k, r[2], r[3])) mask |= 12u;
    } else {
        // q = 0: y^2 = z, z^2 + p z + rr = 0
        double z0, z1;
        if (quadratic(p, rr, z0, z1)) {
            if (z0 >= 0.0) {
                r[0] = sqrt(z0);
                r[1] = -r[0];
                mask |= 3u;
            }
            if (z1 >= 0.0) {
                r[2] = sqrt(z1);
                r[3] = -r[2];
                mask |= 12u;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (mask >> i & 1u) ? r[i] - 0.25 * b : 0.0;
    return mask;
}

// Unit bearings f (f1, f2, f3) and world points X (X1, X2, X3), 9 doubles
// each.  S[k] receives the depths (s1, s2, s3) of the solution in slot k; the
// mask of the filled slots is returned (0: degenerate, non-finite, or no real
// solution with positive depths).
ACM_P3P_FN unsigned depths(const double (&f)[9], const double (&X)[9], double (&S)[4][3]) {
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) fin = fin && __builtin_isfinite(f[i]) && __builtin_isfinite(X[i]);
    if (!fin) return 0;
    const double d12[3] = {X[3] - X[0], X[4] - X[1], X[5] - X[2]};
    const double d13[3] = {X[6] - X[0], X[7] - X[1], X[8] - X[2]};
    const double d23[3] = {X[6] - X[3], X[7] - X[4], X[8] - X[5]};
    const double c2 = d12[0] * d12[0] + d12[1] * d12[1] + d12[2] * d12[2];
    const double b2 = d13[0] * d13[0] + d13[1] * d13[1] + d13[2] * d13[2];
    const double a2 = d23[0] * d23[0] + d23[1] * d23[1] + d23[2] * d23[2];
    if (!(a2 > 0.0 && b2 > 0.0 && c2 > 0.0)) return 0;
    constexpr double sin2 = kDegenerateSin * kDegenerateSin;
    {
        const double n0 = d12[1] * d13[2] - d12[2] * d13[1];
        const double n1 = d12[2] * d13[0] - d12[0] * d13[2];
        const double n2 = d12[0] * d13[1] - d12[1] * d13[0];
        if (!(n0 * n0 + n1 * n1 + n2 * n2 > sin2 * b2 * c2)) return 0;
    }
#pragma unroll
    for (int pr = 0; pr < 3; ++pr) {
        const int i = pr == 2 ? 3 : 0, j = pr == 0 ? 3 : 6;
        const double w0 = f[i + 1] * f[j + 2] - f[i + 2] * f[j + 1];
        const double w1 = f[i + 2] * f[j] - f[i] * f[j + 2];
        const double w2 = f[i] * f[j + 1] - f[i + 1] * f[j];
        if (!(w0 * w0 + w1 * w1 + w2 * w2 > sin2)) return 0;
    }
    const double ca = f[3] * f[6] + f[4] * f[7] + f[5] * f[8];
    const double cb = f[0] * f[6] + f[1] * f[7] + f[2] * f[8];
    const double cg = f[0] * f[3] + f[1] * f[4] + f[2] * f[5];
    const double q = (a2 - c2) / b2, p = (a2 + c2) / b2;
    const double cb2 = c2 / b2, ab2 = a2 / b2;
    const double A4 = (q - 1.0) * (q - 1.0) - 4.0 * cb2 * ca * ca;
    const double A3 = 4.0 * (q * (1.0 - q) * cb - (1.0 - p) * ca * cg + 2.0 * cb2 * ca * ca * cb);
    const double A2 = 2.0 * (q * q - 1.0 + 2.0 * q * q * cb * cb + 2.0 * ((b2 - c2) / b2) * ca * ca -
                             4.0 * p * ca * cb * cg + 2.0 * ((b2 - a2) / b2) * cg * cg);
    const double A1 = 4.0 * (-q * (1.0 + q) * cb + 2.0 * ab2 * cg * cg * cb - (1.0 - p) * ca * cg);
    const double A0 = (1.0 + q) * (1.0 + q) - 4.0 * ab2 * cg * cg;
    if (!(__builtin_isfinite(A4) && __builtin_isfinite(A3) && __builtin_isfinite(A2) &&
          __builtin_isfinite(A1) && __builtin_isfinite(A0)))
        return 0;
    // the larger of the end coefficients leads: v, or w = 1 / v
    const bool rev = fabs(A4) < fabs(A0);
    if (!(fabs(rev ? A0 : A4) > 0.0)) return 0;
    double root[4];
    const unsigned roots = rev ? quartic(A0, A1, A2, A3, A4, root) : quartic(A4, A3, A2, A1, A0, root);
    unsigned mask = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        S[k][0] = S[k][1] = S[k][2] = 0.0;
        if (!(roots >> k & 1u)) continue;
        double v = rev ? 1.0 / root[k] : root[k];
        if (!__builtin_isfinite(v)) continue;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const double g = (((A4 * v + A3) * v + A2) * v + A1) * v + A0;
            const double dg = ((4.0 * A4 * v + 3.0 * A3) * v + 2.0 * A2) * v + A1;
            const double step = g / dg;
            if (__builtin_isfinite(step)) v -= step;
        }
        if (!(v > 0.0)) continue;
        const double u = ((q - 1.0) * v * v - 2.0 * q * cb * v + 1.0 + q) / (2.0 * (cg - v * ca));
        if (!(u > 0.0)) continue;
        const double w = 1.0 + v * v - 2.0 * v * cb;
        if (!(w > 0.0)) continue;
        double s1 = sqrt(b2 / w), s2 = u * s1, s3 = v * s1;
        bool ok = true;
#pragma unroll
        for (int it = 0; it < 3; ++it) {
            const double g1 = s2 * s2 + s3 * s3 - 2.0 * s2 * s3 * ca - a2;
            const double g2 = s1 * s1 + s3 * s3 - 2.0 * s1 * s3 * cb - b2;
            const double g3 = s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * cg - c2;
            // J = [0 j01 j02; j10 0 j12; j20 j21 0]
            const double j01 = 2.0 * s2 - 2.0 * s3 * ca, j02 = 2.0 * s3 - 2.0 * s2 * ca;
            const double j10 = 2.0 * s1 - 2.0 * s3 * cb, j12 = 2.0 * s3 - 2.0 * s1 * cb;
            const double j20 = 2.0 * s1 - 2.0 * s2 * cg, j21 = 2.0 * s2 - 2.0 * s1 * cg;
            const double det = j01 * j12 * j20 + j02 * j10 * j21;
            // Cramer: columns replaced by g
            const double e1 = g2 * j21 * j02 + g3 * j01 * j12 - g1 * j12 * j21;
            const double e2 = g1 * j12 * j20 + g3 * j02 * j10 - g2 * j02 * j20;
            const double e3 = g1 * j10 * j21 + g2 * j01 * j20 - g3 * j01 * j10;
            if (!(__builtin_isfinite(det) && det != 0.0)) {
                ok = false;
                break;
            }
            s1 -= e1 / det;
            s2 -= e2 / det;
            s3 -= e3 / det;
        }
        if (!(ok && finite3(s1, s2, s3) && s1 > 0.0 && s2 > 0.0 && s3 > 0.0)) continue;
        const double g1 = s2 * s2 + s3 * s3 - 2.0 * s2 * s3 * ca - a2;
        const double g2 = s1 * s1 + s3 * s3 - 2.0 * s1 * s3 * cb - b2;
        const double g3 = s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * cg - c2;
        if (!(fmax(fabs(g1), fmax(fabs(g2), fabs(g3))) <= kResidualTol * (a2 + b2 + c2))) continue;
        S[k][0] = s1;
        S[k][1] = s2;
        S[k][2] = s3;
        mask |= 1u << k;
    }
    return mask;
}

// the orthonormal frame (columns e1, e2, e3, row-major 3 x 3) of three points:
// e1 along p2 - p1, e3 the triangle's normal, e2 = e3 x e1
ACM_P3P_FN void frame(const double (&P)[9], double (&F)[9]) {
    double a[3] = {P[3] - P[0], P[4] - P[1], P[5] - P[2]};
    const double b[3] = {P[6] - P[0], P[7] - P[1], P[8] - P[2]};
    const double na = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) a[i] /= na;
    double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) n[i] /= nn;
    const double m[3] = {n[1] * a[2] - n[2] * a[1], n[2] * a[0] - n[0] * a[2], n[0] * a[1] - n[1] * a[0]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        F[3 * i] = a[i];
        F[3 * i + 1] = m[i];
        F[3 * i + 2] = n[i];
    }
}

// pose (R row-major, then t; acm_pose's layout) of the solution with depths s:
// false when it is not finite
ACM_P3P_FN bool pose(const double (&f)[9], const double (&X)[9], const double (&s)[3],
                     double (&out)[12]) {
    double P[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) P[3 * i + k] = s[i] * f[3 * i + k];
    }
    double Fp[9], Fx[9];
    frame(P, Fp);
    frame(X, Fx);
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            out[3 * i + j] = Fp[3 * i] * Fx[3 * j] + Fp[3 * i + 1] * Fx[3 * j + 1] +
                             Fp[3 * i + 2] * Fx[3 * j + 2];
            fin = fin && __builtin_isfinite(out[3 * i + j]);
        }
    }
    const double mx[3] = {(X[0] + X[3] + X[6]) / 3.0, (X[1] + X[4] + X[7]) / 3.0,
                          (X[2] + X[5] + X[8]) / 3.0};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double mp = (P[i] + P[3 + i] + P[6 + i]) / 3.0;
        out[9 + i] = mp - (out[3 * i] * mx[0] + out[3 * i + 1] * mx[1] + out[3 * i + 2] * mx[2]);
        fin = fin && __builtin_isfinite(out[9 + i]);
    }
    return fin;
}

// f <- f / |f| for the three bearings; false when one has no direction
ACM_P3P_FN bool normalize(double (&f)[9]) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double n = sqrt(f[3 * i] * f[3 * i] + f[3 * i + 1] * f[3 * i + 1] +
                              f[3 * i + 2] * f[3 * i + 2]);
        ok = ok && n > 0.0 && __builtin_isfinite(n);
#pragma unroll
        for (int k = 0; k < 3; ++k) f[3 * i + k] /= n;
    }
    return ok;
}

// acm_p3p for one triplet: the solutions' poses in order, NaN beyond the count
ACM_P3P_FN int solve(const double* bearings, const double* points, double* poses48) {
    double f[9], X[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        f[i] = bearings[i];
        X[i] = points[i];
    }
    int n = 0;
    if (normalize(f)) {
        double S[4][3];
        const unsigned mask = depths(f, X, S);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!(mask >> k & 1u)) continue;
            double out[12];
            if (!pose(f, X, S[k], out)) continue;
#pragma unroll
            for (int i = 0; i < 12; ++i) poses48[12 * n + i] = out[i];
            ++n;
        }
    }
    for (int i = 12 * n; i < 48; ++i) poses48[i] = __builtin_nan("");
    return n;
}

}  // namespace p3p
}  // namespace acm
