// srk_locate_math.hpp -- the arithmetic of resection without a start pose (srk_locate_frames, srk_ba_locate)
// as plain functions of doubles, compiled for the device by srk_locate.hip and for the host by srk_locate.cpp: the kernels and the
// host walk of one frame (srk_locate_host_frame, tests/cpp/test_locate_host.cpp) run the same statements in the same order.  The
// sampler, the bearing, P3P, the choice by the fourth point and one observation's term of the score.  No HIP header is needed
// here.  Every loop has constant bounds and is unrolled for the device, so that no per-lane array is indexed at run time.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__)
#define SRK_LC_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SRK_LC_HD inline
#endif
#if defined(__clang__)
#define SRK_LC_UNROLL _Pragma("unroll")
#else
#define SRK_LC_UNROLL
#endif

#define SRK_LOCATE_LANES 64  // hypotheses that share a wave
#define SRK_LOCATE_STRIP 8   // doubles of a gathered observation: X (3), uv (2), q, two of padding (64 bytes)
#define SRK_LOCATE_SLOT 20   // doubles of a wave's best: score, h, inliers, poses in the wave, e4, padding, R (6-14), T (15-17)
#define SRK_LOCATE_NEWTON 3  // Newton steps that polish a root of the quartic

// the hypothesis of a sample: the pack K [R | T] row by row and row 2 of [R | T] as the score reads them, the pose itself, the
// squared pixel error at the fourth point
struct SrkLocateHyp {
    double p[12], d[4], R[9], T[3], e4;
    int valid;
};

// ---- the sampler: counter-based, no state.  mix = the splitmix64 finaliser of seed + golden * (4 h + k + 1)
SRK_LC_HD uint64_t srk_locate_mix(uint64_t seed, uint32_t h, int k)
{
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (4ull * (uint64_t)h + (uint64_t)k + 1ull);
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// the high 64 bits of a * b, from 32-bit halves: the same integer statements on both sides
SRK_LC_HD uint64_t srk_locate_mulhi(uint64_t a, uint64_t b)
{
    const uint64_t al = a & 0xffffffffull, ah = a >> 32, bl = b & 0xffffffffull, bh = b >> 32;
    const uint64_t ll = al * bl, lh = al * bh, hl = ah * bl, hh = ah * bh;
    const uint64_t mid = (ll >> 32) + (lh & 0xffffffffull) + (hl & 0xffffffffull);
    return hh + (lh >> 32) + (hl >> 32) + (mid >> 32);
}

// four distinct ranks below n (n >= 4): draw k is uniform among the n - k ranks not yet picked
SRK_LC_HD void srk_locate_sample(uint64_t seed, uint32_t h, int64_t n, int64_t& r0, int64_t& r1, int64_t& r2, int64_t& r3)
{
    r0 = (int64_t)srk_locate_mulhi(srk_locate_mix(seed, h, 0), (uint64_t)n);
    r1 = (int64_t)srk_locate_mulhi(srk_locate_mix(seed, h, 1), (uint64_t)(n - 1));
    if (r1 >= r0) ++r1;
    int64_t a = r0 < r1 ? r0 : r1, b = r0 < r1 ? r1 : r0; // the earlier picks in ascending order
    r2 = (int64_t)srk_locate_mulhi(srk_locate_mix(seed, h, 2), (uint64_t)(n - 2));
    if (r2 >= a) ++r2;
    if (r2 >= b) ++r2;
    int64_t c = r2;
    if (c < a) {
        const int64_t t = a;
        a = c;
        c = t;
    }
    if (c < b) {
        const int64_t t = b;
        b = c;
        c = t;
    }
    r3 = (int64_t)srk_locate_mulhi(srk_locate_mix(seed, h, 3), (uint64_t)(n - 3));
    if (r3 >= a) ++r3;
    if (r3 >= b) ++r3;
    if (r3 >= c) ++r3;
}

// ---- the bearing: b ~ K^-1 (u, v, f0), normalised; Ki = the inverse of K by its adjugate
SRK_LC_HD double srk_locate_det3(const double* K)
{
    return K[0] * (K[4] * K[8] - K[5] * K[7]) - K[1] * (K[3] * K[8] - K[5] * K[6]) + K[2] * (K[3] * K[7] - K[4] * K[6]);
}

SRK_LC_HD void srk_locate_inverse3(const double* K, double* Ki)
{
    const double id = 1.0 / srk_locate_det3(K);
    Ki[0] = (K[4] * K[8] - K[5] * K[7]) * id;
    Ki[1] = (K[2] * K[7] - K[1] * K[8]) * id;
    Ki[2] = (K[1] * K[5] - K[2] * K[4]) * id;
    Ki[3] = (K[5] * K[6] - K[3] * K[8]) * id;
    Ki[4] = (K[0] * K[8] - K[2] * K[6]) * id;
    Ki[5] = (K[2] * K[3] - K[0] * K[5]) * id;
    Ki[6] = (K[3] * K[7] - K[4] * K[6]) * id;
    Ki[7] = (K[1] * K[6] - K[0] * K[7]) * id;
    Ki[8] = (K[0] * K[4] - K[1] * K[3]) * id;
}

SRK_LC_HD void srk_locate_bearing(const double* Ki, double u, double v, double f0, double* b)
{
    const double x = Ki[0] * u + Ki[1] * v + Ki[2] * f0, y = Ki[3] * u + Ki[4] * v + Ki[5] * f0, z = Ki[6] * u + Ki[7] * v + Ki[8] * f0;
    const double in = 1.0 / sqrt(x * x + y * y + z * z);
    b[0] = x * in;
    b[1] = y * in;
    b[2] = z * in;
}

// ---- small vector helpers
SRK_LC_HD double srk_locate_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
SRK_LC_HD void srk_locate_cross(const double* a, const double* b, double* c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
// the orthonormal frame of a triangle: e1 along A -> B, e3 its normal, e2 = e3 x e1 (columns of a rotation by construction)
SRK_LC_HD void srk_locate_frame(const double* A, const double* B, const double* Cc, double* e1, double* e2, double* e3)
{
    double ab[3], ac[3];
    SRK_LC_UNROLL
    for (int a = 0; a < 3; ++a) {
        ab[a] = B[a] - A[a];
        ac[a] = Cc[a] - A[a];
    }
    const double i1 = 1.0 / sqrt(srk_locate_dot(ab, ab));
    SRK_LC_UNROLL
    for (int a = 0; a < 3; ++a) e1[a] = ab[a] * i1;
    // the part of A -> C across e1 (Gram-Schmidt, then again: e2 is orthogonal to e1 to rounding of e2 itself)
    double t = srk_locate_dot(ac, e1);
    SRK_LC_UNROLL
    for (int a = 0; a < 3; ++a) ac[a] -= t * e1[a];
    t = srk_locate_dot(ac, e1);
    SRK_LC_UNROLL
    for (int a = 0; a < 3; ++a) ac[a] -= t * e1[a];
    const double i2 = 1.0 / sqrt(srk_locate_dot(ac, ac));
    SRK_LC_UNROLL
    for (int a = 0; a < 3; ++a) e2[a] = ac[a] * i2;
    srk_locate_cross(e1, e2, e3);
}

// ---- the quartic c[4] x^4 + ... + c[0]: its real roots in closed form (Ferrari, through the largest real root of the resolvent
// cubic), each polished by SRK_LOCATE_NEWTON Newton steps on the quartic itself.  ok[k] says whether x[k] is a root.
SRK_LC_HD double srk_locate_cubic_largest(double A, double B, double Cc)
{
    // t^3 + A t^2 + B t + C, t = z - A / 3: z^3 + P z + Q
    const double P = B - A * A / 3.0, Q = 2.0 * A * A * A / 27.0 - A * B / 3.0 + Cc;
    const double D = 0.25 * Q * Q + P * P * P / 27.0;
    double z;
    if (D > 0.0) {
        const double s = sqrt(D);
        z = cbrt(-0.5 * Q + s) + cbrt(-0.5 * Q - s);
    } else if (P < 0.0) {
        double c = 1.5 * Q / P * sqrt(-3.0 / P);
        c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
        z = 2.0 * sqrt(-P / 3.0) * cos(acos(c) / 3.0);
    } else
        z = 0.0;
    double t = z - A / 3.0;
    SRK_LC_UNROLL
    for (int it = 0; it < 2; ++it) { // polish: the closed form loses digits where the terms cancel
        const double f = ((t + A) * t + B) * t + Cc, df = (3.0 * t + 2.0 * A) * t + B;
        const double n = t - f / df;
        if (df != 0.0 && isfinite(n)) t = n;
    }
    return t;
}

SRK_LC_HD void srk_locate_quartic(const double* c, double* x, int* ok)
{
    const double i4 = 1.0 / c[4];
    const double a = c[3] * i4, b = c[2] * i4, cc = c[1] * i4, d = c[0] * i4;
    // x = y - a / 4: y^4 + p y^2 + q y + r
    const double a2 = a * a;
    const double p = b - 0.375 * a2, q = cc - 0.5 * a * b + 0.125 * a2 * a, r = d - 0.25 * a * cc + 0.0625 * a2 * b - 0.01171875 * a2 * a2;
    // (y^2 + p / 2 + m)^2 = 2 m (y - q / (4 m))^2 with m a root of m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8
    const double m = srk_locate_cubic_largest(p, 0.25 * p * p - r, -0.125 * q * q);
    double y[4];
    if (m > 0.0) {
        const double s = sqrt(2.0 * m), t = q / s;
        const double d1 = -2.0 * m - 2.0 * p - 2.0 * t, d2 = -2.0 * m - 2.0 * p + 2.0 * t;
        const double s1 = sqrt(d1 > 0.0 ? d1 : 0.0), s2 = sqrt(d2 > 0.0 ? d2 : 0.0);
        ok[0] = ok[1] = d1 >= 0.0;
        ok[2] = ok[3] = d2 >= 0.0;
        y[0] = 0.5 * (s + s1);
        y[1] = 0.5 * (s - s1);
        y[2] = 0.5 * (-s + s2);
        y[3] = 0.5 * (-s - s2);
    } else { // q = 0: a quadratic in y^2
        const double dd = p * p - 4.0 * r, sd = sqrt(dd > 0.0 ? dd : 0.0);
        const double w1 = 0.5 * (-p + sd), w2 = 0.5 * (-p - sd);
        ok[0] = ok[1] = dd >= 0.0 && w1 >= 0.0;
        ok[2] = ok[3] = dd >= 0.0 && w2 >= 0.0;
        y[0] = sqrt(w1 > 0.0 ? w1 : 0.0);
        y[1] = -y[0];
        y[2] = sqrt(w2 > 0.0 ? w2 : 0.0);
        y[3] = -y[2];
    }
    SRK_LC_UNROLL
    for (int k = 0; k < 4; ++k) {
        double v = y[k] - 0.25 * a;
        SRK_LC_UNROLL
        for (int it = 0; it < SRK_LOCATE_NEWTON; ++it) {
            const double f = (((c[4] * v + c[3]) * v + c[2]) * v + c[1]) * v + c[0];
            const double df = ((4.0 * c[4] * v + 3.0 * c[3]) * v + 2.0 * c[2]) * v + c[1];
            const double n = v - f / df;
            if (df != 0.0 && isfinite(n)) v = n;
        }
        x[k] = v;
        ok[k] = ok[k] && isfinite(v);
    }
}

// the pack K [R | T] and row 2 of [R | T] of a pose
SRK_LC_HD void srk_locate_pack(const double* K, const double* R, const double* T, double* p, double* d)
{
    SRK_LC_UNROLL
    for (int a = 0; a < 3; ++a) {
        SRK_LC_UNROLL
        for (int b = 0; b < 3; ++b) p[4 * a + b] = K[3 * a] * R[b] + K[3 * a + 1] * R[3 + b] + K[3 * a + 2] * R[6 + b];
        p[4 * a + 3] = K[3 * a] * T[0] + K[3 * a + 1] * T[1] + K[3 * a + 2] * T[2];
    }
    d[0] = R[6];
    d[1] = R[7];
    d[2] = R[8];
    d[3] = T[2];
}

// the squared pixel error s of the landmark X under the pack and its depth
SRK_LC_HD void srk_locate_project(const double* p, const double* d, const double* X, double u, double v, double f0, double& s, double& depth)
{
    const double pp = p[0] * X[0] + p[1] * X[1] + p[2] * X[2] + p[3];
    const double pq = p[4] * X[0] + p[5] * X[1] + p[6] * X[2] + p[7];
    const double pr = p[8] * X[0] + p[9] * X[1] + p[10] * X[2] + p[11];
    const double ir = 1.0 / pr;
    const double ex = f0 * pp * ir - u, ey = f0 * pq * ir - v;
    s = ex * ex + ey * ey;
    depth = d[0] * X[0] + d[1] * X[1] + d[2] * X[2] + d[3];
}

// One observation's term of the MSAC score, min(q s, tau^2); an observation at depth <= 0 (or with a non-finite error) counts
// tau^2.  inlier = depth > 0 and q s < tau^2.
SRK_LC_HD double srk_locate_term(const double* p, const double* d, const double* X, double u, double v, double q, double f0, double tau2, int& inlier)
{
    double s, depth;
    srk_locate_project(p, d, X, u, v, f0, s, depth);
    const double z = q * s;
    inlier = depth > 0.0 && z < tau2;
    return inlier ? z : tau2;
}

// ---- P3P: Grunert's quartic in v = s3 / s1 (the distances of the three landmarks from the centre), u = s2 / s1 from v, the
// pose from the orthonormal frames of the triangle in the world and in the camera.  The hypothesis of a sample of four: of the
// poses with positive depths at all four points, the one with the smallest squared pixel error at the fourth; a tie goes to the
// earlier root.  X [4][3], uv [4][2].  Ki = K^-1.
struct SrkLocateP3P {
    double b1[3], b2[3], b3[3], n2, n1, n0, e1, e0, w1, lb, w1v[3], w2v[3], w3v[3], v[4];
    int ok[4];
};

// the quartic of a triple and its roots; X [3][3], uv [3][2]
SRK_LC_HD void srk_locate_p3p_setup(const double* Ki, const double* X, const double* uv, double f0, SrkLocateP3P& g)
{
    double* b1 = g.b1;
    double* b2 = g.b2;
    double* b3 = g.b3;
    srk_locate_bearing(Ki, uv[0], uv[1], f0, b1);
    srk_locate_bearing(Ki, uv[2], uv[3], f0, b2);
    srk_locate_bearing(Ki, uv[4], uv[5], f0, b3);
    const double* X1 = X;
    const double* X2 = X + 3;
    const double* X3 = X + 6;
    double d23[3], d13[3], d12[3];
    SRK_LC_UNROLL
    for (int a = 0; a < 3; ++a) {
        d23[a] = X2[a] - X3[a];
        d13[a] = X1[a] - X3[a];
        d12[a] = X1[a] - X2[a];
    }
    const double aa = srk_locate_dot(d23, d23), bb = srk_locate_dot(d13, d13), cc = srk_locate_dot(d12, d12);
    const double ca = srk_locate_dot(b2, b3), cb = srk_locate_dot(b1, b3), cg = srk_locate_dot(b1, b2);
    const double k1 = (aa - cc) / bb, k2 = cc / bb;
    // u = N(v) / D(v); the third distance equation times D^2: D^2 + N^2 - 2 cos(gamma) N D - k2 W D^2 = 0, W = 1 + v^2 - 2 v cos(beta)
    const double n2 = k1 - 1.0, n1 = -2.0 * k1 * cb, n0 = 1.0 + k1;
    const double e1 = -2.0 * ca, e0 = 2.0 * cg;
    const double q2 = e1 * e1, q1 = 2.0 * e1 * e0, q0 = e0 * e0; // D^2
    const double w1 = -2.0 * cb;                                 // W = v^2 + w1 v + 1
    double c[5];
    c[4] = n2 * n2 - k2 * q2;
    c[3] = 2.0 * n2 * n1 - 2.0 * cg * (n2 * e1) - k2 * (q1 + w1 * q2);
    c[2] = q2 + n1 * n1 + 2.0 * n2 * n0 - 2.0 * cg * (n2 * e0 + n1 * e1) - k2 * (q0 + w1 * q1 + q2);
    c[1] = q1 + 2.0 * n1 * n0 - 2.0 * cg * (n1 * e0 + n0 * e1) - k2 * (w1 * q0 + q1);
    c[0] = q0 + n0 * n0 - 2.0 * cg * (n0 * e0) - k2 * q0;
    srk_locate_quartic(c, g.v, g.ok);
    srk_locate_frame(X1, X2, X3, g.w1v, g.w2v, g.w3v); // the triangle's frame in the world
    g.n2 = n2, g.n1 = n1, g.n0 = n0, g.e1 = e1, g.e0 = e0, g.w1 = w1;
    g.lb = sqrt(bb);
}

// the pose of root k: the distances, the triangle's frame in the camera, R = (camera frame) (world frame)^T, T = Q1 - R X1
SRK_LC_HD void srk_locate_p3p_pose(const SrkLocateP3P& g, int k, const double* X1, double* R, double* T)
{
    const double vk = g.v[k];
    const double u = ((g.n2 * vk + g.n1) * vk + g.n0) / (g.e1 * vk + g.e0);
    const double s1 = g.lb / sqrt((vk + g.w1) * vk + 1.0);
    const double s2 = u * s1, s3 = vk * s1;
    double Q1[3], Q2[3], Q3[3], f1[3], f2[3], f3[3];
    SRK_LC_UNROLL
    for (int a = 0; a < 3; ++a) {
        Q1[a] = s1 * g.b1[a];
        Q2[a] = s2 * g.b2[a];
        Q3[a] = s3 * g.b3[a];
    }
    srk_locate_frame(Q1, Q2, Q3, f1, f2, f3);
    SRK_LC_UNROLL
    for (int a = 0; a < 3; ++a) {
        SRK_LC_UNROLL
        for (int bq = 0; bq < 3; ++bq) R[3 * a + bq] = f1[a] * g.w1v[bq] + f2[a] * g.w2v[bq] + f3[a] * g.w3v[bq];
    }
    SRK_LC_UNROLL
    for (int a = 0; a < 3; ++a) T[a] = Q1[a] - (R[3 * a] * X1[0] + R[3 * a + 1] * X1[1] + R[3 * a + 2] * X1[2]);
}

SRK_LC_HD void srk_locate_hypothesis(const double* K, const double* Ki, const double* X, const double* uv, double f0, SrkLocateHyp& hyp)
{
    SrkLocateP3P g;
    srk_locate_p3p_setup(Ki, X, uv, f0, g);
    const double* X1 = X;
    const double* X2 = X + 3;
    const double* X3 = X + 6;
    hyp.valid = 0;
    hyp.e4 = INFINITY;
    SRK_LC_UNROLL
    for (int e = 0; e < 12; ++e) hyp.p[e] = 0.0;
    SRK_LC_UNROLL
    for (int e = 0; e < 4; ++e) hyp.d[e] = 0.0;
    SRK_LC_UNROLL
    for (int e = 0; e < 9; ++e) hyp.R[e] = (e % 4 == 0) ? 1.0 : 0.0;
    SRK_LC_UNROLL
    for (int e = 0; e < 3; ++e) hyp.T[e] = 0.0;
    SRK_LC_UNROLL
    for (int k = 0; k < 4; ++k) {
        double R[9], T[3];
        srk_locate_p3p_pose(g, k, X1, R, T);
        double p[12], d[4], s, z1, z2, z3, z4, e4;
        srk_locate_pack(K, R, T, p, d);
        srk_locate_project(p, d, X1, uv[0], uv[1], f0, s, z1);
        srk_locate_project(p, d, X2, uv[2], uv[3], f0, s, z2);
        srk_locate_project(p, d, X3, uv[4], uv[5], f0, s, z3);
        srk_locate_project(p, d, X + 9, uv[6], uv[7], f0, e4, z4);
        const int good = g.ok[k] && z1 > 0.0 && z2 > 0.0 && z3 > 0.0 && z4 > 0.0 && isfinite(e4);
        if (good && e4 < hyp.e4) {
            hyp.valid = 1;
            hyp.e4 = e4;
            SRK_LC_UNROLL
            for (int e = 0; e < 12; ++e) hyp.p[e] = p[e];
            SRK_LC_UNROLL
            for (int e = 0; e < 4; ++e) hyp.d[e] = d[e];
            SRK_LC_UNROLL
            for (int e = 0; e < 9; ++e) hyp.R[e] = R[e];
            SRK_LC_UNROLL
            for (int e = 0; e < 3; ++e) hyp.T[e] = T[e];
        }
    }
}
