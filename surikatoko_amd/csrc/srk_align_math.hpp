// srk_align_math.hpp -- the arithmetic of map alignment (srk_align_points, srk_ba_align) as plain functions
// of doubles, compiled for the device by srk_align.hip and for the host by srk_align.cpp: the kernels and the host walk of one
// set (srk_align_host_set, tests/cpp/test_align_host.cpp) run the same statements in the same order.  The sampler, Horn's
// three-point hypothesis, one correspondence's term of the score, and the closed-form weighted least-squares similarity through
// the largest eigenvector of Horn's 4 x 4 matrix by cyclic Jacobi.  No HIP header is needed here.  Every array is indexed by
// constants only (the Jacobi pairs are template arguments), so that no per-lane array is indexed at run time.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__)
#define SRK_AL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SRK_AL_HD inline
#endif
#if defined(__clang__)
#define SRK_AL_UNROLL _Pragma("unroll")
#else
#define SRK_AL_UNROLL
#endif

#define SRK_ALIGN_LANES 64    // hypotheses that share a wave
#define SRK_ALIGN_STRIP 8     // doubles of a gathered correspondence: a (3), b (3), q, one of padding (64 bytes)
#define SRK_ALIGN_SLOT 20     // doubles of a wave's best: score, h, inliers, models in the wave, s, sum of the inliers' r^2, R (6-14), t (15-17)
#define SRK_ALIGN_SWEEPS 12   // the most sweeps of the cyclic Jacobi iteration
#define SRK_ALIGN_SIN2 1e-12  // a sample has no model when sin^2 of the angle between its two edges is at most this

// the model of a sample or of a closed form: b ~ s R a + t; sR is what the score multiplies by
struct SrkAlignModel {
    double s, R[9], t[3];
};

// ---- the sampler: counter-based, no state, a stream of its own.  mix = the splitmix64 finaliser of seed + odd * (4 h + k + 1)
SRK_AL_HD uint64_t srk_align_mix(uint64_t seed, uint32_t h, int k)
{
    uint64_t z = seed + 0xA0761D6478BD642Full * (4ull * (uint64_t)h + (uint64_t)k + 1ull);
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// the high 64 bits of a * b, from 32-bit halves: the same integer statements on both sides
SRK_AL_HD uint64_t srk_align_mulhi(uint64_t a, uint64_t b)
{
    const uint64_t al = a & 0xffffffffull, ah = a >> 32, bl = b & 0xffffffffull, bh = b >> 32;
    const uint64_t ll = al * bl, lh = al * bh, hl = ah * bl, hh = ah * bh;
    const uint64_t mid = (ll >> 32) + (lh & 0xffffffffull) + (hl & 0xffffffffull);
    return hh + (lh >> 32) + (hl >> 32) + (mid >> 32);
}

// three distinct ranks below n (n >= 3): draw k is uniform among the n - k ranks not yet picked
SRK_AL_HD void srk_align_sample(uint64_t seed, uint32_t h, int64_t n, int64_t& r0, int64_t& r1, int64_t& r2)
{
    r0 = (int64_t)srk_align_mulhi(srk_align_mix(seed, h, 0), (uint64_t)n);
    r1 = (int64_t)srk_align_mulhi(srk_align_mix(seed, h, 1), (uint64_t)(n - 1));
    if (r1 >= r0) ++r1;
    const int64_t a = r0 < r1 ? r0 : r1, b = r0 < r1 ? r1 : r0; // the earlier picks in ascending order
    r2 = (int64_t)srk_align_mulhi(srk_align_mix(seed, h, 2), (uint64_t)(n - 2));
    if (r2 >= a) ++r2;
    if (r2 >= b) ++r2;
}

// ---- small vector helpers
SRK_AL_HD double srk_align_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
SRK_AL_HD void srk_align_cross(const double* a, const double* b, double* c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

SRK_AL_HD void srk_align_identity(SrkAlignModel& m)
{
    m.s = 1.0;
    SRK_AL_UNROLL
    for (int e = 0; e < 9; ++e) m.R[e] = (e % 4 == 0) ? 1.0 : 0.0;
    m.t[0] = m.t[1] = m.t[2] = 0.0;
}

// the orthonormal frame of a triple p [3][3]: e1 along p0 -> p1, e3 the triangle's normal, e2 = e3 x e1; spread = the sum of the
// squared distances from the centroid, mean = the centroid.  Returns whether the triple has a frame.
SRK_AL_HD int srk_align_triad(const double* p, double* e1, double* e2, double* e3, double* mean, double& spread)
{
    double d1[3], d2[3], c[3];
    SRK_AL_UNROLL
    for (int a = 0; a < 3; ++a) {
        d1[a] = p[3 + a] - p[a];
        d2[a] = p[6 + a] - p[a];
    }
    srk_align_cross(d1, d2, c);
    const double n1 = srk_align_dot(d1, d1), n2 = srk_align_dot(d2, d2), nc = srk_align_dot(c, c);
    const int ok = nc > SRK_ALIGN_SIN2 * n1 * n2 && isfinite(nc); // also false when anything is NaN
    const double i1 = 1.0 / sqrt(n1), ic = 1.0 / sqrt(nc);
    SRK_AL_UNROLL
    for (int a = 0; a < 3; ++a) {
        e1[a] = d1[a] * i1;
        e3[a] = c[a] * ic;
    }
    srk_align_cross(e3, e1, e2);
    spread = 0.0;
    SRK_AL_UNROLL
    for (int a = 0; a < 3; ++a) {
        mean[a] = (p[a] + p[3 + a] + p[6 + a]) / 3.0;
        const double x0 = p[a] - mean[a], x1 = p[3 + a] - mean[a], x2 = p[6 + a] - mean[a];
        spread += x0 * x0 + x1 * x1 + x2 * x2;
    }
    return ok;
}

// Horn's three-point construction: R = B A^T of the two triads, s from the spreads (1 without scale), t from the centroids.
// a3, b3 [3][3].  Returns whether the sample has a model; without one m is (1, I, 0).
SRK_AL_HD int srk_align_hypothesis(const double* a3, const double* b3, int with_scale, SrkAlignModel& m)
{
    double a1[3], a2[3], a3v[3], b1[3], b2[3], b3v[3], am[3], bm[3], sa, sb;
    const int oka = srk_align_triad(a3, a1, a2, a3v, am, sa);
    const int okb = srk_align_triad(b3, b1, b2, b3v, bm, sb);
    SrkAlignModel g;
    SRK_AL_UNROLL
    for (int i = 0; i < 3; ++i) {
        SRK_AL_UNROLL
        for (int j = 0; j < 3; ++j) g.R[3 * i + j] = b1[i] * a1[j] + b2[i] * a2[j] + b3v[i] * a3v[j];
    }
    g.s = with_scale ? sqrt(sb / sa) : 1.0;
    int ok = oka && okb && isfinite(g.s) && g.s > 0.0;
    SRK_AL_UNROLL
    for (int i = 0; i < 3; ++i) {
        g.t[i] = bm[i] - g.s * (g.R[3 * i] * am[0] + g.R[3 * i + 1] * am[1] + g.R[3 * i + 2] * am[2]);
        ok = ok && isfinite(g.t[i]) && isfinite(g.R[3 * i]) && isfinite(g.R[3 * i + 1]) && isfinite(g.R[3 * i + 2]);
    }
    if (ok) m = g;
    else srk_align_identity(m);
    return ok;
}

// what the score multiplies by: s R, once per model
SRK_AL_HD void srk_align_scaled(const SrkAlignModel& m, double* sR)
{
    SRK_AL_UNROLL
    for (int e = 0; e < 9; ++e) sR[e] = m.s * m.R[e];
}

// One correspondence's term of the MSAC score, min(q r^2, tau^2), r = b - (s R a + t); a non-finite error counts tau^2.
// inlier = q r^2 < tau^2; r2 receives r^2.
SRK_AL_HD double srk_align_term(const double* sR, const double* t, const double* a, const double* b, double q, double tau2, int& inlier, double& r2)
{
    const double x = b[0] - (sR[0] * a[0] + sR[1] * a[1] + sR[2] * a[2] + t[0]);
    const double y = b[1] - (sR[3] * a[0] + sR[4] * a[1] + sR[5] * a[2] + t[1]);
    const double z = b[2] - (sR[6] * a[0] + sR[7] * a[1] + sR[8] * a[2] + t[2]);
    r2 = x * x + y * y + z * z;
    const double w = q * r2;
    inlier = w < tau2;
    return inlier ? w : tau2;
}

// ---- the sums of a round of local optimisation, one inlier at a time.  Pass one, acc [7]: sum w, sum w a, sum w b (w = q).
SRK_AL_HD void srk_align_pass_one(double* acc, const double* a, const double* b, double q)
{
    acc[0] += q;
    SRK_AL_UNROLL
    for (int k = 0; k < 3; ++k) {
        acc[1 + k] += q * a[k];
        acc[4 + k] += q * b[k];
    }
}
// Pass two, acc [10]: M = sum w (b - bm)(a - am)^T row by row, then sum w |a - am|^2: centred before multiplying
SRK_AL_HD void srk_align_pass_two(double* acc, const double* a, const double* b, double q, const double* am, const double* bm)
{
    const double da[3] = { a[0] - am[0], a[1] - am[1], a[2] - am[2] };
    const double db[3] = { q * (b[0] - bm[0]), q * (b[1] - bm[1]), q * (b[2] - bm[2]) };
    SRK_AL_UNROLL
    for (int i = 0; i < 3; ++i) {
        SRK_AL_UNROLL
        for (int j = 0; j < 3; ++j) acc[3 * i + j] += db[i] * da[j];
    }
    acc[9] += q * (da[0] * da[0] + da[1] * da[1] + da[2] * da[2]);
}

// ---- the largest eigenvector of a symmetric 4 x 4 matrix by cyclic Jacobi.  One rotation in the plane (P, Q): skipped when the
// off-diagonal entry is zero; t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), and 1 / (2 theta) where theta^2 would overflow.
template <int P, int Q> SRK_AL_HD void srk_align_rotate(double (&A)[4][4], double (&V)[4][4])
{
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = fabs(theta) > 1e150 ? 0.5 / theta : copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] -= t * apq;
    A[Q][Q] += t * apq;
    A[P][Q] = A[Q][P] = 0.0;
    SRK_AL_UNROLL
    for (int r = 0; r < 4; ++r) {
        if (r != P && r != Q) {
            const double arp = A[r][P], arq = A[r][Q];
            A[r][P] = A[P][r] = c * arp - s * arq;
            A[r][Q] = A[Q][r] = s * arp + c * arq;
        }
        const double vrp = V[r][P], vrq = V[r][Q];
        V[r][P] = c * vrp - s * vrq;
        V[r][Q] = s * vrp + c * vrq;
    }
}

// eigenvalues lam [4] (unordered) and eigenvectors (the columns of V) of the symmetric A, which is destroyed
SRK_AL_HD void srk_align_jacobi4(double (&A)[4][4], double (&V)[4][4], double* lam)
{
    SRK_AL_UNROLL
    for (int i = 0; i < 4; ++i) {
        SRK_AL_UNROLL
        for (int j = 0; j < 4; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < SRK_ALIGN_SWEEPS; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[0][3] * A[0][3] + A[1][2] * A[1][2] + A[1][3] * A[1][3] + A[2][3] * A[2][3];
        if (!(off > 0.0)) break; // zero, or not a number
        srk_align_rotate<0, 1>(A, V);
        srk_align_rotate<0, 2>(A, V);
        srk_align_rotate<0, 3>(A, V);
        srk_align_rotate<1, 2>(A, V);
        srk_align_rotate<1, 3>(A, V);
        srk_align_rotate<2, 3>(A, V);
    }
    SRK_AL_UNROLL
    for (int i = 0; i < 4; ++i) lam[i] = A[i][i];
}

// The closed form of one round: the weighted least-squares similarity of the centred sums.  M [9] = sum w (b - bm)(a - am)^T row by
// row, va = sum w |a - am|^2.  R maximises tr(R^T M): the rotation of the unit quaternion that is the eigenvector of the largest
// eigenvalue of Horn's N(M); s = tr(R^T M) / va (1 without scale); t = bm - s R am; gap = (lam1 - lam2) / |lam1| of the two largest
// eigenvalues.  Returns whether the result is finite with s > 0.
SRK_AL_HD int srk_align_closed_form(const double* M, double va, const double* am, const double* bm, int with_scale, SrkAlignModel& m, double& gap)
{
    // Horn's S_jk = sum a_j b_k = M[k][j]
    const double Sxx = M[0], Sxy = M[3], Sxz = M[6], Syx = M[1], Syy = M[4], Syz = M[7], Szx = M[2], Szy = M[5], Szz = M[8];
    double A[4][4], V[4][4], lam[4];
    A[0][0] = Sxx + Syy + Szz;
    A[1][1] = Sxx - Syy - Szz;
    A[2][2] = -Sxx + Syy - Szz;
    A[3][3] = -Sxx - Syy + Szz;
    A[0][1] = A[1][0] = Syz - Szy;
    A[0][2] = A[2][0] = Szx - Sxz;
    A[0][3] = A[3][0] = Sxy - Syx;
    A[1][2] = A[2][1] = Sxy + Syx;
    A[1][3] = A[3][1] = Szx + Sxz;
    A[2][3] = A[3][2] = Syz + Szy;
    srk_align_jacobi4(A, V, lam);
    // the largest eigenvalue and the next one; an equal value stays with the smaller index
    double l1 = lam[0], l2 = -INFINITY, q[4] = { V[0][0], V[1][0], V[2][0], V[3][0] };
    SRK_AL_UNROLL
    for (int k = 1; k < 4; ++k) {
        if (lam[k] > l1) {
            l2 = l1;
            l1 = lam[k];
            SRK_AL_UNROLL
            for (int r = 0; r < 4; ++r) q[r] = V[r][k];
        } else if (lam[k] > l2)
            l2 = lam[k];
    }
    gap = (l1 - l2) / fabs(l1);
    const double in = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] * in, x = q[1] * in, y = q[2] * in, z = q[3] * in;
    m.R[0] = w * w + x * x - y * y - z * z;
    m.R[1] = 2.0 * (x * y - w * z);
    m.R[2] = 2.0 * (x * z + w * y);
    m.R[3] = 2.0 * (x * y + w * z);
    m.R[4] = w * w - x * x + y * y - z * z;
    m.R[5] = 2.0 * (y * z - w * x);
    m.R[6] = 2.0 * (x * z - w * y);
    m.R[7] = 2.0 * (y * z + w * x);
    m.R[8] = w * w - x * x - y * y + z * z;
    double tr = 0.0;
    SRK_AL_UNROLL
    for (int e = 0; e < 9; ++e) tr += m.R[e] * M[e];
    m.s = with_scale ? tr / va : 1.0;
    int ok = isfinite(m.s) && m.s > 0.0 && isfinite(gap);
    SRK_AL_UNROLL
    for (int i = 0; i < 3; ++i) {
        m.t[i] = bm[i] - m.s * (m.R[3 * i] * am[0] + m.R[3 * i + 1] * am[1] + m.R[3 * i + 2] * am[2]);
        ok = ok && isfinite(m.t[i]) && isfinite(m.R[3 * i]) && isfinite(m.R[3 * i + 1]) && isfinite(m.R[3 * i + 2]);
    }
    return ok;
}
