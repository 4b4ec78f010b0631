// srk_tri_math.hpp -- the arithmetic of batched triangulation (srk_triangulate_tracks) as plain functions
// of doubles, compiled for the device by srk_tri.hip and for the host by srk_tri.cpp: the kernel and the host walk of one track
// (srk_tri_host_track, tests/cpp/test_tri_host.cpp) run the same statements in the same order.  No HIP header is needed here.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__)
#define SRK_TRI_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SRK_TRI_HD inline
#endif

#define SRK_TRI_GROUP 8 // lanes that share a track
#define SRK_TRI_PACK 28 // doubles of a frame's pack: 0-11 P = K [R | T] row by row, 12-14 row 2 of R, 15 T_z, 16-24 the ray map
                        // sign(det K) R^T adj(K), 25-27 padding

// the 3 x 3 triangular factor of the rows seen so far and Q^T b: nine doubles
struct SrkTriFactor {
    double r00, r01, r02, r11, r12, r22, z0, z1, z2;
};

// what one pass over a track's observations at a point X adds up: E = sum q |uv - pi(X)|^2 (pixels^2), H = sum q J^T J (upper
// triangle, row by row), g = sum q J^T (pi - uv), the smallest depth and the largest angle to the first ray (radians)
struct SrkTriSums {
    double E, h00, h01, h02, h11, h12, h22, g0, g1, g2, min_depth, max_angle;
};

SRK_TRI_HD void srk_tri_factor_zero(SrkTriFactor& f) { f.r00 = f.r01 = f.r02 = f.r11 = f.r12 = f.r22 = f.z0 = f.z1 = f.z2 = 0.0; }
SRK_TRI_HD void srk_tri_sums_zero(SrkTriSums& s)
{
    s.E = s.h00 = s.h01 = s.h02 = s.h11 = s.h12 = s.h22 = s.g0 = s.g1 = s.g2 = 0.0;
    s.min_depth = INFINITY;
    s.max_angle = 0.0;
}

// the pack of one frame from its inverse pose and intrinsics
SRK_TRI_HD void srk_tri_pack_frame(const double* R, const double* T, const double* K, double* p)
{
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) p[4 * a + b] = K[3 * a] * R[b] + K[3 * a + 1] * R[3 + b] + K[3 * a + 2] * R[6 + b];
        p[4 * a + 3] = K[3 * a] * T[0] + K[3 * a + 1] * T[1] + K[3 * a + 2] * T[2];
    }
    p[12] = R[6];
    p[13] = R[7];
    p[14] = R[8];
    p[15] = T[2];
    double adj[9];
    adj[0] = K[4] * K[8] - K[5] * K[7];
    adj[1] = K[2] * K[7] - K[1] * K[8];
    adj[2] = K[1] * K[5] - K[2] * K[4];
    adj[3] = K[5] * K[6] - K[3] * K[8];
    adj[4] = K[0] * K[8] - K[2] * K[6];
    adj[5] = K[2] * K[3] - K[0] * K[5];
    adj[6] = K[3] * K[7] - K[4] * K[6];
    adj[7] = K[1] * K[6] - K[0] * K[7];
    adj[8] = K[0] * K[4] - K[1] * K[3];
    const double det = K[0] * adj[0] + K[1] * adj[3] + K[2] * adj[6];
    const double sg = det < 0 ? -1.0 : 1.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) p[16 + 3 * a + b] = sg * (R[a] * adj[b] + R[3 + a] * adj[3 + b] + R[6 + a] * adj[6 + b]);
    p[25] = p[26] = p[27] = 0.0;
}

// one row (a | b) into the factor by three Givens rotations; a zero entry is skipped, so a zero row changes no bit
SRK_TRI_HD void srk_tri_fold(SrkTriFactor& f, double a0, double a1, double a2, double b)
{
    if (a0 != 0.0) {
        const double h = sqrt(f.r00 * f.r00 + a0 * a0), c = f.r00 / h, s = a0 / h;
        f.r00 = h;
        double t = c * f.r01 + s * a1;
        a1 = c * a1 - s * f.r01;
        f.r01 = t;
        t = c * f.r02 + s * a2;
        a2 = c * a2 - s * f.r02;
        f.r02 = t;
        t = c * f.z0 + s * b;
        b = c * b - s * f.z0;
        f.z0 = t;
    }
    if (a1 != 0.0) {
        const double h = sqrt(f.r11 * f.r11 + a1 * a1), c = f.r11 / h, s = a1 / h;
        f.r11 = h;
        double t = c * f.r12 + s * a2;
        a2 = c * a2 - s * f.r12;
        f.r12 = t;
        t = c * f.z1 + s * b;
        b = c * b - s * f.z1;
        f.z1 = t;
    }
    if (a2 != 0.0) {
        const double h = sqrt(f.r22 * f.r22 + a2 * a2), c = f.r22 / h, s = a2 / h;
        f.r22 = h;
        f.z2 = c * f.z2 + s * b;
    }
}

// the factor of the rows of f and of g together (TSQR): the three rows of g folded into f, top row first
SRK_TRI_HD void srk_tri_merge(SrkTriFactor& f, const SrkTriFactor& g)
{
    srk_tri_fold(f, g.r00, g.r01, g.r02, g.z0);
    srk_tri_fold(f, 0.0, g.r11, g.r12, g.z1);
    srk_tri_fold(f, 0.0, 0.0, g.r22, g.z2);
}

// the two rows of one observation (obs-geom.cpp:700-712): x p2 - f0 p0 and y p2 - f0 p1, scaled by sq = sqrt(q)
SRK_TRI_HD void srk_tri_fold_obs(SrkTriFactor& f, const double* p, double x, double y, double f0, double sq)
{
    srk_tri_fold(f, sq * (x * p[8] - f0 * p[0]), sq * (x * p[9] - f0 * p[1]), sq * (x * p[10] - f0 * p[2]), -sq * (x * p[11] - f0 * p[3]));
    srk_tri_fold(f, sq * (y * p[8] - f0 * p[4]), sq * (y * p[9] - f0 * p[5]), sq * (y * p[10] - f0 * p[6]), -sq * (y * p[11] - f0 * p[7]));
}

// the viewing ray of a pixel in world coordinates, any positive length
SRK_TRI_HD void srk_tri_ray(const double* p, double x, double y, double f0, double ray[3])
{
    for (int a = 0; a < 3; ++a) ray[a] = p[16 + 3 * a] * x + p[17 + 3 * a] * y + p[18 + 3 * a] * f0;
}
SRK_TRI_HD double srk_tri_angle(const double a[3], const double b[3])
{
    const double c0 = a[1] * b[2] - a[2] * b[1], c1 = a[2] * b[0] - a[0] * b[2], c2 = a[0] * b[1] - a[1] * b[0];
    return atan2(sqrt(c0 * c0 + c1 * c1 + c2 * c2), a[0] * b[0] + a[1] * b[1] + a[2] * b[2]);
}

// R X = z; returns 0 when a diagonal entry is zero or not finite or X is not finite (the host function's rule for returning 0)
SRK_TRI_HD int srk_tri_solve(const SrkTriFactor& f, double X[3])
{
    X[2] = f.z2 / f.r22;
    X[1] = (f.z1 - f.r12 * X[2]) / f.r11;
    X[0] = (f.z0 - f.r01 * X[1] - f.r02 * X[2]) / f.r00;
    const bool diag = f.r00 != 0.0 && f.r11 != 0.0 && f.r22 != 0.0 && isfinite(f.r00) && isfinite(f.r11) && isfinite(f.r22);
    return diag && isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]) ? 1 : 0;
}

// the 1-norm condition number of the triangular factor: |R|_1 |R^-1|_1 with the inverse written out
SRK_TRI_HD double srk_tri_cond1(const SrkTriFactor& f)
{
    const double n0 = fabs(f.r00), n1 = fabs(f.r01) + fabs(f.r11), n2 = fabs(f.r02) + fabs(f.r12) + fabs(f.r22);
    const double nr = fmax(n0, fmax(n1, n2));
    const double i00 = 1.0 / f.r00, i11 = 1.0 / f.r11, i22 = 1.0 / f.r22;
    const double i01 = -f.r01 * i00 * i11, i12 = -f.r12 * i11 * i22, i02 = -(f.r01 * i12 + f.r02 * i22) * i00;
    const double m0 = fabs(i00), m1 = fabs(i01) + fabs(i11), m2 = fabs(i02) + fabs(i12) + fabs(i22);
    return nr * fmax(m0, fmax(m1, m2));
}

// one observation at X into the sums; q its information (1 without weights)
SRK_TRI_HD void srk_tri_eval_obs(SrkTriSums& s, const double* p, double x, double y, double f0, double q, const double X[3])
{
    const double pp = p[0] * X[0] + p[1] * X[1] + p[2] * X[2] + p[3];
    const double pq = p[4] * X[0] + p[5] * X[1] + p[6] * X[2] + p[7];
    const double pr = p[8] * X[0] + p[9] * X[1] + p[10] * X[2] + p[11];
    const double ir = 1.0 / pr;
    const double ex = f0 * pp * ir - x, ey = f0 * pq * ir - y; // pi - uv
    const double k = f0 * ir * ir;
    double jx[3], jy[3];
    for (int a = 0; a < 3; ++a) {
        jx[a] = k * (pr * p[a] - pp * p[8 + a]);
        jy[a] = k * (pr * p[4 + a] - pq * p[8 + a]);
    }
    s.E += q * (ex * ex + ey * ey);
    s.h00 += q * (jx[0] * jx[0] + jy[0] * jy[0]);
    s.h01 += q * (jx[0] * jx[1] + jy[0] * jy[1]);
    s.h02 += q * (jx[0] * jx[2] + jy[0] * jy[2]);
    s.h11 += q * (jx[1] * jx[1] + jy[1] * jy[1]);
    s.h12 += q * (jx[1] * jx[2] + jy[1] * jy[2]);
    s.h22 += q * (jx[2] * jx[2] + jy[2] * jy[2]);
    s.g0 += q * (jx[0] * ex + jy[0] * ey);
    s.g1 += q * (jx[1] * ex + jy[1] * ey);
    s.g2 += q * (jx[2] * ex + jy[2] * ey);
    s.min_depth = fmin(s.min_depth, p[12] * X[0] + p[13] * X[1] + p[14] * X[2] + p[15]);
}

// the sums of two lanes: a + b entry by entry
SRK_TRI_HD void srk_tri_sums_add(SrkTriSums& a, const SrkTriSums& b)
{
    a.E += b.E;
    a.h00 += b.h00; a.h01 += b.h01; a.h02 += b.h02; a.h11 += b.h11; a.h12 += b.h12; a.h22 += b.h22;
    a.g0 += b.g0; a.g1 += b.g1; a.g2 += b.g2;
    a.min_depth = fmin(a.min_depth, b.min_depth);
    a.max_angle = fmax(a.max_angle, b.max_angle);
}

// (H + c diag H) d = -g by a written-out Cholesky factorisation; 0 when a pivot is not positive or d is not finite
SRK_TRI_HD int srk_tri_lm_step(const SrkTriSums& s, double c, double d[3])
{
    const double a00 = s.h00 + c * s.h00, a11 = s.h11 + c * s.h11, a22 = s.h22 + c * s.h22;
    if (!(a00 > 0.0)) return 0;
    const double l00 = sqrt(a00), l10 = s.h01 / l00, l20 = s.h02 / l00;
    const double p1 = a11 - l10 * l10;
    if (!(p1 > 0.0)) return 0;
    const double l11 = sqrt(p1), l21 = (s.h12 - l20 * l10) / l11;
    const double p2 = a22 - l20 * l20 - l21 * l21;
    if (!(p2 > 0.0)) return 0;
    const double l22 = sqrt(p2);
    const double y0 = -s.g0 / l00, y1 = (-s.g1 - l10 * y0) / l11, y2 = (-s.g2 - l20 * y0 - l21 * y1) / l22;
    d[2] = y2 / l22;
    d[1] = (y1 - l21 * d[2]) / l11;
    d[0] = (y0 - l10 * d[1] - l20 * d[2]) / l00;
    return isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]) ? 1 : 0;
}

// The refinement loop's decisions, shared by the kernel and the host walk: `cur` the sums at the accepted point X, `cand` those
// at X + d.  Accepted iff E decreases; the damping factor c is divided by 10 then, multiplied by 10 otherwise.  Returns 1 when
// an accepted attempt changed E by less than rel_change E (the loop stops).
SRK_TRI_HD int srk_tri_lm_judge(SrkTriSums& cur, const SrkTriSums& cand, int stepped, double X[3], const double Xn[3], double& c, double rel_change)
{
    if (stepped && cand.E < cur.E) {
        const double dE = cur.E - cand.E, bound = rel_change * cur.E;
        const double keep = cur.max_angle;
        cur = cand;
        cur.max_angle = keep;
        X[0] = Xn[0];
        X[1] = Xn[1];
        X[2] = Xn[2];
        c /= 10.0;
        return dE < bound ? 1 : 0;
    }
    c *= 10.0;
    return 0;
}

// quality[4] and the status bits of a finished track (SRK_TRI_* of srk_ba.h; bit values repeated in srk_tri.hpp's static_assert)
SRK_TRI_HD uint32_t srk_tri_finish(const SrkTriFactor& f, const SrkTriSums& cur, int solved, int64_t n_weighted, double min_parallax_deg, int hit_cap,
                                   double quality[4])
{
    const double deg = cur.max_angle * 57.295779513082320877;
    quality[0] = sqrt(cur.E / (double)n_weighted);
    quality[1] = deg;
    quality[2] = srk_tri_cond1(f);
    quality[3] = (double)n_weighted;
    uint32_t st = 0;
    if (!solved) st |= 2u;
    if (!(cur.min_depth > 0.0)) st |= 4u;
    if (min_parallax_deg > 0.0 && !(deg >= min_parallax_deg)) st |= 8u;
    if (hit_cap) st |= 16u;
    return st;
}
