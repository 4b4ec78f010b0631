// srk_resect_math.hpp -- the arithmetic of batched camera resection (srk_resect_frames, srk_ba_resect) as
// plain functions of doubles, compiled for the device by srk_resect.hip and for the host by srk_resect.cpp: the kernel and the
// host walk of one frame (srk_resect_host_frame, tests/cpp/test_resect_host.cpp) run the same statements in the same order.  No
// HIP header is needed here.  Every loop over the six variables has constant bounds and is unrolled for the device, so that no
// per-lane array is indexed at run time (such an array would live in scratch memory).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__)
#define SRK_RS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SRK_RS_HD inline
#endif
#if defined(__clang__)
#define SRK_RS_UNROLL _Pragma("unroll")
#else
#define SRK_RS_UNROLL
#endif

#define SRK_RESECT_LANES 64 // lanes that share a frame: one wave
#define SRK_RESECT_PACK 20  // doubles of a pose's pack: 0-11 P = K [R | T] row by row, 12-15 row 2 of [R | T], 16-18 C = -R^T T, 19 padding
#define SRK_RESECT_NH 21    // the upper triangle of the 6 x 6 H, row by row
#define SRK_RESECT_C0 1e-4  // the damping factor an LM loop starts with

// the pose a loop carries: the inverse rotation R (row-major), the inverse translation T and the centre C = -R^T T
struct SrkResectPose {
    double R[9], T[3], C[3];
};

// What one pass over a frame's weighted observations at a pose adds up: E = sum rho(q s) (pixels^2), H = sum q w J^T J (upper
// triangle, row by row), g = sum q w J^T e, the sum of the robust weights w and the smallest depth
struct SrkResectSums {
    double E, h[SRK_RESECT_NH], g[6], wsum, min_depth;
};

SRK_RS_HD void srk_resect_sums_zero(SrkResectSums& s)
{
    s.E = s.wsum = 0.0;
    SRK_RS_UNROLL
    for (int e = 0; e < SRK_RESECT_NH; ++e) s.h[e] = 0.0;
    SRK_RS_UNROLL
    for (int e = 0; e < 6; ++e) s.g[e] = 0.0;
    s.min_depth = INFINITY;
}

// the sums of two lanes: a + b entry by entry
SRK_RS_HD void srk_resect_sums_add(SrkResectSums& a, const SrkResectSums& b)
{
    a.E += b.E;
    SRK_RS_UNROLL
    for (int e = 0; e < SRK_RESECT_NH; ++e) a.h[e] += b.h[e];
    SRK_RS_UNROLL
    for (int e = 0; e < 6; ++e) a.g[e] += b.g[e];
    a.wsum += b.wsum;
    a.min_depth = fmin(a.min_depth, b.min_depth);
}

// the start pose of a frame: R and T as given (they are returned bit for bit when nothing is accepted), C = -R^T T
SRK_RS_HD void srk_resect_start_pose(const double* R, const double* T, SrkResectPose& p)
{
    SRK_RS_UNROLL
    for (int e = 0; e < 9; ++e) p.R[e] = R[e];
    SRK_RS_UNROLL
    for (int a = 0; a < 3; ++a) {
        p.T[a] = T[a];
        p.C[a] = -(R[a] * T[0] + R[3 + a] * T[1] + R[6 + a] * T[2]);
    }
}

// the pack of a pose and its intrinsics
SRK_RS_HD void srk_resect_pack_pose(const SrkResectPose& s, const double* K, double* p)
{
    SRK_RS_UNROLL
    for (int a = 0; a < 3; ++a) {
        SRK_RS_UNROLL
        for (int b = 0; b < 3; ++b) p[4 * a + b] = K[3 * a] * s.R[b] + K[3 * a + 1] * s.R[3 + b] + K[3 * a + 2] * s.R[6 + b];
        p[4 * a + 3] = K[3 * a] * s.T[0] + K[3 * a + 1] * s.T[1] + K[3 * a + 2] * s.T[2];
    }
    p[12] = s.R[6];
    p[13] = s.R[7];
    p[14] = s.R[8];
    p[15] = s.T[2];
    p[16] = s.C[0];
    p[17] = s.C[1];
    p[18] = s.C[2];
    p[19] = 0.0;
}

// rho(z) and w = rho'(z) of srk_ba_set_robust_loss, z = q s in pixels^2 and d = delta in pixels: none, Huber, Cauchy
SRK_RS_HD void srk_resect_rho(double z, int kind, double d, double& rho, double& w)
{
    rho = z;
    w = 1.0;
    const double d2 = d * d;
    if (kind == 1) {
        if (z > d2) {
            const double rs = sqrt(z);
            rho = 2.0 * d * rs - d2;
            w = d / rs;
        }
    } else if (kind == 2) {
        const double t = z / d2;
        rho = d2 * log1p(t);
        w = 1.0 / (1.0 + t);
    }
}

// the reprojection error (pi - uv, pixels) of the landmark X under the pack p, its squared length and the depth
SRK_RS_HD void srk_resect_residual(const double* p, const double* X, double u, double v, double f0, double& pp, double& pq, double& pr, double& ex,
                                   double& ey)
{
    pp = p[0] * X[0] + p[1] * X[1] + p[2] * X[2] + p[3];
    pq = p[4] * X[0] + p[5] * X[1] + p[6] * X[2] + p[7];
    pr = p[8] * X[0] + p[9] * X[1] + p[10] * X[2] + p[11];
    const double ir = 1.0 / pr;
    ex = f0 * pp * ir - u;
    ey = f0 * pq * ir - v;
}

// One observation into the sums.  With x_cam = R (X - C) and the perturbation [t; w] (C <- C + t, R^T <- Exp(w) R^T):
// d x_cam / d [t; w] = R [ -I | [X - C]x ], so with a = d pi / d X (a row, as in triangulation) the row of J is [ -a | a x (X - C) ].
SRK_RS_HD void srk_resect_obs(SrkResectSums& s, const double* p, const double* X, double u, double v, double f0, double q, int kind, double delta)
{
    double pp, pq, pr, ex, ey;
    srk_resect_residual(p, X, u, v, f0, pp, pq, pr, ex, ey);
    const double k = f0 / (pr * pr);
    double ax[3], ay[3], d[3];
    SRK_RS_UNROLL
    for (int a = 0; a < 3; ++a) {
        ax[a] = k * (pr * p[a] - pp * p[8 + a]);
        ay[a] = k * (pr * p[4 + a] - pq * p[8 + a]);
        d[a] = X[a] - p[16 + a];
    }
    const double jx[6] = { -ax[0], -ax[1], -ax[2], ax[1] * d[2] - ax[2] * d[1], ax[2] * d[0] - ax[0] * d[2], ax[0] * d[1] - ax[1] * d[0] };
    const double jy[6] = { -ay[0], -ay[1], -ay[2], ay[1] * d[2] - ay[2] * d[1], ay[2] * d[0] - ay[0] * d[2], ay[0] * d[1] - ay[1] * d[0] };
    double rho, w;
    srk_resect_rho(q * (ex * ex + ey * ey), kind, delta, rho, w);
    const double qw = q * w;
    s.E += rho;
    s.wsum += w;
    int e = 0;
    SRK_RS_UNROLL
    for (int a = 0; a < 6; ++a) {
        SRK_RS_UNROLL
        for (int b = a; b < 6; ++b) s.h[e++] += qw * (jx[a] * jx[b] + jy[a] * jy[b]);
        s.g[a] += qw * (jx[a] * ex + jy[a] * ey);
    }
    s.min_depth = fmin(s.min_depth, p[12] * X[0] + p[13] * X[1] + p[14] * X[2] + p[15]);
}

// the robust weight rho'(q s) of one observation under the pack p
SRK_RS_HD double srk_resect_weight(const double* p, const double* X, double u, double v, double f0, double q, int kind, double delta)
{
    double pp, pq, pr, ex, ey, rho, w;
    srk_resect_residual(p, X, u, v, f0, pp, pq, pr, ex, ey);
    srk_resect_rho(q * (ex * ex + ey * ey), kind, delta, rho, w);
    return w;
}

// the upper triangle h into a full symmetric 6 x 6
SRK_RS_HD void srk_resect_full(const double* h, double A[6][6])
{
    int e = 0;
    SRK_RS_UNROLL
    for (int a = 0; a < 6; ++a) {
        SRK_RS_UNROLL
        for (int b = a; b < 6; ++b) {
            A[a][b] = h[e];
            A[b][a] = h[e++];
        }
    }
}

// A = L L^T in place (the lower triangle becomes L), written out; 0 when a pivot is not positive (NaN included)
SRK_RS_HD int srk_resect_chol6(double A[6][6])
{
    int ok = 1;
    SRK_RS_UNROLL
    for (int j = 0; j < 6; ++j) {
        double piv = A[j][j];
        SRK_RS_UNROLL
        for (int k = 0; k < j; ++k) piv -= A[j][k] * A[j][k];
        if (!(piv > 0.0)) ok = 0;
        const double l = sqrt(piv);
        A[j][j] = l;
        SRK_RS_UNROLL
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
            SRK_RS_UNROLL
            for (int k = 0; k < j; ++k) v -= A[i][k] * A[j][k];
            A[i][j] = v / l;
        }
    }
    return ok;
}

// (H + c diag H) d = -g by the written-out Cholesky factorisation; 0 when a pivot is not positive or d is not finite
SRK_RS_HD int srk_resect_lm_step(const SrkResectSums& s, double c, double d[6])
{
    double A[6][6], y[6];
    srk_resect_full(s.h, A);
    SRK_RS_UNROLL
    for (int a = 0; a < 6; ++a) A[a][a] = A[a][a] + c * A[a][a];
    int ok = srk_resect_chol6(A);
    SRK_RS_UNROLL
    for (int i = 0; i < 6; ++i) {
        double v = -s.g[i];
        SRK_RS_UNROLL
        for (int k = 0; k < i; ++k) v -= A[i][k] * y[k];
        y[i] = v / A[i][i];
    }
    SRK_RS_UNROLL
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
        SRK_RS_UNROLL
        for (int k = i + 1; k < 6; ++k) v -= A[k][i] * d[k];
        d[i] = v / A[i][i];
    }
    SRK_RS_UNROLL
    for (int i = 0; i < 6; ++i)
        if (!isfinite(d[i])) ok = 0;
    return ok;
}

// Exp of a rotation vector (Rodrigues), row-major; the series below 1e-4 rad, where it is exact to the last bit or two
SRK_RS_HD void srk_resect_exp(const double w[3], double E[9])
{
    const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double a, b;
    if (t2 < 1e-8) {
        a = 1.0 - t2 * (1.0 / 6.0) * (1.0 - t2 * (1.0 / 20.0));
        b = 0.5 - t2 * (1.0 / 24.0) * (1.0 - t2 * (1.0 / 30.0));
    } else {
        const double t = sqrt(t2), h = sin(0.5 * t) / t;
        a = sin(t) / t;
        b = 2.0 * h * h;
    }
    E[0] = 1.0 - b * (w[1] * w[1] + w[2] * w[2]);
    E[4] = 1.0 - b * (w[0] * w[0] + w[2] * w[2]);
    E[8] = 1.0 - b * (w[0] * w[0] + w[1] * w[1]);
    E[1] = b * w[0] * w[1] - a * w[2];
    E[3] = b * w[0] * w[1] + a * w[2];
    E[2] = b * w[0] * w[2] + a * w[1];
    E[6] = b * w[0] * w[2] - a * w[1];
    E[5] = b * w[1] * w[2] - a * w[0];
    E[7] = b * w[1] * w[2] + a * w[0];
}

// the pose moved by d = [t; w]: C + t and R^T <- Exp(w) R^T, that is R Exp(w)^T -- a product of rotations, no entry is added to
SRK_RS_HD void srk_resect_move(const SrkResectPose& s, const double d[6], SrkResectPose& n)
{
    double E[9];
    srk_resect_exp(d + 3, E);
    SRK_RS_UNROLL
    for (int a = 0; a < 3; ++a) {
        SRK_RS_UNROLL
        for (int b = 0; b < 3; ++b) n.R[3 * a + b] = s.R[3 * a] * E[3 * b] + s.R[3 * a + 1] * E[3 * b + 1] + s.R[3 * a + 2] * E[3 * b + 2];
        n.C[a] = s.C[a] + d[a];
    }
    SRK_RS_UNROLL
    for (int a = 0; a < 3; ++a) n.T[a] = -(n.R[3 * a] * n.C[0] + n.R[3 * a + 1] * n.C[1] + n.R[3 * a + 2] * n.C[2]);
}

// The loop's decision, shared by the kernel and the host walk (the rule of srk_tri_lm_judge): `cur` the sums at the accepted
// pose, `cand` those at the moved one.  Accepted iff E decreases (a NaN does not); the damping factor c is divided by 10 then,
// multiplied by 10 otherwise.  Returns bit 0 = accepted, bit 1 = the accepted attempt changed E by less than rel_change E (stop).
SRK_RS_HD int srk_resect_judge(double cur_E, double cand_E, int stepped, double& c, double rel_change)
{
    if (stepped && cand_E < cur_E) {
        const double dE = cur_E - cand_E, bound = rel_change * cur_E;
        c /= 10.0;
        return dE < bound ? 3 : 1;
    }
    c *= 10.0;
    return 0;
}

// cond_1 of the Jacobi-scaled H_s = D^-1/2 H D^-1/2 (A: the full symmetric H, destroyed): |H_s|_1 |H_s^-1|_1 with the inverse
// written out from the Cholesky factor.  NaN when H_s is not positive definite.
SRK_RS_HD double srk_resect_cond1(double A[6][6])
{
    double is[6];
    SRK_RS_UNROLL
    for (int a = 0; a < 6; ++a) is[a] = 1.0 / sqrt(A[a][a]);
    SRK_RS_UNROLL
    for (int a = 0; a < 6; ++a) {
        SRK_RS_UNROLL
        for (int b = 0; b < 6; ++b) A[a][b] = A[a][b] * (is[a] * is[b]);
    }
    double n1 = 0.0;
    SRK_RS_UNROLL
    for (int b = 0; b < 6; ++b) {
        double col = 0.0;
        SRK_RS_UNROLL
        for (int a = 0; a < 6; ++a) col += fabs(A[a][b]);
        n1 = fmax(n1, col);
    }
    const int pd = srk_resect_chol6(A);
    // the inverse of the factor, M = L^-1 (lower), then H_s^-1 = M^T M
    double M[6][6];
    SRK_RS_UNROLL
    for (int j = 0; j < 6; ++j) {
        M[j][j] = 1.0 / A[j][j];
        SRK_RS_UNROLL
        for (int i = j + 1; i < 6; ++i) {
            double v = 0.0;
            SRK_RS_UNROLL
            for (int k = j; k < i; ++k) v -= A[i][k] * M[k][j];
            M[i][j] = v / A[i][i];
        }
    }
    double n2 = 0.0;
    SRK_RS_UNROLL
    for (int b = 0; b < 6; ++b) {
        double col = 0.0;
        SRK_RS_UNROLL
        for (int a = 0; a < 6; ++a) {
            double v = 0.0;
            SRK_RS_UNROLL
            for (int k = (a > b ? a : b); k < 6; ++k) v += M[k][a] * M[k][b];
            col += fabs(v);
        }
        n2 = fmax(n2, col);
    }
    return pd ? n1 * n2 : NAN;
}

// quality[6], info[36] and the status bits of a finished frame with n >= 3 weighted observations (SRK_RESECT_* of srk_ba.h; the bit
// values are repeated in srk_resect.cpp's static_assert)
SRK_RS_HD uint32_t srk_resect_finish(const SrkResectSums& cur, int64_t n, double f0, int hit_cap, int attempts_used, double quality[6], double info[36])
{
    double A[6][6];
    srk_resect_full(cur.h, A);
    const double if2 = 1.0 / (f0 * f0);
    int finite = isfinite(cur.E) ? 1 : 0;
    SRK_RS_UNROLL
    for (int a = 0; a < 6; ++a) {
        SRK_RS_UNROLL
        for (int b = 0; b < 6; ++b) {
            info[6 * a + b] = A[a][b] * if2;
            if (!isfinite(A[a][b])) finite = 0;
        }
    }
    const double cond = srk_resect_cond1(A);
    quality[0] = sqrt(cur.E / (double)n);
    quality[1] = (double)n;
    quality[2] = cur.wsum / (double)n;
    quality[3] = cond;
    quality[4] = cur.min_depth;
    quality[5] = (double)attempts_used;
    uint32_t st = 0;
    if (!finite || !isfinite(cond)) st |= 2u;
    if (!(cur.min_depth > 0.0)) st |= 4u;
    if (hit_cap) st |= 8u;
    return st;
}

// a frame with fewer than three weighted observations: nothing is refined
SRK_RS_HD uint32_t srk_resect_few(int64_t n, double quality[6], double info[36])
{
    quality[0] = NAN;
    quality[1] = (double)n;
    quality[2] = NAN;
    quality[3] = NAN;
    quality[4] = NAN;
    quality[5] = 0.0;
    SRK_RS_UNROLL
    for (int e = 0; e < 36; ++e) info[e] = 0.0;
    return 1u;
}
