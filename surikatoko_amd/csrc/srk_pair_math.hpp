// srk_pair_math.hpp -- the arithmetic of two-view pose refinement (srk_refine_pairs, srk_relate_frames_refined; DESIGN.md section
// 26) as plain functions of doubles, compiled for the device by srk_pair.hip and for the host by srk_pair.cpp: the kernel and the
// host walk of one pair (srk_pair_host_pair, tests/cpp/test_pair_host.cpp) run the same statements in the same order.  No HIP header
// is needed here.  Every loop over the five variables has constant bounds and is unrolled for the device, so that no per-lane array
// is indexed at run time (such an array would live in scratch memory).
//
// Reused, not repeated:
//   from srk_resect_math.hpp  srk_resect_rho (the loss rho / rho' of srk_ba_set_robust_loss), srk_resect_exp (Exp of a rotation
//                             vector), srk_resect_judge (the LM loop's decision) and SRK_RESECT_C0 (the first damping factor);
//   from srk_relate_math.hpp  srk_relate_inverse3 (the adjugate inverse of K), srk_relate_fundamental (F = K_b^-T E K_a^-1),
//                             srk_relate_essential (E = [T]x R), srk_relate_ray, srk_relate_cross, srk_relate_dot, and the terms of
//                             srk_relate_sampson (the same products in the same order, so that s has the bits of relate's score).
// New here: the tangent basis of T, the five dF_k, the residual's Jacobian, the 5 x 5 Cholesky solve and condition number.
#pragma once
#include "srk_relate_math.hpp"
#include "srk_resect_math.hpp"

#define SRK_PR_HD SRK_RS_HD
#define SRK_PR_UNROLL SRK_RS_UNROLL

#define SRK_PAIR_LANES 64 // lanes that share a pair: one wave
#define SRK_PAIR_NV 5     // variables: w (3), beta (2)
#define SRK_PAIR_NH 15    // the upper triangle of the 5 x 5 H, row by row
#define SRK_PAIR_KINV 18  // doubles of a pair's pack: K_a^-1 (0-8), K_b^-1 (9-17)

// the pose a loop carries: R (row-major) and the unit vector T
struct SrkPairPose {
    double R[9], T[3];
};

// What is uniform over a pair at one pose: F and the five dF_k = K_b^-T (dE / dd_k) K_a^-1
struct SrkPairLin {
    double F[9], dF[SRK_PAIR_NV][9];
};

// What one pass over a pair's weighted matches at a pose adds up: E = sum rho(q s) (pixels^2), H = sum q w J^T J (upper triangle,
// row by row), g = sum q w J r and the sum of the robust weights w
struct SrkPairSums {
    double E, h[SRK_PAIR_NH], g[SRK_PAIR_NV], wsum;
};

SRK_PR_HD void srk_pair_sums_zero(SrkPairSums& s)
{
    s.E = s.wsum = 0.0;
    SRK_PR_UNROLL
    for (int e = 0; e < SRK_PAIR_NH; ++e) s.h[e] = 0.0;
    SRK_PR_UNROLL
    for (int e = 0; e < SRK_PAIR_NV; ++e) s.g[e] = 0.0;
}

// the sums of two lanes: a + b entry by entry
SRK_PR_HD void srk_pair_sums_add(SrkPairSums& a, const SrkPairSums& b)
{
    a.E += b.E;
    SRK_PR_UNROLL
    for (int e = 0; e < SRK_PAIR_NH; ++e) a.h[e] += b.h[e];
    SRK_PR_UNROLL
    for (int e = 0; e < SRK_PAIR_NV; ++e) a.g[e] += b.g[e];
    a.wsum += b.wsum;
}

// the start pose of a pair: R and T as given (they are returned bit for bit when nothing is accepted).  With `unrelated` (the
// chained call: relate gave this pair no pose) the start is (I, (1, 0, 0)).
SRK_PR_HD void srk_pair_start_pose(const double* R, const double* T, int unrelated, SrkPairPose& p)
{
    SRK_PR_UNROLL
    for (int e = 0; e < 9; ++e) p.R[e] = unrelated ? (e % 4 == 0 ? 1.0 : 0.0) : R[e];
    SRK_PR_UNROLL
    for (int a = 0; a < 3; ++a) p.T[a] = unrelated ? (a == 0 ? 1.0 : 0.0) : T[a];
}

// The tangent basis of the unit sphere at T, fixed by rule: k the index of the smallest |T_k| (a tie: the smaller k),
// b1 = (e_k x T) / |e_k x T|, b2 = T x b1.  The choice is made among values, not among addresses.
SRK_PR_HD void srk_pair_basis(const double* T, double* b1, double* b2)
{
    const double a0 = fabs(T[0]), a1 = fabs(T[1]), a2 = fabs(T[2]);
    const int k = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
    // e_0 x T = (0, -T2, T1), e_1 x T = (T2, 0, -T0), e_2 x T = (-T1, T0, 0)
    const double c0 = k == 0 ? 0.0 : (k == 1 ? T[2] : -T[1]);
    const double c1 = k == 0 ? -T[2] : (k == 1 ? 0.0 : T[0]);
    const double c2 = k == 0 ? T[1] : (k == 1 ? -T[0] : 0.0);
    const double in = 1.0 / sqrt(c0 * c0 + c1 * c1 + c2 * c2);
    b1[0] = c0 * in;
    b1[1] = c1 * in;
    b1[2] = c2 * in;
    srk_relate_cross(T, b1, b2);
}

// F and the five dF_k at the pose: dE/dw_i = -[T]x R [e_i]x = -E [e_i]x, whose columns are those of E up to sign
// (-E [e_0]x = [0, -E_2, E_1], -E [e_1]x = [E_2, 0, -E_0], -E [e_2]x = [-E_1, E_0, 0]); dE/dbeta_j = [b_j]x R.
SRK_PR_HD void srk_pair_linearise(const double* kinv, const SrkPairPose& p, SrkPairLin& lin)
{
    double E[9], D[9], b1[3], b2[3];
    srk_relate_essential(p.R, p.T, E);
    srk_relate_fundamental(kinv, kinv + 9, E, lin.F);
    SRK_PR_UNROLL
    for (int i = 0; i < 3; ++i) {
        D[3 * i] = 0.0;
        D[3 * i + 1] = -E[3 * i + 2];
        D[3 * i + 2] = E[3 * i + 1];
    }
    srk_relate_fundamental(kinv, kinv + 9, D, lin.dF[0]);
    SRK_PR_UNROLL
    for (int i = 0; i < 3; ++i) {
        D[3 * i] = E[3 * i + 2];
        D[3 * i + 1] = 0.0;
        D[3 * i + 2] = -E[3 * i];
    }
    srk_relate_fundamental(kinv, kinv + 9, D, lin.dF[1]);
    SRK_PR_UNROLL
    for (int i = 0; i < 3; ++i) {
        D[3 * i] = -E[3 * i + 1];
        D[3 * i + 1] = E[3 * i];
        D[3 * i + 2] = 0.0;
    }
    srk_relate_fundamental(kinv, kinv + 9, D, lin.dF[2]);
    srk_pair_basis(p.T, b1, b2);
    srk_relate_essential(p.R, b1, D);
    srk_relate_fundamental(kinv, kinv + 9, D, lin.dF[3]);
    srk_relate_essential(p.R, b2, D);
    srk_relate_fundamental(kinv, kinv + 9, D, lin.dF[4]);
}

// The terms of the Sampson distance of a match under F, in the order of srk_relate_sampson: l = F p_a, m = F^T p_b (two entries),
// e = p_b . l, den = l0^2 + l1^2 + m0^2 + m1^2; s = e e / den has the bits of relate's.
SRK_PR_HD void srk_pair_sampson_terms(const double* F, double ua, double va, double ub, double vb, double f0, double& l0, double& l1, double& m0,
                                      double& m1, double& e, double& den)
{
    l0 = F[0] * ua + F[1] * va + F[2] * f0;
    l1 = F[3] * ua + F[4] * va + F[5] * f0;
    const double l2 = F[6] * ua + F[7] * va + F[8] * f0;
    m0 = F[0] * ub + F[3] * vb + F[6] * f0;
    m1 = F[1] * ub + F[4] * vb + F[7] * f0;
    e = ub * l0 + vb * l1 + f0 * l2;
    den = l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1;
}

// One match into the sums.  r = e / sqrt(den); along variable k, with dl = dF_k p_a, dm = dF_k^T p_b and de = p_b . dl:
// dr = (de - r (l0 dl0 + l1 dl1 + m0 dm0 + m1 dm1) / sqrt(den)) / sqrt(den), the quotient rule with the denominator's derivative.
SRK_PR_HD void srk_pair_obs(SrkPairSums& s, const SrkPairLin& lin, double ua, double va, double ub, double vb, double f0, double q, int kind,
                            double delta)
{
    double l0, l1, m0, m1, e, den;
    srk_pair_sampson_terms(lin.F, ua, va, ub, vb, f0, l0, l1, m0, m1, e, den);
    const double isd = 1.0 / sqrt(den), r = e * isd;
    double J[SRK_PAIR_NV];
    SRK_PR_UNROLL
    for (int k = 0; k < SRK_PAIR_NV; ++k) {
        const double* D = lin.dF[k];
        const double dl0 = D[0] * ua + D[1] * va + D[2] * f0, dl1 = D[3] * ua + D[4] * va + D[5] * f0, dl2 = D[6] * ua + D[7] * va + D[8] * f0;
        const double dm0 = D[0] * ub + D[3] * vb + D[6] * f0, dm1 = D[1] * ub + D[4] * vb + D[7] * f0;
        const double de = ub * dl0 + vb * dl1 + f0 * dl2;
        J[k] = (de - r * ((l0 * dl0 + l1 * dl1 + m0 * dm0 + m1 * dm1) * isd)) * isd;
    }
    double rho, w;
    srk_resect_rho(q * (e * e / den), kind, delta, rho, w);
    const double qw = q * w;
    s.E += rho;
    s.wsum += w;
    int n = 0;
    SRK_PR_UNROLL
    for (int a = 0; a < SRK_PAIR_NV; ++a) {
        SRK_PR_UNROLL
        for (int b = a; b < SRK_PAIR_NV; ++b) s.h[n++] += qw * (J[a] * J[b]);
        s.g[a] += qw * (J[a] * r);
    }
}

// the robust weight rho'(q s) of one match under F
SRK_PR_HD double srk_pair_weight(const double* F, double ua, double va, double ub, double vb, double f0, double q, int kind, double delta)
{
    double l0, l1, m0, m1, e, den, rho, w;
    srk_pair_sampson_terms(F, ua, va, ub, vb, f0, l0, l1, m0, m1, e, den);
    srk_resect_rho(q * (e * e / den), kind, delta, rho, w);
    return w;
}

// whether the point of the two rays of a match lies at a positive distance along both under (R, T): the depth rule of relate's
// vote (srk_relate_front with sign +1, without the parallax)
SRK_PR_HD int srk_pair_front(const double* kinv, const SrkPairPose& p, double ua, double va, double ub, double vb, double f0)
{
    double a[3], b[3], c[3], tb[3], ta[3];
    srk_relate_ray(kinv, ua, va, f0, a);
    srk_relate_ray(kinv + 9, ub, vb, f0, b);
    const double ar[3] = { p.R[0] * a[0] + p.R[1] * a[1] + p.R[2] * a[2], p.R[3] * a[0] + p.R[4] * a[1] + p.R[5] * a[2],
                           p.R[6] * a[0] + p.R[7] * a[1] + p.R[8] * a[2] };
    srk_relate_cross(ar, b, c);
    srk_relate_cross(p.T, b, tb);
    srk_relate_cross(p.T, ar, ta);
    return srk_relate_dot(tb, c) < 0.0 && srk_relate_dot(ta, c) < 0.0;
}

// the upper triangle h into a full symmetric 5 x 5
SRK_PR_HD void srk_pair_full(const double* h, double A[SRK_PAIR_NV][SRK_PAIR_NV])
{
    int e = 0;
    SRK_PR_UNROLL
    for (int a = 0; a < SRK_PAIR_NV; ++a) {
        SRK_PR_UNROLL
        for (int b = a; b < SRK_PAIR_NV; ++b) {
            A[a][b] = h[e];
            A[b][a] = h[e++];
        }
    }
}

// A = L L^T in place (the lower triangle becomes L), written out; 0 when a pivot is not positive (NaN included)
SRK_PR_HD int srk_pair_chol5(double A[SRK_PAIR_NV][SRK_PAIR_NV])
{
    int ok = 1;
    SRK_PR_UNROLL
    for (int j = 0; j < SRK_PAIR_NV; ++j) {
        double piv = A[j][j];
        SRK_PR_UNROLL
        for (int k = 0; k < j; ++k) piv -= A[j][k] * A[j][k];
        if (!(piv > 0.0)) ok = 0;
        const double l = sqrt(piv);
        A[j][j] = l;
        SRK_PR_UNROLL
        for (int i = j + 1; i < SRK_PAIR_NV; ++i) {
            double v = A[i][j];
            SRK_PR_UNROLL
            for (int k = 0; k < j; ++k) v -= A[i][k] * A[j][k];
            A[i][j] = v / l;
        }
    }
    return ok;
}

// (H + c diag H) d = -g by the written-out Cholesky factorisation; 0 when a pivot is not positive or d is not finite
SRK_PR_HD int srk_pair_lm_step(const SrkPairSums& s, double c, double d[SRK_PAIR_NV])
{
    double A[SRK_PAIR_NV][SRK_PAIR_NV], y[SRK_PAIR_NV];
    srk_pair_full(s.h, A);
    SRK_PR_UNROLL
    for (int a = 0; a < SRK_PAIR_NV; ++a) A[a][a] = A[a][a] + c * A[a][a];
    int ok = srk_pair_chol5(A);
    SRK_PR_UNROLL
    for (int i = 0; i < SRK_PAIR_NV; ++i) {
        double v = -s.g[i];
        SRK_PR_UNROLL
        for (int k = 0; k < i; ++k) v -= A[i][k] * y[k];
        y[i] = v / A[i][i];
    }
    SRK_PR_UNROLL
    for (int i = SRK_PAIR_NV - 1; i >= 0; --i) {
        double v = y[i];
        SRK_PR_UNROLL
        for (int k = i + 1; k < SRK_PAIR_NV; ++k) v -= A[k][i] * d[k];
        d[i] = v / A[i][i];
    }
    SRK_PR_UNROLL
    for (int i = 0; i < SRK_PAIR_NV; ++i)
        if (!isfinite(d[i])) ok = 0;
    return ok;
}

// the pose moved by d = [w; beta]: R Exp(w)^T -- a product of rotations, no entry is added to -- and T + b1 beta_1 + b2 beta_2
// brought back to the unit sphere, with the basis of the pose that is left
SRK_PR_HD void srk_pair_move(const SrkPairPose& s, const double d[SRK_PAIR_NV], SrkPairPose& n)
{
    double X[9], b1[3], b2[3], t[3];
    srk_resect_exp(d, X);
    SRK_PR_UNROLL
    for (int a = 0; a < 3; ++a) {
        SRK_PR_UNROLL
        for (int b = 0; b < 3; ++b) n.R[3 * a + b] = s.R[3 * a] * X[3 * b] + s.R[3 * a + 1] * X[3 * b + 1] + s.R[3 * a + 2] * X[3 * b + 2];
    }
    srk_pair_basis(s.T, b1, b2);
    SRK_PR_UNROLL
    for (int a = 0; a < 3; ++a) t[a] = s.T[a] + b1[a] * d[3] + b2[a] * d[4];
    const double in = 1.0 / sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    SRK_PR_UNROLL
    for (int a = 0; a < 3; ++a) n.T[a] = t[a] * in;
}

// cond_1 of the Jacobi-scaled H_s = D^-1/2 H D^-1/2 (A: the full symmetric H, destroyed): |H_s|_1 |H_s^-1|_1 with the inverse
// written out from the Cholesky factor.  NaN when H_s is not positive definite.
SRK_PR_HD double srk_pair_cond1(double A[SRK_PAIR_NV][SRK_PAIR_NV])
{
    double is[SRK_PAIR_NV];
    SRK_PR_UNROLL
    for (int a = 0; a < SRK_PAIR_NV; ++a) is[a] = 1.0 / sqrt(A[a][a]);
    SRK_PR_UNROLL
    for (int a = 0; a < SRK_PAIR_NV; ++a) {
        SRK_PR_UNROLL
        for (int b = 0; b < SRK_PAIR_NV; ++b) A[a][b] = A[a][b] * (is[a] * is[b]);
    }
    double n1 = 0.0;
    SRK_PR_UNROLL
    for (int b = 0; b < SRK_PAIR_NV; ++b) {
        double col = 0.0;
        SRK_PR_UNROLL
        for (int a = 0; a < SRK_PAIR_NV; ++a) col += fabs(A[a][b]);
        n1 = fmax(n1, col);
    }
    const int pd = srk_pair_chol5(A);
    // the inverse of the factor, M = L^-1 (lower), then H_s^-1 = M^T M
    double M[SRK_PAIR_NV][SRK_PAIR_NV];
    SRK_PR_UNROLL
    for (int j = 0; j < SRK_PAIR_NV; ++j) {
        M[j][j] = 1.0 / A[j][j];
        SRK_PR_UNROLL
        for (int i = j + 1; i < SRK_PAIR_NV; ++i) {
            double v = 0.0;
            SRK_PR_UNROLL
            for (int k = j; k < i; ++k) v -= A[i][k] * M[k][j];
            M[i][j] = v / A[i][i];
        }
    }
    double n2 = 0.0;
    SRK_PR_UNROLL
    for (int b = 0; b < SRK_PAIR_NV; ++b) {
        double col = 0.0;
        SRK_PR_UNROLL
        for (int a = 0; a < SRK_PAIR_NV; ++a) {
            double v = 0.0;
            SRK_PR_UNROLL
            for (int k = (a > b ? a : b); k < SRK_PAIR_NV; ++k) v += M[k][a] * M[k][b];
            col += fabs(v);
        }
        n2 = fmax(n2, col);
    }
    return pd ? n1 * n2 : NAN;
}

// quality[6], info[25], basis[6], E[9] and the status bits of a finished pair with n >= 5 weighted matches (SRK_PAIR_* of srk_ba.h;
// the bit values are repeated in srk_pair.cpp's static_assert); `front` the matches in front of both cameras at the result
SRK_PR_HD uint32_t srk_pair_finish(const SrkPairSums& cur, const SrkPairPose& p, int64_t n, int64_t front, double f0, int hit_cap, int attempts_used,
                                   double E[9], double quality[6], double info[25], double basis[6])
{
    double A[SRK_PAIR_NV][SRK_PAIR_NV];
    srk_pair_full(cur.h, A);
    const double if2 = 1.0 / (f0 * f0);
    int finite = isfinite(cur.E) ? 1 : 0;
    SRK_PR_UNROLL
    for (int a = 0; a < SRK_PAIR_NV; ++a) {
        SRK_PR_UNROLL
        for (int b = 0; b < SRK_PAIR_NV; ++b) {
            info[SRK_PAIR_NV * a + b] = A[a][b] * if2;
            if (!isfinite(A[a][b])) finite = 0;
        }
    }
    const double cond = srk_pair_cond1(A);
    srk_relate_essential(p.R, p.T, E);
    srk_pair_basis(p.T, basis, basis + 3);
    quality[0] = sqrt(cur.E / (double)n);
    quality[1] = (double)n;
    quality[2] = cur.wsum / (double)n;
    quality[3] = cond;
    quality[4] = (double)front;
    quality[5] = (double)attempts_used;
    uint32_t st = 0;
    if (!finite || !isfinite(cond)) st |= 2u;
    if (hit_cap) st |= 8u;
    return st;
}

// a pair with fewer than five weighted matches: nothing is refined
SRK_PR_HD uint32_t srk_pair_few(const SrkPairPose& p, int64_t n, double E[9], double quality[6], double info[25], double basis[6])
{
    srk_relate_essential(p.R, p.T, E);
    srk_pair_basis(p.T, basis, basis + 3);
    quality[0] = NAN;
    quality[1] = (double)n;
    quality[2] = NAN;
    quality[3] = NAN;
    quality[4] = NAN;
    quality[5] = 0.0;
    SRK_PR_UNROLL
    for (int e = 0; e < 25; ++e) info[e] = 0.0;
    return 1u;
}
