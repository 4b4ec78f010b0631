// srk_fund_math.hpp -- the arithmetic of the two-view fundamental matrix (srk_relate_uncalibrated) as plain
// functions of doubles, compiled for the device by srk_fund.hip and for the host by srk_fund.cpp: the kernels and the host walk of
// one pair (srk_fundamental_host_pair, tests/cpp/test_fund_host.cpp) run the same statements in the same order.  The sampler, the
// seven-point model (null space, the cubic det(F1 + z F2) and its real roots by the derivative chain, the choice by the eighth
// match), the orthonormal representation F = U diag(1, sigma, 0) V^T, and a Levenberg-Marquardt attempt on the Sampson error over
// its seven variables.  No HIP header is needed here.  Every array is indexed by constants only (loops are unrolled, positions
// known at run time are moved by comparisons), so that no per-lane array is indexed at run time.
//
// Reused, not repeated:
//   from srk_relate_math.hpp  srk_relate_sampson and srk_relate_term (the squared Sampson distance in pixels and the score's term);
//   from srk_pair_math.hpp    srk_pair_sampson_terms (the same products in the same order, for the residual and its derivative);
//   from srk_resect_math.hpp  srk_resect_exp (Exp of a rotation vector);
//   from srk_align_math.hpp   srk_align_mulhi, srk_align_dot, srk_align_cross;
//   from srk_homog_math.hpp   srk_homog_jacobi3 (the written-out cyclic Jacobi), srk_homog_det3, srk_homog_adj3, srk_homog_mulv.
#pragma once
#include "srk_homog_math.hpp"
#include "srk_pair_math.hpp"

#define SRK_FD_HD SRK_AL_HD
#define SRK_FD_UNROLL SRK_AL_UNROLL

#define SRK_FUND_LANES 64     // hypotheses that share a wave of the score
#define SRK_FUND_STRIP 8      // doubles of a gathered match: uv_a (2), uv_b (2), q, three of padding (64 bytes)
#define SRK_FUND_HYP 12       // doubles of a hypothesis: F (0-8), the squared eighth-match error, the real roots, valid (96 bytes)
#define SRK_FUND_SLOT 4       // doubles of a wave's best: score, h, inliers, models in the wave
#define SRK_FUND_NV 7         // variables of an attempt: a (3), b (3), delta
#define SRK_FUND_NH 28        // the upper triangle of the 7 x 7 H, row by row
#define SRK_FUND_ACC 35       // the sums of a linearisation: H (28), then g (7)
#define SRK_FUND_BISECT 80    // halvings of a bracket
#define SRK_FUND_NEWTON 4     // Newton steps that polish a root
#define SRK_FUND_PIVOT 1e-12  // a last pivot at most this share of the first: the seven rows are dependent
#define SRK_FUND_LEAD 1e-14   // a leading coefficient at most this share of the others: the cubic is a quadratic
#define SRK_FUND_C0 1e-4      // the first damping factor
#define SRK_FUND_STOP 1e-9    // an attempt whose candidate score is within this share of the current one is the last
#define SRK_FUND_MIN_INLIERS 8

// the orthonormal representation: U, V proper rotations (row by row), 0 <= sigma <= 1; F = U diag(1, sigma, 0) V^T / sqrt(1 + sigma^2)
struct SrkFundRep {
    double U[9], V[9], sigma;
};

// ---- the sampler: counter-based, no state, a stream of its own.  mix = the splitmix64 finaliser of seed + odd * (8 h + k + 1)
SRK_FD_HD uint64_t srk_fund_mix(uint64_t seed, uint32_t h, int k)
{
    uint64_t z = seed + 0x8EBC6AF09C88C6E3ull * (8ull * (uint64_t)h + (uint64_t)k + 1ull);
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// eight distinct ranks below n (n >= 8): draw k is uniform among the n - k ranks not yet picked
SRK_FD_HD void srk_fund_sample(uint64_t seed, uint32_t h, int64_t n, int64_t* r)
{
    int64_t s[8]; // the earlier picks in ascending order
    SRK_FD_UNROLL
    for (int k = 0; k < 8; ++k) {
        int64_t v = (int64_t)srk_align_mulhi(srk_fund_mix(seed, h, k), (uint64_t)(n - k));
        SRK_FD_UNROLL
        for (int j = 0; j < k; ++j)
            if (v >= s[j]) ++v;
        r[k] = v;
        s[k] = v;
        SRK_FD_UNROLL
        for (int j = k; j > 0; --j)
            if (s[j] < s[j - 1]) {
                const int64_t t = s[j];
                s[j] = s[j - 1];
                s[j - 1] = t;
            }
    }
}

// ---- the null space of the 7 x 9 matrix of rows p_b (x) p_a by Gauss-Jordan elimination with complete pivoting, as
// srk_relate_nullspace: rows and columns are exchanged in place by comparisons against every position, the two null vectors are
// then made orthonormal (Gram-Schmidt, twice).  pa, pb [7][3] with a third entry of 1.  N [2][9].  Returns whether the seven rows
// are independent: every pivot above SRK_FUND_PIVOT of the first.
SRK_FD_HD int srk_fund_nullspace(const double* pa, const double* pb, double* N)
{
    double A[7][9];
    int perm[9];
    SRK_FD_UNROLL
    for (int m = 0; m < 7; ++m) {
        SRK_FD_UNROLL
        for (int i = 0; i < 3; ++i) {
            SRK_FD_UNROLL
            for (int j = 0; j < 3; ++j) A[m][3 * i + j] = pb[3 * m + i] * pa[3 * m + j];
        }
    }
    SRK_FD_UNROLL
    for (int c = 0; c < 9; ++c) perm[c] = c;
    double first = 0.0;
    bool deficient = false;
    SRK_FD_UNROLL
    for (int k = 0; k < 7; ++k) {
        double best = -1.0;
        int pi = k, pj = k;
        SRK_FD_UNROLL
        for (int i = k; i < 7; ++i) {
            SRK_FD_UNROLL
            for (int j = k; j < 9; ++j) {
                const double a = fabs(A[i][j]);
                if (a > best) {
                    best = a;
                    pi = i;
                    pj = j;
                }
            }
        }
        first = k == 0 ? best : first;
        deficient = deficient || !(best > SRK_FUND_PIVOT * first);
        SRK_FD_UNROLL
        for (int i = k + 1; i < 7; ++i) {
            const bool sw = i == pi;
            SRK_FD_UNROLL
            for (int j = 0; j < 9; ++j) {
                const double a = A[k][j], b = A[i][j];
                A[k][j] = sw ? b : a;
                A[i][j] = sw ? a : b;
            }
        }
        SRK_FD_UNROLL
        for (int j = k + 1; j < 9; ++j) {
            const bool sw = j == pj;
            SRK_FD_UNROLL
            for (int i = 0; i < 7; ++i) {
                const double a = A[i][k], b = A[i][j];
                A[i][k] = sw ? b : a;
                A[i][j] = sw ? a : b;
            }
            const int a = perm[k], b = perm[j];
            perm[k] = sw ? b : a;
            perm[j] = sw ? a : b;
        }
        const double inv = 1.0 / A[k][k];
        SRK_FD_UNROLL
        for (int j = 0; j < 9; ++j) A[k][j] *= inv;
        SRK_FD_UNROLL
        for (int i = 0; i < 7; ++i) {
            if (i == k) continue;
            const double f = A[i][k];
            SRK_FD_UNROLL
            for (int j = 0; j < 9; ++j) A[i][j] -= f * A[k][j];
        }
    }
    // null vector f in the exchanged columns: -A[.][7 + f] on the pivots, 1 at 7 + f
    SRK_FD_UNROLL
    for (int f = 0; f < 2; ++f) {
        SRK_FD_UNROLL
        for (int e = 0; e < 9; ++e) {
            double v = 0.0;
            SRK_FD_UNROLL
            for (int c = 0; c < 7; ++c) v = perm[c] == e ? -A[c][7 + f] : v;
            v = perm[7 + f] == e ? 1.0 : v;
            N[9 * f + e] = v;
        }
    }
    SRK_FD_UNROLL
    for (int f = 0; f < 2; ++f) {
        SRK_FD_UNROLL
        for (int pass = 0; pass < 2; ++pass) {
            SRK_FD_UNROLL
            for (int g = 0; g < f; ++g) {
                double d = 0.0;
                SRK_FD_UNROLL
                for (int e = 0; e < 9; ++e) d += N[9 * f + e] * N[9 * g + e];
                SRK_FD_UNROLL
                for (int e = 0; e < 9; ++e) N[9 * f + e] -= d * N[9 * g + e];
            }
        }
        double s = 0.0;
        SRK_FD_UNROLL
        for (int e = 0; e < 9; ++e) s += N[9 * f + e] * N[9 * f + e];
        const double in = 1.0 / sqrt(s);
        SRK_FD_UNROLL
        for (int e = 0; e < 9; ++e) N[9 * f + e] *= in;
    }
    return !deficient;
}

// ---- the cubic det(F1 + z F2) = c0 + c1 z + c2 z^2 + c3 z^3: c0 = det F1, c3 = det F2, c1 = sum F2_ij cof(F1)_ij and
// c2 = sum F1_ij cof(F2)_ij (sums of 2 x 2 minors)
SRK_FD_HD void srk_fund_cubic(const double* F1, const double* F2, double* c)
{
    double a1[9], a2[9]; // the adjugates: adj_ji = cof_ij
    srk_homog_adj3(F1, a1);
    srk_homog_adj3(F2, a2);
    c[0] = srk_homog_det3(F1);
    c[3] = srk_homog_det3(F2);
    double s1 = 0.0, s2 = 0.0;
    SRK_FD_UNROLL
    for (int i = 0; i < 3; ++i) {
        SRK_FD_UNROLL
        for (int j = 0; j < 3; ++j) {
            s1 += F2[3 * i + j] * a1[3 * j + i];
            s2 += F1[3 * i + j] * a2[3 * j + i];
        }
    }
    c[1] = s1;
    c[2] = s2;
}

// the cubic (D = 3), its derivative (D = 2) and its second derivative (D = 1) at z
template <int D> SRK_FD_HD double srk_fund_eval(const double* c, double z);
template <> SRK_FD_HD double srk_fund_eval<3>(const double* c, double z) { return ((c[3] * z + c[2]) * z + c[1]) * z + c[0]; }
template <> SRK_FD_HD double srk_fund_eval<2>(const double* c, double z) { return (3.0 * c[3] * z + 2.0 * c[2]) * z + c[1]; }
template <> SRK_FD_HD double srk_fund_eval<1>(const double* c, double z) { return 6.0 * c[3] * z + 2.0 * c[2]; }

// the root of level D in [lo, hi], if the signs at the ends differ: halving, then Newton steps that stay inside (as
// srk_relate_interval)
template <int D> SRK_FD_HD int srk_fund_interval(const double* c, double lo, double hi, double& root)
{
    const double lo0 = lo, hi0 = hi;
    const double fl = srk_fund_eval<D>(c, lo), fh = srk_fund_eval<D>(c, hi);
    const int found = isfinite(fl) && isfinite(fh) && ((fl < 0.0) != (fh < 0.0));
    for (int it = 0; it < SRK_FUND_BISECT; ++it) {
        const double mid = 0.5 * (lo + hi), fm = srk_fund_eval<D>(c, mid);
        const bool left = (fm < 0.0) == (fl < 0.0);
        lo = left ? mid : lo;
        hi = left ? hi : mid;
    }
    double z = 0.5 * (lo + hi);
    SRK_FD_UNROLL
    for (int it = 0; it < SRK_FUND_NEWTON; ++it) {
        const double f = srk_fund_eval<D>(c, z), df = srk_fund_eval<D - 1>(c, z);
        const double n = z - f / df;
        z = (n >= lo0 && n <= hi0) ? n : z;
    }
    root = z;
    return found;
}

// the real roots of c0 + c1 z + c2 z^2 in ascending order (a cubic whose leading coefficient vanishes); a vanishing c2 leaves the
// line's root
SRK_FD_HD int srk_fund_quadratic(const double* c, double* z)
{
    const double scale = fmax(fabs(c[0]), fabs(c[1]));
    if (!(fabs(c[2]) > SRK_FUND_LEAD * scale)) {
        const double r = -c[0] / c[1];
        z[0] = r;
        return isfinite(r) ? 1 : 0;
    }
    const double disc = c[1] * c[1] - 4.0 * c[2] * c[0];
    if (!(disc >= 0.0)) return 0;
    const double t = -0.5 * (c[1] + copysign(sqrt(disc), c[1]));
    const double ra = t / c[2], rb = t != 0.0 ? c[0] / t : ra;
    z[0] = fmin(ra, rb);
    z[1] = fmax(ra, rb);
    return disc > 0.0 ? 2 : 1;
}

// the real roots of the cubic in ascending order, z [3]; returns their number.  The derivative chain inside the Cauchy bound: the
// root of c'' splits [-B, B] for the roots of c', which split it for those of c.  An interval without a sign change holds none.
SRK_FD_HD int srk_fund_roots(const double* c, double* z)
{
    z[0] = z[1] = z[2] = 0.0;
    const double scale = fmax(fmax(fabs(c[0]), fabs(c[1])), fabs(c[2]));
    if (!(fabs(c[3]) > SRK_FUND_LEAD * scale)) return srk_fund_quadratic(c, z);
    const double B = 1.0 + fmax(fmax(fabs(c[0] / c[3]), fabs(c[1] / c[3])), fabs(c[2] / c[3]));
    const double z2 = -c[2] / (3.0 * c[3]);
    double e0, e1, r0, r1, r2;
    const int g0 = srk_fund_interval<2>(c, -B, z2, e0);
    const int g1 = srk_fund_interval<2>(c, z2, B, e1);
    const double a = g0 ? e0 : z2, b = g1 ? e1 : z2;
    const int f0 = srk_fund_interval<3>(c, -B, a, r0);
    const int f1 = srk_fund_interval<3>(c, a, b, r1);
    const int f2 = srk_fund_interval<3>(c, b, B, r2);
    z[0] = f0 ? r0 : (f1 ? r1 : r2);
    z[1] = f0 ? (f1 ? r1 : r2) : r2;
    z[2] = r2;
    return f0 + f1 + f2;
}

// ---- the seven-point model.  pa, pb [7][3]: the sample's pixels over f0, (u / f0, v / f0, 1); e8 = the eighth match's record
// {ua, va, ub, vb}.  F receives the root's matrix at Frobenius norm 1 that has the smallest Sampson error at the eighth match (an
// equal error: the smaller root); err8 that squared error, roots the number of real roots.  Returns whether the sample has a model;
// without one F is zero.
SRK_FD_HD int srk_fund_hypothesis(const double* pa, const double* pb, const double* e8, double f0, double* F, double& err8, int& roots)
{
    double N[18], F1[9], F2[9], c[4], z[3];
    const int independent = srk_fund_nullspace(pa, pb, N);
    srk_fund_cubic(N, N + 9, c);
    const bool sw = fabs(c[0]) > fabs(c[3]); // the leading coefficient is the larger determinant
    SRK_FD_UNROLL
    for (int e = 0; e < 9; ++e) {
        F1[e] = sw ? N[9 + e] : N[e];
        F2[e] = sw ? N[e] : N[9 + e];
    }
    const double k0 = c[0], k1 = c[1], k2 = c[2], k3 = c[3];
    c[0] = sw ? k3 : k0;
    c[1] = sw ? k2 : k1;
    c[2] = sw ? k1 : k2;
    c[3] = sw ? k0 : k3;
    roots = srk_fund_roots(c, z);
    double best = INFINITY;
    SRK_FD_UNROLL
    for (int e = 0; e < 9; ++e) F[e] = 0.0;
    SRK_FD_UNROLL
    for (int k = 0; k < 3; ++k) {
        double G[9], ss = 0.0;
        SRK_FD_UNROLL
        for (int e = 0; e < 9; ++e) {
            G[e] = F1[e] + z[k] * F2[e];
            ss += G[e] * G[e];
        }
        const double in = 1.0 / sqrt(ss);
        SRK_FD_UNROLL
        for (int e = 0; e < 9; ++e) G[e] *= in;
        const double s = srk_relate_sampson(G, e8[0], e8[1], e8[2], e8[3], f0);
        const bool take = independent && k < roots && s < best; // a NaN is never taken
        best = take ? s : best;
        SRK_FD_UNROLL
        for (int e = 0; e < 9; ++e) F[e] = take ? G[e] : F[e];
    }
    err8 = best;
    return best < INFINITY;
}

// ---- the orthonormal representation
SRK_FD_HD void srk_fund_identity(SrkFundRep& r)
{
    SRK_FD_UNROLL
    for (int e = 0; e < 9; ++e) r.U[e] = r.V[e] = (e % 4 == 0) ? 1.0 : 0.0;
    r.sigma = 0.0;
}

// a unit vector orthogonal to the unit vector u, fixed by rule: e_k x u with k the index of the smallest |u_k| (a tie: the smaller k)
SRK_FD_HD void srk_fund_orthogonal(const double* u, double* o)
{
    const double a0 = fabs(u[0]), a1 = fabs(u[1]), a2 = fabs(u[2]);
    const int k = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
    const double c0 = k == 0 ? 0.0 : (k == 1 ? u[2] : -u[1]);
    const double c1 = k == 0 ? -u[2] : (k == 1 ? 0.0 : u[0]);
    const double c2 = k == 0 ? u[1] : (k == 1 ? -u[0] : 0.0);
    const double in = 1.0 / sqrt(c0 * c0 + c1 * c1 + c2 * c2);
    o[0] = c0 * in;
    o[1] = c1 * in;
    o[2] = c2 * in;
}

// 0 <= sigma <= 1 with the same F up to scale: a negative sigma turns u_2 and u_3 round; a sigma above 1 exchanges the first two
// columns of U and of V (F / sigma has the singular values 1 / sigma and 1) and turns both third columns round.  U and V stay proper.
SRK_FD_HD void srk_fund_canon(SrkFundRep& r)
{
    if (r.sigma < 0.0) {
        r.sigma = -r.sigma;
        SRK_FD_UNROLL
        for (int i = 0; i < 3; ++i) r.U[3 * i + 1] = -r.U[3 * i + 1], r.U[3 * i + 2] = -r.U[3 * i + 2];
    }
    if (r.sigma > 1.0) {
        r.sigma = 1.0 / r.sigma;
        SRK_FD_UNROLL
        for (int i = 0; i < 3; ++i) {
            const double u0 = r.U[3 * i], v0 = r.V[3 * i];
            r.U[3 * i] = r.U[3 * i + 1];
            r.U[3 * i + 1] = u0;
            r.U[3 * i + 2] = -r.U[3 * i + 2];
            r.V[3 * i] = r.V[3 * i + 1];
            r.V[3 * i + 1] = v0;
            r.V[3 * i + 2] = -r.V[3 * i + 2];
        }
    }
}

// the unit eigenvector of M^T M with the largest eigenvalue, by the cyclic Jacobi of srk_homog_math.hpp; the position of the largest is
// found by comparisons (a tie: the first)
SRK_FD_HD void srk_fund_dominant(const double* M, double* v)
{
    double S[3][3], V[3][3], lam[3];
    SRK_FD_UNROLL
    for (int i = 0; i < 3; ++i) {
        SRK_FD_UNROLL
        for (int j = 0; j < 3; ++j) S[i][j] = M[i] * M[j] + M[3 + i] * M[3 + j] + M[6 + i] * M[6 + j];
    }
    srk_homog_jacobi3(S, V, lam);
    const int k = (lam[0] >= lam[1] && lam[0] >= lam[2]) ? 0 : (lam[1] >= lam[2] ? 1 : 2);
    SRK_FD_UNROLL
    for (int r = 0; r < 3; ++r) v[r] = k == 0 ? V[r][0] : (k == 1 ? V[r][1] : V[r][2]);
}

// F (any scale) into the representation, the smallest singular value dropped.  v_1 = the dominant eigenvector of F^T F, u_1 =
// F v_1 / |F v_1|; v_2 = the dominant eigenvector of B^T B for the deflated B = F - (F v_1) v_1^T, made orthogonal to v_1 (twice):
// the second Jacobi works at B's own scale, so a sigma far below sqrt(eps) keeps its digits, which the eigenvalues of F^T F alone
// would lose; v_3 = v_1 x v_2; u_2 = F v_2 made orthogonal to u_1 (twice) and scaled, u_3 = u_1 x u_2; sigma = |F v_2| / |F v_1|.
// An F of rank 1 (|F v_2| at most 1e-14 of |F v_1|) takes u_2 (and, where B gives no direction, v_2) by the rule of
// srk_fund_orthogonal and sigma = 0.  Returns whether everything is finite.
SRK_FD_HD int srk_fund_represent(const double* F, SrkFundRep& r)
{
    double v1[3], v2[3], v3[3], t1[3], t2[3], u1[3], u2[3], u3[3], alt[3], B[9];
    srk_fund_dominant(F, v1);
    srk_homog_mulv(F, v1, t1);
    const double n1 = sqrt(srk_align_dot(t1, t1));
    SRK_FD_UNROLL
    for (int k = 0; k < 3; ++k) u1[k] = t1[k] / n1;
    SRK_FD_UNROLL
    for (int i = 0; i < 3; ++i) {
        SRK_FD_UNROLL
        for (int j = 0; j < 3; ++j) B[3 * i + j] = F[3 * i + j] - t1[i] * v1[j];
    }
    srk_fund_dominant(B, v2);
    SRK_FD_UNROLL
    for (int pass = 0; pass < 2; ++pass) {
        const double d = srk_align_dot(v1, v2);
        SRK_FD_UNROLL
        for (int k = 0; k < 3; ++k) v2[k] -= d * v1[k];
    }
    const double nv = sqrt(srk_align_dot(v2, v2));
    const bool lost = !(nv > 1e-3); // B = 0: Jacobi's answer is a unit vector of the identity, possibly v_1 itself
    srk_fund_orthogonal(v1, alt);
    SRK_FD_UNROLL
    for (int k = 0; k < 3; ++k) v2[k] = lost ? alt[k] : v2[k] / nv;
    srk_align_cross(v1, v2, v3); // a proper frame whatever the signs Jacobi left
    srk_homog_mulv(F, v2, t2);
    SRK_FD_UNROLL
    for (int pass = 0; pass < 2; ++pass) {
        const double d = srk_align_dot(u1, t2);
        SRK_FD_UNROLL
        for (int k = 0; k < 3; ++k) t2[k] -= d * u1[k];
    }
    const double n2 = sqrt(srk_align_dot(t2, t2));
    const bool rank1 = !(n2 > 1e-14 * n1);
    srk_fund_orthogonal(u1, alt);
    SRK_FD_UNROLL
    for (int k = 0; k < 3; ++k) u2[k] = rank1 ? alt[k] : t2[k] / n2;
    srk_align_cross(u1, u2, u3);
    int ok = 1;
    SRK_FD_UNROLL
    for (int i = 0; i < 3; ++i) {
        r.U[3 * i] = u1[i], r.U[3 * i + 1] = u2[i], r.U[3 * i + 2] = u3[i];
        r.V[3 * i] = v1[i], r.V[3 * i + 1] = v2[i], r.V[3 * i + 2] = v3[i];
    }
    r.sigma = rank1 ? 0.0 : n2 / n1;
    SRK_FD_UNROLL
    for (int e = 0; e < 9; ++e) ok = ok && isfinite(r.U[e]) && isfinite(r.V[e]);
    ok = ok && isfinite(r.sigma);
    srk_fund_canon(r);
    return ok;
}

// D += s (column cu of U) (column cv of V)^T
SRK_FD_HD void srk_fund_outer(const double* U, int cu, const double* V, int cv, double s, double* D)
{
    SRK_FD_UNROLL
    for (int i = 0; i < 3; ++i) {
        SRK_FD_UNROLL
        for (int j = 0; j < 3; ++j) D[3 * i + j] += s * (U[3 * i + cu] * V[3 * j + cv]);
    }
}

// F = U diag(1, sigma, 0) V^T at Frobenius norm 1
SRK_FD_HD void srk_fund_build(const SrkFundRep& r, double* F)
{
    const double in = 1.0 / sqrt(1.0 + r.sigma * r.sigma);
    SRK_FD_UNROLL
    for (int e = 0; e < 9; ++e) F[e] = 0.0;
    srk_fund_outer(r.U, 0, r.V, 0, in, F);
    srk_fund_outer(r.U, 1, r.V, 1, r.sigma * in, F);
}

// the sign of the returned F: its entry of largest magnitude is positive (a tie: the first row by row).  -F turns u_1 and u_2 round.
SRK_FD_HD void srk_fund_sign(SrkFundRep& r, double* F)
{
    double big = -1.0, val = 0.0;
    SRK_FD_UNROLL
    for (int e = 0; e < 9; ++e) {
        const bool more = fabs(F[e]) > big;
        big = more ? fabs(F[e]) : big;
        val = more ? F[e] : val;
    }
    if (val < 0.0) {
        SRK_FD_UNROLL
        for (int e = 0; e < 9; ++e) F[e] = -F[e];
        SRK_FD_UNROLL
        for (int i = 0; i < 3; ++i) r.U[3 * i] = -r.U[3 * i], r.U[3 * i + 1] = -r.U[3 * i + 1];
    }
}

// What is uniform over a pair at one model: F (norm 1) and the seven dF_k.  With G = U S V^T, S = diag(1, sigma, 0) and F = G / nu,
// the Sampson distance does not depend on nu, so dF_k = (dG / dd_k) / nu is exact for the residual:
//   dG/da_i = U [e_i]x S V^T:  sigma u_3 v_2^T,  -u_3 v_1^T,  u_2 v_1^T - sigma u_1 v_2^T
//   dG/db_i = -U S [e_i]x V^T: sigma u_2 v_3^T,  -u_1 v_3^T,  u_1 v_2^T - sigma u_2 v_1^T
//   dG/ddelta = u_2 v_2^T
struct SrkFundLin {
    double F[9], dF[SRK_FUND_NV][9];
};
SRK_FD_HD void srk_fund_linearise(const SrkFundRep& r, SrkFundLin& lin)
{
    const double in = 1.0 / sqrt(1.0 + r.sigma * r.sigma), sg = r.sigma * in;
    srk_fund_build(r, lin.F);
    SRK_FD_UNROLL
    for (int k = 0; k < SRK_FUND_NV; ++k) {
        SRK_FD_UNROLL
        for (int e = 0; e < 9; ++e) lin.dF[k][e] = 0.0;
    }
    srk_fund_outer(r.U, 2, r.V, 1, sg, lin.dF[0]);
    srk_fund_outer(r.U, 2, r.V, 0, -in, lin.dF[1]);
    srk_fund_outer(r.U, 1, r.V, 0, in, lin.dF[2]);
    srk_fund_outer(r.U, 0, r.V, 1, -sg, lin.dF[2]);
    srk_fund_outer(r.U, 1, r.V, 2, sg, lin.dF[3]);
    srk_fund_outer(r.U, 0, r.V, 2, -in, lin.dF[4]);
    srk_fund_outer(r.U, 0, r.V, 1, in, lin.dF[5]);
    srk_fund_outer(r.U, 1, r.V, 0, -sg, lin.dF[5]);
    srk_fund_outer(r.U, 1, r.V, 1, in, lin.dF[6]);
}

// the residual r = e / sqrt(den) of one match in pixels and its row of the Jacobian, by the quotient rule with the denominator's
// derivative (as srk_pair_obs)
SRK_FD_HD double srk_fund_row(const SrkFundLin& lin, double ua, double va, double ub, double vb, double f0, double* J)
{
    double l0, l1, m0, m1, e, den;
    srk_pair_sampson_terms(lin.F, ua, va, ub, vb, f0, l0, l1, m0, m1, e, den);
    const double isd = 1.0 / sqrt(den), r = e * isd;
    SRK_FD_UNROLL
    for (int k = 0; k < SRK_FUND_NV; ++k) {
        const double* D = lin.dF[k];
        const double dl0 = D[0] * ua + D[1] * va + D[2] * f0, dl1 = D[3] * ua + D[4] * va + D[5] * f0, dl2 = D[6] * ua + D[7] * va + D[8] * f0;
        const double dm0 = D[0] * ub + D[3] * vb + D[6] * f0, dm1 = D[1] * ub + D[4] * vb + D[7] * f0;
        const double de = ub * dl0 + vb * dl1 + f0 * dl2;
        J[k] = (de - r * ((l0 * dl0 + l1 * dl1 + m0 * dm0 + m1 * dm1) * isd)) * isd;
    }
    return r;
}

// an inlier's share of the sums: acc [35] += q (J^T J upper triangle row by row, then J^T r)
SRK_FD_HD void srk_fund_accumulate(double* acc, const SrkFundLin& lin, const double* rec, double f0)
{
    double J[SRK_FUND_NV];
    const double r = srk_fund_row(lin, rec[0], rec[1], rec[2], rec[3], f0, J);
    const double q = rec[4];
    int at = 0;
    SRK_FD_UNROLL
    for (int a = 0; a < SRK_FUND_NV; ++a) {
        const double qa = q * J[a];
        SRK_FD_UNROLL
        for (int b = a; b < SRK_FUND_NV; ++b) acc[at++] += qa * J[b];
        acc[SRK_FUND_NH + a] += qa * r;
    }
}

// the upper triangle h into a full symmetric 7 x 7
SRK_FD_HD void srk_fund_full(const double* h, double A[SRK_FUND_NV][SRK_FUND_NV])
{
    int e = 0;
    SRK_FD_UNROLL
    for (int a = 0; a < SRK_FUND_NV; ++a) {
        SRK_FD_UNROLL
        for (int b = a; b < SRK_FUND_NV; ++b) {
            A[a][b] = h[e];
            A[b][a] = h[e++];
        }
    }
}

// A = L L^T in place (the lower triangle becomes L), written out; 0 when a pivot is not positive (NaN included)
SRK_FD_HD int srk_fund_chol7(double A[SRK_FUND_NV][SRK_FUND_NV])
{
    int ok = 1;
    SRK_FD_UNROLL
    for (int j = 0; j < SRK_FUND_NV; ++j) {
        double piv = A[j][j];
        SRK_FD_UNROLL
        for (int k = 0; k < j; ++k) piv -= A[j][k] * A[j][k];
        if (!(piv > 0.0)) ok = 0;
        const double l = sqrt(piv);
        A[j][j] = l;
        SRK_FD_UNROLL
        for (int i = j + 1; i < SRK_FUND_NV; ++i) {
            double v = A[i][j];
            SRK_FD_UNROLL
            for (int k = 0; k < j; ++k) v -= A[i][k] * A[j][k];
            A[i][j] = v / l;
        }
    }
    return ok;
}

// (H + c diag H) d = -g by the written-out Cholesky factorisation; 0 when a pivot is not positive or d is not finite
SRK_FD_HD int srk_fund_lm_step(const double* acc, double c, double d[SRK_FUND_NV])
{
    double A[SRK_FUND_NV][SRK_FUND_NV], y[SRK_FUND_NV];
    srk_fund_full(acc, A);
    SRK_FD_UNROLL
    for (int a = 0; a < SRK_FUND_NV; ++a) A[a][a] = A[a][a] + c * A[a][a];
    int ok = srk_fund_chol7(A);
    SRK_FD_UNROLL
    for (int i = 0; i < SRK_FUND_NV; ++i) {
        double v = -acc[SRK_FUND_NH + i];
        SRK_FD_UNROLL
        for (int k = 0; k < i; ++k) v -= A[i][k] * y[k];
        y[i] = v / A[i][i];
    }
    SRK_FD_UNROLL
    for (int i = SRK_FUND_NV - 1; i >= 0; --i) {
        double v = y[i];
        SRK_FD_UNROLL
        for (int k = i + 1; k < SRK_FUND_NV; ++k) v -= A[k][i] * d[k];
        d[i] = v / A[i][i];
    }
    SRK_FD_UNROLL
    for (int i = 0; i < SRK_FUND_NV; ++i)
        if (!isfinite(d[i])) ok = 0;
    return ok;
}

// the model moved by d = [a; b; delta]: U Exp(a), V Exp(b), sigma + delta, brought back to 0 <= sigma <= 1
SRK_FD_HD void srk_fund_move(const SrkFundRep& s, const double d[SRK_FUND_NV], SrkFundRep& n)
{
    double Xa[9], Xb[9];
    srk_resect_exp(d, Xa);
    srk_resect_exp(d + 3, Xb);
    srk_homog_mul3(s.U, Xa, n.U);
    srk_homog_mul3(s.V, Xb, n.V);
    n.sigma = s.sigma + d[6];
    srk_fund_canon(n);
}

// cond_1 of the Jacobi-scaled H_s = D^-1/2 H D^-1/2 (A: the full symmetric H, destroyed): |H_s|_1 |H_s^-1|_1 with the inverse
// written out from the Cholesky factor (as srk_pair_cond1).  `none` (a NaN formed at run time) when H_s is not positive definite.
SRK_FD_HD double srk_fund_cond1(double A[SRK_FUND_NV][SRK_FUND_NV], double none)
{
    double is[SRK_FUND_NV];
    SRK_FD_UNROLL
    for (int a = 0; a < SRK_FUND_NV; ++a) is[a] = 1.0 / sqrt(A[a][a]);
    SRK_FD_UNROLL
    for (int a = 0; a < SRK_FUND_NV; ++a) {
        SRK_FD_UNROLL
        for (int b = 0; b < SRK_FUND_NV; ++b) A[a][b] = A[a][b] * (is[a] * is[b]);
    }
    double n1 = 0.0;
    SRK_FD_UNROLL
    for (int b = 0; b < SRK_FUND_NV; ++b) {
        double col = 0.0;
        SRK_FD_UNROLL
        for (int a = 0; a < SRK_FUND_NV; ++a) col += fabs(A[a][b]);
        n1 = fmax(n1, col);
    }
    const int pd = srk_fund_chol7(A);
    double M[SRK_FUND_NV][SRK_FUND_NV]; // the inverse of the factor, M = L^-1 (lower), then H_s^-1 = M^T M
    SRK_FD_UNROLL
    for (int j = 0; j < SRK_FUND_NV; ++j) {
        M[j][j] = 1.0 / A[j][j];
        SRK_FD_UNROLL
        for (int i = j + 1; i < SRK_FUND_NV; ++i) {
            double v = 0.0;
            SRK_FD_UNROLL
            for (int k = j; k < i; ++k) v -= A[i][k] * M[k][j];
            M[i][j] = v / A[i][i];
        }
    }
    double n2 = 0.0;
    SRK_FD_UNROLL
    for (int b = 0; b < SRK_FUND_NV; ++b) {
        double col = 0.0;
        SRK_FD_UNROLL
        for (int a = 0; a < SRK_FUND_NV; ++a) {
            double v = 0.0;
            SRK_FD_UNROLL
            for (int k = (a > b ? a : b); k < SRK_FUND_NV; ++k) v += M[k][a] * M[k][b];
            col += fabs(v);
        }
        n2 = fmax(n2, col);
    }
    const double cond = n1 * n2;
    return pd && isfinite(cond) ? cond : none;
}

// One match's term of the score, relate's: min(q s, tau^2) with s the squared Sampson distance in pixels; inlier = q s < tau^2;
// s2 receives s.  rec = the strip's record {ua, va, ub, vb, q}.
SRK_FD_HD double srk_fund_term(const double* F, const double* rec, double f0, double tau2, int& inlier, double& s2)
{
    s2 = srk_relate_sampson(F, rec[0], rec[1], rec[2], rec[3], f0);
    return srk_relate_term(F, rec[0], rec[1], rec[2], rec[3], rec[4], f0, tau2, inlier);
}
