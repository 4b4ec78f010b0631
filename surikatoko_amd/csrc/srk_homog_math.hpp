// srk_homog_math.hpp -- the arithmetic of the two-view homography (srk_relate_homography) as plain functions
// of doubles, compiled for the device by srk_homog.hip and for the host by srk_homog.cpp: the kernels and the host walk of one
// pair (srk_homography_host_pair, tests/cpp/test_homog_host.cpp) run the same statements in the same order.  The sampler, the
// four-point model through the projective basis, one match's term of the score, the sums and the step of a Gauss-Newton round,
// and the decomposition into the plane's two poses.  No HIP header is needed here.  Every array is indexed by constants only
// (loops are unrolled, the Jacobi pairs are template arguments), so that no per-lane array is indexed at run time.
#pragma once
#include "srk_align_math.hpp" // the nearest rotation (srk_align_closed_form), dot and cross

#define SRK_HG_HD SRK_AL_HD
#define SRK_HG_UNROLL SRK_AL_UNROLL

#define SRK_HOMOG_LANES 64      // hypotheses that share a wave
#define SRK_HOMOG_STRIP 8       // doubles of a gathered match: uv_a (2), uv_b (2), q, three of padding (64 bytes)
#define SRK_HOMOG_SLOT 16       // doubles of a wave's best: score, h, inliers, models in the wave, sum of the inliers' s, G (5-13), two of padding
#define SRK_HOMOG_ACC 44        // the sums of a round: the upper triangle of J^T J row by row (36), then J^T r (8)
#define SRK_HOMOG_SWEEPS 12     // the most sweeps of the cyclic Jacobi iteration
#define SRK_HOMOG_COLLINEAR 1e-9 // a triple of a sample is collinear when its determinant is at most this share of the product of its norms
#define SRK_HOMOG_DET 1e-12     // a model of Frobenius norm 1 is singular when |det G| is at most this
#define SRK_HOMOG_GAP 1e-10     // w1 - w3 of the normalised H^T H at or below this: a rotation, no plane

// a model: G (Frobenius norm 1, row by row) and Gi = sign(det G) adj(G), so that p_a ~ Gi p_b with a positive third entry in front
struct SrkHomogModel {
    double G[9], Gi[9];
};

// ---- the sampler: counter-based, no state, a stream of its own.  mix = the splitmix64 finaliser of seed + odd * (4 h + k + 1)
SRK_HG_HD uint64_t srk_homog_mix(uint64_t seed, uint32_t h, int k)
{
    uint64_t z = seed + 0xE7037ED1A0B428DBull * (4ull * (uint64_t)h + (uint64_t)k + 1ull);
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// four distinct ranks below n (n >= 4): draw k is uniform among the n - k ranks not yet picked
SRK_HG_HD void srk_homog_sample(uint64_t seed, uint32_t h, int64_t n, int64_t& r0, int64_t& r1, int64_t& r2, int64_t& r3)
{
    r0 = (int64_t)srk_align_mulhi(srk_homog_mix(seed, h, 0), (uint64_t)n);
    r1 = (int64_t)srk_align_mulhi(srk_homog_mix(seed, h, 1), (uint64_t)(n - 1));
    if (r1 >= r0) ++r1;
    const int64_t a = r0 < r1 ? r0 : r1, b = r0 < r1 ? r1 : r0; // the earlier picks in ascending order
    r2 = (int64_t)srk_align_mulhi(srk_homog_mix(seed, h, 2), (uint64_t)(n - 2));
    if (r2 >= a) ++r2;
    if (r2 >= b) ++r2;
    const int64_t lo = r2 < a ? r2 : a, hi = r2 > b ? r2 : b, mid = r2 < a ? a : (r2 > b ? b : r2);
    r3 = (int64_t)srk_align_mulhi(srk_homog_mix(seed, h, 3), (uint64_t)(n - 3));
    if (r3 >= lo) ++r3;
    if (r3 >= mid) ++r3;
    if (r3 >= hi) ++r3;
}

// ---- 3 x 3 helpers, matrices row by row
SRK_HG_HD double srk_homog_det3(const double* M)
{
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}
SRK_HG_HD void srk_homog_adj3(const double* M, double* A)
{
    A[0] = M[4] * M[8] - M[5] * M[7];
    A[1] = M[2] * M[7] - M[1] * M[8];
    A[2] = M[1] * M[5] - M[2] * M[4];
    A[3] = M[5] * M[6] - M[3] * M[8];
    A[4] = M[0] * M[8] - M[2] * M[6];
    A[5] = M[2] * M[3] - M[0] * M[5];
    A[6] = M[3] * M[7] - M[4] * M[6];
    A[7] = M[1] * M[6] - M[0] * M[7];
    A[8] = M[0] * M[4] - M[1] * M[3];
}
SRK_HG_HD void srk_homog_mul3(const double* A, const double* B, double* C)
{
    SRK_HG_UNROLL
    for (int i = 0; i < 3; ++i) {
        SRK_HG_UNROLL
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
    }
}
SRK_HG_HD void srk_homog_mulv(const double* A, const double* x, double* y)
{
    SRK_HG_UNROLL
    for (int i = 0; i < 3; ++i) y[i] = A[3 * i] * x[0] + A[3 * i + 1] * x[1] + A[3 * i + 2] * x[2];
}
// the inverse of an upper-left-anything K by the adjugate (the checks have refused a singular K)
SRK_HG_HD void srk_homog_inv3(const double* K, double* Ki)
{
    const double d = 1.0 / srk_homog_det3(K);
    srk_homog_adj3(K, Ki);
    SRK_HG_UNROLL
    for (int e = 0; e < 9; ++e) Ki[e] *= d;
}

SRK_HG_HD void srk_homog_identity(SrkHomogModel& m)
{
    SRK_HG_UNROLL
    for (int e = 0; e < 9; ++e) m.G[e] = m.Gi[e] = (e % 4 == 0) ? 1.0 : 0.0;
}

// the signed adjugate of m.G as it stands (the pick kernel's way back from a slot's G to the model).  Returns whether the model
// stands: everything finite, |det G| above the bound.
SRK_HG_HD int srk_homog_complete(SrkHomogModel& m)
{
    const double det = srk_homog_det3(m.G);
    srk_homog_adj3(m.G, m.Gi);
    const double sg = det < 0.0 ? -1.0 : 1.0;
    int ok = isfinite(det) && fabs(det) > SRK_HOMOG_DET;
    SRK_HG_UNROLL
    for (int e = 0; e < 9; ++e) {
        m.Gi[e] *= sg;
        ok = ok && isfinite(m.G[e]) && isfinite(m.Gi[e]);
    }
    return ok;
}

// G scaled to Frobenius norm 1 and its signed adjugate.  Returns whether the model stands.
SRK_HG_HD int srk_homog_prepare(const double* G, SrkHomogModel& m)
{
    double ss = 0.0;
    SRK_HG_UNROLL
    for (int e = 0; e < 9; ++e) ss += G[e] * G[e];
    const double in = 1.0 / sqrt(ss);
    SRK_HG_UNROLL
    for (int e = 0; e < 9; ++e) m.G[e] = G[e] * in;
    return srk_homog_complete(m);
}

// The projective basis of four points p [4][3]: M = [l0 p0, l1 p1, l2 p2] (columns) with [p0 p1 p2] l = p3, by the adjugate: l_k is
// the determinant of the triple without p_k over the determinant of the first three.  Returns whether no triple is collinear: each
// of the four determinants above SRK_HOMOG_COLLINEAR of the product of the norms of its three columns.
SRK_HG_HD int srk_homog_basis(const double* p, double* M)
{
    const double *p0 = p, *p1 = p + 3, *p2 = p + 6, *p3 = p + 9;
    double c0[3], c1[3], c2[3];
    srk_align_cross(p1, p2, c0);
    srk_align_cross(p2, p0, c1);
    srk_align_cross(p0, p1, c2);
    const double det = srk_align_dot(p0, c0);
    const double l0 = srk_align_dot(c0, p3), l1 = srk_align_dot(c1, p3), l2 = srk_align_dot(c2, p3);
    const double n0 = sqrt(srk_align_dot(p0, p0)), n1 = sqrt(srk_align_dot(p1, p1)), n2 = sqrt(srk_align_dot(p2, p2)), n3 = sqrt(srk_align_dot(p3, p3));
    const int ok = fabs(det) > SRK_HOMOG_COLLINEAR * (n0 * n1 * n2) && fabs(l0) > SRK_HOMOG_COLLINEAR * (n1 * n2 * n3) &&
                   fabs(l1) > SRK_HOMOG_COLLINEAR * (n2 * n0 * n3) && fabs(l2) > SRK_HOMOG_COLLINEAR * (n0 * n1 * n3);
    const double id = 1.0 / det;
    const double s0 = l0 * id, s1 = l1 * id, s2 = l2 * id;
    SRK_HG_UNROLL
    for (int r = 0; r < 3; ++r) {
        M[3 * r] = s0 * p0[r];
        M[3 * r + 1] = s1 * p1[r];
        M[3 * r + 2] = s2 * p2[r];
    }
    return ok;
}

// The model of a sample: pa, pb [4][3] homogeneous pixels (u, v, f0).  G = B adj(A) of the two bases, signed so that (G pa0)_3 > 0,
// scaled to norm 1.  Returns whether the sample has a model; without one m is the identity.
SRK_HG_HD int srk_homog_hypothesis(const double* pa, const double* pb, SrkHomogModel& m)
{
    double A[9], B[9], Aa[9], G[9];
    const int oka = srk_homog_basis(pa, A);
    const int okb = srk_homog_basis(pb, B);
    srk_homog_adj3(A, Aa);
    srk_homog_mul3(B, Aa, G);
    const double z0 = G[6] * pa[0] + G[7] * pa[1] + G[8] * pa[2];
    const double z1 = G[6] * pa[3] + G[7] * pa[4] + G[8] * pa[5];
    const double z2 = G[6] * pa[6] + G[7] * pa[7] + G[8] * pa[8];
    const double z3 = G[6] * pa[9] + G[7] * pa[10] + G[8] * pa[11];
    const int same = (z0 > 0.0 && z1 > 0.0 && z2 > 0.0 && z3 > 0.0) || (z0 < 0.0 && z1 < 0.0 && z2 < 0.0 && z3 < 0.0);
    if (z0 < 0.0) {
        SRK_HG_UNROLL
        for (int e = 0; e < 9; ++e) G[e] = -G[e];
    }
    SrkHomogModel g;
    const int ok = srk_homog_prepare(G, g) && oka && okb && same;
    SRK_HG_UNROLL
    for (int e = 0; e < 9; ++e) { // selected entry by entry: the model stays in registers
        const double id = (e % 4 == 0) ? 1.0 : 0.0;
        m.G[e] = ok ? g.G[e] : id;
        m.Gi[e] = ok ? g.Gi[e] : id;
    }
    return ok;
}

// One match's symmetric transfer: y = G p_a, x = Gi p_b, the residuals rf = pi(y) - uv_b and rb = pi(x) - uv_a (pi(y) = f0 y_xy / y_3).
// Returns whether both third entries are in front and everything is finite.
SRK_HG_HD int srk_homog_transfer(const SrkHomogModel& m, const double* e, double f0, double* y, double* x, double* rf, double* rb)
{
    const double pa[3] = { e[0], e[1], f0 }, pb[3] = { e[2], e[3], f0 };
    srk_homog_mulv(m.G, pa, y);
    srk_homog_mulv(m.Gi, pb, x);
    const double iy = f0 / y[2], ix = f0 / x[2];
    rf[0] = y[0] * iy - e[2];
    rf[1] = y[1] * iy - e[3];
    rb[0] = x[0] * ix - e[0];
    rb[1] = x[1] * ix - e[1];
    return y[2] > 0.0 && x[2] > 0.0 && isfinite(rf[0]) && isfinite(rf[1]) && isfinite(rb[0]) && isfinite(rb[1]);
}

// One match's term of the MSAC score, min(q s, tau^2), s the symmetric transfer error in pixels squared; a match behind either
// image or with a non-finite error counts tau^2.  e = the strip's record {ua, va, ub, vb, q}.  inlier = q s < tau^2; s2 receives s.
SRK_HG_HD double srk_homog_term(const SrkHomogModel& m, const double* e, double f0, double tau2, int& inlier, double& s2)
{
    double y[3], x[3], rf[2], rb[2];
    const int front = srk_homog_transfer(m, e, f0, y, x, rf, rb);
    s2 = rf[0] * rf[0] + rf[1] * rf[1] + rb[0] * rb[0] + rb[1] * rb[1];
    const double w = e[4] * s2;
    inlier = front && w < tau2;
    return inlier ? w : tau2;
}

// ---- a round of local optimisation: G <- G (I + sum d_k B_k) over the basis of the traceless matrices
//   B_0 = E01, B_1 = E02, B_2 = E10, B_3 = E12, B_4 = E20, B_5 = E21, B_6 = E00 - E22, B_7 = E11 - E22   (E_ij: one at row i, column j)
// the row of the Jacobian of one residual pair: v_k = c (B_k z) for the three 2-vectors c0, c1, c2 = the images of the unit vectors
SRK_HG_HD void srk_homog_jrow(const double* c0, const double* c1, const double* c2, const double* z, int a, double* J)
{
    J[0] = z[1] * c0[a];
    J[1] = z[2] * c0[a];
    J[2] = z[0] * c1[a];
    J[3] = z[2] * c1[a];
    J[4] = z[0] * c2[a];
    J[5] = z[1] * c2[a];
    J[6] = z[0] * c0[a] - z[2] * c2[a];
    J[7] = z[1] * c1[a] - z[2] * c2[a];
}
// acc [44] += q (J^T J upper triangle row by row, then J^T r) of one residual
SRK_HG_HD void srk_homog_add_row(double* acc, const double* J, double r, double q)
{
    int at = 0;
    SRK_HG_UNROLL
    for (int i = 0; i < 8; ++i) {
        const double qi = q * J[i];
        SRK_HG_UNROLL
        for (int j = i; j < 8; ++j) acc[at++] += qi * J[j];
        acc[36 + i] += qi * r;
    }
}
// The Jacobians at d = 0 of one match's four residuals.  Forward: d pi(y) G B_k p_a, c_i = d pi(y) (column i of G).  Backward:
// -d pi(x) B_k x, c_i = -d pi(x) e_i.  Jf, Jb [2][8].
SRK_HG_HD void srk_homog_jacobians(const SrkHomogModel& m, const double* e, double f0, const double* y, const double* x, double* Jf, double* Jb)
{
    const double pa[3] = { e[0], e[1], f0 };
    const double iy = f0 / y[2], yx = y[0] / y[2], yy = y[1] / y[2];
    double c0[2], c1[2], c2[2];
    c0[0] = iy * (m.G[0] - yx * m.G[6]), c0[1] = iy * (m.G[3] - yy * m.G[6]);
    c1[0] = iy * (m.G[1] - yx * m.G[7]), c1[1] = iy * (m.G[4] - yy * m.G[7]);
    c2[0] = iy * (m.G[2] - yx * m.G[8]), c2[1] = iy * (m.G[5] - yy * m.G[8]);
    srk_homog_jrow(c0, c1, c2, pa, 0, Jf);
    srk_homog_jrow(c0, c1, c2, pa, 1, Jf + 8);
    const double ix = f0 / x[2];
    const double d0[2] = { -ix, 0.0 }, d1[2] = { 0.0, -ix }, d2[2] = { ix * (x[0] / x[2]), ix * (x[1] / x[2]) };
    srk_homog_jrow(d0, d1, d2, x, 0, Jb);
    srk_homog_jrow(d0, d1, d2, x, 1, Jb + 8);
}
// an inlier's share of the round's sums
SRK_HG_HD void srk_homog_accumulate(double* acc, const SrkHomogModel& m, const double* e, double f0)
{
    double y[3], x[3], rf[2], rb[2], Jf[16], Jb[16];
    srk_homog_transfer(m, e, f0, y, x, rf, rb);
    srk_homog_jacobians(m, e, f0, y, x, Jf, Jb);
    srk_homog_add_row(acc, Jf, rf[0], e[4]);
    srk_homog_add_row(acc, Jf + 8, rf[1], e[4]);
    srk_homog_add_row(acc, Jb, rb[0], e[4]);
    srk_homog_add_row(acc, Jb + 8, rb[1], e[4]);
}

// The step of a round: (J^T J) d = -J^T r by a written-out Cholesky factorisation, then G (I + D) scaled to norm 1.  Returns
// whether the factorisation stands (every pivot positive and finite) and the candidate is a model.
SRK_HG_HD int srk_homog_step(const double* acc, const SrkHomogModel& cur, SrkHomogModel& cand)
{
    double L[8][8], d[8];
    int at = 0, ok = 1;
    SRK_HG_UNROLL
    for (int i = 0; i < 8; ++i) {
        SRK_HG_UNROLL
        for (int j = i; j < 8; ++j) L[j][i] = acc[at++]; // the lower triangle, column by column
    }
    SRK_HG_UNROLL
    for (int j = 0; j < 8; ++j) {
        double p = L[j][j];
        SRK_HG_UNROLL
        for (int k = 0; k < j; ++k) p -= L[j][k] * L[j][k];
        ok = ok && p > 0.0 && isfinite(p);
        const double l = sqrt(p), il = 1.0 / l;
        L[j][j] = l;
        SRK_HG_UNROLL
        for (int i = j + 1; i < 8; ++i) {
            double v = L[i][j];
            SRK_HG_UNROLL
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v * il;
        }
    }
    SRK_HG_UNROLL
    for (int i = 0; i < 8; ++i) { // L z = -g
        double v = -acc[36 + i];
        SRK_HG_UNROLL
        for (int k = 0; k < i; ++k) v -= L[i][k] * d[k];
        d[i] = v / L[i][i];
    }
    SRK_HG_UNROLL
    for (int i = 7; i >= 0; --i) { // L^T d = z
        double v = d[i];
        SRK_HG_UNROLL
        for (int k = i + 1; k < 8; ++k) v -= L[k][i] * d[k];
        d[i] = v / L[i][i];
    }
    const double D[9] = { d[6], d[0], d[1], d[2], d[7], d[3], d[4], d[5], -d[6] - d[7] };
    double GD[9], G[9];
    srk_homog_mul3(cur.G, D, GD);
    SRK_HG_UNROLL
    for (int e = 0; e < 9; ++e) G[e] = cur.G[e] + GD[e];
    const int model = srk_homog_prepare(G, cand);
    return ok && model;
}

// ---- the eigen-decomposition of a symmetric 3 x 3 matrix by cyclic Jacobi, as align's 4 x 4 one
template <int P, int Q> SRK_HG_HD void srk_homog_rotate(double (&A)[3][3], double (&V)[3][3])
{
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = fabs(theta) > 1e150 ? 0.5 / theta : copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] -= t * apq;
    A[Q][Q] += t * apq;
    A[P][Q] = A[Q][P] = 0.0;
    SRK_HG_UNROLL
    for (int r = 0; r < 3; ++r) {
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
// eigenvalues lam [3] (unordered) and eigenvectors (the columns of V) of the symmetric A, which is destroyed
SRK_HG_HD void srk_homog_jacobi3(double (&A)[3][3], double (&V)[3][3], double* lam)
{
    SRK_HG_UNROLL
    for (int i = 0; i < 3; ++i) {
        SRK_HG_UNROLL
        for (int j = 0; j < 3; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < SRK_HOMOG_SWEEPS; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        if (!(off > 0.0)) break; // zero, or not a number
        srk_homog_rotate<0, 1>(A, V);
        srk_homog_rotate<0, 2>(A, V);
        srk_homog_rotate<1, 2>(A, V);
    }
    SRK_HG_UNROLL
    for (int i = 0; i < 3; ++i) lam[i] = A[i][i];
}

// the rotation nearest to M (the maximiser of tr(R^T M)) through align's closed form
SRK_HG_HD void srk_homog_nearest_rotation(const double* M, double* R)
{
    const double zero[3] = { 0.0, 0.0, 0.0 };
    SrkAlignModel a;
    double gap;
    srk_align_closed_form(M, 1.0, zero, zero, 0, a, gap);
    SRK_HG_UNROLL
    for (int e = 0; e < 9; ++e) R[e] = a.R[e];
}

// what the decomposition holds between its passes over the inliers
struct SrkHomogPlanes {
    double H[9];       // normalised (middle singular value 1) and signed
    double gap;        // w1 - w3
    int n_poses;       // 1: a rotation (R[0] alone); 2: the plane's twins
    double R[2][9], N[2][3];
};

// Ma, Soatto, Kosecka, Sastry, algorithm 5.2.  Hraw = K_b^-1 G K_a at any scale; sign_sum = sum q x_b^T Hraw x_a over the inliers.
// H = Hraw over its middle singular value, signed so that the sum is positive; with the eigenvalues w1 >= 1 >= w3 of H^T H and
// their vectors v1, v2, v3 (a proper frame): u_k = (sqrt(1 - w3) v1 +- sqrt(w1 - 1) v3) / sqrt(w1 - w3), U_k = [v2, u_k, v2 x u_k],
// W_k = [H v2, H u_k, H v2 x H u_k], R_k = the rotation nearest to W_k U_k^T, N_k = v2 x u_k.  The normals are not yet flipped.
SRK_HG_HD void srk_homog_planes(const double* Hraw, double sign_sum, SrkHomogPlanes& P)
{
    double S[3][3], V[3][3], lam[3];
    SRK_HG_UNROLL
    for (int i = 0; i < 3; ++i) {
        SRK_HG_UNROLL
        for (int j = 0; j < 3; ++j) S[i][j] = Hraw[i] * Hraw[j] + Hraw[3 + i] * Hraw[3 + j] + Hraw[6 + i] * Hraw[6 + j];
    }
    srk_homog_jacobi3(S, V, lam);
    // descending order by three compare-and-swaps of (value, column)
    double w1 = lam[0], w2 = lam[1], w3 = lam[2];
    double v1[3] = { V[0][0], V[1][0], V[2][0] }, v2[3] = { V[0][1], V[1][1], V[2][1] }, v3[3] = { V[0][2], V[1][2], V[2][2] };
#define SRK_HG_SWAP(wa, va, wb, vb)                                   \
    if (wb > wa) {                                                    \
        const double tw = wa;                                         \
        wa = wb;                                                      \
        wb = tw;                                                      \
        SRK_HG_UNROLL                                                 \
        for (int r = 0; r < 3; ++r) {                                 \
            const double tv = va[r];                                  \
            va[r] = vb[r];                                            \
            vb[r] = tv;                                               \
        }                                                             \
    }
    SRK_HG_SWAP(w1, v1, w2, v2)
    SRK_HG_SWAP(w2, v2, w3, v3)
    SRK_HG_SWAP(w1, v1, w2, v2)
#undef SRK_HG_SWAP
    srk_align_cross(v1, v2, v3); // a proper frame whatever the signs Jacobi left
    const double is = (sign_sum < 0.0 ? -1.0 : 1.0) / sqrt(w2);
    SRK_HG_UNROLL
    for (int e = 0; e < 9; ++e) P.H[e] = Hraw[e] * is;
    const double e1 = w1 / w2, e3 = w3 / w2;
    P.gap = e1 - e3;
    SRK_HG_UNROLL
    for (int k = 0; k < 2; ++k) {
        SRK_HG_UNROLL
        for (int e = 0; e < 9; ++e) P.R[k][e] = 0.0;
        P.N[k][0] = P.N[k][1] = P.N[k][2] = 0.0;
    }
    if (!(P.gap > SRK_HOMOG_GAP)) { // a rotation (or the plane at infinity): H itself, made a rotation
        P.n_poses = 1;
        srk_homog_nearest_rotation(P.H, P.R[0]);
        return;
    }
    P.n_poses = 2;
    const double a = sqrt(fmax(1.0 - e3, 0.0)), b = sqrt(fmax(e1 - 1.0, 0.0)), ig = 1.0 / sqrt(P.gap);
    double hv2[3];
    srk_homog_mulv(P.H, v2, hv2);
    SRK_HG_UNROLL
    for (int k = 0; k < 2; ++k) {
        const double sb = k == 0 ? b : -b;
        double u[3], n[3], hu[3], hn[3], W[9];
        SRK_HG_UNROLL
        for (int r = 0; r < 3; ++r) u[r] = (a * v1[r] + sb * v3[r]) * ig;
        srk_align_cross(v2, u, n);
        srk_homog_mulv(P.H, u, hu);
        srk_align_cross(hv2, hu, hn);
        SRK_HG_UNROLL
        for (int i = 0; i < 3; ++i) {
            SRK_HG_UNROLL
            for (int j = 0; j < 3; ++j) W[3 * i + j] = hv2[i] * v2[j] + hu[i] * u[j] + hn[i] * n[j]; // W_k U_k^T
        }
        srk_homog_nearest_rotation(W, P.R[k]);
        SRK_HG_UNROLL
        for (int r = 0; r < 3; ++r) P.N[k][r] = n[r];
    }
}

// The end of the decomposition: ahead [k] = the inliers with N_k^T x_a > 0 before any flip, of n_inl.  N_k is flipped when fewer
// than half are ahead, T_k = (H - R_k) N_k, and the candidate with more inliers in front comes first (a tie stays with u_1).
// R [2][9], T [2][3], N [2][3], front [2]; unused entries are zero.
SRK_HG_HD void srk_homog_finish(const SrkHomogPlanes& P, const int64_t* ahead, int64_t n_inl, double* R, double* T, double* N, int32_t* front)
{
    SRK_HG_UNROLL
    for (int e = 0; e < 18; ++e) R[e] = 0.0;
    SRK_HG_UNROLL
    for (int e = 0; e < 6; ++e) T[e] = N[e] = 0.0;
    front[0] = front[1] = 0;
    if (P.n_poses == 1) {
        SRK_HG_UNROLL
        for (int e = 0; e < 9; ++e) R[e] = P.R[0][e];
        return;
    }
    const int flip0 = 2 * ahead[0] < n_inl, flip1 = 2 * ahead[1] < n_inl;
    const int64_t f0 = flip0 ? n_inl - ahead[0] : ahead[0], f1 = flip1 ? n_inl - ahead[1] : ahead[1];
    const int first = f1 > f0 ? 1 : 0;
    SRK_HG_UNROLL
    for (int k = 0; k < 2; ++k) {
        const int src = k == 0 ? first : 1 - first;
        const double sg = (src == 0 ? flip0 : flip1) ? -1.0 : 1.0;
        double n[3], d[9];
        SRK_HG_UNROLL
        for (int r = 0; r < 3; ++r) n[r] = sg * (src == 0 ? P.N[0][r] : P.N[1][r]); // selected by value: no pointer into the registers
        SRK_HG_UNROLL
        for (int e = 0; e < 9; ++e) {
            const double rk = src == 0 ? P.R[0][e] : P.R[1][e];
            R[9 * k + e] = rk;
            d[e] = P.H[e] - rk;
        }
        srk_homog_mulv(d, n, T + 3 * k);
        SRK_HG_UNROLL
        for (int r = 0; r < 3; ++r) N[3 * k + r] = n[r];
        front[k] = (int32_t)(src == 0 ? f0 : f1);
    }
}

// the rays of a match and its share of the sign sum: x_a = K_a^-1 p_a, x_b = K_b^-1 p_b, q x_b^T Hraw x_a
SRK_HG_HD double srk_homog_sign_term(const double* Kai, const double* Kbi, const double* Hraw, const double* e, double f0, double* xa)
{
    const double pa[3] = { e[0], e[1], f0 }, pb[3] = { e[2], e[3], f0 };
    double xb[3], hx[3];
    srk_homog_mulv(Kai, pa, xa);
    srk_homog_mulv(Kbi, pb, xb);
    srk_homog_mulv(Hraw, xa, hx);
    return e[4] * srk_align_dot(xb, hx);
}
