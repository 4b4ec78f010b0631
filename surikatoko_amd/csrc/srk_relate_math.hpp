// srk_relate_math.hpp -- the arithmetic of two-view relative pose (srk_relate_frames) as plain functions of
// doubles, compiled for the device by srk_relate.hip and for the host by srk_relate.cpp: the kernels and the host walk of one pair
// (srk_relate_host_pair, tests/cpp/test_relate_host.cpp) run the same statements in the same order.  The sampler, the rays, the
// five-point solve after Nister (null space, the ten cubic constraints by polynomial arithmetic, the degree-10 polynomial and its
// real roots by the derivative chain, back-substitution, a polish of each solution on the constraints), the Sampson error, and
// the decomposition of an essential matrix without an SVD.  No HIP header is needed here.  Every loop has constant bounds and is
// unrolled for the device, and every index into a per-lane array is a constant after unrolling: where a position is known at run
// time only (a pivot, a lane's row) the value is moved by comparisons against every candidate position.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__)
#define SRK_RL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SRK_RL_HD inline
#endif
#if defined(__clang__)
#define SRK_RL_UNROLL _Pragma("unroll")
#else
#define SRK_RL_UNROLL
#endif

#define SRK_RELATE_LANES 64  // hypotheses that share a wave of the score
#define SRK_RELATE_GROUP 16  // lanes that solve one hypothesis
#define SRK_RELATE_STRIP 8   // doubles of a gathered match: uv_a (2), uv_b (2), q, the match's number in its pair, two of padding
#define SRK_RELATE_HYP 20    // doubles of a hypothesis: F (0-8), E (9-17), the squared sixth-match error, valid (160 bytes)
#define SRK_RELATE_SLOT 4    // doubles of a wave's best: score, h, inliers, models in the wave
#define SRK_RELATE_BISECT 80 // halvings of a bracket
#define SRK_RELATE_NEWTON 4  // Newton steps that polish a root

// ---- the sampler: counter-based, no state, a stream of its own.  mix = the splitmix64 finaliser of seed + c * (8 h + k + 1)
SRK_RL_HD uint64_t srk_relate_mix(uint64_t seed, uint32_t h, int k)
{
    uint64_t z = seed + 0xD1B54A32D192ED03ull * (8ull * (uint64_t)h + (uint64_t)k + 1ull);
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

SRK_RL_HD uint64_t srk_relate_mulhi(uint64_t a, uint64_t b)
{
    const uint64_t al = a & 0xffffffffull, ah = a >> 32, bl = b & 0xffffffffull, bh = b >> 32;
    const uint64_t ll = al * bl, lh = al * bh, hl = ah * bl, hh = ah * bh;
    const uint64_t mid = (ll >> 32) + (lh & 0xffffffffull) + (hl & 0xffffffffull);
    return hh + (lh >> 32) + (hl >> 32) + (mid >> 32);
}

// six distinct ranks below n (n >= 6): draw k is uniform among the n - k ranks not yet picked
SRK_RL_HD void srk_relate_sample(uint64_t seed, uint32_t h, int64_t n, int64_t* r)
{
    int64_t s[6]; // the earlier picks in ascending order
    SRK_RL_UNROLL
    for (int k = 0; k < 6; ++k) {
        int64_t v = (int64_t)srk_relate_mulhi(srk_relate_mix(seed, h, k), (uint64_t)(n - k));
        SRK_RL_UNROLL
        for (int j = 0; j < k; ++j)
            if (v >= s[j]) ++v;
        r[k] = v;
        s[k] = v;
        SRK_RL_UNROLL
        for (int j = k; j > 0; --j)
            if (s[j] < s[j - 1]) {
                const int64_t t = s[j];
                s[j] = s[j - 1];
                s[j - 1] = t;
            }
    }
}

// ---- 3 x 3 helpers
SRK_RL_HD double srk_relate_det3(const double* K)
{
    return K[0] * (K[4] * K[8] - K[5] * K[7]) - K[1] * (K[3] * K[8] - K[5] * K[6]) + K[2] * (K[3] * K[7] - K[4] * K[6]);
}

SRK_RL_HD void srk_relate_inverse3(const double* K, double* Ki)
{
    const double id = 1.0 / srk_relate_det3(K);
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

// the ray of a pixel: K^-1 (u, v, f0), normalised
SRK_RL_HD void srk_relate_ray(const double* Ki, double u, double v, double f0, double* b)
{
    const double x = Ki[0] * u + Ki[1] * v + Ki[2] * f0, y = Ki[3] * u + Ki[4] * v + Ki[5] * f0, z = Ki[6] * u + Ki[7] * v + Ki[8] * f0;
    const double in = 1.0 / sqrt(x * x + y * y + z * z);
    b[0] = x * in;
    b[1] = y * in;
    b[2] = z * in;
}

SRK_RL_HD double srk_relate_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
SRK_RL_HD void srk_relate_cross(const double* a, const double* b, double* c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// F = K_b^-T E K_a^-1, so that (u_b, v_b, f0) F (u_a, v_a, f0)^T = 0
SRK_RL_HD void srk_relate_fundamental(const double* Kai, const double* Kbi, const double* E, double* F)
{
    double t[9]; // E K_a^-1
    SRK_RL_UNROLL
    for (int i = 0; i < 3; ++i) {
        SRK_RL_UNROLL
        for (int j = 0; j < 3; ++j) t[3 * i + j] = E[3 * i] * Kai[j] + E[3 * i + 1] * Kai[3 + j] + E[3 * i + 2] * Kai[6 + j];
    }
    SRK_RL_UNROLL
    for (int i = 0; i < 3; ++i) {
        SRK_RL_UNROLL
        for (int j = 0; j < 3; ++j) F[3 * i + j] = Kbi[i] * t[j] + Kbi[3 + i] * t[3 + j] + Kbi[6 + i] * t[6 + j];
    }
}

// the squared Sampson distance in pixels of a match under F
SRK_RL_HD double srk_relate_sampson(const double* F, double ua, double va, double ub, double vb, double f0)
{
    const double l0 = F[0] * ua + F[1] * va + F[2] * f0, l1 = F[3] * ua + F[4] * va + F[5] * f0, l2 = F[6] * ua + F[7] * va + F[8] * f0;
    const double m0 = F[0] * ub + F[3] * vb + F[6] * f0, m1 = F[1] * ub + F[4] * vb + F[7] * f0;
    const double e = ub * l0 + vb * l1 + f0 * l2;
    return e * e / (l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1);
}

// One match's term of the MSAC score, min(q s, tau^2); a match whose error is not finite counts tau^2.  inlier = q s < tau^2.
SRK_RL_HD double srk_relate_term(const double* F, double ua, double va, double ub, double vb, double q, double f0, double tau2, int& inlier)
{
    const double z = q * srk_relate_sampson(F, ua, va, ub, vb, f0);
    inlier = z < tau2;
    return inlier ? z : tau2;
}

// ---- the null space of the 5 x 9 epipolar matrix (rows x_b (x) x_a) by Gauss-Jordan elimination with complete pivoting.  Rows
// and columns are exchanged in place by comparisons against every position; the four null vectors are then made orthonormal
// (Gram-Schmidt, twice).  A pivot below 1e-12 of the first (the rays are unit vectors) says that the five rows are dependent, as
// for five copies of one match: N is then NaN and the sample gives no model.  N [4][9]: E = x N0 + y N1 + z N2 + N3.  xa, xb [5][3].
SRK_RL_HD void srk_relate_nullspace(const double* xa, const double* xb, double* N)
{
    double A[5][9];
    int perm[9];
    SRK_RL_UNROLL
    for (int m = 0; m < 5; ++m) {
        SRK_RL_UNROLL
        for (int i = 0; i < 3; ++i) {
            SRK_RL_UNROLL
            for (int j = 0; j < 3; ++j) A[m][3 * i + j] = xb[3 * m + i] * xa[3 * m + j];
        }
    }
    SRK_RL_UNROLL
    for (int c = 0; c < 9; ++c) perm[c] = c;
    double first = 0.0;
    bool deficient = false; // fewer than five independent rows, to rounding: the sample has no model
    SRK_RL_UNROLL
    for (int k = 0; k < 5; ++k) {
        double best = -1.0;
        int pi = k, pj = k;
        SRK_RL_UNROLL
        for (int i = k; i < 5; ++i) {
            SRK_RL_UNROLL
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
        deficient = deficient || !(best > 1e-12 * first);
        SRK_RL_UNROLL
        for (int i = k + 1; i < 5; ++i) {
            const bool sw = i == pi;
            SRK_RL_UNROLL
            for (int j = 0; j < 9; ++j) {
                const double a = A[k][j], b = A[i][j];
                A[k][j] = sw ? b : a;
                A[i][j] = sw ? a : b;
            }
        }
        SRK_RL_UNROLL
        for (int j = k + 1; j < 9; ++j) {
            const bool sw = j == pj;
            SRK_RL_UNROLL
            for (int i = 0; i < 5; ++i) {
                const double a = A[i][k], b = A[i][j];
                A[i][k] = sw ? b : a;
                A[i][j] = sw ? a : b;
            }
            const int a = perm[k], b = perm[j];
            perm[k] = sw ? b : a;
            perm[j] = sw ? a : b;
        }
        const double inv = 1.0 / A[k][k];
        SRK_RL_UNROLL
        for (int j = 0; j < 9; ++j) A[k][j] *= inv;
        SRK_RL_UNROLL
        for (int i = 0; i < 5; ++i) {
            if (i == k) continue;
            const double f = A[i][k];
            SRK_RL_UNROLL
            for (int j = 0; j < 9; ++j) A[i][j] -= f * A[k][j];
        }
    }
    // null vector f in the exchanged columns: -A[.][5 + f] on the pivots, 1 at 5 + f
    SRK_RL_UNROLL
    for (int f = 0; f < 4; ++f) {
        SRK_RL_UNROLL
        for (int e = 0; e < 9; ++e) {
            double v = 0.0;
            SRK_RL_UNROLL
            for (int c = 0; c < 5; ++c) v = perm[c] == e ? -A[c][5 + f] : v;
            v = perm[5 + f] == e ? 1.0 : v;
            N[9 * f + e] = v;
        }
    }
    SRK_RL_UNROLL
    for (int f = 0; f < 4; ++f) {
        SRK_RL_UNROLL
        for (int pass = 0; pass < 2; ++pass) {
            SRK_RL_UNROLL
            for (int g = 0; g < f; ++g) {
                double d = 0.0;
                SRK_RL_UNROLL
                for (int e = 0; e < 9; ++e) d += N[9 * f + e] * N[9 * g + e];
                SRK_RL_UNROLL
                for (int e = 0; e < 9; ++e) N[9 * f + e] -= d * N[9 * g + e];
            }
        }
        double s = 0.0;
        SRK_RL_UNROLL
        for (int e = 0; e < 9; ++e) s += N[9 * f + e] * N[9 * f + e];
        const double in = deficient ? NAN : 1.0 / sqrt(s);
        SRK_RL_UNROLL
        for (int e = 0; e < 9; ++e) N[9 * f + e] *= in;
    }
}

// ---- polynomials in (x, y, z).  Degree 1: [x y z 1].  Degree 2: [x^2 y^2 xy xz x yz y z^2 z 1].  Degree 3, the order of the
// elimination: [x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1].  The position of a product is a
// constant expression of the loop counters.
constexpr int srk_relate_code1(int l) { return l == 0 ? 100 : (l == 1 ? 10 : (l == 2 ? 1 : 0)); } // exponents as digits x y z
constexpr int srk_relate_code2(int m)
{
    return m == 0 ? 200 : m == 1 ? 20 : m == 2 ? 110 : m == 3 ? 101 : m == 4 ? 100 : m == 5 ? 11 : m == 6 ? 10 : m == 7 ? 2 : m == 8 ? 1 : 0;
}
constexpr int srk_relate_pos2(int code)
{
    return code == 200 ? 0 : code == 20 ? 1 : code == 110 ? 2 : code == 101 ? 3 : code == 100 ? 4 : code == 11 ? 5 : code == 10 ? 6 : code == 2 ? 7 : code == 1 ? 8 : 9;
}
constexpr int srk_relate_pos3(int code)
{
    return code == 300   ? 0
           : code == 30  ? 1
           : code == 210 ? 2
           : code == 120 ? 3
           : code == 201 ? 4
           : code == 200 ? 5
           : code == 21  ? 6
           : code == 20  ? 7
           : code == 111 ? 8
           : code == 110 ? 9
           : code == 102 ? 10
           : code == 101 ? 11
           : code == 100 ? 12
           : code == 12  ? 13
           : code == 11  ? 14
           : code == 10  ? 15
           : code == 3   ? 16
           : code == 2   ? 17
           : code == 1   ? 18
                         : 19;
}

// c2 += a * b (degree 1 times degree 1)
SRK_RL_HD void srk_relate_mul11(const double* a, const double* b, double* c2)
{
    SRK_RL_UNROLL
    for (int i = 0; i < 4; ++i) {
        SRK_RL_UNROLL
        for (int j = 0; j < 4; ++j) c2[srk_relate_pos2(srk_relate_code1(i) + srk_relate_code1(j))] += a[i] * b[j];
    }
}
// c3 += s * a2 * b (degree 2 times degree 1)
SRK_RL_HD void srk_relate_mul21(double s, const double* a2, const double* b, double* c3)
{
    SRK_RL_UNROLL
    for (int i = 0; i < 10; ++i) {
        SRK_RL_UNROLL
        for (int j = 0; j < 4; ++j) c3[srk_relate_pos3(srk_relate_code2(i) + srk_relate_code1(j))] += s * (a2[i] * b[j]);
    }
}

// Row r of the ten constraints over the 20 monomials: r = 0 is det E, r = 1 + 3 i + j the entry (i, j) of 2 E E^T E - tr(E E^T) E.
SRK_RL_HD void srk_relate_row(const double* N, int r, double* row)
{
    SRK_RL_UNROLL
    for (int e = 0; e < 20; ++e) row[e] = 0.0;
    if (r == 0) {
        SRK_RL_UNROLL
        for (int t = 0; t < 3; ++t) { // + E[0][t] (E[1][t+1] E[2][t+2] - E[1][t+2] E[2][t+1])
            const int u = (t + 1) % 3, v = (t + 2) % 3;
            double e0[4], a[4], b[4], c[4], d[4], m[10];
            SRK_RL_UNROLL
            for (int l = 0; l < 4; ++l) {
                e0[l] = N[9 * l + t];
                a[l] = N[9 * l + 3 + u];
                b[l] = N[9 * l + 6 + v];
                c[l] = -N[9 * l + 3 + v];
                d[l] = N[9 * l + 6 + u];
            }
            SRK_RL_UNROLL
            for (int e = 0; e < 10; ++e) m[e] = 0.0;
            srk_relate_mul11(a, b, m);
            srk_relate_mul11(c, d, m);
            srk_relate_mul21(1.0, m, e0, row);
        }
        return;
    }
    const int i = (r - 1) / 3, j = (r - 1) % 3;
    double Ai[3][4], cj[3][4], eij[4], tr[10];
    SRK_RL_UNROLL
    for (int m = 0; m < 3; ++m) {
        SRK_RL_UNROLL
        for (int l = 0; l < 4; ++l) {
            // every candidate is read first and the choice is made among values, not among addresses
            const double r0 = N[9 * l + m], r1 = N[9 * l + 3 + m], r2 = N[9 * l + 6 + m];
            const double k0 = N[9 * l + 3 * m], k1 = N[9 * l + 3 * m + 1], k2 = N[9 * l + 3 * m + 2];
            Ai[m][l] = i == 0 ? r0 : (i == 1 ? r1 : r2); // E[i][m]
            cj[m][l] = j == 0 ? k0 : (j == 1 ? k1 : k2); // E[m][j]
        }
    }
    SRK_RL_UNROLL
    for (int l = 0; l < 4; ++l) {
        const double a0 = Ai[0][l], a1 = Ai[1][l], a2 = Ai[2][l];
        eij[l] = j == 0 ? a0 : (j == 1 ? a1 : a2);
    }
    SRK_RL_UNROLL
    for (int e = 0; e < 10; ++e) tr[e] = 0.0;
    SRK_RL_UNROLL
    for (int k = 0; k < 3; ++k) {
        double g[10]; // (E E^T)[i][k]
        SRK_RL_UNROLL
        for (int e = 0; e < 10; ++e) g[e] = 0.0;
        SRK_RL_UNROLL
        for (int m = 0; m < 3; ++m) {
            double ek[4];
            SRK_RL_UNROLL
            for (int l = 0; l < 4; ++l) ek[l] = N[9 * l + 3 * k + m];
            srk_relate_mul11(Ai[m], ek, g);
            srk_relate_mul11(ek, ek, tr);
        }
        srk_relate_mul21(2.0, g, cj[k], row);
    }
    srk_relate_mul21(-1.0, tr, eij, row);
}

// ---- B(z) from the six rows of [I | G] that belong to x^2z, x^2, y^2z, y^2, xyz, xy (G4 .. G9: the right halves, 10 each):
// z * row(x^2) - row(x^2z) and its two likes are linear in (x, y, 1) with coefficients in z.  bx, by [3][4], b1 [3][5], ascending.
SRK_RL_HD void srk_relate_bz(const double* G4, const double* G5, const double* G6, const double* G7, const double* G8, const double* G9, double* bx,
                             double* by, double* b1)
{
    SRK_RL_UNROLL
    for (int r = 0; r < 3; ++r) {
        const double* lo = r == 0 ? G4 : (r == 1 ? G6 : G8); // the row of the monomial with z
        const double* hi = r == 0 ? G5 : (r == 1 ? G7 : G9); // the row that is multiplied by z
        bx[4 * r + 3] = hi[0];
        bx[4 * r + 2] = hi[1] - lo[0];
        bx[4 * r + 1] = hi[2] - lo[1];
        bx[4 * r + 0] = -lo[2];
        by[4 * r + 3] = hi[3];
        by[4 * r + 2] = hi[4] - lo[3];
        by[4 * r + 1] = hi[5] - lo[4];
        by[4 * r + 0] = -lo[5];
        b1[5 * r + 4] = hi[6];
        b1[5 * r + 3] = hi[7] - lo[6];
        b1[5 * r + 2] = hi[8] - lo[7];
        b1[5 * r + 1] = hi[9] - lo[8];
        b1[5 * r + 0] = -lo[9];
    }
}

// p [11] = det B(z), ascending, by the third column
SRK_RL_HD void srk_relate_detb(const double* bx, const double* by, const double* b1, double* p)
{
    SRK_RL_UNROLL
    for (int e = 0; e < 11; ++e) p[e] = 0.0;
    SRK_RL_UNROLL
    for (int r = 0; r < 3; ++r) {
        const int u = (r + 1) % 3, v = (r + 2) % 3; // the minor of rows u, v in cyclic order: sign +
        double m[7];
        SRK_RL_UNROLL
        for (int e = 0; e < 7; ++e) m[e] = 0.0;
        SRK_RL_UNROLL
        for (int a = 0; a < 4; ++a) {
            SRK_RL_UNROLL
            for (int b = 0; b < 4; ++b) m[a + b] += bx[4 * u + a] * by[4 * v + b] - by[4 * u + a] * bx[4 * v + b];
        }
        SRK_RL_UNROLL
        for (int a = 0; a < 7; ++a) {
            SRK_RL_UNROLL
            for (int b = 0; b < 5; ++b) p[a + b] += m[a] * b1[5 * r + b];
        }
    }
}

// ---- the real roots of p (degree 10) by the derivative chain: the roots of p^(k+1) bracket those of p^(k) inside the Cauchy bound
constexpr double srk_relate_binom(int n, int k)
{
    double b = 1.0;
    for (int i = 0; i < k; ++i) b = b * (double)(n - i) / (double)(i + 1);
    return b;
}

// p^(10 - D) / (10 - D)! at z: a polynomial of degree D
template <int D> SRK_RL_HD double srk_relate_eval(const double* p, double z)
{
    constexpr int k = 10 - D;
    double v = p[10] * srk_relate_binom(10, k);
    SRK_RL_UNROLL
    for (int j = 9; j >= k; --j) v = v * z + p[j] * srk_relate_binom(j, k);
    return v;
}
template <> SRK_RL_HD double srk_relate_eval<0>(const double* p, double) { return p[10]; }

SRK_RL_HD double srk_relate_bound(const double* p)
{
    double m = 0.0;
    SRK_RL_UNROLL
    for (int j = 0; j < 10; ++j) m = fmax(m, fabs(p[j] / p[10]));
    return 1.0 + m;
}

// the root of level D in [lo, hi], if the signs at the ends differ: halving, then Newton steps that stay inside
template <int D> SRK_RL_HD int srk_relate_interval(const double* p, double lo, double hi, double& root)
{
    const double lo0 = lo, hi0 = hi;
    const double fl = srk_relate_eval<D>(p, lo), fh = srk_relate_eval<D>(p, hi);
    const int found = isfinite(fl) && isfinite(fh) && ((fl < 0.0) != (fh < 0.0));
    for (int it = 0; it < SRK_RELATE_BISECT; ++it) {
        const double mid = 0.5 * (lo + hi), fm = srk_relate_eval<D>(p, mid);
        const bool left = (fm < 0.0) == (fl < 0.0);
        lo = left ? mid : lo;
        hi = left ? hi : mid;
    }
    double z = 0.5 * (lo + hi);
    SRK_RL_UNROLL
    for (int it = 0; it < SRK_RELATE_NEWTON; ++it) {
        const double f = srk_relate_eval<D>(p, z), df = (double)(11 - D) * srk_relate_eval<D - 1>(p, z);
        const double n = z - f / df;
        z = (n >= lo0 && n <= hi0) ? n : z;
    }
    root = z;
    return found;
}

// C = A B and C = A B^T, 3 x 3
SRK_RL_HD void srk_relate_mm(const double* A, const double* B, double* C)
{
    SRK_RL_UNROLL
    for (int i = 0; i < 3; ++i) {
        SRK_RL_UNROLL
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
    }
}
SRK_RL_HD void srk_relate_mmt(const double* A, const double* B, double* C)
{
    SRK_RL_UNROLL
    for (int i = 0; i < 3; ++i) {
        SRK_RL_UNROLL
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1] + A[3 * i + 2] * B[3 * j + 2];
    }
}

// Gauss-Newton steps on the ten constraints themselves, evaluated from E = x N0 + y N1 + z N2 + N3 and not from the eliminated
// coefficients: the elimination and det B(z) lose digits where a root of p is badly conditioned in z, the solution itself rarely
// is.  c(E) = 2 M E - tr(M) E with M = E E^T, and det E; along a direction D, c' = 2 (S + S^T) E + 2 M D - 2 tr(S) E - tr(M) D with
// S = D E^T, and det' = Cof(E) : D.  A step that is not finite is not taken.
#define SRK_RELATE_POLISH 6
SRK_RL_HD void srk_relate_polish(const double* N, double& x, double& y, double& z)
{
    for (int it = 0; it < SRK_RELATE_POLISH; ++it) {
        double E[9], M[9], ME[9], r[10], cof[9], J[3][10];
        SRK_RL_UNROLL
        for (int e = 0; e < 9; ++e) E[e] = x * N[e] + y * N[9 + e] + z * N[18 + e] + N[27 + e];
        srk_relate_mmt(E, E, M);
        srk_relate_mm(M, E, ME);
        const double tr = M[0] + M[4] + M[8];
        SRK_RL_UNROLL
        for (int e = 0; e < 9; ++e) r[e] = 2.0 * ME[e] - tr * E[e];
        srk_relate_cross(E + 3, E + 6, cof);
        srk_relate_cross(E + 6, E, cof + 3);
        srk_relate_cross(E, E + 3, cof + 6);
        r[9] = srk_relate_dot(E, cof);
        SRK_RL_UNROLL
        for (int d = 0; d < 3; ++d) {
            const double* D = N + 9 * d;
            double S[9], P[9], PE[9], MD[9];
            srk_relate_mmt(D, E, S);
            SRK_RL_UNROLL
            for (int i = 0; i < 3; ++i) {
                SRK_RL_UNROLL
                for (int j = 0; j < 3; ++j) P[3 * i + j] = S[3 * i + j] + S[3 * j + i];
            }
            srk_relate_mm(P, E, PE);
            srk_relate_mm(M, D, MD);
            const double ts = S[0] + S[4] + S[8];
            double dd = 0.0;
            SRK_RL_UNROLL
            for (int e = 0; e < 9; ++e) {
                J[d][e] = 2.0 * PE[e] + 2.0 * MD[e] - 2.0 * ts * E[e] - tr * D[e];
                dd += cof[e] * D[e];
            }
            J[d][9] = dd;
        }
        double A[9], Ai[9], g[3];
        SRK_RL_UNROLL
        for (int a = 0; a < 3; ++a) {
            SRK_RL_UNROLL
            for (int b = 0; b < 3; ++b) {
                double s = 0.0;
                SRK_RL_UNROLL
                for (int e = 0; e < 10; ++e) s += J[a][e] * J[b][e];
                A[3 * a + b] = s;
            }
            double s = 0.0;
            SRK_RL_UNROLL
            for (int e = 0; e < 10; ++e) s += J[a][e] * r[e];
            g[a] = s;
        }
        srk_relate_inverse3(A, Ai);
        const double dx = Ai[0] * g[0] + Ai[1] * g[1] + Ai[2] * g[2], dy = Ai[3] * g[0] + Ai[4] * g[1] + Ai[5] * g[2],
                     dz = Ai[6] * g[0] + Ai[7] * g[1] + Ai[8] * g[2];
        const bool ok = isfinite(dx) && isfinite(dy) && isfinite(dz);
        x = ok ? x - dx : x;
        y = ok ? y - dy : y;
        z = ok ? z - dz : z;
    }
}

// ---- the essential matrix of a root: (x, y, 1) spans the null space of B(z), from the cross product of the two rows whose third
// cofactor is the largest; E = x N0 + y N1 + z N2 + N3 scaled to Frobenius norm sqrt(2) (that of [T]x R with |T| = 1)
SRK_RL_HD void srk_relate_model(const double* N, const double* bx, const double* by, const double* b1, double z, double* E)
{
    double M[9];
    SRK_RL_UNROLL
    for (int r = 0; r < 3; ++r) {
        M[3 * r] = ((bx[4 * r + 3] * z + bx[4 * r + 2]) * z + bx[4 * r + 1]) * z + bx[4 * r];
        M[3 * r + 1] = ((by[4 * r + 3] * z + by[4 * r + 2]) * z + by[4 * r + 1]) * z + by[4 * r];
        M[3 * r + 2] = (((b1[5 * r + 4] * z + b1[5 * r + 3]) * z + b1[5 * r + 2]) * z + b1[5 * r + 1]) * z + b1[5 * r];
    }
    double c[3], best[3];
    srk_relate_cross(M, M + 3, best);
    srk_relate_cross(M, M + 6, c);
    if (fabs(c[2]) > fabs(best[2])) best[0] = c[0], best[1] = c[1], best[2] = c[2];
    srk_relate_cross(M + 3, M + 6, c);
    if (fabs(c[2]) > fabs(best[2])) best[0] = c[0], best[1] = c[1], best[2] = c[2];
    double x = best[0] / best[2], y = best[1] / best[2];
    srk_relate_polish(N, x, y, z);
    double s = 0.0;
    SRK_RL_UNROLL
    for (int e = 0; e < 9; ++e) {
        E[e] = x * N[e] + y * N[9 + e] + z * N[18 + e] + N[27 + e];
        s += E[e] * E[e];
    }
    const double in = sqrt(2.0 / s);
    SRK_RL_UNROLL
    for (int e = 0; e < 9; ++e) E[e] *= in;
}

// ---- the decomposition of E (Frobenius norm sqrt(2)) without an SVD: T, a unit vector, from the largest cross product of two
// columns of E (every column is orthogonal to T); with Cof(E) the matrix of cofactors, R1 = Cof(E) - [T]x E and
// R2 = Cof(E) + [T]x E (Horn 1990).  [T]x R1 = E, [-T]x R2 = E, and (R1, -T), (R2, T) give -E.
SRK_RL_HD void srk_relate_decompose(const double* E, double* R1, double* R2, double* T)
{
    double c0[3] = { E[0], E[3], E[6] }, c1[3] = { E[1], E[4], E[7] }, c2[3] = { E[2], E[5], E[8] };
    double t[3], c[3];
    srk_relate_cross(c0, c1, t);
    double best = srk_relate_dot(t, t);
    srk_relate_cross(c0, c2, c);
    double d = srk_relate_dot(c, c);
    if (d > best) best = d, t[0] = c[0], t[1] = c[1], t[2] = c[2];
    srk_relate_cross(c1, c2, c);
    d = srk_relate_dot(c, c);
    if (d > best) best = d, t[0] = c[0], t[1] = c[1], t[2] = c[2];
    const double in = 1.0 / sqrt(best);
    SRK_RL_UNROLL
    for (int a = 0; a < 3; ++a) T[a] = t[a] * in;
    double cof[9];
    srk_relate_cross(E + 3, E + 6, cof);
    srk_relate_cross(E + 6, E, cof + 3);
    srk_relate_cross(E, E + 3, cof + 6);
    SRK_RL_UNROLL
    for (int j = 0; j < 3; ++j) {
        const double col[3] = { E[j], E[3 + j], E[6 + j] };
        double te[3];
        srk_relate_cross(T, col, te); // column j of [T]x E
        SRK_RL_UNROLL
        for (int i = 0; i < 3; ++i) {
            R1[3 * i + j] = cof[3 * i + j] - te[i];
            R2[3 * i + j] = cof[3 * i + j] + te[i];
        }
    }
}

// E = [T]x R
SRK_RL_HD void srk_relate_essential(const double* R, const double* T, double* E)
{
    SRK_RL_UNROLL
    for (int j = 0; j < 3; ++j) {
        const double col[3] = { R[j], R[3 + j], R[6 + j] };
        double te[3];
        srk_relate_cross(T, col, te);
        SRK_RL_UNROLL
        for (int i = 0; i < 3; ++i) E[3 * i + j] = te[i];
    }
}

// One match under the pose (R, sign * T): whether the point of the two rays lies at a positive distance along both (depth_b b =
// depth_a R a + T, so the signs are those of -(T x b) . c and -(T x a') . c with a' = R a, c = a' x b), and the angle between them.
SRK_RL_HD int srk_relate_front(const double* R, const double* T, double sign, const double* a, const double* b, double& angle)
{
    const double ar[3] = { R[0] * a[0] + R[1] * a[1] + R[2] * a[2], R[3] * a[0] + R[4] * a[1] + R[5] * a[2], R[6] * a[0] + R[7] * a[1] + R[8] * a[2] };
    double c[3], tb[3], ta[3];
    srk_relate_cross(ar, b, c);
    srk_relate_cross(T, b, tb);
    srk_relate_cross(T, ar, ta);
    angle = atan2(sqrt(srk_relate_dot(c, c)), srk_relate_dot(ar, b));
    return sign * srk_relate_dot(tb, c) < 0.0 && sign * srk_relate_dot(ta, c) < 0.0;
}

// The order of the four poses of an E, which also breaks a tie of the vote: 0 (R1, T), 1 (R1, -T), 2 (R2, T), 3 (R2, -T).
