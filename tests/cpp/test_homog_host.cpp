// test_homog_host.cpp -- the host half of the two-view homography (surikatoko_amd/csrc/srk_homog.cpp) and its math header without a
// GPU, driven by tests/test_homography_cpu.py.  Built with the host compiler alone:
//   c++ -std=c++17 tests/cpp/test_homog_host.cpp surikatoko_amd/csrc/srk_homog.cpp
// Usage:
//   test_homog_host unit               the argument checks, the option defaults, the Jacobians against central differences, the
//                                      Cholesky step, the decomposition's identities and three walks; exit status 0 = all hold
//   test_homog_host sampler OUT S N H  the ranks of hypotheses 0 .. H - 1 among N matches under seed S: int64 [H][4]
//   test_homog_host model IN OUT       IN: int64 n, double f0, uv_a [n][4][2], uv_b [n][4][2]; OUT: G [n][9], int32 ok [n]
//   test_homog_host eig IN OUT         IN: int64 n, symmetric A [n][9]; OUT: eigenvalues [n][3] in ascending order
#include "../../surikatoko_amd/csrc/srk_homog.hpp"
#include "../../surikatoko_amd/csrc/srk_homog_math.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace {
int failures = 0;
void expect(bool ok, const char* what)
{
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what);
        ++failures;
    }
}
bool refused(const std::string& why, const char* part) { return !why.empty() && why.find(part) != std::string::npos; }

// a fixed linear congruential stream in [-1, 1): the unit test needs no more
struct Lcg {
    uint64_t x = 12345;
    double next()
    {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(x >> 11) / 4503599627370496.0 - 1.0;
    }
};

const double F0 = 600.0;
const double KA[9] = { 1.25, 0.0, 0.53, 0.0, 1.3, 0.4, 0.0, 0.0, 1.0 }, KB[9] = { 1.1, 0.01, 0.5, 0.0, 1.15, 0.42, 0.0, 0.0, 1.0 };

void rodrigues(const double* w, double* R)
{
    const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double k[3] = { w[0] / th, w[1] / th, w[2] / th }, c = std::cos(th), s = std::sin(th);
    const double K[9] = { 0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0 };
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double kk = 0.0;
            for (int m = 0; m < 3; ++m) kk += K[3 * i + m] * K[3 * m + j];
            R[3 * i + j] = (i == j ? 1.0 : 0.0) + s * K[3 * i + j] + (1.0 - c) * kk;
        }
}

void pixel(const double* K, const double* x, double* uv)
{
    double p[3];
    srk_homog_mulv(K, x, p);
    uv[0] = F0 * p[0] / p[2], uv[1] = F0 * p[1] / p[2];
}

// n matches of a pair: points on the plane z = 6 + 0.2 x - 0.1 y (or anywhere with planar false) seen from (I, 0) and (R, T)
void make_pair(Lcg& g, int n, bool planar, const double* R, const double* T, std::vector<double>& ua, std::vector<double>& ub)
{
    ua.assign(2 * n, 0.0), ub.assign(2 * n, 0.0);
    for (int k = 0; k < n; ++k) {
        double X[3] = { 2.0 * g.next(), 1.5 * g.next(), 6.0 + 2.0 * g.next() }, Y[3];
        if (planar) X[2] = 6.0 + 0.2 * X[0] - 0.1 * X[1];
        srk_homog_mulv(R, X, Y);
        for (int r = 0; r < 3; ++r) Y[r] += T[r];
        pixel(KA, X, &ua[2 * k]);
        pixel(KB, Y, &ub[2 * k]);
    }
}

double max_abs_diff(const double* a, const double* b, int n)
{
    double m = 0.0;
    for (int e = 0; e < n; ++e) m = std::fmax(m, std::fabs(a[e] - b[e]));
    return m;
}

void check_rotation(const double* R, const char* what)
{
    double worst = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double d = 0.0;
            for (int m = 0; m < 3; ++m) d += R[3 * i + m] * R[3 * j + m];
            worst = std::fmax(worst, std::fabs(d - (i == j ? 1.0 : 0.0)));
        }
    expect(worst <= 1e-13 && std::fabs(srk_homog_det3(R) - 1.0) <= 1e-13, what);
}

int unit()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    srk_homography_options o;
    std::memset(&o, 0xff, sizeof o);
    srk_homography_default_options(&o);
    expect(o.hypotheses == 256 && o.inlier_pixels == 6.0 && o.seed == 1 && o.refine_rounds == 4, "default options");
    expect(srk_homog_effective_options(nullptr).hypotheses == 256, "NULL options = the defaults");

    // ---- the checks
    const int64_t rp[] = { 0, 0, 1, 4 };
    const double a[] = { 1, 2, 3, 4, 5, 6, 7, 8 }, b[] = { 2, 1, 4, 3, 6, 5, 8, 7 }, q[] = { 1, 0, 2.5, 1 };
    double K3[27];
    for (int i = 0; i < 3; ++i) std::memcpy(K3 + 9 * i, KA, sizeof KA);
    auto chk = [&](int32_t n, const int64_t* row, const double* x, const double* y, const double* w, const double* Ka, const double* Kb, int shared,
                   const srk_homography_options* opts) { return srk_homog_check(n, row, x, y, w, Ka, Kb, shared, opts); };
    expect(chk(3, rp, a, b, q, K3, K3, 0, &o).empty(), "a good batch passes");
    expect(chk(3, rp, a, b, nullptr, KA, KB, 1, nullptr).empty(), "q and the options may be NULL, K shared");
    expect(chk(0, rp, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &o).empty(), "no pairs, no arrays");
    expect(refused(chk(-1, rp, a, b, q, K3, K3, 0, &o), "negative pair count"), "negative count");
    expect(refused(chk(3, nullptr, a, b, q, K3, K3, 0, &o), "row_ptr is NULL"), "NULL row_ptr");
    expect(refused(chk(3, rp, nullptr, b, q, K3, K3, 0, &o), "NULL match array"), "NULL uv_a");
    expect(refused(chk(3, rp, a, b, q, nullptr, K3, 0, &o), "intrinsics array is NULL"), "NULL K_a");
    {
        const int64_t bad[] = { 1, 1, 2, 4 }, dec[] = { 0, 2, 1, 4 }, neg[] = { 0, -1, 1, 4 };
        expect(refused(chk(3, bad, a, b, q, K3, K3, 0, &o), "row_ptr[0]"), "row_ptr starts at 0");
        expect(refused(chk(3, dec, a, b, q, K3, K3, 0, &o), "decreases at pair 1"), "decreasing row_ptr");
        expect(refused(chk(3, neg, a, b, q, K3, K3, 0, &o), "decreases at pair 0"), "negative row_ptr");
    }
    for (double bad : { nan, inf }) {
        double x[8], w[4], K[27];
        std::memcpy(x, a, sizeof x), std::memcpy(w, q, sizeof w), std::memcpy(K, K3, sizeof K);
        x[5] = bad, w[3] = bad, K[9 + 4] = bad;
        expect(refused(chk(3, rp, x, b, q, K3, K3, 0, &o), "uv_a of match 2"), "uv_a not finite");
        expect(refused(chk(3, rp, a, x, q, K3, K3, 0, &o), "uv_b of match 2"), "uv_b not finite");
        expect(refused(chk(3, rp, a, b, w, K3, K3, 0, &o), "q of match 3"), "q not finite");
        expect(refused(chk(3, rp, a, b, q, K, K3, 0, &o), "K_a of pair 1 is not finite"), "K_a not finite");
        expect(refused(chk(3, rp, a, b, q, K3, K, 0, &o), "K_b of pair 1 is not finite"), "K_b not finite");
    }
    {
        double w[4], K[27];
        std::memcpy(w, q, sizeof w), std::memcpy(K, K3, sizeof K);
        w[0] = -1.0;
        K[18 + 8] = 0.0;
        expect(refused(chk(3, rp, a, b, w, K3, K3, 0, &o), "q of match 0"), "negative q");
        expect(refused(chk(3, rp, a, b, q, K3, K, 0, &o), "K_b of pair 2 is singular"), "singular K");
    }
    {
        srk_homography_options p = o;
        p.hypotheses = 0;
        expect(refused(chk(3, rp, a, b, q, K3, K3, 0, &p), "hypotheses outside 1..4096"), "no hypotheses");
        p.hypotheses = 4097;
        expect(refused(chk(3, rp, a, b, q, K3, K3, 0, &p), "hypotheses outside"), "too many hypotheses");
        p = o;
        for (double bad : { 0.0, -1.0, nan, inf }) {
            p.inlier_pixels = bad;
            expect(refused(chk(3, rp, a, b, q, K3, K3, 0, &p), "inlier_pixels"), "inlier_pixels");
        }
        p = o;
        p.refine_rounds = 17;
        expect(refused(chk(3, rp, a, b, q, K3, K3, 0, &p), "refine_rounds outside 0..16"), "too many rounds");
        p.refine_rounds = -1;
        expect(refused(chk(3, rp, a, b, q, K3, K3, 0, &p), "refine_rounds"), "negative rounds");
        p = o;
        p.hypotheses = 4096;
        std::vector<int64_t> many((1 << 16) + 2, 0);
        expect(refused(chk((1 << 16) + 1, many.data(), nullptr, nullptr, nullptr, KA, KB, 1, &p), "split the batch"), "too many waves");
    }
    const char* why = nullptr;
    expect(srk_homography_check_pairs(3, rp, a, b, q, K3, K3, 0, &o, &why) == SRK_OK && why && !*why, "the C entry point passes a good batch");
    expect(srk_homography_check_pairs(3, nullptr, a, b, q, K3, K3, 0, &o, &why) == SRK_E_ARGS && why && *why, "and refuses with a text");

    // ---- the math header
    Lcg g;
    const double w[3] = { 0.11, -0.17, 0.06 }, T[3] = { 0.5, -0.2, 0.3 }, zero[3] = { 0, 0, 0 };
    double R[9];
    rodrigues(w, R);
    std::vector<double> ua, ub;
    make_pair(g, 40, true, R, T, ua, ub);
    // the four-point model transfers every match of the plane
    double pa[12], pb[12];
    for (int k = 0; k < 4; ++k) {
        pa[3 * k] = ua[2 * k], pa[3 * k + 1] = ua[2 * k + 1], pa[3 * k + 2] = F0;
        pb[3 * k] = ub[2 * k], pb[3 * k + 1] = ub[2 * k + 1], pb[3 * k + 2] = F0;
    }
    SrkHomogModel m;
    expect(srk_homog_hypothesis(pa, pb, m) == 1, "a sample of the plane has a model");
    double ss = 0.0, worst = 0.0;
    for (int e = 0; e < 9; ++e) ss += m.G[e] * m.G[e];
    expect(std::fabs(ss - 1.0) <= 1e-14, "the model has norm 1");
    for (int k = 0; k < 40; ++k) {
        const double e[5] = { ua[2 * k], ua[2 * k + 1], ub[2 * k], ub[2 * k + 1], 1.0 };
        int in;
        double s2;
        srk_homog_term(m, e, F0, 1.0, in, s2);
        worst = std::fmax(worst, s2);
        expect(in == 1, "every match of the plane is an inlier");
    }
    expect(worst <= 1e-18, "the transfer error of the plane's matches is rounding");
    {
        double pc[12];
        std::memcpy(pc, pa, sizeof pc);
        for (int c = 0; c < 2; ++c) pc[6 + c] = 0.5 * (pc[c] + pc[3 + c]); // the third point on the line of the first two
        SrkHomogModel bad;
        expect(srk_homog_hypothesis(pc, pb, bad) == 0 && bad.G[0] == 1.0 && bad.G[1] == 0.0, "a collinear triple has no model");
    }
    // the Jacobians against central differences of the residuals under G (I + d B_k)
    {
        SrkHomogModel noisy = m;
        double G[9];
        for (int e = 0; e < 9; ++e) G[e] = m.G[e] * (1.0 + 1e-3 * g.next());
        srk_homog_prepare(G, noisy);
        double jworst = 0.0;
        for (int k = 0; k < 40; ++k) {
            const double e[5] = { ua[2 * k], ua[2 * k + 1], ub[2 * k], ub[2 * k + 1], 1.0 };
            double y[3], x[3], rf[2], rb[2], Jf[16], Jb[16];
            srk_homog_transfer(noisy, e, F0, y, x, rf, rb);
            srk_homog_jacobians(noisy, e, F0, y, x, Jf, Jb);
            for (int d = 0; d < 8; ++d) {
                // two central differences, steps 2e-3 and 1e-3, and their Richardson extrapolation (4 D(h / 2) - D(h)) / 3: the
                // h^2 term cancels, the h^4 term is left (1e-12 relative) beside the rounding eps f / h (1e-13)
                double res[4][4];
                const double steps[4] = { -2e-3, 2e-3, -1e-3, 1e-3 };
                for (int side = 0; side < 4; ++side) {
                    const double h = steps[side];
                    double dl[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
                    dl[d] = h;
                    const double D[9] = { 1.0 + dl[6], dl[0], dl[1], dl[2], 1.0 + dl[7], dl[3], dl[4], dl[5], 1.0 - dl[6] - dl[7] };
                    double GD[9];
                    srk_homog_mul3(noisy.G, D, GD);
                    SrkHomogModel p;
                    for (int c = 0; c < 9; ++c) p.G[c] = GD[c]; // not normalised: the residuals do not depend on the scale
                    srk_homog_complete(p);
                    double y2[3], x2[3];
                    srk_homog_transfer(p, e, F0, y2, x2, res[side], res[side] + 2);
                }
                double num[4];
                for (int c = 0; c < 4; ++c) num[c] = (4.0 * (res[3][c] - res[2][c]) / 2e-3 - (res[1][c] - res[0][c]) / 4e-3) / 3.0;
                const double ana[4] = { Jf[d], Jf[8 + d], Jb[d], Jb[8 + d] };
                for (int c = 0; c < 4; ++c) jworst = std::fmax(jworst, std::fabs(num[c] - ana[c]) / (1.0 + std::fabs(ana[c])));
            }
        }
        expect(jworst <= 1e-9, "the Jacobians agree with central differences to 1e-9");
        // one round from the disturbed model returns to the plane's: the step solves its normal equations
        double acc[SRK_HOMOG_ACC] = { 0 };
        for (int k = 0; k < 40; ++k) {
            const double e[5] = { ua[2 * k], ua[2 * k + 1], ub[2 * k], ub[2 * k + 1], 1.0 };
            srk_homog_accumulate(acc, noisy, e, F0);
        }
        SrkHomogModel c1, c2;
        expect(srk_homog_step(acc, noisy, c1) == 1, "the step stands");
        for (int e = 0; e < SRK_HOMOG_ACC; ++e) acc[e] = 0.0;
        for (int k = 0; k < 40; ++k) {
            const double e[5] = { ua[2 * k], ua[2 * k + 1], ub[2 * k], ub[2 * k + 1], 1.0 };
            srk_homog_accumulate(acc, c1, e, F0);
        }
        expect(srk_homog_step(acc, c1, c2) == 1, "and the next");
        expect(max_abs_diff(c2.G, m.G, 9) <= 1e-9, "two Gauss-Newton steps return to the noise-free model");
        double bad[SRK_HOMOG_ACC] = { 0 };
        expect(srk_homog_step(bad, noisy, c1) == 0, "a zero system fails the factorisation");
    }
    // the decomposition: H = R + (T/d) N^T, one candidate the truth
    {
        const double nn = std::sqrt(0.2 * 0.2 + 0.1 * 0.1 + 1.0), N[3] = { -0.2 / nn, 0.1 / nn, 1.0 / nn }, d = 6.0 / nn;
        double H[9], xa[120], xb[120], Kai[9], Kbi[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) H[3 * i + j] = -2.5 * (R[3 * i + j] + T[i] * N[j] / d); // any scale, any sign
        srk_homog_inv3(KA, Kai);
        srk_homog_inv3(KB, Kbi);
        for (int k = 0; k < 40; ++k) {
            const double p[3] = { ua[2 * k], ua[2 * k + 1], F0 }, p2[3] = { ub[2 * k], ub[2 * k + 1], F0 };
            srk_homog_mulv(Kai, p, xa + 3 * k);
            srk_homog_mulv(Kbi, p2, xb + 3 * k);
        }
        double Ho[9], Rr[18], Tt[6], Nn[6], gap;
        int32_t front[2];
        expect(srk_homography_decompose(H, 40, xa, xb, nullptr, Ho, Rr, Tt, Nn, front, &gap) == 2, "a plane has two poses");
        int hits = 0;
        for (int k = 0; k < 2; ++k) {
            check_rotation(Rr + 9 * k, "a candidate's R is a proper rotation");
            double rec[9];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) rec[3 * i + j] = Rr[9 * k + 3 * i + j] + Tt[3 * k + i] * Nn[3 * k + j];
            expect(max_abs_diff(rec, Ho, 9) <= 1e-13, "H = R + (T/d) N^T");
            const double Td[3] = { T[0] / d, T[1] / d, T[2] / d };
            hits += max_abs_diff(Rr + 9 * k, R, 9) <= 1e-12 && max_abs_diff(Tt + 3 * k, Td, 3) <= 1e-12 && max_abs_diff(Nn + 3 * k, N, 3) <= 1e-12;
        }
        expect(hits == 1 && front[0] == 40, "exactly one candidate is the truth, every ray in front");
        // without a baseline: the rotation alone
        double Hr[9];
        for (int e = 0; e < 9; ++e) Hr[e] = 3.0 * R[e];
        std::vector<double> ra, rb;
        make_pair(g, 40, false, R, zero, ra, rb);
        for (int k = 0; k < 40; ++k) {
            const double p[3] = { ra[2 * k], ra[2 * k + 1], F0 }, p2[3] = { rb[2 * k], rb[2 * k + 1], F0 };
            srk_homog_mulv(Kai, p, xa + 3 * k);
            srk_homog_mulv(Kbi, p2, xb + 3 * k);
        }
        expect(srk_homography_decompose(Hr, 40, xa, xb, nullptr, Ho, Rr, Tt, Nn, front, &gap) == 1 && gap <= 1e-10, "a rotation has one");
        expect(max_abs_diff(Rr, R, 9) <= 1e-13 && max_abs_diff(Ho, R, 9) <= 1e-13, "and it is the rotation");
        bool zeros = front[0] == 0 && front[1] == 0;
        for (int e = 0; e < 6; ++e) zeros = zeros && Tt[e] == 0.0 && Nn[e] == 0.0;
        for (int e = 9; e < 18; ++e) zeros = zeros && Rr[e] == 0.0;
        expect(zeros, "unused entries are zero");
        expect(srk_homography_decompose(nullptr, 40, xa, xb, nullptr, Ho, Rr, Tt, Nn, front, &gap) == SRK_E_ARGS, "NULL H is refused");
        Hr[4] = nan;
        expect(srk_homography_decompose(Hr, 40, xa, xb, nullptr, Ho, Rr, Tt, Nn, front, &gap) == SRK_E_ARGS, "and one that is not finite");
    }
    // ---- three walks: the plane, too few matches, collinear matches
    {
        double Gw[9], Hw[9], Rw[18], Tw[6], Nw[6], hg[8];
        int32_t poses, front[2];
        std::vector<uint8_t> inl(40);
        int rc = srk_homography_host_pair(40, ua.data(), ub.data(), nullptr, KA, KB, F0, nullptr, Gw, Hw, &poses, Rw, Tw, Nw, front, hg, inl.data());
        expect(rc == 0 && poses == 2 && hg[1] == 40 && hg[2] == 40 && hg[0] <= 1e-9, "the walk of a plane");
        expect(max_abs_diff(Gw, m.G, 9) <= 1e-10, "finds the plane's homography");
        bool all = true;
        for (uint8_t f : inl) all = all && f == 1;
        expect(all, "with every match an inlier");
        rc = srk_homography_host_pair(3, ua.data(), ub.data(), nullptr, KA, KB, F0, nullptr, Gw, Hw, &poses, Rw, Tw, Nw, front, hg, inl.data());
        expect(rc == SRK_HOMOGRAPHY_FEW_POINTS && poses == 0 && Gw[0] == 1.0 && Gw[1] == 0.0 && std::isnan(hg[0]) && hg[1] == 3 && hg[2] == 0,
               "three matches are too few");
        const double qz[5] = { 1, 1, 0, 1, 0 };
        rc = srk_homography_host_pair(5, ua.data(), ub.data(), qz, KA, KB, F0, nullptr, Gw, Hw, &poses, Rw, Tw, Nw, front, hg, inl.data());
        expect(rc == SRK_HOMOGRAPHY_FEW_POINTS && hg[1] == 3, "matches of q = 0 do not count");
        double line[8] = { 100, 100, 200, 150, 300, 200, 400, 250 };
        rc = srk_homography_host_pair(4, line, ub.data(), nullptr, KA, KB, F0, nullptr, Gw, Hw, &poses, Rw, Tw, Nw, front, hg, inl.data());
        expect(rc == SRK_HOMOGRAPHY_NO_MODEL && poses == 0 && hg[4] == 0 && std::isnan(hg[3]) && Hw[0] == 1.0, "collinear matches have no model");
        expect(srk_homography_host_pair(4, line, ub.data(), nullptr, KA, KB, nan, nullptr, Gw, Hw, &poses, Rw, Tw, Nw, front, hg, nullptr) == SRK_E_ARGS,
               "f0 must be finite");
        expect(srk_homography_host_pair(4, line, ub.data(), nullptr, KA, KB, F0, nullptr, nullptr, Hw, &poses, Rw, Tw, Nw, front, hg, nullptr) == SRK_E_ARGS,
               "NULL outputs are refused");
    }
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}

std::vector<char> slurp(const char* path)
{
    std::vector<char> out;
    if (FILE* f = std::fopen(path, "rb")) {
        char buf[65536];
        size_t got;
        while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + got);
        std::fclose(f);
    }
    return out;
}
} // namespace

int main(int argc, char** argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "unit")) return unit();
    if (argc == 6 && !std::strcmp(argv[1], "sampler")) {
        const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
        const int64_t n = std::strtoll(argv[4], nullptr, 10), H = std::strtoll(argv[5], nullptr, 10);
        std::vector<int64_t> out((size_t)(4 * H));
        for (int64_t h = 0; h < H; ++h) srk_homog_sample(seed, (uint32_t)h, n, out[4 * h], out[4 * h + 1], out[4 * h + 2], out[4 * h + 3]);
        FILE* f = std::fopen(argv[2], "wb");
        if (!f) return 2;
        std::fwrite(out.data(), 8, out.size(), f);
        return std::fclose(f) ? 2 : 0;
    }
    if (argc == 4 && (!std::strcmp(argv[1], "model") || !std::strcmp(argv[1], "eig"))) {
        const std::vector<char> in = slurp(argv[2]);
        if (in.size() < 8) return 2;
        int64_t n;
        std::memcpy(&n, in.data(), 8);
        FILE* f = std::fopen(argv[3], "wb");
        if (!f) return 2;
        if (argv[1][0] == 'm') {
            if (n < 0 || in.size() != (size_t)(16 + 128 * n)) return 2;
            double f0;
            std::memcpy(&f0, in.data() + 8, 8);
            std::vector<double> uv((size_t)(16 * n)), G((size_t)(9 * n));
            std::vector<int32_t> ok((size_t)n);
            std::memcpy(uv.data(), in.data() + 16, (size_t)(128 * n));
            for (int64_t i = 0; i < n; ++i) {
                double pa[12], pb[12];
                for (int k = 0; k < 4; ++k) {
                    pa[3 * k] = uv[8 * i + 2 * k], pa[3 * k + 1] = uv[8 * i + 2 * k + 1], pa[3 * k + 2] = f0;
                    pb[3 * k] = uv[8 * (n + i) + 2 * k], pb[3 * k + 1] = uv[8 * (n + i) + 2 * k + 1], pb[3 * k + 2] = f0;
                }
                SrkHomogModel m;
                ok[(size_t)i] = srk_homog_hypothesis(pa, pb, m);
                std::memcpy(&G[(size_t)(9 * i)], m.G, sizeof m.G);
            }
            std::fwrite(G.data(), 8, G.size(), f);
            std::fwrite(ok.data(), 4, ok.size(), f);
        } else {
            if (n < 0 || in.size() != (size_t)(8 + 72 * n)) return 2;
            std::vector<double> A((size_t)(9 * n)), out((size_t)(3 * n));
            std::memcpy(A.data(), in.data() + 8, (size_t)(72 * n));
            for (int64_t i = 0; i < n; ++i) {
                double S[3][3], V[3][3], lam[3];
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c) S[r][c] = A[(size_t)(9 * i + 3 * r + c)];
                srk_homog_jacobi3(S, V, lam);
                std::sort(lam, lam + 3);
                std::memcpy(&out[(size_t)(3 * i)], lam, sizeof lam);
            }
            std::fwrite(out.data(), 8, out.size(), f);
        }
        return std::fclose(f) ? 2 : 0;
    }
    std::fprintf(stderr, "usage: test_homog_host unit | sampler OUT SEED N H | model IN OUT | eig IN OUT\n");
    return 2;
}
