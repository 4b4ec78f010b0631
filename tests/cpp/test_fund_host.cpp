// test_fund_host.cpp -- the host half of the two-view fundamental matrix (surikatoko_amd/csrc/srk_fund.cpp) and its math header
// without a GPU, driven by tests/test_fundamental_cpu.py.  Built with the host compiler alone:
//   c++ -std=c++17 tests/cpp/test_fund_host.cpp surikatoko_amd/csrc/srk_fund.cpp
// Usage:
//   test_fund_host unit               the argument checks, the option defaults, the Jacobian against central differences, the 7 x 7
//                                     Cholesky step, the representation (sigma = 1 and sigma near 0 included), the cubic with a
//                                     vanishing leading coefficient and three walks; exit status 0 = all hold
//   test_fund_host sampler OUT S N H  the ranks of hypotheses 0 .. H - 1 among N matches under seed S: int64 [H][8]
//   test_fund_host model IN OUT       IN: int64 n, double f0, uv_a [n][8][2], uv_b [n][8][2] (seven matches and the eighth that
//                                     chooses); OUT: F [n][9], int32 roots [n], int32 ok [n]
#include "../../surikatoko_amd/csrc/srk_fund.hpp"
#include "../../surikatoko_amd/csrc/srk_fund_math.hpp"

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

void pixel(const double* K, const double* x, double* uv)
{
    double p[3];
    srk_homog_mulv(K, x, p);
    uv[0] = F0 * p[0] / p[2], uv[1] = F0 * p[1] / p[2];
}

// n matches of a pair: points anywhere (or on the plane z = 6 + 0.2 x - 0.1 y) seen from (I, 0) and (R, T)
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
            for (int k = 0; k < 3; ++k) d += R[3 * k + i] * R[3 * k + j];
            worst = std::fmax(worst, std::fabs(d - (i == j ? 1.0 : 0.0)));
        }
    expect(worst <= 1e-13 && std::fabs(srk_homog_det3(R) - 1.0) <= 1e-13, what);
}

SrkFundRep random_rep(Lcg& g, double sigma)
{
    SrkFundRep r;
    const double a[3] = { 2.0 * g.next(), 2.0 * g.next(), 2.0 * g.next() }, b[3] = { 2.0 * g.next(), 2.0 * g.next(), 2.0 * g.next() };
    srk_resect_exp(a, r.U);
    srk_resect_exp(b, r.V);
    r.sigma = sigma;
    return r;
}

void check_arguments()
{
    const int64_t rp[3] = { 0, 9, 18 }, down[3] = { 0, 9, 5 }, off[2] = { 1, 9 };
    std::vector<double> ua(36, 10.0), ub(36, 20.0), q(18, 1.0);
    srk_fundamental_options o;
    srk_fundamental_default_options(&o);
    expect(o.hypotheses == 256 && o.inlier_pixels == 2.0 && o.seed == 1 && o.refine_rounds == 8, "the option defaults");
    expect(srk_fund_check(2, rp, ua.data(), ub.data(), q.data(), &o).empty(), "a good call passes");
    expect(srk_fund_check(2, rp, ua.data(), ub.data(), nullptr, nullptr).empty(), "q and the options may be NULL");
    expect(srk_fund_check(0, rp, nullptr, nullptr, nullptr, &o).empty(), "no pairs pass");
    expect(refused(srk_fund_check(-1, rp, ua.data(), ub.data(), nullptr, &o), "negative pair count"), "a negative pair count");
    expect(refused(srk_fund_check(2, nullptr, ua.data(), ub.data(), nullptr, &o), "row_ptr is NULL"), "row_ptr NULL");
    srk_fundamental_options b = o;
    b.hypotheses = 0;
    expect(refused(srk_fund_check(2, rp, ua.data(), ub.data(), nullptr, &b), "hypotheses outside 1..4096"), "no hypotheses");
    b.hypotheses = 4097;
    expect(refused(srk_fund_check(2, rp, ua.data(), ub.data(), nullptr, &b), "hypotheses outside 1..4096"), "too many hypotheses");
    b = o, b.inlier_pixels = 0.0;
    expect(refused(srk_fund_check(2, rp, ua.data(), ub.data(), nullptr, &b), "inlier_pixels"), "tau = 0");
    b.inlier_pixels = std::numeric_limits<double>::infinity();
    expect(refused(srk_fund_check(2, rp, ua.data(), ub.data(), nullptr, &b), "inlier_pixels"), "tau infinite");
    b = o, b.refine_rounds = -1;
    expect(refused(srk_fund_check(2, rp, ua.data(), ub.data(), nullptr, &b), "refine_rounds outside 0..16"), "negative rounds");
    b.refine_rounds = 17;
    expect(refused(srk_fund_check(2, rp, ua.data(), ub.data(), nullptr, &b), "refine_rounds outside 0..16"), "17 rounds");
    b = o, b.hypotheses = 4096;
    {
        std::vector<int64_t> many((size_t)(1 << 16) + 2, 0);
        expect(refused(srk_fund_check((1 << 16) + 1, many.data(), nullptr, nullptr, nullptr, &b), "split the batch"), "too many waves");
    }
    expect(refused(srk_fund_check(1, off, ua.data(), ub.data(), nullptr, &o), "row_ptr[0] != 0"), "row_ptr[0]");
    expect(refused(srk_fund_check(2, down, ua.data(), ub.data(), nullptr, &o), "row_ptr decreases at pair 1"), "a descending row_ptr");
    expect(refused(srk_fund_check(2, rp, nullptr, ub.data(), nullptr, &o), "a NULL match array"), "uv_a NULL");
    expect(refused(srk_fund_check(2, rp, ua.data(), nullptr, nullptr, &o), "a NULL match array"), "uv_b NULL");
    ua[7] = std::numeric_limits<double>::quiet_NaN();
    expect(refused(srk_fund_check(2, rp, ua.data(), ub.data(), nullptr, &o), "uv_a of match 3 is not finite"), "uv_a NaN");
    ua[7] = 10.0, ub[10] = std::numeric_limits<double>::infinity();
    expect(refused(srk_fund_check(2, rp, ua.data(), ub.data(), nullptr, &o), "uv_b of match 5 is not finite"), "uv_b infinite");
    ub[10] = 20.0, q[4] = -1.0;
    expect(refused(srk_fund_check(2, rp, ua.data(), ub.data(), q.data(), &o), "q of match 4"), "q negative");
    q[4] = std::numeric_limits<double>::quiet_NaN();
    expect(refused(srk_fund_check(2, rp, ua.data(), ub.data(), q.data(), &o), "q of match 4"), "q NaN");
    const char* why = nullptr;
    q[4] = 1.0;
    expect(srk_fundamental_check_pairs(2, rp, ua.data(), ub.data(), q.data(), &o, &why) == SRK_OK && why && !*why, "the C entry point passes");
    expect(srk_fundamental_check_pairs(2, down, ua.data(), ub.data(), q.data(), &o, &why) == SRK_E_ARGS && why && std::strstr(why, "decreases"),
           "the C entry point refuses with a text");
    double F[9], U[9], V[9], sg, fd[12], info[49];
    expect(srk_fundamental_host_pair(9, ua.data(), ub.data(), nullptr, 0.0, &o, F, U, V, &sg, fd, info, nullptr) == SRK_E_ARGS, "f0 = 0");
    expect(srk_fundamental_host_pair(9, ua.data(), ub.data(), nullptr, F0, &o, nullptr, U, V, &sg, fd, info, nullptr) == SRK_E_ARGS, "a NULL output");
}

void check_jacobian(Lcg& g)
{
    const double sigmas[4] = { 0.7, 1.0, 1e-6, 0.3 };
    double worst = 0.0;
    for (double sigma : sigmas) {
        const SrkFundRep r = random_rep(g, sigma);
        SrkFundLin lin;
        srk_fund_linearise(r, lin);
        for (int m = 0; m < 5; ++m) {
            const double ua = 300.0 + 300.0 * g.next(), va = 240.0 + 240.0 * g.next(), ub = 300.0 + 300.0 * g.next(), vb = 240.0 + 240.0 * g.next();
            double J[SRK_FUND_NV];
            const double r0 = srk_fund_row(lin, ua, va, ub, vb, F0, J);
            double scale = std::fabs(r0);
            for (int k = 0; k < SRK_FUND_NV; ++k) scale = std::fmax(scale, std::fabs(J[k]));
            for (int k = 0; k < SRK_FUND_NV; ++k) {
                double res[2];
                for (int s = 0; s < 2; ++s) {
                    double d[SRK_FUND_NV] = { 0 };
                    d[k] = s == 0 ? 1e-6 : -1e-6;
                    // the move without the canonical exchange, which is no smooth function of d at sigma = 1
                    SrkFundRep n;
                    double Xa[9], Xb[9], Jn[SRK_FUND_NV];
                    srk_resect_exp(d, Xa);
                    srk_resect_exp(d + 3, Xb);
                    srk_homog_mul3(r.U, Xa, n.U);
                    srk_homog_mul3(r.V, Xb, n.V);
                    n.sigma = r.sigma + d[6];
                    SrkFundLin ln;
                    srk_fund_linearise(n, ln);
                    res[s] = srk_fund_row(ln, ua, va, ub, vb, F0, Jn);
                }
                worst = std::fmax(worst, std::fabs((res[0] - res[1]) / 2e-6 - J[k]) / scale);
            }
        }
    }
    std::fprintf(stderr, "jacobian against central differences: %.3e relative\n", worst);
    expect(worst <= 1e-7, "the Jacobian against central differences (step 1e-6: truncation 1e-12, rounding 1e-10 of the row's scale)");
}

void check_cholesky(Lcg& g)
{
    double acc[SRK_FUND_ACC] = { 0 }, A[7][7] = { { 0 } };
    for (int m = 0; m < 20; ++m) {
        double J[7];
        for (int k = 0; k < 7; ++k) J[k] = g.next();
        const double r = g.next();
        int at = 0;
        for (int a = 0; a < 7; ++a) {
            for (int b = a; b < 7; ++b) acc[at++] += J[a] * J[b];
            acc[SRK_FUND_NH + a] += J[a] * r;
        }
    }
    srk_fund_full(acc, A);
    const double c = 1e-4;
    double d[7];
    expect(srk_fund_lm_step(acc, c, d) == 1, "a positive definite system factors");
    double worst = 0.0;
    for (int a = 0; a < 7; ++a) {
        double s = acc[SRK_FUND_NH + a] + c * A[a][a] * d[a];
        for (int b = 0; b < 7; ++b) s += A[a][b] * d[b];
        worst = std::fmax(worst, std::fabs(s));
    }
    expect(worst <= 1e-12, "(H + c diag H) d = -g");
    double bad[SRK_FUND_ACC];
    std::memcpy(bad, acc, sizeof bad);
    bad[0] = -1.0;
    expect(srk_fund_lm_step(bad, c, d) == 0, "a negative pivot fails");
    bad[0] = std::numeric_limits<double>::quiet_NaN();
    expect(srk_fund_lm_step(bad, c, d) == 0, "a NaN fails");
    double B[7][7];
    srk_fund_full(acc, B);
    const double cond = srk_fund_cond1(B, std::numeric_limits<double>::quiet_NaN());
    expect(std::isfinite(cond) && cond >= 1.0, "cond_1 of a positive definite H");
    double Z[7][7] = { { 0 } };
    expect(std::isnan(srk_fund_cond1(Z, std::numeric_limits<double>::quiet_NaN())), "cond_1 of zero is NaN");
}

void check_representation(Lcg& g)
{
    const double sigmas[6] = { 0.6, 1.0, 1e-9, 0.0, 0.999999999, 0.05 };
    for (double sigma : sigmas)
        for (int sign = 0; sign < 2; ++sign) {
            const SrkFundRep r = random_rep(g, sigma);
            double F[9], G[9];
            srk_fund_build(r, F);
            for (int e = 0; e < 9; ++e) F[e] *= sign ? -3.0 : 2.0; // any scale and sign
            SrkFundRep got;
            expect(srk_fund_represent(F, got) == 1, "a finite F has a representation");
            check_rotation(got.U, "U is a proper rotation");
            check_rotation(got.V, "V is a proper rotation");
            expect(got.sigma >= 0.0 && got.sigma <= 1.0, "0 <= sigma <= 1");
            expect(std::fabs(got.sigma - sigma) <= 1e-12, "sigma is kept, a small one to its digits");
            srk_fund_build(got, G);
            double n = 0.0, dot = 0.0;
            for (int e = 0; e < 9; ++e) n += F[e] * F[e], dot += F[e] * G[e];
            const double sg = dot < 0.0 ? -1.0 : 1.0;
            for (int e = 0; e < 9; ++e) F[e] *= sg / std::sqrt(n);
            expect(max_abs_diff(F, G, 9) <= 1e-13, "F = U diag(1, sigma, 0) V^T up to scale and sign");
            srk_fund_sign(got, G);
            double big = 0.0, val = 0.0, H[9];
            for (int e = 0; e < 9; ++e)
                if (std::fabs(G[e]) > big) big = std::fabs(G[e]), val = G[e];
            expect(val > 0.0, "the largest entry is positive");
            check_rotation(got.U, "U stays proper under the sign");
            srk_fund_build(got, H);
            expect(max_abs_diff(G, H, 9) <= 1e-15, "the signed F is still U diag(1, sigma, 0) V^T");
            // the epipoles
            const double v3[3] = { got.V[2], got.V[5], got.V[8] }, u3[3] = { got.U[2], got.U[5], got.U[8] };
            double fv[3], Gt[9], fu[3];
            srk_homog_mulv(G, v3, fv);
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) Gt[3 * i + j] = G[3 * j + i];
            srk_homog_mulv(Gt, u3, fu);
            expect(std::sqrt(srk_align_dot(fv, fv)) <= 1e-15 && std::sqrt(srk_align_dot(fu, fu)) <= 1e-15, "F v_3 = 0 and F^T u_3 = 0");
        }
    // the canonical form after a move: sigma above 1 and below 0
    SrkFundRep r = random_rep(g, 0.9), n;
    double d[7] = { 0, 0, 0, 0, 0, 0, 0.3 }, F[9], G[9];
    srk_fund_move(r, d, n);
    expect(n.sigma > 0.0 && n.sigma <= 1.0 && std::fabs(n.sigma - 1.0 / 1.2) <= 1e-15, "sigma above 1 is exchanged");
    check_rotation(n.U, "U proper after the exchange");
    check_rotation(n.V, "V proper after the exchange");
    r.sigma = 1.2;
    srk_fund_build(r, F);
    srk_fund_build(n, G);
    expect(max_abs_diff(F, G, 9) <= 1e-15, "the exchange keeps F");
    r.sigma = 0.1, d[6] = -0.3;
    srk_fund_move(r, d, n);
    expect(std::fabs(n.sigma - 0.2) <= 1e-15, "a negative sigma is turned round");
    check_rotation(n.U, "U proper after the turn");
    r.sigma = -0.2;
    srk_fund_build(r, F);
    srk_fund_build(n, G);
    expect(max_abs_diff(F, G, 9) <= 1e-15, "the turn keeps F");
}

void check_cubic()
{
    double z[3];
    const double three[4] = { -6.0, 11.0, -6.0, 1.0 }; // (z - 1)(z - 2)(z - 3)
    expect(srk_fund_roots(three, z) == 3 && std::fabs(z[0] - 1.0) <= 1e-14 && std::fabs(z[1] - 2.0) <= 1e-14 && std::fabs(z[2] - 3.0) <= 1e-14,
           "three real roots in ascending order");
    const double one[4] = { -2.0, 1.0, -2.0, 1.0 }; // (z - 2)(z^2 + 1)
    expect(srk_fund_roots(one, z) == 1 && std::fabs(z[0] - 2.0) <= 1e-14, "one real root");
    const double neg[4] = { 2.0, -1.0, 2.0, -1.0 };
    expect(srk_fund_roots(neg, z) == 1 && std::fabs(z[0] - 2.0) <= 1e-14, "a negative leading coefficient");
    const double quad[4] = { 2.0, -3.0, 1.0, 0.0 }; // (z - 1)(z - 2)
    expect(srk_fund_roots(quad, z) == 2 && std::fabs(z[0] - 1.0) <= 1e-14 && std::fabs(z[1] - 2.0) <= 1e-14, "a vanishing leading coefficient: the quadratic");
    const double tiny[4] = { 2.0, -3.0, 1.0, 1e-17 };
    expect(srk_fund_roots(tiny, z) == 2 && std::fabs(z[0] - 1.0) <= 1e-14 && std::fabs(z[1] - 2.0) <= 1e-14, "a leading coefficient at rounding: the quadratic");
    const double none[4] = { 1.0, 0.0, 1.0, 0.0 };
    expect(srk_fund_roots(none, z) == 0, "a quadratic without a real root");
    const double line[4] = { -4.0, 2.0, 0.0, 0.0 };
    expect(srk_fund_roots(line, z) == 1 && std::fabs(z[0] - 2.0) <= 1e-14, "two vanishing coefficients: the line");
    const double zero[4] = { 0.0, 0.0, 0.0, 0.0 };
    expect(srk_fund_roots(zero, z) == 0, "the zero polynomial has no root to offer");
    // the cubic of two matrices against det at a point
    const double A[9] = { 1, 2, 0.5, -1, 0.3, 2, 0.7, 1, -1 }, B[9] = { 0.2, -1, 1, 1, 0.5, 0, 2, -0.3, 0.4 };
    double c[4], M[9];
    srk_fund_cubic(A, B, c);
    for (int e = 0; e < 9; ++e) M[e] = A[e] + 0.7 * B[e];
    expect(std::fabs(((c[3] * 0.7 + c[2]) * 0.7 + c[1]) * 0.7 + c[0] - srk_homog_det3(M)) <= 1e-13, "det(F1 + z F2) from the minors");
}

void check_walks(Lcg& g)
{
    const double w[3] = { 0.05, -0.2, 0.1 }, T[3] = { 0.8, -0.1, 0.3 };
    double R[9];
    srk_resect_exp(w, R);
    srk_fundamental_options o;
    srk_fundamental_default_options(&o);
    o.hypotheses = 64;
    std::vector<double> ua, ub;
    SrkFundResult out;
    make_pair(g, 40, false, R, T, ua, ub);
    std::vector<uint8_t> inl(40);
    expect(srk_fund_host_walk(40, ua.data(), ub.data(), nullptr, F0, o, out, inl.data()) == 0, "a general pair has a model");
    expect(std::count(inl.begin(), inl.end(), 1) == 40 && out.fund[2] == 40.0 && out.fund[0] <= 1e-8, "every noise-free match is an inlier");
    // the truth K_b^-T [T]x R K_a^-1
    double E[9], Ft[9], Kai[9], Kbi[9];
    srk_relate_essential(R, T, E);
    srk_relate_inverse3(KA, Kai);
    srk_relate_inverse3(KB, Kbi);
    srk_relate_fundamental(Kai, Kbi, E, Ft);
    double n = 0.0, dot = 0.0;
    for (int e = 0; e < 9; ++e) n += Ft[e] * Ft[e], dot += Ft[e] * out.F[e];
    for (int e = 0; e < 9; ++e) Ft[e] *= (dot < 0.0 ? -1.0 : 1.0) / std::sqrt(n);
    expect(max_abs_diff(Ft, out.F, 9) <= 1e-9, "F is the truth");
    check_rotation(out.U, "the walk's U");
    check_rotation(out.V, "the walk's V");
    make_pair(g, 40, true, R, T, ua, ub);
    expect(srk_fund_host_walk(40, ua.data(), ub.data(), nullptr, F0, o, out, inl.data()) == SRK_FUNDAMENTAL_NO_MODEL, "a noise-free plane has no model");
    expect(out.fund[4] == 0.0 && std::isnan(out.fund[0]) && out.sigma == 0.0 && out.U[0] == 1.0 && out.F[0] == 0.0, "and the outputs of none");
    expect(srk_fund_host_walk(7, ua.data(), ub.data(), nullptr, F0, o, out, inl.data()) == SRK_FUNDAMENTAL_FEW_POINTS, "seven matches are too few");
}
} // namespace

int main(int argc, char** argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "unit")) {
        Lcg g;
        check_arguments();
        check_jacobian(g);
        check_cholesky(g);
        check_representation(g);
        check_cubic();
        check_walks(g);
        std::printf("%d failure(s)\n", failures);
        return failures ? 1 : 0;
    }
    if (argc == 6 && !std::strcmp(argv[1], "sampler")) {
        const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
        const int64_t n = std::atoll(argv[4]), H = std::atoll(argv[5]);
        std::vector<int64_t> out((size_t)(8 * H));
        for (int64_t h = 0; h < H; ++h) srk_fund_sample(seed, (uint32_t)h, n, &out[(size_t)(8 * h)]);
        FILE* f = std::fopen(argv[2], "wb");
        if (!f || std::fwrite(out.data(), 8, out.size(), f) != out.size()) return 2;
        std::fclose(f);
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "model")) {
        FILE* f = std::fopen(argv[2], "rb");
        int64_t n = 0;
        double f0 = 0.0;
        if (!f || std::fread(&n, 8, 1, f) != 1 || std::fread(&f0, 8, 1, f) != 1 || n < 0) return 2;
        std::vector<double> ua((size_t)(16 * n)), ub((size_t)(16 * n)), F((size_t)(9 * n));
        std::vector<int32_t> roots((size_t)n), ok((size_t)n);
        if (std::fread(ua.data(), 8, ua.size(), f) != ua.size() || std::fread(ub.data(), 8, ub.size(), f) != ub.size()) return 2;
        std::fclose(f);
        for (int64_t i = 0; i < n; ++i) {
            double pa[21], pb[21];
            for (int k = 0; k < 7; ++k) {
                pa[3 * k] = ua[(size_t)(16 * i + 2 * k)] / f0, pa[3 * k + 1] = ua[(size_t)(16 * i + 2 * k + 1)] / f0, pa[3 * k + 2] = 1.0;
                pb[3 * k] = ub[(size_t)(16 * i + 2 * k)] / f0, pb[3 * k + 1] = ub[(size_t)(16 * i + 2 * k + 1)] / f0, pb[3 * k + 2] = 1.0;
            }
            const double e8[4] = { ua[(size_t)(16 * i + 14)], ua[(size_t)(16 * i + 15)], ub[(size_t)(16 * i + 14)], ub[(size_t)(16 * i + 15)] };
            double err8;
            int nr;
            ok[(size_t)i] = srk_fund_hypothesis(pa, pb, e8, f0, &F[(size_t)(9 * i)], err8, nr);
            roots[(size_t)i] = nr;
        }
        f = std::fopen(argv[3], "wb");
        if (!f || std::fwrite(F.data(), 8, F.size(), f) != F.size() || std::fwrite(roots.data(), 4, roots.size(), f) != roots.size() ||
            std::fwrite(ok.data(), 4, ok.size(), f) != ok.size())
            return 2;
        std::fclose(f);
        return 0;
    }
    std::fprintf(stderr, "usage: test_fund_host unit | sampler OUT S N H | model IN OUT\n");
    return 2;
}
