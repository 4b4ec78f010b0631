// Runtime test of BundleAdjustmentKanatani::RelateUncalibrated (include/suriko_amd/bundle-adj-kanatani.hpp): two general pairs with a
// fifth of the targets wrong give the C ABI's bits on the same handle, mark no wrong match an inlier, return the true fundamental
// matrix and epipoles; a planar pair has no model; refusals of the library throw std::invalid_argument with the check's text.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "suriko_amd/bundle-adj-kanatani.hpp"
using namespace suriko_amd;

static std::string refusal;
template <typename F> static bool throws_invalid(F f)
{
    try { f(); } catch (const std::invalid_argument& e) { refusal = e.what(); return true; }
    return false;
}

static Point2f pixel(const Matrix3& K, const double* x, double f0)
{
    const double p[3] = { K[0] * x[0] + K[1] * x[1] + K[2] * x[2], K[3] * x[0] + K[4] * x[1] + K[5] * x[2], K[6] * x[0] + K[7] * x[1] + K[8] * x[2] };
    return { f0 * p[0] / p[2], f0 * p[1] / p[2] };
}

int main()
{
    using BA = BundleAdjustmentKanatani;
    const double f0 = 600.0, c = std::cos(0.15), sn = std::sin(0.15);
    const Matrix3 Ka{ 1.25, 0, 0.53, 0, 1.3, 0.4, 0, 0, 1 }, Kb{ 1.1, 0.01, 0.5, 0, 1.15, 0.42, 0, 0, 1 };
    const Matrix3 Rt{ c, 0, sn, 0, 1, 0, -sn, 0, c };
    const double Tt[3] = { 0.6, -0.2, 0.3 };
    uint64_t x = 99;
    auto next = [&x] { x = x * 6364136223846793005ull + 1442695040888963407ull; return (double)(x >> 11) / 4503599627370496.0 - 1.0; };
    std::vector<std::vector<BA::Match>> pairs(3);
    for (int p = 0; p < 3; ++p)
        for (int i = 0; i < 100 + 30 * p; ++i) {
            double X[3] = { 2 * next(), 1.5 * next(), 6 + 2 * next() }, Y[3];
            if (p == 2) X[2] = 6 + 0.2 * X[0] - 0.1 * X[1]; // the third pair lies on a plane
            for (int r = 0; r < 3; ++r) Y[r] = Rt[3 * r] * X[0] + Rt[3 * r + 1] * X[1] + Rt[3 * r + 2] * X[2] + Tt[r];
            BA::Match m;
            m.a = pixel(Ka, X, f0);
            m.b = pixel(Kb, Y, f0);
            if (p < 2 && i % 5 == p) m.b.y += 40.0 + 3.0 * (i % 7); // a wrong match
            pairs[(size_t)p].push_back(m);
        }
    pairs[1][7].information = 0; // and one switched off
    srk_fundamental_options lo;
    srk_fundamental_default_options(&lo);
    lo.hypotheses = 512;
    lo.inlier_pixels = 0.01;
    BA ba;
    const std::vector<BA::UncalibratedPair> res = ba.RelateUncalibrated(f0, pairs, &lo, true);
    if (res.size() != 3) return 12;

    // the C ABI on the same handle: the same bits
    std::vector<int64_t> rp{ 0 };
    std::vector<double> ua, ub, q, F(27), U(27), V(27), sg(3), fd(36), info(147);
    std::vector<uint32_t> st(3);
    for (int p = 0; p < 3; ++p) {
        for (const BA::Match& m : pairs[(size_t)p]) {
            ua.insert(ua.end(), { m.a.x, m.a.y });
            ub.insert(ub.end(), { m.b.x, m.b.y });
            q.push_back(m.information);
        }
        rp.push_back((int64_t)q.size());
    }
    std::vector<uint8_t> ci(q.size());
    if (srk_relate_uncalibrated(ba.Handle(), f0, 3, rp.data(), ua.data(), ub.data(), q.data(), &lo, F.data(), U.data(), V.data(), sg.data(), fd.data(),
                                info.data(), st.data(), ci.data()) != 0)
        return 13;
    for (int p = 0; p < 3; ++p) {
        const BA::UncalibratedPair& r = res[(size_t)p];
        if (std::memcmp(r.F.data(), F.data() + 9 * p, 72) || std::memcmp(r.U.data(), U.data() + 9 * p, 72) || std::memcmp(r.V.data(), V.data() + 9 * p, 72) ||
            std::memcmp(&r.sigma, &sg[(size_t)p], 8) || std::memcmp(r.information.data(), info.data() + 49 * p, 392))
            return 14;
        if (std::memcmp(&r.rms_pixels, &fd[12 * p], 8) || std::memcmp(&r.eighth_match_pixels, &fd[12 * p + 5], 8) ||
            std::memcmp(&r.inlier_rms_pixels, &fd[12 * p + 8], 8) || std::memcmp(&r.condition, &fd[12 * p + 10], 8))
            return 16;
        if (r.matches != (size_t)fd[12 * p + 1] || r.inlier_count != (size_t)fd[12 * p + 2] || r.hypotheses_with_model != (size_t)fd[12 * p + 4] ||
            r.attempts_accepted != (size_t)fd[12 * p + 6] || r.attempts_used != (size_t)fd[12 * p + 7] || r.real_roots != (size_t)fd[12 * p + 11] ||
            r.status != st[(size_t)p] || r.winner != (st[(size_t)p] ? -1 : (int64_t)fd[12 * p + 3]))
            return 17;
        const size_t n = pairs[(size_t)p].size();
        if (r.inliers.size() != n || std::memcmp(r.inliers.data(), ci.data() + rp[(size_t)p], n)) return 18;
        if (r.epipole_a.x != r.V[2] || r.epipole_a.z != r.V[8] || r.epipole_b.y != r.U[5]) return 19;
    }
    // the truth: K_b^-T [T]x R K_a^-1 at norm 1, its largest entry positive
    const double Tx[9] = { 0, -Tt[2], Tt[1], Tt[2], 0, -Tt[0], -Tt[1], Tt[0], 0 };
    auto inv = [](const Matrix3& K) { // upper triangular with K[8] = 1
        return Matrix3{ 1 / K[0], -K[1] / (K[0] * K[4]), (K[1] * K[5] - K[2] * K[4]) / (K[0] * K[4]), 0, 1 / K[4], -K[5] / K[4], 0, 0, 1 };
    };
    const Matrix3 Kai = inv(Ka), Kbi = inv(Kb);
    double E[9], EK[9], Ft[9], nn = 0, big = 0, val = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) E[3 * i + j] = Tx[3 * i] * Rt[j] + Tx[3 * i + 1] * Rt[3 + j] + Tx[3 * i + 2] * Rt[6 + j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) EK[3 * i + j] = E[3 * i] * Kai[j] + E[3 * i + 1] * Kai[3 + j] + E[3 * i + 2] * Kai[6 + j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            Ft[3 * i + j] = Kbi[i] * EK[j] + Kbi[3 + i] * EK[3 + j] + Kbi[6 + i] * EK[6 + j];
            nn += Ft[3 * i + j] * Ft[3 * i + j];
        }
    for (int e = 0; e < 9; ++e)
        if (std::fabs(Ft[e]) > big) big = std::fabs(Ft[e]), val = Ft[e];
    for (int e = 0; e < 9; ++e) Ft[e] *= (val < 0 ? -1.0 : 1.0) / std::sqrt(nn);
    for (int p = 0; p < 2; ++p) {
        const BA::UncalibratedPair& r = res[(size_t)p];
        const size_t n = pairs[(size_t)p].size();
        if (r.status != 0 || r.matches != n - (size_t)p) return 20;
        for (size_t i = 0; i < n; ++i)
            if (r.inliers[i] != (i % 5 != (size_t)p && !(p == 1 && i == 7))) return 21;
        double df = 0;
        for (size_t e = 0; e < 9; ++e) df = std::fmax(df, std::fabs(r.F[e] - Ft[e]));
        std::printf("pair %d: |F - F_true| %.3e, sigma %.6f, cond_1 %.3e, %zu of %zu attempts accepted\n", p, df, r.sigma, r.condition, r.attempts_accepted,
                    r.attempts_used);
        if (df > 1e-9) return 22;
    }
    if (res[2].status != SRK_FUNDAMENTAL_NO_MODEL || res[2].winner != -1 || res[2].F[0] != 0 || res[2].U[0] != 1 || !std::isnan(res[2].rms_pixels)) return 23;

    // refusals of the library carry the check's text
    srk_fundamental_options bad = lo;
    bad.inlier_pixels = 0;
    if (!throws_invalid([&] { ba.RelateUncalibrated(f0, pairs, &bad); }) || refusal.find("inlier_pixels") == std::string::npos) return 40;
    bad = lo, bad.refine_rounds = 17;
    if (!throws_invalid([&] { ba.RelateUncalibrated(f0, pairs, &bad); }) || refusal.find("refine_rounds") == std::string::npos) return 41;
    if (!throws_invalid([&] { ba.RelateUncalibrated(0.0, pairs, &lo); }) || refusal.find("f0") == std::string::npos) return 42;
    pairs[0][3].a.x = NAN;
    if (!throws_invalid([&] { ba.RelateUncalibrated(f0, pairs, &lo); }) || refusal.find("uv_a of match 3") == std::string::npos) return 43;
    if (!ba.RelateUncalibrated(f0, {}, &lo).empty()) return 44;
    std::printf("fundamental adapter ok\n");
    return 0;
}
