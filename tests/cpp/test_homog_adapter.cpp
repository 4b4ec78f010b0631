// Runtime test of BundleAdjustmentKanatani::RelateHomography (include/suriko_amd/bundle-adj-kanatani.hpp): a planar pair with a
// fifth of the targets wrong and a pure rotation give the C ABI's bits on the same handle, mark no wrong match an inlier, return
// the plane's two poses with one of them the truth and the rotation alone; refusals of the library throw std::invalid_argument
// with the check's text.
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
    const double Tt[2][3] = { { 0.6, -0.2, 0.3 }, { 0, 0, 0 } };
    const double nn = std::sqrt(0.2 * 0.2 + 0.1 * 0.1 + 1.0), Nt[3] = { -0.2 / nn, 0.1 / nn, 1.0 / nn }, d = 6.0 / nn;
    uint64_t x = 99;
    auto next = [&x] { x = x * 6364136223846793005ull + 1442695040888963407ull; return (double)(x >> 11) / 4503599627370496.0 - 1.0; };
    std::vector<std::vector<BA::Match>> pairs(2);
    for (int p = 0; p < 2; ++p)
        for (int i = 0; i < 100 + 30 * p; ++i) {
            double X[3] = { 2 * next(), 1.5 * next(), 6 + 2 * next() }, Y[3];
            if (p == 0) X[2] = 6 + 0.2 * X[0] - 0.1 * X[1];
            for (int r = 0; r < 3; ++r) Y[r] = Rt[3 * r] * X[0] + Rt[3 * r + 1] * X[1] + Rt[3 * r + 2] * X[2] + Tt[p][r];
            BA::Match m;
            m.a = pixel(Ka, X, f0);
            m.b = pixel(Kb, Y, f0);
            if (i % 5 == p) m.b.y += 40.0; // a wrong match
            pairs[(size_t)p].push_back(m);
        }
    pairs[1][7].information = 0; // and one switched off
    srk_homography_options lo;
    srk_homography_default_options(&lo);
    lo.hypotheses = 128;
    lo.inlier_pixels = 0.01;
    BA ba;
    const std::vector<BA::HomographyPair> res = ba.RelateHomography(f0, pairs, &Ka, &Kb, nullptr, nullptr, &lo, true);
    if (res.size() != 2) return 12;

    // the C ABI on the same handle: the same bits
    std::vector<int64_t> rp{ 0 };
    std::vector<double> ua, ub, q, G(18), H(18), R(36), T(12), N(12), hg(16);
    std::vector<int32_t> poses(2), front(4);
    std::vector<uint32_t> st(2);
    for (int p = 0; p < 2; ++p) {
        for (const BA::Match& m : pairs[(size_t)p]) {
            ua.insert(ua.end(), { m.a.x, m.a.y });
            ub.insert(ub.end(), { m.b.x, m.b.y });
            q.push_back(m.information);
        }
        rp.push_back((int64_t)q.size());
    }
    std::vector<uint8_t> ci(q.size());
    if (srk_relate_homography(ba.Handle(), f0, 2, rp.data(), ua.data(), ub.data(), q.data(), Ka.data(), Kb.data(), 1, &lo, G.data(), H.data(), poses.data(),
                              R.data(), T.data(), N.data(), front.data(), hg.data(), st.data(), ci.data()) != 0)
        return 13;
    for (int p = 0; p < 2; ++p) {
        const BA::HomographyPair& r = res[(size_t)p];
        if (std::memcmp(r.G.data(), G.data() + 9 * p, 72) || std::memcmp(r.H.data(), H.data() + 9 * p, 72) || r.poses.size() != (size_t)poses[(size_t)p]) return 14;
        for (size_t k = 0; k < r.poses.size(); ++k) {
            const double t[3] = { r.poses[k].pose.T.x, r.poses[k].pose.T.y, r.poses[k].pose.T.z }, n[3] = { r.poses[k].normal.x, r.poses[k].normal.y, r.poses[k].normal.z };
            if (std::memcmp(r.poses[k].pose.R.data(), R.data() + 18 * p + 9 * k, 72) || std::memcmp(t, T.data() + 6 * p + 3 * k, 24) ||
                std::memcmp(n, N.data() + 6 * p + 3 * k, 24) || r.poses[k].in_front != (size_t)front[(size_t)(2 * p) + k])
                return 15;
        }
        if (std::memcmp(&r.rms_pixels, &hg[8 * p], 8) || std::memcmp(&r.singular_gap, &hg[8 * p + 6], 8) || std::memcmp(&r.inlier_rms_pixels, &hg[8 * p + 7], 8))
            return 16;
        if (r.matches != (size_t)hg[8 * p + 1] || r.inlier_count != (size_t)hg[8 * p + 2] || r.winner != (int64_t)hg[8 * p + 3] ||
            r.hypotheses_with_model != (size_t)hg[8 * p + 4] || r.rounds != (size_t)hg[8 * p + 5] || r.status != st[(size_t)p])
            return 17;
        const size_t n = pairs[(size_t)p].size();
        if (r.inliers.size() != n || std::memcmp(r.inliers.data(), ci.data() + rp[(size_t)p], n)) return 18;
        if (r.status != 0 || r.matches != n - (size_t)p) return 19;
        for (size_t i = 0; i < n; ++i)
            if (r.inliers[i] != (i % 5 != (size_t)p && !(p == 1 && i == 7))) return 20;
    }
    // the plane: two poses, one of them the truth; the rotation: one pose, no translation, no normal
    if (res[0].poses.size() != 2 || res[1].poses.size() != 1 || !(res[1].singular_gap <= 1e-10)) return 21;
    int hits = 0;
    for (const BA::PlanePose& k : res[0].poses) {
        double dr = 0;
        for (size_t e = 0; e < 9; ++e) dr = std::fmax(dr, std::fabs(k.pose.R[e] - Rt[e]));
        const double dt = std::fabs(k.pose.T.x - Tt[0][0] / d) + std::fabs(k.pose.T.y - Tt[0][1] / d) + std::fabs(k.pose.T.z - Tt[0][2] / d);
        const double dn = std::fabs(k.normal.x - Nt[0]) + std::fabs(k.normal.y - Nt[1]) + std::fabs(k.normal.z - Nt[2]);
        std::printf("plane: |R - R_true| %.3e, |T/d - truth| %.3e, |N - N_true| %.3e, %zu in front\n", dr, dt, dn, k.in_front);
        hits += dr <= 1e-9 && dt <= 1e-9 && dn <= 1e-9;
    }
    if (hits != 1) return 22;
    double dr = 0;
    for (size_t e = 0; e < 9; ++e) dr = std::fmax(dr, std::fabs(res[1].poses[0].pose.R[e] - Rt[e]));
    std::printf("rotation: |R - R_true| %.3e, gap %.3e\n", dr, res[1].singular_gap);
    if (dr > 1e-9 || res[1].poses[0].pose.T.x != 0 || res[1].poses[0].normal.z != 0) return 23;

    // refusals of the library carry the check's text
    srk_homography_options bad = lo;
    bad.inlier_pixels = 0;
    if (!throws_invalid([&] { ba.RelateHomography(f0, pairs, &Ka, &Kb, nullptr, nullptr, &bad); }) || refusal.find("inlier_pixels") == std::string::npos) return 40;
    bad = lo, bad.refine_rounds = 17;
    if (!throws_invalid([&] { ba.RelateHomography(f0, pairs, &Ka, &Kb, nullptr, nullptr, &bad); }) || refusal.find("refine_rounds") == std::string::npos) return 41;
    if (!throws_invalid([&] { ba.RelateHomography(f0, pairs, &Ka, nullptr, nullptr, nullptr, &lo); })) return 42;
    pairs[0][3].a.x = NAN;
    if (!throws_invalid([&] { ba.RelateHomography(f0, pairs, &Ka, &Kb, nullptr, nullptr, &lo); }) || refusal.find("uv_a of match 3") == std::string::npos) return 43;
    std::printf("homography adapter ok\n");
    return 0;
}
