// Runtime test of BundleAdjustmentKanatani::AlignPoints, Align and ApplySimilarity (include/suriko_amd/bundle-adj-kanatani.hpp):
// two sets of points under known similarities, a fifth of the targets wrong, give the C ABI's bits on the same handle, mark no
// wrong correspondence an inlier and recover the similarity; after ComputeInplace over a generated scene, Align over the map's
// landmarks equals AlignPoints over the downloaded ones; ApplySimilarity keeps a landmark's camera coordinates up to the scale;
// refusals of the library throw std::invalid_argument with the check's text.
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

static Point3 map_point(double s, const Matrix3& R, const Point3& t, const Point3& a)
{
    return { s * (R[0] * a.x + R[1] * a.y + R[2] * a.z) + t.x, s * (R[3] * a.x + R[4] * a.y + R[5] * a.z) + t.y,
             s * (R[6] * a.x + R[7] * a.y + R[8] * a.z) + t.z };
}

int main()
{
    using BA = BundleAdjustmentKanatani;
    const double c = std::cos(0.4), sn = std::sin(0.4);
    const Matrix3 Rt[2] = { { c, -sn, 0, sn, c, 0, 0, 0, 1 }, { 1, 0, 0, 0, c, -sn, 0, sn, c } };
    const Point3 tt[2] = { { 1, -2, 0.5 }, { -3, 0, 2 } };
    const double st[2] = { 1.5, 0.25 };
    uint64_t x = 99;
    auto next = [&x] { x = x * 6364136223846793005ull + 1442695040888963407ull; return (double)(x >> 11) / 4503599627370496.0 - 1.0; };
    std::vector<std::vector<BA::Correspondence>> sets(2);
    for (int p = 0; p < 2; ++p)
        for (int i = 0; i < 100 + 30 * p; ++i) {
            BA::Correspondence k;
            k.a = { 2 * next(), 2 * next(), 2 * next() };
            k.b = map_point(st[p], Rt[p], tt[p], k.a);
            if (i % 5 == p) k.b.y += 3.0; // a wrong correspondence
            sets[(size_t)p].push_back(k);
        }
    sets[1][7].information = 0; // and one switched off
    srk_align_options lo;
    srk_align_default_options(&lo);
    lo.hypotheses = 128;
    lo.inlier_distance = 0.01;
    BA ba;
    const std::vector<BA::AlignedSet> res = ba.AlignPoints(sets, lo, true);
    if (res.size() != 2) return 12;

    // the C ABI on the same handle: the same bits
    std::vector<int64_t> rp{ 0 };
    std::vector<double> a, b, q, cs(2), cR(18), ct(6), cl(16);
    std::vector<uint32_t> cst(2);
    for (int p = 0; p < 2; ++p) {
        for (const BA::Correspondence& k : sets[(size_t)p]) {
            a.insert(a.end(), { k.a.x, k.a.y, k.a.z });
            b.insert(b.end(), { k.b.x, k.b.y, k.b.z });
            q.push_back(k.information);
        }
        rp.push_back((int64_t)q.size());
    }
    std::vector<uint8_t> ci(q.size());
    if (srk_align_points(ba.Handle(), 2, rp.data(), a.data(), b.data(), q.data(), &lo, cs.data(), cR.data(), ct.data(), cl.data(), cst.data(), ci.data()) != 0)
        return 13;
    for (int p = 0; p < 2; ++p) {
        const BA::AlignedSet& r = res[(size_t)p];
        const double t[3] = { r.t.x, r.t.y, r.t.z };
        if (std::memcmp(&r.scale, &cs[(size_t)p], 8) || std::memcmp(r.R.data(), cR.data() + 9 * p, 72) || std::memcmp(t, ct.data() + 3 * p, 24)) return 14;
        if (std::memcmp(&r.rms_distance, &cl[8 * p], 8) || std::memcmp(&r.eigen_gap, &cl[8 * p + 6], 8) || std::memcmp(&r.inlier_rms_distance, &cl[8 * p + 7], 8))
            return 15;
        if (r.points != (size_t)cl[8 * p + 1] || r.inlier_count != (size_t)cl[8 * p + 2] || r.winner != (int64_t)cl[8 * p + 3] ||
            r.hypotheses_with_model != (size_t)cl[8 * p + 4] || r.rounds != (size_t)cl[8 * p + 5] || r.status != cst[(size_t)p])
            return 16;
        const size_t n = sets[(size_t)p].size();
        if (r.inliers.size() != n || std::memcmp(r.inliers.data(), ci.data() + rp[(size_t)p], n)) return 17;
        if (r.status != 0 || r.points != n - (size_t)p) return 18;
        for (size_t i = 0; i < n; ++i)
            if (r.inliers[i] != (i % 5 != (size_t)p && !(p == 1 && i == 7))) return 19;
        double dr = 0;
        for (size_t e = 0; e < 9; ++e) dr = std::fmax(dr, std::fabs(r.R[e] - Rt[p][e]));
        const double dt = std::fabs(r.t.x - tt[p].x) + std::fabs(r.t.y - tt[p].y) + std::fabs(r.t.z - tt[p].z);
        std::printf("set %d: |s / s_true - 1| %.3e, |R - R_true| %.3e, |t - t_true| %.3e, %zu inliers, %zu round(s)\n", p, std::fabs(r.scale / st[p] - 1), dr, dt,
                    r.inlier_count, r.rounds);
        if (std::fabs(r.scale / st[p] - 1) > 1e-10 || dr > 1e-10 || dt > 1e-9) return 20;
    }

    // a resident scene: Align over the map's landmarks against AlignPoints over the same landmarks read back
    srk_scene_spec spec{};
    spec.n_frames = 10; spec.grid_nx = 10; spec.grid_ny = 8; spec.vis_window = 0;
    spec.half_extent_x = spec.half_extent_y = 1; spec.f0 = 600; spec.noise_x3d_hi = 0.005; spec.noise_r_hi = 0.005;
    spec.noise_uv_pix = 0.3; spec.seed = 95;
    const int64_t N = (int64_t)spec.grid_nx * spec.grid_ny, O = srk_scene_num_observations(&spec);
    const int32_t M = spec.n_frames;
    std::vector<double> pts(3 * N), R(9 * M), T(3 * M), K(9 * M), uv(2 * O);
    std::vector<int64_t> row_ptr(N + 1);
    std::vector<int32_t> fr(O);
    if (srk_scene_generate(&spec, pts.data(), nullptr, R.data(), T.data(), nullptr, nullptr, K.data(), row_ptr.data(), fr.data(), uv.data()) != 0) return 30;
    FragmentMap map; CornerTrackRepository rep; std::vector<SE3Transform> cams((size_t)M);
    std::vector<Matrix3> Ks((size_t)M);
    for (int64_t i = 0; i < N; ++i) {
        CornerTrack& t = rep.AddCornerTrackObj();
        t.SalientPointId = map.AddSalientPoint({ pts[3 * i], pts[3 * i + 1], pts[3 * i + 2] });
        for (int64_t o = row_ptr[i]; o < row_ptr[i + 1]; ++o) t.AddCorner((size_t)fr[o], { uv[2 * o], uv[2 * o + 1] });
    }
    for (int32_t j = 0; j < M; ++j) {
        for (int e = 0; e < 9; ++e) { cams[(size_t)j].R[(size_t)e] = R[9 * j + e]; Ks[(size_t)j][(size_t)e] = K[9 * j + e]; }
        cams[(size_t)j].T = { T[3 * j], T[3 * j + 1], T[3 * j + 2] };
    }
    BundleAdjustmentKanataniTermCriteria crit;
    crit.AllowedReprojErrRelativeChange(1e-12);
    crit.MaxHessianFactor(1e6);
    ba.SetFixedIntrinsics(true);
    ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 6);
    std::vector<std::vector<BA::MapCorrespondence>> onmap(1);
    std::vector<std::vector<BA::Correspondence>> same(1);
    size_t idx = 0;
    for (const CornerTrack& t : rep.CornerTracks) {
        const Point3 lm = map.GetSalientPoint(*t.SalientPointId);
        Point3 target = map_point(st[0], Rt[0], tt[0], lm);
        if (idx % 5 == 2) target.x -= 2.0;
        onmap[0].push_back({ idx, target, 1.0 });
        same[0].push_back({ lm, target, 1.0 });
        ++idx;
    }
    lo.inlier_distance = 1e-3;
    const BA::AlignedSet m = ba.Align(onmap, lo, true)[0], o = ba.AlignPoints(same, lo, true)[0];
    double dr = 0;
    for (size_t e = 0; e < 9; ++e) dr = std::fmax(dr, std::fabs(m.R[e] - o.R[e]));
    std::printf("resident: |s ratio - 1| %.3e, |R - R'| %.3e, |t - t'| %.3e\n", std::fabs(m.scale / o.scale - 1), dr,
                std::fabs(m.t.x - o.t.x) + std::fabs(m.t.y - o.t.y) + std::fabs(m.t.z - o.t.z));
    if (m.status != 0 || o.status != 0 || m.inlier_count != o.inlier_count || m.inliers != o.inliers || m.inlier_count != (size_t)N - (size_t)N / 5)
        return 31;
    // the two runs differ by the map through the normalised coordinates: a few hundred roundings of numbers of size 10
    if (std::fabs(m.scale / o.scale - 1) > 1e-10 || dr > 1e-10 || std::fabs(m.t.x - o.t.x) + std::fabs(m.t.y - o.t.y) + std::fabs(m.t.z - o.t.z) > 1e-9) return 32;

    // ApplySimilarity: a landmark's camera coordinates scale by s
    std::vector<Point3> P{ map.GetSalientPoint(*rep.CornerTracks[3].SalientPointId) };
    std::vector<SE3Transform> C{ cams[4] };
    const Point3 before = map_point(1.0, C[0].R, C[0].T, P[0]);
    BA::ApplySimilarity(m.scale, m.R, m.t, &P, &C);
    const Point3 after = map_point(1.0, C[0].R, C[0].T, P[0]);
    if (std::fabs(after.x - m.scale * before.x) + std::fabs(after.y - m.scale * before.y) + std::fabs(after.z - m.scale * before.z) > 1e-12) return 33;
    BA::ApplySimilarity(m.scale, m.R, m.t, nullptr, nullptr);
    if (!throws_invalid([&] { BA::ApplySimilarity(0.0, m.R, m.t, &P, nullptr); })) return 34;

    // refusals of the library carry the check's text
    srk_align_options bad = lo;
    bad.inlier_distance = 0;
    if (!throws_invalid([&] { ba.AlignPoints(sets, bad); }) || refusal.find("inlier_distance") == std::string::npos) return 40;
    bad = lo, bad.hypotheses = 0;
    if (!throws_invalid([&] { ba.Align(onmap, bad); }) || refusal.find("hypotheses") == std::string::npos) return 41;
    onmap[0][5].point = (size_t)N;
    if (!throws_invalid([&] { ba.Align(onmap, lo); }) || refusal.find("beyond the map") == std::string::npos) return 42;
    sets[0][3].a.x = NAN;
    if (!throws_invalid([&] { ba.AlignPoints(sets, lo); }) || refusal.find("a of correspondence 3") == std::string::npos) return 43;
    std::printf("align adapter ok\n");
    return 0;
}
