// Runtime test of BundleAdjustmentKanatani::SetRelativePoseFactors / ClearRelativePoseFactors
// (include/suriko_amd/bundle-adj-kanatani.hpp): factors given in any order reach the library sorted by (min, max) of their
// cameras, the solve matches one through the C ABI with the arrays built by hand, a camera beyond the cameras and a pair named
// twice throw, the factors change the result, the reported error carries the factor sum, and clearing leaves the handle
// without a setting.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "suriko_amd/bundle-adj-kanatani.hpp"
using namespace suriko_amd;

template <typename F> static bool throws_invalid(F f)
{
    try { f(); } catch (const std::invalid_argument&) { return true; }
    return false;
}

int main()
{
    srk_scene_spec spec{};
    spec.n_frames = 12; spec.grid_nx = 10; spec.grid_ny = 8; spec.vis_window = 6;
    spec.half_extent_x = spec.half_extent_y = 1; spec.f0 = 600; spec.noise_x3d_hi = 0.005; spec.noise_r_hi = 0.005;
    spec.noise_uv_pix = 0.3; spec.seed = 91;
    const int64_t N = (int64_t)spec.grid_nx * spec.grid_ny, O = srk_scene_num_observations(&spec);
    const int32_t M = spec.n_frames;
    std::vector<double> pts(3 * N), R(9 * M), T(3 * M), K(9 * M), uv(2 * O);
    std::vector<int64_t> row_ptr(N + 1);
    std::vector<int32_t> fr(O);
    if (srk_scene_generate(&spec, pts.data(), nullptr, R.data(), T.data(), nullptr, nullptr, K.data(), row_ptr.data(),
                           fr.data(), uv.data()) != 0) return 10;

    auto build = [&](FragmentMap& map, CornerTrackRepository& rep, std::vector<SE3Transform>& cams, std::vector<Matrix3>& Ks) {
        for (int64_t i = 0; i < N; ++i) {
            CornerTrack& t = rep.AddCornerTrackObj();
            t.SalientPointId = map.AddSalientPoint({ pts[3 * i], pts[3 * i + 1], pts[3 * i + 2] });
            for (int64_t o = row_ptr[i]; o < row_ptr[i + 1]; ++o) t.AddCorner((size_t)fr[o], { uv[2 * o], uv[2 * o + 1] });
        }
        cams.resize((size_t)M);
        Ks.resize((size_t)M);
        for (int32_t j = 0; j < M; ++j) {
            for (int e = 0; e < 9; ++e) { cams[(size_t)j].R[(size_t)e] = R[9 * j + e]; Ks[(size_t)j][(size_t)e] = K[9 * j + e]; }
            cams[(size_t)j].T = { T[3 * j], T[3 * j + 1], T[3 * j + 2] };
        }
    };
    auto centre = [&](int32_t j, double c[3]) {
        for (int e = 0; e < 3; ++e) c[e] = -(R[9 * j + e] * T[3 * j] + R[9 * j + 3 + e] * T[3 * j + 1] + R[9 * j + 6 + e] * T[3 * j + 2]);
    };
    // a factor on (a, b): the scene's own relative pose, the translation moved by 4e-3 in x; diagonal information
    using Factor = BundleAdjustmentKanatani::RelativePoseFactor;
    auto make = [&](int32_t a, int32_t b) {
        Factor f;
        f.frame_a = (size_t)a;
        f.frame_b = (size_t)b;
        double ca[3], cb[3], z[3];
        centre(a, ca);
        centre(b, cb);
        for (int r = 0; r < 3; ++r) {
            z[r] = 0;
            for (int k = 0; k < 3; ++k) z[r] += R[9 * a + 3 * r + k] * (cb[k] - ca[k]);
            for (int c = 0; c < 3; ++c) {
                double v = 0;
                for (int k = 0; k < 3; ++k) v += R[9 * a + 3 * r + k] * R[9 * b + 3 * c + k];
                f.rel_R[(size_t)(3 * r + c)] = v;
            }
        }
        f.rel_t = { z[0] + 4e-3, z[1], z[2] };
        const double diag[6] = { 100, 100, 100, 50, 50, 50 };
        int k = 0;
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c, ++k) f.info[(size_t)k] = r == c ? diag[r] : 0.0;
        return f;
    };
    // given unsorted, one pair backwards; sorted by (min, max) of the cameras: (1, 2), (2, 11), (7, 3), (5, 6)
    const std::vector<Factor> given = { make(5, 6), make(2, 11), make(7, 3), make(1, 2) };
    const std::vector<Factor> sorted = { given[3], given[1], given[2], given[0] };
    std::vector<int32_t> fa, fb;
    std::vector<double> fR, ft, fL;
    for (const Factor& f : sorted) {
        fa.push_back((int32_t)f.frame_a);
        fb.push_back((int32_t)f.frame_b);
        fR.insert(fR.end(), f.rel_R.begin(), f.rel_R.end());
        ft.insert(ft.end(), { f.rel_t.x, f.rel_t.y, f.rel_t.z });
        fL.insert(fL.end(), f.info.begin(), f.info.end());
    }

    BundleAdjustmentKanataniTermCriteria crit;
    crit.AllowedReprojErrRelativeChange(1e-12);
    crit.MaxHessianFactor(1e6);
    BundleAdjustmentKanatani ba;
    {
        FragmentMap map; CornerTrackRepository rep; std::vector<SE3Transform> cams; std::vector<Matrix3> Ks;
        build(map, rep, cams, Ks);
        auto bad = given;
        bad[0].frame_b = (size_t)M; // beyond the cameras: the upload refuses it
        ba.SetRelativePoseFactors(bad);
        if (!throws_invalid([&] { ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 8); })) return 11;
        bad = given;
        bad.push_back(make(6, 5)); // the pair (5, 6) named twice, the other way round
        ba.SetRelativePoseFactors(bad);
        if (!throws_invalid([&] { ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 8); })) return 12;
        bad = given;
        bad[1].frame_b = bad[1].frame_a;
        ba.SetRelativePoseFactors(bad);
        if (!throws_invalid([&] { ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 8); })) return 13;
    }

    FragmentMap map; CornerTrackRepository rep; std::vector<SE3Transform> cams; std::vector<Matrix3> Ks;
    build(map, rep, cams, Ks);
    ba.SetRelativePoseFactors(given);
    ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 8);
    const srk_ba_report ra = ba.Report();
    int32_t n = 0;
    if (srk_ba_relative_pose_factor_count(ba.Handle(), &n) != 1 || n != 4) return 14;
    std::vector<int32_t> ga(4), gb(4);
    std::vector<double> gR(36), gt(12), gL(84);
    if (srk_ba_relative_pose_factors(ba.Handle(), ga.data(), gb.data(), gR.data(), gt.data(), gL.data()) != 1) return 14;
    if (ga != fa || gb != fb || gR != fR || gt != ft || gL != fL) return 15;
    double e_a = 0;
    if (srk_ba_relative_pose_error(ba.Handle(), &e_a) != SRK_OK) return 15;

    // the same solve through the C ABI, the arrays built by hand
    auto pts2 = pts, R2 = R, T2 = T;
    srk_ba* h = srk_ba_create(0);
    srk_ba_report rb{};
    const double a = 1e-12, mx = 1e6;
    if (srk_ba_set_relative_pose_factors(h, 4, fa.data(), fb.data(), fR.data(), ft.data(), fL.data()) != SRK_OK) return 16;
    int rc2 = srk_ba_compute_inplace(h, 600.0, N, pts2.data(), M, R2.data(), T2.data(), K.data(), 0, row_ptr.data(), fr.data(),
                                     uv.data(), &a, &mx, 8, &rb);
    double e_b = 0;
    if (rc2 < 0 || srk_ba_relative_pose_error(h, &e_b) != SRK_OK) return 16;
    std::vector<double> res(24);
    if (srk_ba_relative_pose_residuals(h, res.data()) != SRK_OK) return 16;
    // and without factors, for the difference they make
    auto pts3 = pts, R3 = R, T3 = T;
    srk_ba_report rep_none{};
    if (srk_ba_set_relative_pose_factors(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr) != SRK_OK) return 16;
    if (srk_ba_compute_inplace(h, 600.0, N, pts3.data(), M, R3.data(), T3.data(), K.data(), 0, row_ptr.data(), fr.data(),
                               uv.data(), &a, &mx, 8, &rep_none) < 0) return 16;
    srk_ba_destroy(h);
    double maxd = 0, pull = 0;
    for (int32_t j = 0; j < M; ++j) {
        const double t[3] = { cams[(size_t)j].T.x, cams[(size_t)j].T.y, cams[(size_t)j].T.z };
        for (int e = 0; e < 3; ++e) {
            maxd = std::fmax(maxd, std::fabs(t[e] - T2[3 * j + e]));
            pull = std::fmax(pull, std::fabs(t[e] - T3[3 * j + e]));
        }
    }
    double eres = 0; // the factor sum from the residual download and the diagonal information
    for (int k = 0; k < 4; ++k)
        for (int e = 0; e < 6; ++e) eres += (e < 3 ? 100.0 : 50.0) * res[6 * k + e] * res[6 * k + e];
    std::printf("iterations %lld / %lld err %.17g / %.17g maxdiff %.3e; factor sum %.3e (from residuals %.3e); moved by the factors %.3e\n",
                (long long)ra.iterations, (long long)rb.iterations, ra.err_final, rb.err_final, maxd, e_a, eres, pull);
    if (ra.iterations != rb.iterations || ra.attempts != rb.attempts || ra.iterations < 1) return 17;
    if (std::fabs(ra.err_final - rb.err_final) > 1e-10 * std::fabs(rb.err_final) || maxd > 1e-8) return 18;
    if (std::fabs(e_a - e_b) > 1e-8 * e_b || !(e_a > 0)) return 19;
    if (std::fabs(eres - e_b) > 1e-6 * e_b) return 20;
    if (!(pull > 1e-5)) return 21;                // the factors changed the result
    if (!(ra.err_final > e_a)) return 22;         // the reported error is the reprojection sum plus the factor sum

    // cleared: the handle holds no setting
    ba.ClearRelativePoseFactors();
    if (srk_ba_relative_pose_factor_count(ba.Handle(), nullptr) != 0) return 23;
    FragmentMap map3; CornerTrackRepository rep3; std::vector<SE3Transform> cams3; std::vector<Matrix3> Ks3;
    build(map3, rep3, cams3, Ks3);
    ba.ComputeInplace(600.0, map3, cams3, rep3, nullptr, &Ks3, crit, 8);
    double maxd3 = 0;
    for (int32_t j = 0; j < M; ++j) {
        const double t[3] = { cams3[(size_t)j].T.x, cams3[(size_t)j].T.y, cams3[(size_t)j].T.z };
        for (int e = 0; e < 3; ++e) maxd3 = std::fmax(maxd3, std::fabs(t[e] - T3[3 * j + e]));
    }
    if (maxd3 > 1e-8) return 24; // the run without factors
    std::printf("relpose adapter ok\n");
    return 0;
}
