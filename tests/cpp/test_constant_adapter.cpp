// Runtime test of BundleAdjustmentKanatani::SetConstantBlocks / ClearConstantBlocks (include/suriko_amd/bundle-adj-kanatani.hpp)
// on a map whose salient points are NOT in track order: the point flags are given in salient-point order and must reach the
// library in pnt_ind order (the order of the tracks).  Constant points and frames stay bit-identical in the caller's
// containers, the solve matches one through the C ABI with the flags mapped by hand, wrong sizes and an all-constant scene throw,
// and clearing lets every point move again.
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

    // the map holds the points in REVERSE track order: track (pnt_ind) i carries salient point N - 1 - i
    auto build = [&](FragmentMap& map, CornerTrackRepository& rep, std::vector<SE3Transform>& cams, std::vector<Matrix3>& Ks) {
        std::vector<size_t> id((size_t)N);
        for (int64_t k = 0; k < N; ++k) {
            const int64_t i = N - 1 - k;
            id[(size_t)i] = map.AddSalientPoint({ pts[3 * i], pts[3 * i + 1], pts[3 * i + 2] });
        }
        for (int64_t i = 0; i < N; ++i) {
            CornerTrack& t = rep.AddCornerTrackObj();
            t.SalientPointId = id[(size_t)i];
            for (int64_t o = row_ptr[i]; o < row_ptr[i + 1]; ++o) t.AddCorner((size_t)fr[o], { uv[2 * o], uv[2 * o + 1] });
        }
        cams.resize((size_t)M);
        Ks.resize((size_t)M);
        for (int32_t j = 0; j < M; ++j) {
            for (int e = 0; e < 9; ++e) { cams[(size_t)j].R[(size_t)e] = R[9 * j + e]; Ks[(size_t)j][(size_t)e] = K[9 * j + e]; }
            cams[(size_t)j].T = { T[3 * j], T[3 * j + 1], T[3 * j + 2] };
        }
    };
    // constant: frames 0, 1 and 7; salient points 0, 5, 10, ... (map order) = landmarks N - 1, N - 6, ... (pnt_ind)
    std::vector<uint8_t> ff((size_t)M, 0), pf_map((size_t)N, 0), pf_ind((size_t)N, 0);
    ff[0] = ff[1] = ff[7] = 1;
    for (int64_t k = 0; k < N; k += 5) { pf_map[(size_t)k] = 1; pf_ind[(size_t)(N - 1 - k)] = 1; }

    BundleAdjustmentKanataniTermCriteria crit;
    crit.AllowedReprojErrRelativeChange(1e-12);
    crit.MaxHessianFactor(1e6);
    BundleAdjustmentKanatani ba;
    {
        FragmentMap map; CornerTrackRepository rep; std::vector<SE3Transform> cams; std::vector<Matrix3> Ks;
        build(map, rep, cams, Ks);
        ba.SetConstantBlocks(std::vector<uint8_t>((size_t)M + 1, 0), pf_map, true); // one frame flag too many
        if (!throws_invalid([&] { ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 8); })) return 11;
        ba.SetConstantBlocks(ff, std::vector<uint8_t>((size_t)N - 1, 0), true);       // one point flag too few
        if (!throws_invalid([&] { ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 8); })) return 12;
        ba.SetConstantBlocks(std::vector<uint8_t>((size_t)M, 1), std::vector<uint8_t>((size_t)N, 1), true); // nothing left
        if (!throws_invalid([&] { ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 8); })) return 13;
    }

    FragmentMap map; CornerTrackRepository rep; std::vector<SE3Transform> cams; std::vector<Matrix3> Ks;
    build(map, rep, cams, Ks);
    const size_t id0 = 1000001; // FragmentMap's default offset: the first salient point
    ba.SetConstantBlocks(ff, pf_map, true);
    ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 8);
    const srk_ba_report ra = ba.Report();
    // the flags reached the handle in pnt_ind order
    std::vector<uint8_t> gf((size_t)M, 9), gp((size_t)N, 9);
    int kg = -1;
    if (srk_ba_constant_blocks(ba.Handle(), gf.data(), gp.data(), &kg) != 1 || kg != 1 || gf != ff || gp != pf_ind) return 14;

    // the same solve through the C ABI, flags mapped by hand
    auto pts2 = pts, R2 = R, T2 = T;
    srk_ba* h = srk_ba_create(0);
    srk_ba_report rb{};
    const double a = 1e-12, mx = 1e6;
    if (srk_ba_set_constant_blocks(h, ff.data(), M, pf_ind.data(), N, 1) != SRK_OK) return 15;
    int rc2 = srk_ba_compute_inplace(h, 600.0, N, pts2.data(), M, R2.data(), T2.data(), K.data(), 0, row_ptr.data(), fr.data(),
                                     uv.data(), &a, &mx, 8, &rb);
    srk_ba_destroy(h);
    if (rc2 < 0) return 16;
    double maxd = 0, moved_free = 1e300;
    int const_changed = 0;
    for (int64_t i = 0; i < N; ++i) {
        const Point3& p = map.GetSalientPoint(id0 + (size_t)(N - 1 - i)); // landmark i is salient point N - 1 - i
        const double q[3] = { p.x, p.y, p.z };
        maxd = std::fmax(maxd, std::fmax(std::fabs(q[0] - pts2[3 * i]), std::fmax(std::fabs(q[1] - pts2[3 * i + 1]), std::fabs(q[2] - pts2[3 * i + 2]))));
        if (pf_ind[(size_t)i]) const_changed += std::memcmp(q, &pts[3 * i], 24) != 0;
        else moved_free = std::fmin(moved_free, std::fabs(q[0] - pts[3 * i]) + std::fabs(q[1] - pts[3 * i + 1]) + std::fabs(q[2] - pts[3 * i + 2]));
    }
    int free_frames_moved = 0;
    for (int32_t j = 0; j < M; ++j) {
        const double t[3] = { cams[(size_t)j].T.x, cams[(size_t)j].T.y, cams[(size_t)j].T.z };
        const bool same = std::memcmp(t, &T[3 * j], 24) == 0 && std::memcmp(cams[(size_t)j].R.data(), &R[9 * j], 72) == 0;
        if (ff[(size_t)j]) const_changed += !same;
        else free_frames_moved += !same;
        for (int e = 0; e < 3; ++e) maxd = std::fmax(maxd, std::fabs(t[e] - T2[3 * j + e]));
    }
    std::printf("iterations %lld / %lld err %.17g / %.17g maxdiff %.3e constant changed %d free frames moved %d smallest free point move %.3e\n",
                (long long)ra.iterations, (long long)rb.iterations, ra.err_final, rb.err_final, maxd, const_changed, free_frames_moved, moved_free);
    if (ra.iterations != rb.iterations || ra.attempts != rb.attempts || ra.iterations < 1) return 17;
    if (std::fabs(ra.err_final - rb.err_final) > 1e-10 * std::fabs(rb.err_final) || maxd > 1e-8) return 18;
    if (const_changed != 0) return 19;
    if (free_frames_moved != M - 3 || !(moved_free > 0)) return 20;

    // cleared: the handle holds no setting and every point moves
    ba.ClearConstantBlocks();
    if (srk_ba_constant_blocks(ba.Handle(), nullptr, nullptr, nullptr) != 0) return 21;
    FragmentMap map3; CornerTrackRepository rep3; std::vector<SE3Transform> cams3; std::vector<Matrix3> Ks3;
    build(map3, rep3, cams3, Ks3);
    ba.ComputeInplace(600.0, map3, cams3, rep3, nullptr, &Ks3, crit, 8);
    int still = 0;
    for (int64_t i = 0; i < N; ++i) {
        const Point3& p = map3.GetSalientPoint(id0 + (size_t)(N - 1 - i));
        const double q[3] = { p.x, p.y, p.z };
        still += std::memcmp(q, &pts[3 * i], 24) == 0;
    }
    if (still != 0) return 22;
    std::printf("constant adapter ok\n");
    return 0;
}
