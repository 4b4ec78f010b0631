// Runtime test of BundleAdjustmentKanatani::MarginalizationPrior (include/suriko_amd/bundle-adj-kanatani.hpp): after a
// ComputeInplace the prior of dropping camera 0 with the salient points it sees equals the C ABI's on the same handle bit for bit,
// is symmetric, ties the cameras 1..5, and can be set on the next solve; a point left out, a camera beyond the cameras and a
// salient point no track carries throw.
#include <cmath>
#include <cstdio>
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
    FragmentMap map; CornerTrackRepository rep; std::vector<SE3Transform> cams((size_t)M); std::vector<Matrix3> Ks((size_t)M);
    std::vector<size_t> seen0; // the salient points camera 0 sees, by their place in the map
    for (int64_t i = 0; i < N; ++i) {
        CornerTrack& t = rep.AddCornerTrackObj();
        t.SalientPointId = map.AddSalientPoint({ pts[3 * i], pts[3 * i + 1], pts[3 * i + 2] });
        for (int64_t o = row_ptr[i]; o < row_ptr[i + 1]; ++o) t.AddCorner((size_t)fr[o], { uv[2 * o], uv[2 * o + 1] });
        if (fr[row_ptr[i]] == 0) seen0.push_back((size_t)i);
    }
    for (int32_t j = 0; j < M; ++j) {
        for (int e = 0; e < 9; ++e) { cams[(size_t)j].R[(size_t)e] = R[9 * j + e]; Ks[(size_t)j][(size_t)e] = K[9 * j + e]; }
        cams[(size_t)j].T = { T[3 * j], T[3 * j + 1], T[3 * j + 2] };
    }
    if (seen0.size() < 3) return 11;

    BundleAdjustmentKanataniTermCriteria crit;
    crit.AllowedReprojErrRelativeChange(1e-12);
    crit.MaxHessianFactor(1e6);
    BundleAdjustmentKanatani ba;
    ba.SetFixedIntrinsics(true);
    ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 6);

    using Set = BundleAdjustmentKanatani::JointPosePrior;
    Set prior;
    std::vector<Scalar> eta;
    srk_ba_marg_report mrep{};
    if (!ba.MarginalizationPrior({ 0 }, seen0, &prior, &eta, &mrep)) return 12;
    const size_t k = prior.frames.size(), n = 6 * k;
    if (k != 5 || prior.lin_R.size() != k || prior.lin_C.size() != k || prior.mean.size() != n || prior.info.size() != n * n || eta.size() != n) return 13;
    for (size_t q = 0; q < k; ++q)
        if (prior.frames[q] != q + 1) return 14;
    if (mrep.landmarks_used != (int64_t)seen0.size() || mrep.landmarks_skipped != 0 || mrep.sets != 0 || !(mrep.defect < 1e-6)) return 15;
    for (size_t a = 0; a < n; ++a)
        for (size_t b = 0; b < n; ++b)
            if (prior.info[a * n + b] != prior.info[b * n + a]) return 16;

    // the C ABI on the same handle: the same bits
    std::vector<int64_t> pi(seen0.begin(), seen0.end()); // (the tracks were added in the points' order: pnt_ind = place in the map)
    const int32_t drop = 0;
    std::vector<int32_t> kept(k);
    std::vector<double> cR(9 * k), cC(3 * k), cL(n * n), ce(n), cm(n);
    int32_t nk = 0;
    if (srk_ba_marginalization_prior(ba.Handle(), 1, &drop, (int64_t)pi.size(), pi.data(), (int32_t)k, kept.data(), &nk, cR.data(), cC.data(),
                                     cL.data(), ce.data(), cm.data(), nullptr) != SRK_OK || nk != (int32_t)k) return 17;
    if (cL != prior.info || cm != prior.mean || ce != eta) return 18;
    for (size_t q = 0; q < k; ++q) {
        for (int e = 0; e < 9; ++e)
            if (cR[9 * q + (size_t)e] != prior.lin_R[q][(size_t)e]) return 19;
        if (cC[3 * q] != prior.lin_C[q].x || cC[3 * q + 1] != prior.lin_C[q].y || cC[3 * q + 2] != prior.lin_C[q].z) return 19;
    }

    // refusals
    std::vector<size_t> fewer(seen0.begin() + 1, seen0.end());
    if (!throws_invalid([&] { ba.MarginalizationPrior({ 0 }, fewer, &prior); })) return 20;         // a point of camera 0 stays
    if (!throws_invalid([&] { ba.MarginalizationPrior({ (size_t)M }, seen0, &prior); })) return 21;  // beyond the cameras
    if (!throws_invalid([&] { ba.MarginalizationPrior({ 0 }, { (size_t)N + 5 }, &prior); })) return 22;
    if (prior.frames.size() != k) return 23; // a refused call leaves the outputs alone

    // the result is a set the next solve accepts
    ba.SetJointPosePriors({ prior });
    ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 2);
    if (srk_ba_joint_pose_prior_counts(ba.Handle(), nullptr, nullptr, nullptr) != 1) return 24;
    ba.ClearJointPosePriors();
    std::printf("landmarks %lld, kept %zu, defect %.3e, kernels %.3f + %.3f ms\n", (long long)mrep.landmarks_used, k, mrep.defect, mrep.ms_rows, mrep.ms_gram);
    std::printf("marginal adapter ok\n");
    return 0;
}
