// Runtime test of BundleAdjustmentKanatani::Covariances / SetCovarianceBatch (include/suriko_amd/bundle-adj-kanatani.hpp) on a
// map whose salient points are NOT in track order: points are named in salient-point order and must reach the library in
// pnt_ind order (the order of the tracks).  The blocks equal those of srk_ba_covariances on a handle that ran the same solve
// through the C ABI with the indices mapped by hand, whatever the batch cap; bad indices and a bad sigma throw; and the caller's
// containers are not touched by the call.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "suriko_amd/bundle-adj-kanatani.hpp"
using namespace suriko_amd;

// largest difference of two arrays over the largest entry of the second.  Two calls build the system twice, and the derivative
// and Schur kernels add with atomics: the systems agree to rounding, not to the bit, and the inverse of the undamped system
// moves by that rounding times its scaled condition number (1e10 .. 1e11 with six variables a frame: tests/covariance_cases.py),
// i.e. by up to 64 eps cond ~ 1e-3 in the terms of tests/test_gpu_covariance.py.  An index that went to the wrong frame or
// landmark moves a block by its own size.
#define COV_TOL 1e-3
static double rel_diff(const std::vector<double>& a, const std::vector<double>& b)
{
    if (a.size() != b.size()) return 1e300;
    double d = 0, v = 0;
    for (size_t e = 0; e < a.size(); ++e) { d = std::fmax(d, std::fabs(a[e] - b[e])); v = std::fmax(v, std::fabs(b[e])); }
    return v > 0 ? d / v : (d > 0 ? 1e300 : 0.0);
}

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
    FragmentMap map; CornerTrackRepository rep; std::vector<SE3Transform> cams((size_t)M); std::vector<Matrix3> Ks((size_t)M);
    {
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
        for (int32_t j = 0; j < M; ++j) {
            for (int e = 0; e < 9; ++e) { cams[(size_t)j].R[(size_t)e] = R[9 * j + e]; Ks[(size_t)j][(size_t)e] = K[9 * j + e]; }
            cams[(size_t)j].T = { T[3 * j], T[3 * j + 1], T[3 * j + 2] };
        }
    }
    BundleAdjustmentKanataniTermCriteria crit;
    crit.AllowedReprojErrRelativeChange(1e-12);
    crit.MaxHessianFactor(1e6);
    BundleAdjustmentKanatani ba;
    ba.SetFixedIntrinsics(true);
    ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 8);
    const std::vector<SE3Transform> cams_before = cams;

    const std::vector<size_t> frames = { 0, 1, 5, 11, 5 }, points = { 0, 3, (size_t)N - 1, 3 }; // salient-point order
    std::vector<double> fc, pc;
    if (!ba.Covariances(frames, points, 0.5, &fc, &pc)) return 11;
    if (fc.size() != 36 * frames.size() || pc.size() != 9 * points.size()) return 12;
    for (size_t j = 0; j < cams.size(); ++j)
        if (std::memcmp(cams[j].R.data(), cams_before[j].R.data(), 72) != 0 || cams[j].T.x != cams_before[j].T.x) return 13;
    // frame 0 is gauge-fixed: zeros; frame 5 twice: the same bits; every block symmetric with a positive diagonal elsewhere
    for (int e = 0; e < 36; ++e) if (fc[(size_t)e] != 0.0) return 14;
    if (std::memcmp(&fc[36 * 2], &fc[36 * 4], 36 * 8) != 0 || std::memcmp(&pc[9 * 1], &pc[9 * 3], 72) != 0) return 15;
    for (size_t b = 2; b < 4; ++b)
        for (int i = 0; i < 6; ++i) {
            if (!(fc[36 * b + 7 * (size_t)i] > 0)) return 16;
            for (int j = 0; j < 6; ++j) if (fc[36 * b + 6 * (size_t)i + (size_t)j] != fc[36 * b + 6 * (size_t)j + (size_t)i]) return 17;
        }
    // a small batch cap: the same blocks
    std::vector<double> fc2, pc2;
    ba.SetCovarianceBatch(12);
    if (!ba.Covariances(frames, points, 0.5, &fc2, &pc2) || rel_diff(fc2, fc) > COV_TOL || rel_diff(pc2, pc) > COV_TOL) return 18;
    ba.SetCovarianceBatch(0);

    // the same solve and the same question through the C ABI, indices mapped by hand (salient point k = landmark N - 1 - k)
    auto pts2 = pts, R2 = R, T2 = T;
    srk_ba* h = srk_ba_create(0);
    srk_ba_report rb{};
    const double a = 1e-12, mx = 1e6;
    if (srk_ba_set_fixed_intrinsics(h, 1) != SRK_OK) return 19;
    if (srk_ba_compute_inplace(h, 600.0, N, pts2.data(), M, R2.data(), T2.data(), K.data(), 0, row_ptr.data(), fr.data(), uv.data(),
                               &a, &mx, 8, &rb) < 0) return 20;
    const int32_t fi[5] = { 0, 1, 5, 11, 5 };
    const int64_t pi[4] = { N - 1, N - 4, 0, N - 4 };
    std::vector<double> fcr(36 * 5), pcr(9 * 4);
    const int rc = srk_ba_covariances(h, 0.5, 5, fi, fcr.data(), 4, pi, pcr.data(), 1);
    srk_ba_destroy(h);
    if (rc != 0) return 21;
    const double df = rel_diff(fc, fcr), dp = rel_diff(pc, pcr);
    std::printf("frame blocks differ by %.3e, point blocks by %.3e (of the largest entry)\n", df, dp);
    if (df > COV_TOL || dp > COV_TOL) return 22;

    if (!throws_invalid([&] { ba.Covariances({ (size_t)M }, {}, 1.0, &fc2, &pc2); })) return 23;
    if (!throws_invalid([&] { ba.Covariances({}, { (size_t)N }, 1.0, &fc2, &pc2); })) return 24;
    if (!throws_invalid([&] { ba.Covariances({ 1 }, {}, 0.0, &fc2, &pc2); })) return 25;
    if (!ba.Covariances({}, {}, 1.0, &fc2, &pc2) || !fc2.empty() || !pc2.empty()) return 26;
    std::printf("covariance adapter ok\n");
    return 0;
}
