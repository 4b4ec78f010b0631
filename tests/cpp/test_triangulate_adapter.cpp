// Runtime test of BundleAdjustmentKanatani::Triangulate and ::TriangulateTracks (include/suriko_amd/bundle-adj-kanatani.hpp):
// after a ComputeInplace the landmarks triangulated from the scene's own tracks over the resident cameras equal the C ABI's on
// the same handle bit for bit and lie at the refined salient points; over the refined cameras handed in by the caller the result
// is the same to rounding; a refinement lowers no track's error; mismatched intrinsics and a track beyond the cameras throw.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "distinct_intrinsics.hpp"
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
    distinct_intrinsics(M, spec.f0, K, fr, uv); // every frame its own fx, fy, u0, v0: the adapter must hand each frame's own K on
    if (!intrinsics_are_distinct(M, K)) return 10;
    FragmentMap map; CornerTrackRepository rep; std::vector<SE3Transform> cams((size_t)M); std::vector<Matrix3> Ks((size_t)M);
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
    BundleAdjustmentKanatani ba;
    ba.SetFixedIntrinsics(true);
    ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 6);

    using TP = BundleAdjustmentKanatani::TriangulatedPoint;
    const std::vector<TP> res = ba.Triangulate(rep.CornerTracks);
    if (res.size() != (size_t)N) return 11;
    // the C ABI on the same handle: the same bits
    std::vector<double> cX(3 * N), cq(4 * N);
    std::vector<uint32_t> cs((size_t)N);
    if (srk_ba_triangulate(ba.Handle(), N, row_ptr.data(), fr.data(), uv.data(), nullptr, nullptr, 1, cX.data(), cq.data(), cs.data()) != SRK_OK) return 12;
    double worst = 0;
    for (int64_t i = 0; i < N; ++i) {
        const TP& p = res[(size_t)i];
        if (p.X.x != cX[3 * i] || p.X.y != cX[3 * i + 1] || p.X.z != cX[3 * i + 2] || p.rms_pixels != cq[4 * i] || p.status != cs[(size_t)i]) return 13;
        if (p.status != 0 || p.views != (size_t)(row_ptr[i + 1] - row_ptr[i]) || !(p.cond1 >= 1) || !(p.max_ray_angle_deg > 0)) return 14;
        // the refined salient point of the same track: both fit the same corners over the same cameras
        const Point3& s = map.GetSalientPoint(*rep.CornerTracks[(size_t)i].SalientPointId);
        worst = std::fmax(worst, std::sqrt((p.X.x - s.x) * (p.X.x - s.x) + (p.X.y - s.y) * (p.X.y - s.y) + (p.X.z - s.z) * (p.X.z - s.z)));
    }
    if (!(worst < 0.05)) return 15;
    // over the refined cameras, handed in: the same points up to the rounding of another coordinate frame
    const std::vector<TP> own = ba.TriangulateTracks(600.0, rep.CornerTracks, cams, nullptr, &Ks);
    if (own.size() != (size_t)N) return 16;
    for (int64_t i = 0; i < N; ++i) {
        const Point3 &a = own[(size_t)i].X, &b = res[(size_t)i].X;
        if (!(std::fabs(a.x - b.x) + std::fabs(a.y - b.y) + std::fabs(a.z - b.z) < 1e-9) || own[(size_t)i].status != 0) return 17;
    }
    // a refinement lowers no track's error
    srk_tri_options opt;
    srk_tri_default_options(&opt);
    const std::vector<TP> fine = ba.Triangulate(rep.CornerTracks, &opt);
    for (int64_t i = 0; i < N; ++i)
        if (!(fine[(size_t)i].rms_pixels <= res[(size_t)i].rms_pixels) || (fine[(size_t)i].status & ~(uint32_t)SRK_TRI_NOT_CONVERGED)) return 18;
    // refusals
    std::vector<Matrix3> fewer(Ks.begin(), Ks.end() - 1);
    if (!throws_invalid([&] { ba.TriangulateTracks(600.0, rep.CornerTracks, cams, nullptr, &fewer); })) return 20;
    if (!throws_invalid([&] { ba.TriangulateTracks(600.0, rep.CornerTracks, cams, nullptr, nullptr); })) return 21;
    opt.refine_attempts = 65;
    if (!throws_invalid([&] { ba.Triangulate(rep.CornerTracks, &opt); })) return 22;
    // a track with one corner
    std::vector<CornerTrack> lone(1);
    lone[0].AddCorner(3, { 100, 100 });
    const std::vector<TP> few = ba.Triangulate(lone);
    if (few.size() != 1 || few[0].status != SRK_TRI_FEW_VIEWS || !std::isnan(few[0].X.x) || few[0].views != 1) return 23;
    std::printf("tracks %lld, worst distance to the refined points %.3e\n", (long long)N, worst);
    std::printf("triangulate adapter ok\n");
    return 0;
}
