// Runtime test of BundleAdjustmentKanatani::Resect and ::ResectFrames (include/suriko_amd/bundle-adj-kanatani.hpp): after a
// ComputeInplace over the first ten frames of an all-visible scene, the two held-out frames are resected from their corners over
// the resident landmarks; the result equals the C ABI's on the same handle bit for bit, lies at the generated poses, and equals
// the resection over the refined salient points handed in by the caller to rounding; a Cauchy loss gives the moved corners a small
// weight; mismatched sizes and a landmark beyond the scene throw.
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
    spec.n_frames = 12; spec.grid_nx = 10; spec.grid_ny = 8; spec.vis_window = 0;
    spec.half_extent_x = spec.half_extent_y = 1; spec.f0 = 600; spec.noise_x3d_hi = 0.005; spec.noise_r_hi = 0.005;
    spec.noise_uv_pix = 0.3; spec.seed = 92;
    const int64_t N = (int64_t)spec.grid_nx * spec.grid_ny, O = srk_scene_num_observations(&spec);
    const int32_t M = spec.n_frames, held = 2, used = M - held;
    std::vector<double> pts(3 * N), R(9 * M), T(3 * M), K(9 * M), uv(2 * O);
    std::vector<int64_t> row_ptr(N + 1);
    std::vector<int32_t> fr(O);
    if (srk_scene_generate(&spec, pts.data(), nullptr, R.data(), T.data(), nullptr, nullptr, K.data(), row_ptr.data(),
                           fr.data(), uv.data()) != 0) return 10;
    distinct_intrinsics(M, spec.f0, K, fr, uv); // every frame its own fx, fy, u0, v0: the adapter must hand each frame's own K on
    if (!intrinsics_are_distinct(M, K)) return 10;
    using BA = BundleAdjustmentKanatani;
    FragmentMap map; CornerTrackRepository rep; std::vector<SE3Transform> cams((size_t)used), start((size_t)held);
    std::vector<Matrix3> Ks((size_t)used), Kh((size_t)held);
    std::vector<std::vector<BA::ResectObservation>> frames((size_t)held);
    for (int64_t i = 0; i < N; ++i) {
        CornerTrack& t = rep.AddCornerTrackObj();
        t.SalientPointId = map.AddSalientPoint({ pts[3 * i], pts[3 * i + 1], pts[3 * i + 2] });
        for (int64_t o = row_ptr[i]; o < row_ptr[i + 1]; ++o) {
            if (fr[o] < used) t.AddCorner((size_t)fr[o], { uv[2 * o], uv[2 * o + 1] });
            else frames[(size_t)(fr[o] - used)].push_back({ (size_t)i, { uv[2 * o], uv[2 * o + 1] }, 1.0 });
        }
    }
    for (int32_t j = 0; j < M; ++j) {
        SE3Transform& c = j < used ? cams[(size_t)j] : start[(size_t)(j - used)];
        Matrix3& k = j < used ? Ks[(size_t)j] : Kh[(size_t)(j - used)];
        for (int e = 0; e < 9; ++e) { c.R[(size_t)e] = R[9 * j + e]; k[(size_t)e] = K[9 * j + e]; }
        c.T = { T[3 * j], T[3 * j + 1], T[3 * j + 2] };
    }
    if (frames[0].size() != (size_t)N || frames[1].size() != (size_t)N) return 11;
    BundleAdjustmentKanataniTermCriteria crit;
    crit.AllowedReprojErrRelativeChange(1e-12);
    crit.MaxHessianFactor(1e6);
    BA ba;
    ba.SetFixedIntrinsics(true);
    ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 6);

    srk_resect_options opt;
    srk_resect_default_options(&opt);
    opt.attempts = 20;
    opt.rel_change = 0; // to the minimum: both runs below end where no attempt lowers E any more
    const std::vector<BA::ResectedFrame> res = ba.Resect(frames, start, nullptr, &Kh, &opt);
    if (res.size() != (size_t)held) return 12;
    // the C ABI on the same handle: the same bits
    std::vector<int64_t> rp{ 0, N, 2 * N };
    std::vector<int32_t> pt;
    std::vector<double> m, R0, T0, Kf, cR(9 * held), cT(3 * held), cq(6 * held), ci(36 * held);
    std::vector<uint32_t> cs((size_t)held);
    for (int j = 0; j < held; ++j) {
        for (const BA::ResectObservation& o : frames[(size_t)j]) { pt.push_back((int32_t)o.point); m.push_back(o.uv.x); m.push_back(o.uv.y); }
        R0.insert(R0.end(), start[(size_t)j].R.begin(), start[(size_t)j].R.end());
        T0.insert(T0.end(), { start[(size_t)j].T.x, start[(size_t)j].T.y, start[(size_t)j].T.z });
        Kf.insert(Kf.end(), Kh[(size_t)j].begin(), Kh[(size_t)j].end());
    }
    if (srk_ba_resect(ba.Handle(), held, rp.data(), pt.data(), m.data(), nullptr, Kf.data(), 0, R0.data(), T0.data(), &opt, 1, cR.data(), cT.data(),
                      cq.data(), ci.data(), cs.data(), nullptr) != SRK_OK) return 13;
    for (int j = 0; j < held; ++j) {
        const BA::ResectedFrame& f = res[(size_t)j];
        for (int e = 0; e < 9; ++e) if (f.pose.R[(size_t)e] != cR[9 * j + e]) return 14;
        if (f.pose.T.x != cT[3 * j] || f.pose.T.y != cT[3 * j + 1] || f.pose.T.z != cT[3 * j + 2] || f.rms_pixels != cq[6 * j] || f.status != cs[(size_t)j]) return 14;
        for (int e = 0; e < 36; ++e) if (f.info[(size_t)e] != ci[36 * j + e]) return 14;
        // q = 1 given explicitly is q = NULL, a multiply by 1.0; all points weighted, a well-posed frame at sub-pixel error
        if (f.status != SRK_RESECT_NOT_CONVERGED || f.points != (size_t)N || f.attempts != 20 || f.inlier_share != 1.0 || !(f.cond1 >= 1) ||
            !(f.min_depth > 0) || !(f.rms_pixels < 1.0) || !f.weights.empty())
            return 15;
        // near the generated pose (its noise is 0.005)
        double dr = 0, dt = 0;
        for (int e = 0; e < 9; ++e) dr = std::fmax(dr, std::fabs(f.pose.R[(size_t)e] - start[(size_t)j].R[(size_t)e]));
        dt = std::fabs(f.pose.T.x - start[(size_t)j].T.x) + std::fabs(f.pose.T.y - start[(size_t)j].T.y) + std::fabs(f.pose.T.z - start[(size_t)j].T.z);
        if (!(dr < 0.05 && dt < 0.2)) return 16;
    }
    // over the refined salient points, handed in: the same minimum up to the rounding of another coordinate frame
    std::vector<Point3> lm;
    for (const CornerTrack& t : rep.CornerTracks) lm.push_back(map.GetSalientPoint(*t.SalientPointId));
    const std::vector<BA::ResectedFrame> own = ba.ResectFrames(600.0, frames, lm, start, nullptr, &Kh, &opt);
    if (own.size() != (size_t)held) return 17;
    double worst = 0;
    for (int j = 0; j < held; ++j) {
        const BA::ResectedFrame &a = own[(size_t)j], &b = res[(size_t)j];
        for (int e = 0; e < 9; ++e) worst = std::fmax(worst, std::fabs(a.pose.R[(size_t)e] - b.pose.R[(size_t)e]));
        worst = std::fmax(worst, std::fabs(a.pose.T.x - b.pose.T.x) + std::fabs(a.pose.T.y - b.pose.T.y) + std::fabs(a.pose.T.z - b.pose.T.z));
        if (a.status != b.status || !(std::fabs(a.rms_pixels - b.rms_pixels) < 1e-9)) return 18;
    }
    if (!(worst < 1e-8)) return 18;
    // a loss: ten corners of the first frame moved by 40 px get a small weight, the rest a large one
    std::vector<std::vector<BA::ResectObservation>> moved = frames;
    for (size_t k = 0; k < 10; ++k) moved[0][7 * k].uv.x += 40;
    opt.attempts = 12;
    opt.loss_kind = 2;
    opt.loss_delta_pixels = 2;
    const std::vector<BA::ResectedFrame> robust = ba.Resect(moved, start, nullptr, &Kh, &opt, true);
    if (robust[0].weights.size() != (size_t)N || robust[1].weights.size() != (size_t)N) return 19;
    for (size_t k = 0; k < (size_t)N; ++k) {
        const bool is_moved = k % 7 == 0 && k / 7 < 10;
        if (is_moved ? !(robust[0].weights[k] < 0.05) : !(robust[0].weights[k] > 0.5)) return 19;
    }
    if (!(robust[0].inlier_share < 0.95) || !(robust[0].inlier_share > 0.5)) return 19;
    // refusals
    std::vector<Matrix3> fewer(Kh.begin(), Kh.end() - 1);
    if (!throws_invalid([&] { ba.Resect(frames, start, nullptr, &fewer); })) return 20;
    if (!throws_invalid([&] { ba.Resect(frames, start, nullptr, nullptr); })) return 21;
    std::vector<std::vector<BA::ResectObservation>> beyond = frames;
    beyond[1][3].point = (size_t)N;
    if (!throws_invalid([&] { ba.Resect(beyond, start, nullptr, &Kh); })) return 22;
    opt.attempts = 65;
    if (!throws_invalid([&] { ba.ResectFrames(600.0, frames, lm, start, nullptr, &Kh, &opt); })) return 23;
    // a frame with two corners
    std::vector<std::vector<BA::ResectObservation>> two(1, std::vector<BA::ResectObservation>(frames[0].begin(), frames[0].begin() + 2));
    const std::vector<BA::ResectedFrame> few = ba.Resect(two, { start[0] }, &Kh[0], nullptr);
    if (few.size() != 1 || few[0].status != SRK_RESECT_FEW_POINTS || few[0].points != 2 || !std::isnan(few[0].cond1) || few[0].pose.T.x != start[0].T.x) return 24;
    std::printf("frames %d, points %lld, worst distance between the two resections %.3e\n", held, (long long)N, worst);
    std::printf("resect adapter ok\n");
    return 0;
}
