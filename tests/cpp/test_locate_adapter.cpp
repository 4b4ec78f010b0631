// Runtime test of BundleAdjustmentKanatani::Locate and ::LocateFrames (include/suriko_amd/bundle-adj-kanatani.hpp): after a
// ComputeInplace over the first ten frames of an all-visible scene, the two held-out frames are located from their corners over
// the resident landmarks, thirty of them moved by 40 px and no pose given; the result equals the C ABI's on the same handle bit
// for bit, lies at the generated poses and marks no moved corner an inlier; the caller's landmarks give the same winner, and refined on the
// device they give ResectFrames from the located poses bit for bit; mismatched sizes and a landmark beyond the scene throw.
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
    FragmentMap map; CornerTrackRepository rep; std::vector<SE3Transform> cams((size_t)used), truth((size_t)held);
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
        SE3Transform& c = j < used ? cams[(size_t)j] : truth[(size_t)(j - used)];
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

    // thirty corners of each held-out frame moved by 40 px: wrong matches
    std::vector<std::vector<BA::ResectObservation>> moved = frames;
    for (int j = 0; j < held; ++j)
        for (size_t k = 0; k < 30; ++k) moved[(size_t)j][2 * k + (size_t)j].uv.x += 40;
    srk_locate_options lo;
    srk_locate_default_options(&lo);
    lo.hypotheses = 128;
    const std::vector<BA::LocatedFrame> res = ba.Locate(moved, nullptr, &Kh, &lo, nullptr, true);
    if (res.size() != (size_t)held) return 12;
    // the C ABI on the same handle: the same bits
    std::vector<int64_t> rp{ 0, N, 2 * N };
    std::vector<int32_t> pt;
    std::vector<double> m, Kf, cR(9 * held), cT(3 * held), cl(6 * held);
    std::vector<uint32_t> cs((size_t)held);
    std::vector<uint8_t> ci((size_t)(2 * N));
    for (int j = 0; j < held; ++j) {
        for (const BA::ResectObservation& o : moved[(size_t)j]) { pt.push_back((int32_t)o.point); m.push_back(o.uv.x); m.push_back(o.uv.y); }
        Kf.insert(Kf.end(), Kh[(size_t)j].begin(), Kh[(size_t)j].end());
    }
    if (srk_ba_locate(ba.Handle(), held, rp.data(), pt.data(), m.data(), nullptr, Kf.data(), 0, &lo, nullptr, 1, cR.data(), cT.data(), cl.data(), cs.data(),
                      ci.data(), nullptr, nullptr, nullptr, nullptr) != SRK_OK) return 13;
    for (int j = 0; j < held; ++j) {
        const BA::LocatedFrame& f = res[(size_t)j];
        for (int e = 0; e < 9; ++e) if (f.pose.R[(size_t)e] != cR[9 * j + e]) return 14;
        if (f.pose.T.x != cT[3 * j] || f.pose.T.y != cT[3 * j + 1] || f.pose.T.z != cT[3 * j + 2] || f.rms_pixels != cl[6 * j] ||
            f.located_status != cs[(size_t)j] || f.winner != (int64_t)cl[6 * j + 3])
            return 14;
        if (f.located_status != 0 || f.points != (size_t)N || f.inliers.size() != (size_t)N || f.hypotheses_with_pose == 0 || f.winner < 0 || f.winner >= 128)
            return 15;
        size_t marked = 0;
        for (size_t k = 0; k < (size_t)N; ++k) {
            if (f.inliers[k] != ci[(size_t)(j * N) + k]) return 14;
            const bool is_moved = k >= (size_t)j && (k - (size_t)j) % 2 == 0 && (k - (size_t)j) / 2 < 30;
            if (is_moved && f.inliers[k]) return 16; // 40 px against a threshold of 4
            marked += f.inliers[k];
        }
        if (marked != f.inlier_count || !(marked >= (size_t)(N - 30) * 8 / 10)) return 16;
        // near the generated pose (its noise is 0.005; a minimal sample at 0.3 px of noise adds its own)
        double dr = 0;
        for (int e = 0; e < 9; ++e) dr = std::fmax(dr, std::fabs(f.pose.R[(size_t)e] - truth[(size_t)j].R[(size_t)e]));
        const double dt = std::fabs(f.pose.T.x - truth[(size_t)j].T.x) + std::fabs(f.pose.T.y - truth[(size_t)j].T.y) + std::fabs(f.pose.T.z - truth[(size_t)j].T.z);
        if (!(dr < 0.05 && dt < 0.3)) return 17;
    }
    // over the refined salient points, handed in: the same winner and inliers
    std::vector<Point3> lm;
    for (const CornerTrack& t : rep.CornerTracks) lm.push_back(map.GetSalientPoint(*t.SalientPointId));
    const std::vector<BA::LocatedFrame> own = ba.LocateFrames(600.0, moved, lm, nullptr, &Kh, &lo);
    if (own.size() != (size_t)held) return 19;
    for (int j = 0; j < held; ++j)
        if (own[(size_t)j].winner != res[(size_t)j].winner || own[(size_t)j].inlier_count != res[(size_t)j].inlier_count) return 19;
    // refined on the device: what ResectFrames gives from the located poses, bit for bit (over the caller's landmarks: the resident
    // form maps the located poses out of and the starts into the normalised coordinates, which rounds)
    srk_resect_options opt;
    srk_resect_default_options(&opt);
    opt.attempts = 12;
    opt.loss_kind = 2;
    opt.loss_delta_pixels = 2;
    const std::vector<BA::LocatedFrame> fine = ba.LocateFrames(600.0, moved, lm, nullptr, &Kh, &lo, &opt, false, true);
    std::vector<SE3Transform> start;
    for (const BA::LocatedFrame& f : own) start.push_back(f.pose);
    const std::vector<BA::ResectedFrame> chained = ba.ResectFrames(600.0, moved, lm, start, nullptr, &Kh, &opt, true);
    for (int j = 0; j < held; ++j) {
        const BA::ResectedFrame &a = fine[(size_t)j].refined, &b = chained[(size_t)j];
        if (fine[(size_t)j].winner != own[(size_t)j].winner || a.weights.size() != (size_t)N) return 18;
        if (a.rms_pixels != b.rms_pixels || a.status != b.status || a.attempts != b.attempts || a.weights != b.weights) return 18;
        for (int e = 0; e < 9; ++e) if (a.pose.R[(size_t)e] != b.pose.R[(size_t)e] || fine[(size_t)j].pose.R[(size_t)e] != b.pose.R[(size_t)e]) return 18;
        if (a.pose.T.x != b.pose.T.x || a.pose.T.y != b.pose.T.y || a.pose.T.z != b.pose.T.z) return 18;
    }
    // and on the resident scene: the same located frame, a refined pose at the generated one
    const std::vector<BA::LocatedFrame> resident = ba.Locate(moved, nullptr, &Kh, &lo, &opt);
    for (int j = 0; j < held; ++j) {
        const BA::LocatedFrame& f = resident[(size_t)j];
        double dr = 0;
        for (int e = 0; e < 9; ++e) dr = std::fmax(dr, std::fabs(f.pose.R[(size_t)e] - truth[(size_t)j].R[(size_t)e]));
        if (f.winner != res[(size_t)j].winner || !(dr < 0.05) || !(f.refined.rms_pixels > 0) || f.refined.points != (size_t)N) return 25;
    }
    // refusals
    std::vector<Matrix3> fewer(Kh.begin(), Kh.end() - 1);
    if (!throws_invalid([&] { ba.Locate(frames, nullptr, &fewer); })) return 20;
    if (!throws_invalid([&] { ba.Locate(frames, nullptr, nullptr); })) return 21;
    std::vector<std::vector<BA::ResectObservation>> beyond = frames;
    beyond[1][3].point = (size_t)N;
    if (!throws_invalid([&] { ba.Locate(beyond, nullptr, &Kh); })) return 22;
    lo.hypotheses = 4097;
    if (!throws_invalid([&] { ba.LocateFrames(600.0, frames, lm, nullptr, &Kh, &lo); })) return 23;
    // a frame with three corners
    std::vector<std::vector<BA::ResectObservation>> three(1, std::vector<BA::ResectObservation>(frames[0].begin(), frames[0].begin() + 3));
    const std::vector<BA::LocatedFrame> few = ba.Locate(three, &Kh[0], nullptr);
    if (few.size() != 1 || few[0].located_status != SRK_LOCATE_FEW_POINTS || few[0].points != 3 || few[0].winner != -1 || !std::isnan(few[0].rms_pixels) ||
        few[0].pose.T.x != 0 || few[0].pose.R[0] != 1)
        return 24;
    std::printf("frames %d, points %lld, winners %lld %lld\n", held, (long long)N, (long long)res[0].winner, (long long)res[1].winner);
    std::printf("locate adapter ok\n");
    return 0;
}
