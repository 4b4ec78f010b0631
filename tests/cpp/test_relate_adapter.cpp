// Runtime test of BundleAdjustmentKanatani::RelateFrames (include/suriko_amd/bundle-adj-kanatani.hpp): two pairs of frames of an
// all-visible generated scene are related from the corners of their common landmarks, twenty of them moved by 40 px; the result
// equals the C ABI's on the same handle bit for bit and marks no moved match an inlier; shared intrinsics give the same bits as one
// matrix per pair; mismatched sizes throw.
#include <cmath>
#include <cstdio>
#include <cstring>
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
    spec.noise_uv_pix = 0.3; spec.seed = 93;
    const int64_t N = (int64_t)spec.grid_nx * spec.grid_ny, O = srk_scene_num_observations(&spec);
    const int32_t M = spec.n_frames;
    std::vector<double> pts(3 * N), R(9 * M), T(3 * M), K(9 * M), uv(2 * O);
    std::vector<int64_t> row_ptr(N + 1);
    std::vector<int32_t> fr(O);
    if (srk_scene_generate(&spec, pts.data(), nullptr, R.data(), T.data(), nullptr, nullptr, K.data(), row_ptr.data(),
                           fr.data(), uv.data()) != 0) return 10;
    distinct_intrinsics(M, spec.f0, K, fr, uv); // every frame its own fx, fy, u0, v0: the adapter must hand each frame's own K on
    if (!intrinsics_are_distinct(M, K)) return 10;
    using BA = BundleAdjustmentKanatani;
    const int32_t fa[2] = { 0, 2 }, fb[2] = { 5, 9 };
    std::vector<std::vector<BA::Match>> pairs(2);
    for (int p = 0; p < 2; ++p)
        for (int64_t i = 0; i < N; ++i) {
            BA::Match m;
            int seen = 0;
            for (int64_t o = row_ptr[i]; o < row_ptr[i + 1]; ++o) {
                if (fr[o] == fa[p]) m.a = { uv[2 * o], uv[2 * o + 1] }, ++seen;
                if (fr[o] == fb[p]) m.b = { uv[2 * o], uv[2 * o + 1] }, ++seen;
            }
            if (seen == 2) pairs[(size_t)p].push_back(m);
        }
    if (pairs[0].size() != (size_t)N || pairs[1].size() != (size_t)N) return 11;
    for (int p = 0; p < 2; ++p)
        for (size_t k = 0; k < 20; ++k) pairs[(size_t)p][3 * k + (size_t)p].b.x += 40; // wrong matches
    pairs[1][70].information = 0;                                                         // and one switched off
    std::vector<Matrix3> Kas(2), Kbs(2);
    for (int p = 0; p < 2; ++p)
        for (int e = 0; e < 9; ++e) { Kas[(size_t)p][(size_t)e] = K[9 * fa[p] + e]; Kbs[(size_t)p][(size_t)e] = K[9 * fb[p] + e]; }
    srk_relate_options lo;
    srk_relate_default_options(&lo);
    lo.hypotheses = 128;
    BA ba;
    const std::vector<BA::RelatedPair> res = ba.RelateFrames(600.0, pairs, nullptr, nullptr, &Kas, &Kbs, &lo, true);
    if (res.size() != 2) return 12;

    // the C ABI on the same handle: the same bits
    std::vector<int64_t> rp{ 0, N, 2 * N };
    std::vector<double> ua, ub, q, Ka, Kb, cR(18), cT(6), cE(18), cl(16);
    std::vector<uint32_t> cs(2);
    std::vector<uint8_t> ci((size_t)(2 * N));
    for (int p = 0; p < 2; ++p) {
        for (const BA::Match& m : pairs[(size_t)p]) {
            ua.insert(ua.end(), { m.a.x, m.a.y });
            ub.insert(ub.end(), { m.b.x, m.b.y });
            q.push_back(m.information);
        }
        Ka.insert(Ka.end(), Kas[(size_t)p].begin(), Kas[(size_t)p].end());
        Kb.insert(Kb.end(), Kbs[(size_t)p].begin(), Kbs[(size_t)p].end());
    }
    if (srk_relate_frames(ba.Handle(), 600.0, 2, rp.data(), ua.data(), ub.data(), q.data(), Ka.data(), Kb.data(), 0, &lo, cR.data(), cT.data(), cE.data(),
                          cl.data(), cs.data(), ci.data()) != 0) return 13;
    for (int p = 0; p < 2; ++p) {
        const BA::RelatedPair& r = res[(size_t)p];
        const double t[3] = { r.pose.T.x, r.pose.T.y, r.pose.T.z };
        if (std::memcmp(r.pose.R.data(), cR.data() + 9 * p, 72) || std::memcmp(t, cT.data() + 3 * p, 24) || std::memcmp(r.E.data(), cE.data() + 9 * p, 72)) return 14;
        if (std::memcmp(&r.rms_pixels, &cl[8 * p], 8) || std::memcmp(&r.sixth_match_pixels, &cl[8 * p + 5], 8) || std::memcmp(&r.parallax_rad, &cl[8 * p + 7], 8)) return 15;
        if (r.matches != (size_t)cl[8 * p + 1] || r.inlier_count != (size_t)cl[8 * p + 2] || r.winner != (int64_t)cl[8 * p + 3] ||
            r.hypotheses_with_model != (size_t)cl[8 * p + 4] || r.in_front != (size_t)cl[8 * p + 6] || r.status != cs[(size_t)p])
            return 16;
        if (r.inliers.size() != (size_t)N || std::memcmp(r.inliers.data(), ci.data() + N * p, (size_t)N)) return 17;
        // related, no moved match among the inliers; the distance to the generated relative pose (R_b R_a^T, T_b - R_rel T_a up to
        // scale) is printed only: the generated landmarks lie on a plane, where two essential matrices fit every match
        if (r.status != 0 || r.matches != (size_t)(N - p) || r.inlier_count < (size_t)(N - 25)) return 18;
        for (size_t k = 0; k < 20; ++k)
            if (r.inliers[3 * k + (size_t)p]) return 19;
        if (p == 1 && r.inliers[70]) return 20;
        const double* Ra = R.data() + 9 * fa[p];
        const double* Rb = R.data() + 9 * fb[p];
        double Rrel[9], Trel[3], tr = 0, nt = 0, dot = 0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Rrel[3 * i + j] = Rb[3 * i] * Ra[3 * j] + Rb[3 * i + 1] * Ra[3 * j + 1] + Rb[3 * i + 2] * Ra[3 * j + 2];
        for (int i = 0; i < 3; ++i)
            Trel[i] = T[3 * fb[p] + i] - (Rrel[3 * i] * T[3 * fa[p]] + Rrel[3 * i + 1] * T[3 * fa[p] + 1] + Rrel[3 * i + 2] * T[3 * fa[p] + 2]);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) tr += Rrel[3 * i + j] * r.pose.R[(size_t)(3 * i + j)];
        for (int i = 0; i < 3; ++i) nt += Trel[i] * Trel[i], dot += Trel[i] * t[i];
        const double angle = std::acos(std::fmin(1.0, 0.5 * (tr - 1.0))), dir = std::acos(std::fmin(1.0, dot / std::sqrt(nt)));
        std::printf("pair %d: rotation %.3e rad, direction %.3e rad from the generated pose, %zu inliers\n", p, angle, dir, r.inlier_count);
    }

    // shared intrinsics (K_a != K_b): the bits of the call that repeats the two matrices per pair.  The frames carry distinct K, so
    // pair 1 of that call is not pair 1 above, and pair 0 is
    if (std::memcmp(Kas[0].data(), Kas[1].data(), 72) == 0 || std::memcmp(Kbs[0].data(), Kbs[1].data(), 72) == 0 ||
        std::memcmp(Kas[0].data(), Kbs[0].data(), 72) == 0) return 21;
    const std::vector<Matrix3> Ka0(2, Kas[0]), Kb0(2, Kbs[0]);
    const std::vector<BA::RelatedPair> sh = ba.RelateFrames(600.0, pairs, &Kas[0], &Kbs[0], nullptr, nullptr, &lo);
    const std::vector<BA::RelatedPair> rep = ba.RelateFrames(600.0, pairs, nullptr, nullptr, &Ka0, &Kb0, &lo);
    for (int p = 0; p < 2; ++p) {
        const BA::RelatedPair &s = sh[(size_t)p], &r = rep[(size_t)p];
        if (std::memcmp(s.pose.R.data(), r.pose.R.data(), 72) || std::memcmp(s.E.data(), r.E.data(), 72) || std::memcmp(&s.rms_pixels, &r.rms_pixels, 8) ||
            s.winner != r.winner || s.inlier_count != r.inlier_count || s.status != r.status || !s.inliers.empty())
            return 22;
    }
    if (std::memcmp(sh[0].pose.R.data(), res[0].pose.R.data(), 72) || sh[0].winner != res[0].winner) return 22;
    if (std::memcmp(sh[1].pose.R.data(), res[1].pose.R.data(), 72) == 0) return 22;   // pair 1 with pair 0's cameras is another problem

    std::vector<Matrix3> one(1);
    if (!throws_invalid([&] { ba.RelateFrames(600.0, pairs, nullptr, nullptr, &one, &Kbs); })) return 23;       // one K_a for two pairs
    if (!throws_invalid([&] { ba.RelateFrames(600.0, pairs, &Kas[0], nullptr, nullptr, &Kbs); })) return 24;    // shared and separate mixed
    if (!throws_invalid([&] { ba.RelateFrames(600.0, pairs, nullptr, nullptr, nullptr, nullptr); })) return 25; // no intrinsics
    lo.hypotheses = 0;
    if (!throws_invalid([&] { ba.RelateFrames(600.0, pairs, nullptr, nullptr, &Kas, &Kbs, &lo); })) return 26;  // a refusal of the library
    std::printf("relate adapter ok\n");
    return 0;
}
