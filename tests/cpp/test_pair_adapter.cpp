// Runtime test of BundleAdjustmentKanatani::RefinePairs, RelateFramesRefined and PairFactor
// (include/suriko_amd/bundle-adj-kanatani.hpp): two pairs of frames of an all-visible generated scene, each frame with its own
// intrinsics, twenty matches of each moved by 40 px.  The chained call equals the C ABI's on the same handle bit for bit and
// RelateFrames followed by RefinePairs (on q times the inlier flags) gives the same bits again; the factor equals srk_pair_factor's;
// mismatched sizes and the library's refusals throw.
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
    srk_pair_options po;
    srk_pair_default_options(&po);
    po.attempts = 6, po.loss_kind = 2, po.loss_delta_pixels = 2.0, po.inliers_only = 1;
    BA ba;
    std::vector<BA::RelatedPair> related;
    const std::vector<BA::RefinedPair> res = ba.RelateFramesRefined(600.0, pairs, nullptr, nullptr, &Kas, &Kbs, &lo, po, &related, true, true);
    if (res.size() != 2 || related.size() != 2) return 12;

    // the C ABI on the same handle: the same bits
    std::vector<int64_t> rp{ 0, N, 2 * N };
    std::vector<double> ua, ub, q, Ka, Kb, cR(18), cT(6), cE(18), cl(16), cq(12), ci(50), cb(12), cw((size_t)(2 * N));
    std::vector<uint32_t> cs(2), crs(2);
    std::vector<uint8_t> cin((size_t)(2 * N));
    for (int p = 0; p < 2; ++p) {
        for (const BA::Match& m : pairs[(size_t)p]) {
            ua.insert(ua.end(), { m.a.x, m.a.y });
            ub.insert(ub.end(), { m.b.x, m.b.y });
            q.push_back(m.information);
        }
        Ka.insert(Ka.end(), Kas[(size_t)p].begin(), Kas[(size_t)p].end());
        Kb.insert(Kb.end(), Kbs[(size_t)p].begin(), Kbs[(size_t)p].end());
    }
    if (srk_relate_frames_refined(ba.Handle(), 600.0, 2, rp.data(), ua.data(), ub.data(), q.data(), Ka.data(), Kb.data(), 0, &lo, &po, cR.data(), cT.data(),
                                  cE.data(), cl.data(), crs.data(), cin.data(), cq.data(), ci.data(), cb.data(), cs.data(), cw.data()) != 0) return 13;
    const double ms = srk_ba_pair_kernel_ms(ba.Handle());
    if (!(ms > 0)) return 13;
    for (int p = 0; p < 2; ++p) {
        const BA::RefinedPair& r = res[(size_t)p];
        const BA::RelatedPair& l = related[(size_t)p];
        const double t[3] = { r.pose.T.x, r.pose.T.y, r.pose.T.z };
        if (std::memcmp(r.pose.R.data(), cR.data() + 9 * p, 72) || std::memcmp(t, cT.data() + 3 * p, 24) || std::memcmp(r.E.data(), cE.data() + 9 * p, 72)) return 14;
        if (std::memcmp(&r.rms_pixels, &cq[6 * p], 8) || std::memcmp(&r.mean_weight, &cq[6 * p + 2], 8) || std::memcmp(&r.condition, &cq[6 * p + 3], 8)) return 15;
        if (r.matches != (size_t)cq[6 * p + 1] || r.in_front != (size_t)cq[6 * p + 4] || r.attempts != (size_t)cq[6 * p + 5] || r.status != cs[(size_t)p]) return 16;
        if (std::memcmp(r.info.data(), ci.data() + 25 * p, 200) || std::memcmp(r.basis.data(), cb.data() + 6 * p, 48)) return 17;
        if (r.weights.size() != (size_t)N || std::memcmp(r.weights.data(), cw.data() + N * p, (size_t)(8 * N))) return 17;
        if (l.status != crs[(size_t)p] || l.winner != (int64_t)cl[8 * p + 3] || l.inlier_count != (size_t)cl[8 * p + 2] || std::memcmp(&l.rms_pixels, &cl[8 * p], 8)) return 18;
        if (l.inliers.size() != (size_t)N || std::memcmp(l.inliers.data(), cin.data() + N * p, (size_t)N)) return 18;
        // related and refined on the inliers: the moved matches are not among them and carry no weight
        if (l.status != 0 || r.status & (SRK_PAIR_FEW_POINTS | SRK_PAIR_DEGENERATE) || r.matches != l.inlier_count || r.matches < (size_t)(N - 25)) return 19;
        for (size_t k = 0; k < 20; ++k)
            if (l.inliers[3 * k + (size_t)p] || r.weights[3 * k + (size_t)p] != 0) return 19;
        if (std::fabs(t[0] * t[0] + t[1] * t[1] + t[2] * t[2] - 1.0) > 1e-15) return 20;
        std::printf("pair %d: rms %.3f px over %zu matches, %zu attempts, cond %.3e\n", p, r.rms_pixels, r.matches, r.attempts, r.condition);
    }

    // RelateFrames, then RefinePairs from its poses on q times the inlier flags: the same bits
    const std::vector<BA::RelatedPair> rel = ba.RelateFrames(600.0, pairs, nullptr, nullptr, &Kas, &Kbs, &lo, true);
    std::vector<std::vector<BA::Match>> masked = pairs;
    std::vector<SE3Transform> starts(2);
    for (int p = 0; p < 2; ++p) {
        starts[(size_t)p] = rel[(size_t)p].pose;
        for (size_t k = 0; k < (size_t)N; ++k) masked[(size_t)p][k].information *= (double)rel[(size_t)p].inliers[k];
    }
    srk_pair_options alone = po;
    alone.inliers_only = 0;
    const std::vector<BA::RefinedPair> two = ba.RefinePairs(600.0, masked, nullptr, nullptr, &Kas, &Kbs, starts, &alone, true);
    for (int p = 0; p < 2; ++p) {
        const BA::RefinedPair &a = two[(size_t)p], &b = res[(size_t)p];
        if (std::memcmp(a.pose.R.data(), b.pose.R.data(), 72) || std::memcmp(&a.pose.T, &b.pose.T, 24) || std::memcmp(a.info.data(), b.info.data(), 200) ||
            std::memcmp(&a.rms_pixels, &b.rms_pixels, 8) || a.status != b.status || a.attempts != b.attempts ||
            std::memcmp(a.weights.data(), b.weights.data(), (size_t)(8 * N)))
            return 21;
    }

    // the factor: srk_pair_factor's, and its null direction
    {
        const BA::RefinedPair& r = res[0];
        const BA::RelativePoseFactor f = BA::PairFactor(r, 2.0, 3, 7);
        const double t[3] = { r.pose.T.x, r.pose.T.y, r.pose.T.z };
        double Z[9], z[3], L[21];
        if (srk_pair_factor(r.pose.R.data(), t, r.info.data(), r.basis.data(), 2.0, Z, z, L) != 0) return 22;
        const double ft[3] = { f.rel_t.x, f.rel_t.y, f.rel_t.z };
        if (std::memcmp(Z, f.rel_R.data(), 72) || std::memcmp(z, ft, 24) || std::memcmp(L, f.info.data(), 168) || f.frame_a != 3 || f.frame_b != 7) return 22;
        if (std::fabs(std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]) - 2.0) > 1e-14) return 22;
        if (!throws_invalid([&] { BA::PairFactor(r, 0.0); })) return 22;
    }

    std::vector<Matrix3> one(1);
    std::vector<SE3Transform> short_starts(1);
    if (!throws_invalid([&] { ba.RefinePairs(600.0, pairs, nullptr, nullptr, &Kas, &Kbs, short_starts); })) return 23;       // one start for two pairs
    if (!throws_invalid([&] { ba.RefinePairs(600.0, pairs, nullptr, nullptr, &one, &Kbs, starts); })) return 24;            // one K_a for two pairs
    if (!throws_invalid([&] { ba.RelateFramesRefined(600.0, pairs, &Kas[0], nullptr, nullptr, &Kbs, &lo, po); })) return 25; // shared and separate mixed
    if (!throws_invalid([&] { ba.RefinePairs(600.0, pairs, nullptr, nullptr, &Kas, &Kbs, starts, &po); })) return 26;       // inliers_only without relate
    po.attempts = 65;
    if (!throws_invalid([&] { ba.RelateFramesRefined(600.0, pairs, nullptr, nullptr, &Kas, &Kbs, &lo, po); })) return 27;    // a refusal of the library
    if (srk_ba_pair_kernel_ms(ba.Handle()) <= 0) return 28;
    std::printf("pair adapter ok\n");
    return 0;
}
