// Runtime test of BundleAdjustmentKanatani::SetPositionPriors / ClearPositionPriors (include/suriko_amd/bundle-adj-kanatani.hpp)
// on a map whose salient points are NOT in track order: the landmark priors name salient points in map order and must reach the
// library in pnt_ind order (the order of the tracks), ascending.  The solve matches one through the C ABI with the indices
// mapped by hand, an index beyond the map and a repeated one throw, the priors change the result, the reported error carries the
// prior sums, and clearing leaves the handle without a setting.
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
    // priors: salient points 0, 5, 10, ... (map order, given in DESCENDING order) = landmarks N - 1, N - 6, ... (pnt_ind), each
    // at its own position moved by 4e-3 in x, with a full information matrix; frames 7 and 2 (given unsorted) at their centres
    // moved by 4e-3 in z
    using Prior = BundleAdjustmentKanatani::PositionPrior;
    std::vector<Prior> pp, fp;
    std::vector<int64_t> pi_ind;
    std::vector<double> pos_ind, info_ind;
    const std::array<double, 6> Lp = { 12.0, 1.5, -0.5, 9.0, 0.75, 15.0 }, Lf = { 120.0, 0, 0, 90.0, 0, 150.0 };
    for (int64_t k = ((N - 1) / 5) * 5; k >= 0; k -= 5) {
        const int64_t i = N - 1 - k;
        pp.push_back({ (size_t)k, { pts[3 * i] + 4e-3, pts[3 * i + 1], pts[3 * i + 2] }, Lp });
    }
    for (int64_t i = 0; i < N; ++i) {
        if ((N - 1 - i) % 5 != 0) continue;
        pi_ind.push_back(i);
        pos_ind.insert(pos_ind.end(), { pts[3 * i] + 4e-3, pts[3 * i + 1], pts[3 * i + 2] });
        info_ind.insert(info_ind.end(), Lp.begin(), Lp.end());
    }
    auto centre = [&](int32_t j, double c[3]) {
        for (int e = 0; e < 3; ++e) c[e] = -(R[9 * j + e] * T[3 * j] + R[9 * j + 3 + e] * T[3 * j + 1] + R[9 * j + 6 + e] * T[3 * j + 2]);
    };
    const int32_t fi_ind[2] = { 2, 7 };
    std::vector<double> fpos_ind, finfo_ind;
    for (int32_t j : { 7, 2 }) {
        double c[3];
        centre(j, c);
        fp.push_back({ (size_t)j, { c[0], c[1], c[2] + 4e-3 }, Lf });
    }
    for (int32_t j : fi_ind) {
        double c[3];
        centre(j, c);
        fpos_ind.insert(fpos_ind.end(), { c[0], c[1], c[2] + 4e-3 });
        finfo_ind.insert(finfo_ind.end(), Lf.begin(), Lf.end());
    }

    BundleAdjustmentKanataniTermCriteria crit;
    crit.AllowedReprojErrRelativeChange(1e-12);
    crit.MaxHessianFactor(1e6);
    BundleAdjustmentKanatani ba;
    {
        FragmentMap map; CornerTrackRepository rep; std::vector<SE3Transform> cams; std::vector<Matrix3> Ks;
        build(map, rep, cams, Ks);
        auto bad = pp;
        bad[0].index = (size_t)N; // beyond the map
        ba.SetPositionPriors(bad, fp, true);
        if (!throws_invalid([&] { ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 8); })) return 11;
        bad = pp;
        bad[1].index = bad[0].index; // named twice
        ba.SetPositionPriors(bad, fp, true);
        if (!throws_invalid([&] { ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 8); })) return 12;
        auto badf = fp;
        badf[0].index = (size_t)M; // a frame beyond the cameras: the upload refuses it
        ba.SetPositionPriors(pp, badf, true);
        if (!throws_invalid([&] { ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 8); })) return 13;
    }

    FragmentMap map; CornerTrackRepository rep; std::vector<SE3Transform> cams; std::vector<Matrix3> Ks;
    build(map, rep, cams, Ks);
    const size_t id0 = 1000001; // FragmentMap's default offset: the first salient point
    ba.SetPositionPriors(pp, fp, true);
    ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 8);
    const srk_ba_report ra = ba.Report();
    // the priors reached the handle in pnt_ind order
    int64_t np = 0;
    int32_t nf = 0;
    if (srk_ba_position_prior_counts(ba.Handle(), &np, &nf) != 1 || np != (int64_t)pi_ind.size() || nf != 2) return 14;
    std::vector<int64_t> gi((size_t)np);
    std::vector<double> gpos(3 * (size_t)np), ginfo(6 * (size_t)np), gfpos(6), gfinfo(12);
    int32_t gfi[2] = { -1, -1 };
    int kg = -1;
    if (srk_ba_position_priors(ba.Handle(), gi.data(), gpos.data(), ginfo.data(), gfi, gfpos.data(), gfinfo.data(), &kg) != 1) return 14;
    if (kg != 1 || gi != pi_ind || gpos != pos_ind || ginfo != info_ind || gfi[0] != 2 || gfi[1] != 7 || gfpos != fpos_ind || gfinfo != finfo_ind) return 15;
    double ep_a = 0, ef_a = 0;
    if (srk_ba_prior_error(ba.Handle(), &ep_a, &ef_a) != SRK_OK) return 15;

    // the same solve through the C ABI, indices mapped by hand
    auto pts2 = pts, R2 = R, T2 = T;
    srk_ba* h = srk_ba_create(0);
    srk_ba_report rb{};
    const double a = 1e-12, mx = 1e6;
    if (srk_ba_set_position_priors(h, (int64_t)pi_ind.size(), pi_ind.data(), pos_ind.data(), info_ind.data(), 2, fi_ind,
                                   fpos_ind.data(), finfo_ind.data(), 1) != SRK_OK) return 16;
    int rc2 = srk_ba_compute_inplace(h, 600.0, N, pts2.data(), M, R2.data(), T2.data(), K.data(), 0, row_ptr.data(), fr.data(),
                                     uv.data(), &a, &mx, 8, &rb);
    double ep_b = 0, ef_b = 0;
    if (rc2 < 0 || srk_ba_prior_error(h, &ep_b, &ef_b) != SRK_OK) return 16;
    // and without priors, for the difference they make
    auto pts3 = pts, R3 = R, T3 = T;
    srk_ba_report rep_none{};
    if (srk_ba_set_position_priors(h, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 1) != SRK_OK) return 16;
    if (srk_ba_compute_inplace(h, 600.0, N, pts3.data(), M, R3.data(), T3.data(), K.data(), 0, row_ptr.data(), fr.data(),
                               uv.data(), &a, &mx, 8, &rep_none) < 0) return 16;
    srk_ba_destroy(h);
    double maxd = 0, pull = 0;
    for (int64_t i = 0; i < N; ++i) {
        const Point3& p = map.GetSalientPoint(id0 + (size_t)(N - 1 - i)); // landmark i is salient point N - 1 - i
        const double q[3] = { p.x, p.y, p.z };
        for (int e = 0; e < 3; ++e) {
            maxd = std::fmax(maxd, std::fabs(q[e] - pts2[3 * i + e]));
            pull = std::fmax(pull, std::fabs(q[e] - pts3[3 * i + e]));
        }
    }
    for (int32_t j = 0; j < M; ++j) {
        const double t[3] = { cams[(size_t)j].T.x, cams[(size_t)j].T.y, cams[(size_t)j].T.z };
        for (int e = 0; e < 3; ++e) maxd = std::fmax(maxd, std::fabs(t[e] - T2[3 * j + e]));
    }
    std::printf("iterations %lld / %lld err %.17g / %.17g maxdiff %.3e; prior sums %.3e %.3e; moved by the priors %.3e\n",
                (long long)ra.iterations, (long long)rb.iterations, ra.err_final, rb.err_final, maxd, ep_a, ef_a, pull);
    if (ra.iterations != rb.iterations || ra.attempts != rb.attempts || ra.iterations < 1) return 17;
    if (std::fabs(ra.err_final - rb.err_final) > 1e-10 * std::fabs(rb.err_final) || maxd > 1e-8) return 18;
    if (std::fabs(ep_a - ep_b) > 1e-8 * ep_b || std::fabs(ef_a - ef_b) > 1e-8 * ef_b) return 19;
    if (!(ep_a > 0 && ef_a > 0)) return 20;
    if (!(pull > 1e-5)) return 21;                       // the priors changed the result
    if (!(ra.err_final > ep_a + ef_a)) return 22;        // the reported error is the reprojection sum plus the prior sums

    // cleared: the handle holds no setting
    ba.ClearPositionPriors();
    if (srk_ba_position_prior_counts(ba.Handle(), nullptr, nullptr) != 0) return 23;
    FragmentMap map3; CornerTrackRepository rep3; std::vector<SE3Transform> cams3; std::vector<Matrix3> Ks3;
    build(map3, rep3, cams3, Ks3);
    ba.ComputeInplace(600.0, map3, cams3, rep3, nullptr, &Ks3, crit, 8);
    double maxd3 = 0;
    for (int64_t i = 0; i < N; ++i) {
        const Point3& p = map3.GetSalientPoint(id0 + (size_t)(N - 1 - i));
        maxd3 = std::fmax(maxd3, std::fmax(std::fabs(p.x - pts3[3 * i]), std::fmax(std::fabs(p.y - pts3[3 * i + 1]), std::fabs(p.z - pts3[3 * i + 2]))));
    }
    if (maxd3 > 1e-8) return 24; // the run without priors
    std::printf("prior adapter ok\n");
    return 0;
}
