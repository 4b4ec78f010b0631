// Runtime test of BundleAdjustmentKanatani::SetObservationInformation / ObservationResiduals
// (include/suriko_amd/bundle-adj-kanatani.hpp): refusals throw std::invalid_argument, the values reach the handle, a solve on
// that handle matches one with the information set through the C ABI on a handle of its own, an empty vector clears it, and
// the residuals are those the C ABI returns.
#include <cmath>
#include <cstdio>
#include <limits>
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
    spec.noise_uv_pix = 0.5; spec.seed = 77;
    const int64_t N = (int64_t)spec.grid_nx * spec.grid_ny, O = srk_scene_num_observations(&spec);
    const int32_t M = spec.n_frames;
    std::vector<double> pts(3 * N), R(9 * M), T(3 * M), K(9 * M), uv(2 * O);
    std::vector<int64_t> row_ptr(N + 1);
    std::vector<int32_t> fr(O);
    if (srk_scene_generate(&spec, pts.data(), nullptr, R.data(), T.data(), nullptr, nullptr, K.data(), row_ptr.data(),
                           fr.data(), uv.data()) != 0) return 14;
    // every 17th observation 40 px off and switched off; the others between 0.5 and 2
    std::vector<Scalar> q((size_t)O);
    for (int64_t o = 0; o < O; ++o) q[(size_t)o] = o % 17 == 0 ? 0.0 : 0.5 + 0.25 * (double)(o % 7);
    for (int64_t o = 0; o < O; o += 17) uv[2 * o] += 40.0;

    BundleAdjustmentKanatani ba;
    std::vector<Scalar> bad = q;
    bad[3] = -1.0;
    if (!throws_invalid([&] { ba.SetObservationInformation(bad); })) return 10;
    bad[3] = std::numeric_limits<double>::quiet_NaN();
    if (!throws_invalid([&] { ba.SetObservationInformation(bad); })) return 11;
    bad[3] = std::numeric_limits<double>::infinity();
    if (!throws_invalid([&] { ba.SetObservationInformation(bad); })) return 12;
    ba.SetObservationInformation(q);
    std::vector<double> back((size_t)O);
    if (srk_ba_observation_information(ba.Handle(), back.data(), O) != SRK_OK || back != q) return 13;

    auto pts2 = pts, R2 = R, T2 = T, pts3 = pts, R3 = R, T3 = T;
    srk_ba_report ra{}, rb{}, rc3{};
    int rc = srk_ba_compute_inplace(ba.Handle(), 600.0, N, pts.data(), M, R.data(), T.data(), K.data(), 0, row_ptr.data(),
                                    fr.data(), uv.data(), nullptr, nullptr, 8, &ra);
    std::vector<Scalar> res = ba.ObservationResiduals();
    srk_ba* h = srk_ba_create(0);
    if (srk_ba_set_observation_information(h, q.data(), O) != SRK_OK) return 15;
    int rc2 = srk_ba_compute_inplace(h, 600.0, N, pts2.data(), M, R2.data(), T2.data(), K.data(), 0, row_ptr.data(),
                                     fr.data(), uv.data(), nullptr, nullptr, 8, &rb);
    std::vector<double> res2((size_t)(2 * O));
    int rcr = srk_ba_observation_residuals(h, res2.data(), O);
    srk_ba_destroy(h);
    if (rc < 0 || rc2 < 0 || rcr != SRK_OK || (int64_t)res.size() != 2 * O) return 16;
    double maxd = 0, maxr = 0, min_off = 1e300, max_on = 0;
    for (size_t i = 0; i < pts.size(); ++i) maxd = std::fmax(maxd, std::fabs(pts[i] - pts2[i]));
    for (int64_t o = 0; o < O; ++o) {
        maxr = std::fmax(maxr, std::fmax(std::fabs(res[2 * o] - res2[2 * o]), std::fabs(res[2 * o + 1] - res2[2 * o + 1])));
        const double pix = std::hypot(res[2 * o], res[2 * o + 1]);
        if (o % 17 == 0) min_off = std::fmin(min_off, pix);
        else max_on = std::fmax(max_on, pix);
    }
    // an empty vector clears the setting: the 40 px observations pull again and the result differs
    ba.SetObservationInformation({});
    int rc4 = srk_ba_compute_inplace(ba.Handle(), 600.0, N, pts3.data(), M, R3.data(), T3.data(), K.data(), 0, row_ptr.data(),
                                     fr.data(), uv.data(), nullptr, nullptr, 8, &rc3);
    if (rc4 < 0) return 20;
    std::printf("iterations %lld / %lld err %.17g / %.17g maxdiff %.3e residual diff %.3e px; switched off >= %.2f px, others <= %.2f px; "
                "cleared err %.6g\n", (long long)ra.iterations, (long long)rb.iterations, ra.err_final, rb.err_final, maxd, maxr,
                min_off, max_on, rc3.err_final);
    if (ra.iterations != rb.iterations || ra.attempts != rb.attempts) return 17;
    if (std::fabs(ra.err_final - rb.err_final) > 1e-10 * std::fabs(rb.err_final) || maxd > 1e-8 || maxr > 1e-6) return 18;
    // switched off, the moved observations keep their 40 px; the others settle at the noise (0.5 px: below 5 px)
    if (!(min_off > 30.0 && max_on < 5.0)) return 19;
    if (!(rc3.err_final > 10 * ra.err_final)) return 21;
    std::printf("information adapter ok\n");
    return 0;
}
