// Runtime test of BundleAdjustmentKanatani::SetJointPosePriors / ClearJointPosePriors
// (include/suriko_amd/bundle-adj-kanatani.hpp): the sets reach the library as given, the solve matches one through the C ABI
// with the arrays built by hand, a camera beyond the cameras, sizes that do not fit and two sets sharing two cameras throw, the
// priors change the result, the reported error carries the prior sum, and clearing leaves the handle without a setting.
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

    auto build = [&](FragmentMap& map, CornerTrackRepository& rep, std::vector<SE3Transform>& cams, std::vector<Matrix3>& Ks) {
        for (int64_t i = 0; i < N; ++i) {
            CornerTrack& t = rep.AddCornerTrackObj();
            t.SalientPointId = map.AddSalientPoint({ pts[3 * i], pts[3 * i + 1], pts[3 * i + 2] });
            for (int64_t o = row_ptr[i]; o < row_ptr[i + 1]; ++o) t.AddCorner((size_t)fr[o], { uv[2 * o], uv[2 * o + 1] });
        }
        cams.resize((size_t)M);
        Ks.resize((size_t)M);
        for (int32_t j = 0; j < M; ++j) {
            for (int e = 0; e < 9; ++e) { cams[(size_t)j].R[(size_t)e] = R[9 * j + e]; Ks[(size_t)j][(size_t)e] = K[9 * j + e]; }
            cams[(size_t)j].T = { T[3 * j], T[3 * j + 1], T[3 * j + 2] };
        }
    };
    // a set over the given cameras: linearised at the scene's own poses with the centres moved by 4e-3 in x; the information
    // matrix diagonally dominant with every block non-zero: 100 / 50 on the diagonal, 2 everywhere else in the [t; t] and
    // [r; r] positions of the off-diagonal blocks
    using Set = BundleAdjustmentKanatani::JointPosePrior;
    auto make = [&](std::vector<int32_t> frames, bool with_mean) {
        Set s;
        const size_t k = frames.size(), n = 6 * k;
        for (int32_t j : frames) {
            s.frames.push_back((size_t)j);
            std::array<Scalar, 9> r;
            for (int e = 0; e < 9; ++e) r[(size_t)e] = R[9 * j + e];
            s.lin_R.push_back(r);
            double c[3];
            for (int e = 0; e < 3; ++e) c[e] = -(R[9 * j + e] * T[3 * j] + R[9 * j + 3 + e] * T[3 * j + 1] + R[9 * j + 6 + e] * T[3 * j + 2]);
            s.lin_C.push_back({ c[0] + 4e-3, c[1], c[2] });
        }
        s.info.assign(n * n, 0.0);
        for (size_t a = 0; a < n; ++a)
            for (size_t b = 0; b < n; ++b)
                s.info[a * n + b] = a == b ? (a % 6 < 3 ? 100.0 : 50.0) : (a / 6 != b / 6 && a % 6 == b % 6 ? 2.0 : 0.0);
        if (with_mean) {
            s.mean.assign(n, 0.0);
            s.mean[1] = 1e-3;
        }
        return s;
    };
    const std::vector<Set> given = { make({ 1, 2, 5 }, true), make({ 5, 6, 11 }, false), make({ 8 }, false) };
    std::vector<int32_t> ptr(1, 0), ff;
    std::vector<double> fR, fC, fm, fL;
    for (const Set& s : given) {
        ptr.push_back(ptr.back() + (int32_t)s.frames.size());
        for (size_t i = 0; i < s.frames.size(); ++i) {
            ff.push_back((int32_t)s.frames[i]);
            fR.insert(fR.end(), s.lin_R[i].begin(), s.lin_R[i].end());
            fC.insert(fC.end(), { s.lin_C[i].x, s.lin_C[i].y, s.lin_C[i].z });
        }
        if (s.mean.empty()) fm.insert(fm.end(), 6 * s.frames.size(), 0.0);
        else fm.insert(fm.end(), s.mean.begin(), s.mean.end());
        fL.insert(fL.end(), s.info.begin(), s.info.end());
    }

    BundleAdjustmentKanataniTermCriteria crit;
    crit.AllowedReprojErrRelativeChange(1e-12);
    crit.MaxHessianFactor(1e6);
    BundleAdjustmentKanatani ba;
    {
        FragmentMap map; CornerTrackRepository rep; std::vector<SE3Transform> cams; std::vector<Matrix3> Ks;
        build(map, rep, cams, Ks);
        auto bad = given;
        bad[1].frames[2] = (size_t)M; // beyond the cameras: the upload refuses it
        ba.SetJointPosePriors(bad);
        if (!throws_invalid([&] { ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 8); })) return 11;
        bad = given;
        bad[1].info.pop_back(); // sizes that do not fit
        ba.SetJointPosePriors(bad);
        if (!throws_invalid([&] { ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 8); })) return 12;
        bad = given;
        bad.push_back(make({ 2, 5, 9 }, false)); // shares cameras 2 and 5 with the first set
        ba.SetJointPosePriors(bad);
        if (!throws_invalid([&] { ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 8); })) return 13;
    }

    FragmentMap map; CornerTrackRepository rep; std::vector<SE3Transform> cams; std::vector<Matrix3> Ks;
    build(map, rep, cams, Ks);
    ba.SetJointPosePriors(given);
    ba.ComputeInplace(600.0, map, cams, rep, nullptr, &Ks, crit, 8);
    const srk_ba_report ra = ba.Report();
    int32_t ns = 0, nq = 0;
    int64_t ni = 0;
    if (srk_ba_joint_pose_prior_counts(ba.Handle(), &ns, &nq, &ni) != 1 || ns != 3 || nq != 7 || ni != (int64_t)fL.size()) return 14;
    std::vector<int32_t> gp(4), gf(7);
    std::vector<double> gR(63), gC(21), gm(42), gL((size_t)ni);
    int kg = 0;
    if (srk_ba_joint_pose_priors(ba.Handle(), gp.data(), gf.data(), gR.data(), gC.data(), gm.data(), gL.data(), &kg) != 1) return 14;
    if (gp != ptr || gf != ff || gR != fR || gC != fC || gm != fm || gL != fL || kg != 1) return 15;
    double e_a = 0;
    if (srk_ba_joint_pose_prior_error(ba.Handle(), &e_a) != SRK_OK) return 15;

    // the same solve through the C ABI, the arrays built by hand
    auto pts2 = pts, R2 = R, T2 = T;
    srk_ba* h = srk_ba_create(0);
    srk_ba_report rb{};
    const double a = 1e-12, mx = 1e6;
    if (srk_ba_set_joint_pose_priors(h, 3, ptr.data(), ff.data(), fR.data(), fC.data(), fm.data(), fL.data(), 1) != SRK_OK) return 16;
    int rc2 = srk_ba_compute_inplace(h, 600.0, N, pts2.data(), M, R2.data(), T2.data(), K.data(), 0, row_ptr.data(), fr.data(),
                                     uv.data(), &a, &mx, 8, &rb);
    double e_b = 0;
    if (rc2 < 0 || srk_ba_joint_pose_prior_error(h, &e_b) != SRK_OK) return 16;
    std::vector<double> res(42);
    if (srk_ba_joint_pose_prior_residuals(h, res.data()) != SRK_OK) return 16;
    // and without priors, for the difference they make
    auto pts3 = pts, R3 = R, T3 = T;
    srk_ba_report rep_none{};
    if (srk_ba_set_joint_pose_priors(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1) != SRK_OK) return 16;
    if (srk_ba_compute_inplace(h, 600.0, N, pts3.data(), M, R3.data(), T3.data(), K.data(), 0, row_ptr.data(), fr.data(),
                               uv.data(), &a, &mx, 8, &rep_none) < 0) return 16;
    srk_ba_destroy(h);
    double maxd = 0, pull = 0;
    for (int32_t j = 0; j < M; ++j) {
        const double t[3] = { cams[(size_t)j].T.x, cams[(size_t)j].T.y, cams[(size_t)j].T.z };
        for (int e = 0; e < 3; ++e) {
            maxd = std::fmax(maxd, std::fabs(t[e] - T2[3 * j + e]));
            pull = std::fmax(pull, std::fabs(t[e] - T3[3 * j + e]));
        }
    }
    double eres = 0; // the prior sum from the residual download and the information matrices
    size_t q = 0;
    for (const Set& s : given) {
        const size_t n = 6 * s.frames.size();
        for (size_t x = 0; x < n; ++x)
            for (size_t y = 0; y < n; ++y) eres += res[6 * q + x] * s.info[x * n + y] * res[6 * q + y];
        q += s.frames.size();
    }
    std::printf("iterations %lld / %lld err %.17g / %.17g maxdiff %.3e; prior sum %.3e (from residuals %.3e); moved by the priors %.3e\n",
                (long long)ra.iterations, (long long)rb.iterations, ra.err_final, rb.err_final, maxd, e_a, eres, pull);
    if (ra.iterations != rb.iterations || ra.attempts != rb.attempts || ra.iterations < 1) return 17;
    if (std::fabs(ra.err_final - rb.err_final) > 1e-10 * std::fabs(rb.err_final) || maxd > 1e-8) return 18;
    if (std::fabs(e_a - e_b) > 1e-8 * e_b || !(e_a > 0)) return 19;
    if (std::fabs(eres - e_b) > 1e-6 * e_b) return 20;
    if (!(pull > 1e-5)) return 21;                // the priors changed the result
    if (!(ra.err_final > e_a)) return 22;         // the reported error is the reprojection sum plus the prior sum

    // cleared: the handle holds no setting
    ba.ClearJointPosePriors();
    if (srk_ba_joint_pose_prior_counts(ba.Handle(), nullptr, nullptr, nullptr) != 0) return 23;
    FragmentMap map3; CornerTrackRepository rep3; std::vector<SE3Transform> cams3; std::vector<Matrix3> Ks3;
    build(map3, rep3, cams3, Ks3);
    ba.ComputeInplace(600.0, map3, cams3, rep3, nullptr, &Ks3, crit, 8);
    double maxd3 = 0;
    for (int32_t j = 0; j < M; ++j) {
        const double t[3] = { cams3[(size_t)j].T.x, cams3[(size_t)j].T.y, cams3[(size_t)j].T.z };
        for (int e = 0; e < 3; ++e) maxd3 = std::fmax(maxd3, std::fabs(t[e] - T3[3 * j + e]));
    }
    if (maxd3 > 1e-8) return 24; // the run without priors
    std::printf("jointprior adapter ok\n");
    return 0;
}
