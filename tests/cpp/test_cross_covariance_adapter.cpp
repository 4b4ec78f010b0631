// Runtime test of BundleAdjustmentKanatani::CrossCovariances / RelativePoseCovariances (include/suriko_amd/bundle-adj-kanatani.hpp)
// on a map whose salient points are NOT in track order: points are named in salient-point order and must reach the library in
// pnt_ind order.  Pairs of a block with itself equal Covariances' blocks, (b, a) is the transpose of (a, b), the blocks equal
// those of srk_ba_cross_covariances on a handle that ran the same solve through the C ABI with the indices mapped by hand, the
// relative-pose covariance equals its propagation from the adapter's own blocks, bad indices and a bad sigma throw, and the
// caller's containers are not touched by the call.
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

    typedef std::vector<std::pair<size_t, size_t>> Pairs;
    const Pairs ff = { { 5, 11 }, { 11, 5 }, { 5, 5 }, { 0, 5 }, { 10, 11 } };
    const Pairs pf = { { 0, 5 }, { 3, 11 }, { (size_t)N - 1, 2 } };        // (salient point, camera)
    const Pairs pp = { { 0, 3 }, { 3, 0 }, { 3, 3 }, { 0, (size_t)N - 1 } }; // salient-point order
    std::vector<double> cff, cpf, cpp;
    if (!ba.CrossCovariances(ff, pf, pp, 0.5, &cff, &cpf, &cpp)) return 11;
    if (cff.size() != 36 * ff.size() || cpf.size() != 18 * pf.size() || cpp.size() != 9 * pp.size()) return 12;
    for (size_t j = 0; j < cams.size(); ++j)
        if (std::memcmp(cams[j].R.data(), cams_before[j].R.data(), 72) != 0 || cams[j].T.x != cams_before[j].T.x) return 13;
    // one call, one system: (11, 5) is the transpose of (5, 11) and (3, 0) of (0, 3) to the bit; frame 0 is gauge-fixed: zeros
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) if (cff[36 * 0 + 6 * (size_t)i + (size_t)j] != cff[36 * 1 + 6 * (size_t)j + (size_t)i]) return 14;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) if (cpp[9 * 0 + 3 * (size_t)i + (size_t)j] != cpp[9 * 1 + 3 * (size_t)j + (size_t)i]) return 15;
    for (int e = 0; e < 36; ++e) if (cff[36 * 3 + (size_t)e] != 0.0) return 16;
    double big = 0;
    for (int e = 0; e < 36; ++e) big = std::fmax(big, std::fabs(cff[(size_t)e]));
    if (!(big > 0)) return 17;
    // (5, 5) and (3, 3) against Covariances (another build of the system: to rounding times the conditioning)
    std::vector<double> fc, pc;
    if (!ba.Covariances({ 5 }, { 3 }, 0.5, &fc, &pc)) return 18;
    if (rel_diff(std::vector<double>(cff.begin() + 72, cff.begin() + 108), fc) > COV_TOL) return 19;
    if (rel_diff(std::vector<double>(cpp.begin() + 18, cpp.begin() + 27), pc) > COV_TOL) return 20;

    // the same solve and the same question through the C ABI, indices mapped by hand (salient point k = landmark N - 1 - k)
    auto pts2 = pts, R2 = R, T2 = T;
    srk_ba* h = srk_ba_create(0);
    srk_ba_report rb{};
    const double a = 1e-12, mx = 1e6;
    if (srk_ba_set_fixed_intrinsics(h, 1) != SRK_OK) return 21;
    if (srk_ba_compute_inplace(h, 600.0, N, pts2.data(), M, R2.data(), T2.data(), K.data(), 0, row_ptr.data(), fr.data(), uv.data(),
                               &a, &mx, 8, &rb) < 0) return 22;
    const int32_t fa[5] = { 5, 11, 5, 0, 10 }, fb[5] = { 11, 5, 5, 5, 11 }, pff[3] = { 5, 11, 2 };
    const int64_t pfp[3] = { N - 1, N - 4, 0 }, pa[4] = { N - 1, N - 4, N - 4, N - 1 }, pb[4] = { N - 4, N - 1, N - 4, 0 };
    std::vector<double> rff(36 * 5), rpf(18 * 3), rpp(9 * 4), rrel(36 * 2);
    const int rc = srk_ba_cross_covariances(h, 0.5, 5, fa, fb, rff.data(), 3, pfp, pff, rpf.data(), 4, pa, pb, rpp.data(), 1);
    const int32_t ra[2] = { 10, 11 }, rbb[2] = { 11, 2 };
    const int rc2 = srk_ba_relative_pose_covariances(h, 0.5, 2, ra, rbb, rrel.data());
    srk_ba_destroy(h);
    if (rc != 0 || rc2 != 0) return 23;
    const double dff = rel_diff(cff, rff), dpf = rel_diff(cpf, rpf), dpp = rel_diff(cpp, rpp);
    std::printf("frame x frame blocks differ by %.3e, point x frame by %.3e, point x point by %.3e (of the largest entry)\n", dff, dpf, dpp);
    if (dff > COV_TOL || dpf > COV_TOL || dpp > COV_TOL) return 24;

    // relative poses: the C ABI's answer, symmetric, and for (10, 11) the propagation of the adapter's own blocks
    std::vector<double> rel;
    if (!ba.RelativePoseCovariances({ { 10, 11 }, { 11, 2 } }, 0.5, &rel) || rel.size() != 72) return 25;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) if (rel[6 * (size_t)i + (size_t)j] != rel[6 * (size_t)j + (size_t)i]) return 26;
    const double drel = rel_diff(rel, rrel);
    std::printf("relative-pose covariances differ by %.3e\n", drel);
    if (drel > COV_TOL) return 27;
    {
        // J = [J_a J_b], J_a = [[-R_a, R_a [d]x], [0, -R_b]], J_b = [[R_a, 0], [0, R_b]], d = C_b - C_a, C = -R^T T, on the cameras as returned
        std::vector<double> f2;
        if (!ba.Covariances({ 10, 11 }, {}, 0.5, &f2, nullptr)) return 28;
        const double* Ra = cams[10].R.data(); const double* Rb = cams[11].R.data();
        const double Ta[3] = { cams[10].T.x, cams[10].T.y, cams[10].T.z }, Tb[3] = { cams[11].T.x, cams[11].T.y, cams[11].T.z };
        double d[3];
        for (int i = 0; i < 3; ++i) {
            double ca = 0, cb = 0;
            for (int k = 0; k < 3; ++k) { ca -= Ra[3 * k + i] * Ta[k]; cb -= Rb[3 * k + i] * Tb[k]; }
            d[i] = cb - ca;
        }
        const double dx[9] = { 0, -d[2], d[1], d[2], 0, -d[0], -d[1], d[0], 0 };
        double J[6][12] = {};
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                double v = 0;
                for (int k = 0; k < 3; ++k) v += Ra[3 * r + k] * dx[3 * k + c];
                J[r][c] = -Ra[3 * r + c]; J[r][3 + c] = v; J[3 + r][3 + c] = -Rb[3 * r + c];
                J[r][6 + c] = Ra[3 * r + c]; J[3 + r][9 + c] = Rb[3 * r + c];
            }
        double S[12][12];
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) {
                S[r][c] = f2[6 * (size_t)r + (size_t)c]; S[6 + r][6 + c] = f2[36 + 6 * (size_t)r + (size_t)c];
                S[r][6 + c] = S[6 + c][r] = cff[36 * 4 + 6 * (size_t)r + (size_t)c];
            }
        std::vector<double> prop(36), mine(rel.begin(), rel.begin() + 36);
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) {
                double v = 0;
                for (int x = 0; x < 12; ++x)
                    for (int y = 0; y < 12; ++y) v += J[r][x] * S[x][y] * J[c][y];
                prop[6 * (size_t)r + (size_t)c] = v;
            }
        // the terms of the sum are of the size of the marginals, the result far smaller: compare on the marginals' scale.  Each
        // entry of S is another build's within COV_TOL of the largest; the rows of |J| sum to less than 4
        double top = 0, dmax = 0;
        for (double v : f2) top = std::fmax(top, std::fabs(v));
        for (int e = 0; e < 36; ++e) dmax = std::fmax(dmax, std::fabs(prop[(size_t)e] - mine[(size_t)e]));
        std::printf("relative pose (10, 11): propagated from the blocks within %.3e of the marginals' largest entry\n", dmax / top);
        if (!(dmax / top < 16 * COV_TOL)) return 29;
    }

    Pairs none;
    if (!throws_invalid([&] { ba.CrossCovariances({ { (size_t)M, 0 } }, none, none, 1.0, &cff, &cpf, &cpp); })) return 30;
    if (!throws_invalid([&] { ba.CrossCovariances(none, { { (size_t)N, 0 } }, none, 1.0, &cff, &cpf, &cpp); })) return 31;
    if (!throws_invalid([&] { ba.CrossCovariances(none, none, { { 0, (size_t)N } }, 1.0, &cff, &cpf, &cpp); })) return 32;
    if (!throws_invalid([&] { ba.CrossCovariances({ { 1, 2 } }, none, none, 0.0, &cff, &cpf, &cpp); })) return 33;
    if (!throws_invalid([&] { ba.RelativePoseCovariances({ { 3, 3 } }, 1.0, &rel); })) return 34;
    if (!throws_invalid([&] { ba.RelativePoseCovariances({ { 3, (size_t)M } }, 1.0, &rel); })) return 35;
    if (!ba.CrossCovariances(none, none, none, 1.0, &cff, &cpf, &cpp) || !cff.empty() || !cpf.empty() || !cpp.empty()) return 36;
    if (!ba.RelativePoseCovariances(none, 1.0, &rel) || !rel.empty()) return 37;
    std::printf("cross-covariance adapter ok\n");
    return 0;
}
