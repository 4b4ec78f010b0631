// srk_locate.cpp -- resection without a start pose, the host half: see srk_locate.hpp.  No HIP.
#include "srk_locate.hpp"
#include "srk_locate_math.hpp"

#include <cmath>
#include <limits>

static_assert(SRK_LOCATE_FEW_POINTS == 1 && SRK_LOCATE_NO_MODEL == 2, "srk_locate.hip writes the status bits as numbers");
static_assert(SRK_LOCATE_LANES_HOST == SRK_LOCATE_LANES, "a wave of srk_locate.hip holds 64 hypotheses");

srk_locate_options srk_locate_effective_options(const srk_locate_options* opts)
{
    if (opts) return *opts;
    srk_locate_options o;
    srk_locate_default_options(&o);
    return o;
}

namespace {
bool all_finite(const double* v, int64_t n)
{
    for (int64_t e = 0; e < n; ++e)
        if (!std::isfinite(v[e])) return false;
    return true;
}
} // namespace

std::string srk_locate_check(int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv, const double* q, int64_t n_points,
                             const double* X, const double* K, int shared_k, const srk_locate_options* opts, const srk_resect_options* refine,
                             const int64_t* point_int, std::vector<int32_t>* mapped)
{
    if (n_frames < 0) return "locate: a negative frame count";
    if (n_frames > SRK_RESECT_MAX_FRAMES_HOST) return "locate: too many frames in one call";
    if (n_points < 0 || n_points > 2147483647LL) return "locate: the landmark count is outside 0..2^31 - 1";
    if (!row_ptr) return "locate: row_ptr is NULL";
    const srk_locate_options lo = srk_locate_effective_options(opts);
    if (lo.hypotheses < 1 || lo.hypotheses > SRK_LOCATE_MAX_HYPOTHESES_HOST)
        return "locate: hypotheses outside 1.." + std::to_string(SRK_LOCATE_MAX_HYPOTHESES_HOST);
    if (!(lo.inlier_pixels > 0.0) || !std::isfinite(lo.inlier_pixels)) return "locate: inlier_pixels must be finite and > 0";
    if ((int64_t)n_frames * ((lo.hypotheses + SRK_LOCATE_LANES - 1) / SRK_LOCATE_LANES) > SRK_LOCATE_MAX_WAVES_HOST)
        return "locate: frames x ceil(hypotheses / 64) exceeds " + std::to_string(SRK_LOCATE_MAX_WAVES_HOST) + ": split the batch";
    if (refine) {
        if (refine->attempts < 0 || refine->attempts > SRK_RESECT_MAX_ATTEMPTS_HOST)
            return "locate: refine attempts outside 0.." + std::to_string(SRK_RESECT_MAX_ATTEMPTS_HOST);
        if (!(refine->rel_change >= 0.0) || !std::isfinite(refine->rel_change)) return "locate: refine rel_change must be finite and not negative";
        if (refine->loss_kind < 0 || refine->loss_kind > 2) return "locate: refine loss_kind outside 0..2";
        if (refine->loss_kind != 0 && (!(refine->loss_delta_pixels > 0.0) || !std::isfinite(refine->loss_delta_pixels)))
            return "locate: a refine loss needs a finite loss_delta_pixels > 0";
    }
    if (row_ptr[0] != 0) return "locate: row_ptr[0] != 0";
    for (int32_t i = 0; i < n_frames; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) return "locate: row_ptr decreases at frame " + std::to_string(i);
    const int64_t O = row_ptr[n_frames];
    if (O > 0 && (!point || !uv)) return "locate: a NULL observation array";
    if (n_frames > 0 && !K) return "locate: the intrinsics array is NULL";
    if (mapped) mapped->resize((size_t)O);
    for (int64_t o = 0; o < O; ++o) {
        if (point[o] < 0 || point[o] >= n_points) return "locate: the point of observation " + std::to_string(o) + " is out of range";
        if (mapped) (*mapped)[(size_t)o] = point_int ? (int32_t)point_int[point[o]] : point[o];
        if (!std::isfinite(uv[2 * o]) || !std::isfinite(uv[2 * o + 1])) return "locate: uv of observation " + std::to_string(o) + " is not finite";
        if (q && (!(q[o] >= 0.0) || !std::isfinite(q[o]))) return "locate: q of observation " + std::to_string(o) + " must be finite and not negative";
    }
    if (X)
        for (int64_t i = 0; i < n_points; ++i)
            if (!all_finite(X + 3 * i, 3)) return "locate: landmark " + std::to_string(i) + " is not finite";
    for (int32_t i = 0; i < (shared_k ? (n_frames > 0 ? 1 : 0) : n_frames); ++i) {
        const double* k = K + 9 * (int64_t)i;
        if (!all_finite(k, 9)) return "locate: K of frame " + std::to_string(i) + " is not finite";
        double big = 0.0;
        for (int e = 0; e < 9; ++e) big = std::fmax(big, std::fabs(k[e]));
        // singular to rounding: the determinant is a sum of products of three entries
        if (!(std::fabs(srk_locate_det3(k)) > 1e-12 * big * big * big)) return "locate: K of frame " + std::to_string(i) + " is singular";
    }
    return std::string();
}

uint32_t srk_locate_host_frame(int64_t n_obs, const int32_t* point, const double* uv, const double* q, const double* X, const double* K,
                               double f0, const srk_locate_options& opts, double R[9], double T[3], double located[6], uint8_t* inlier_out,
                               std::vector<double>* scores)
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    std::vector<int64_t> rank; // the gather: the weighted observations in ascending o
    for (int64_t o = 0; o < n_obs; ++o)
        if (!q || q[o] > 0.0) rank.push_back(o);
    const int64_t n = (int64_t)rank.size();
    const double tau2 = opts.inlier_pixels * opts.inlier_pixels;
    for (int e = 0; e < 9; ++e) R[e] = (e % 4 == 0) ? 1.0 : 0.0;
    T[0] = T[1] = T[2] = 0.0;
    located[0] = located[3] = located[5] = nan;
    located[1] = (double)n;
    located[2] = located[4] = 0.0;
    if (inlier_out)
        for (int64_t o = 0; o < n_obs; ++o) inlier_out[o] = 0;
    if (scores) scores->assign((size_t)opts.hypotheses, inf);
    if (n < 4) return SRK_LOCATE_FEW_POINTS;
    double Ki[9];
    srk_locate_inverse3(K, Ki);
    SrkLocateHyp best;
    double best_score = inf;
    int32_t best_h = -1, best_inl = 0, poses = 0;
    for (int32_t h = 0; h < opts.hypotheses; ++h) {
        int64_t r[4];
        srk_locate_sample(opts.seed, (uint32_t)h, n, r[0], r[1], r[2], r[3]);
        double X4[12], uv4[8];
        for (int k = 0; k < 4; ++k) {
            const int64_t o = rank[(size_t)r[k]];
            for (int a = 0; a < 3; ++a) X4[3 * k + a] = X[3 * (int64_t)point[o] + a];
            uv4[2 * k] = uv[2 * o];
            uv4[2 * k + 1] = uv[2 * o + 1];
        }
        SrkLocateHyp hyp;
        srk_locate_hypothesis(K, Ki, X4, uv4, f0, hyp);
        if (!hyp.valid) continue;
        ++poses;
        double score = 0.0;
        int32_t inl = 0;
        for (int64_t k = 0; k < n; ++k) { // ascending rank, one accumulator
            const int64_t o = rank[(size_t)k];
            int in;
            score += srk_locate_term(hyp.p, hyp.d, X + 3 * (int64_t)point[o], uv[2 * o], uv[2 * o + 1], q ? q[o] : 1.0, f0, tau2, in);
            inl += in;
        }
        if (scores) (*scores)[(size_t)h] = score;
        if (score < best_score) { // an equal score stays with the smaller h
            best_score = score;
            best_h = h;
            best_inl = inl;
            best = hyp;
        }
    }
    located[4] = (double)poses;
    if (best_h < 0) return SRK_LOCATE_NO_MODEL;
    for (int e = 0; e < 9; ++e) R[e] = best.R[e];
    for (int e = 0; e < 3; ++e) T[e] = best.T[e];
    located[0] = std::sqrt(best_score / (double)n);
    located[2] = (double)best_inl;
    located[3] = (double)best_h;
    located[5] = std::sqrt(best.e4);
    if (inlier_out)
        for (int64_t k = 0; k < n; ++k) {
            const int64_t o = rank[(size_t)k];
            int in;
            srk_locate_term(best.p, best.d, X + 3 * (int64_t)point[o], uv[2 * o], uv[2 * o + 1], q ? q[o] : 1.0, f0, tau2, in);
            inlier_out[o] = (uint8_t)in;
        }
    return 0;
}

int srk_locate_p3p_all(const double* K, double f0, const double* X, const double* uv, double* R, double* T, int* ok)
{
    double Ki[9];
    srk_locate_inverse3(K, Ki);
    SrkLocateP3P g;
    srk_locate_p3p_setup(Ki, X, uv, f0, g);
    int count = 0;
    for (int k = 0; k < 4; ++k) {
        srk_locate_p3p_pose(g, k, X, R + 9 * k, T + 3 * k);
        ok[k] = g.ok[k] && all_finite(R + 9 * k, 9) && all_finite(T + 3 * k, 3);
        count += ok[k];
    }
    return count;
}

extern "C" {

void srk_locate_default_options(srk_locate_options* o)
{
    if (!o) return;
    o->hypotheses = 256;
    o->inlier_pixels = 4.0;
    o->seed = 1;
}

int srk_locate_check_frames(int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv, const double* q, int64_t n_points,
                            const double* X, const double* K, int shared_k, const srk_locate_options* opts, const srk_resect_options* refine,
                            const char** why)
{
    static thread_local std::string text;
    text = srk_locate_check(n_frames, row_ptr, point, uv, q, n_points, X, K, shared_k, opts, refine);
    if (text.empty() && n_points > 0 && !X) text = "locate: the landmark array is NULL";
    if (why) *why = text.c_str();
    return text.empty() ? SRK_OK : SRK_E_ARGS;
}

int64_t srk_ransac_hypotheses(int sample_size, double outlier_ratio, double success_probability)
{
    if (sample_size < 1 || !(outlier_ratio >= 0.0 && outlier_ratio < 1.0) || !(success_probability > 0.0 && success_probability < 1.0)) return SRK_E_ARGS;
    if (outlier_ratio == 0.0) return 1;
    const double good = std::pow(1.0 - outlier_ratio, sample_size); // a sample without a wrong match
    if (!(good > 0.0)) return SRK_E_ARGS;                           // underflow: no count is enough
    const double k = std::ceil(std::log(1.0 - success_probability) / std::log(1.0 - good));
    return k < 1.0 ? 1 : (k > 9.0e18 ? INT64_MAX : (int64_t)k);
}

} // extern "C"
