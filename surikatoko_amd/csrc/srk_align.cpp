// srk_align.cpp -- map alignment, the host half: see srk_align.hpp.  No HIP.
#include "srk_align.hpp"
#include "srk_align_math.hpp"

#include <cmath>
#include <limits>

static_assert(SRK_ALIGN_FEW_POINTS == 1 && SRK_ALIGN_NO_MODEL == 2, "srk_align.hip writes the status bits as numbers");
static_assert(SRK_ALIGN_LANES_HOST == SRK_ALIGN_LANES, "a wave of srk_align.hip holds 64 hypotheses");

srk_align_options srk_align_effective_options(const srk_align_options* opts)
{
    if (opts) return *opts;
    srk_align_options o;
    srk_align_default_options(&o);
    return o;
}

std::string srk_align_check(int32_t n_sets, const int64_t* row_ptr, const int32_t* point, int64_t n_points, const double* a, const double* b,
                            const double* q, const srk_align_options* opts, const int64_t* point_int, std::vector<int32_t>* mapped)
{
    if (n_sets < 0) return "align: a negative set count";
    if (n_points < 0 || n_points > 2147483647LL) return "align: the landmark count is outside 0..2^31 - 1";
    if (!row_ptr) return "align: row_ptr is NULL";
    const srk_align_options lo = srk_align_effective_options(opts);
    if (lo.hypotheses < 1 || lo.hypotheses > SRK_ALIGN_MAX_HYPOTHESES_HOST)
        return "align: hypotheses outside 1.." + std::to_string(SRK_ALIGN_MAX_HYPOTHESES_HOST);
    if (!(lo.inlier_distance > 0.0) || !std::isfinite(lo.inlier_distance)) return "align: inlier_distance must be finite and > 0 (it has no default)";
    if (lo.refine_rounds < 0 || lo.refine_rounds > SRK_ALIGN_MAX_ROUNDS_HOST)
        return "align: refine_rounds outside 0.." + std::to_string(SRK_ALIGN_MAX_ROUNDS_HOST);
    if (lo.with_scale != 0 && lo.with_scale != 1) return "align: with_scale must be 0 or 1";
    if ((int64_t)n_sets * ((lo.hypotheses + SRK_ALIGN_LANES - 1) / SRK_ALIGN_LANES) > SRK_ALIGN_MAX_WAVES_HOST)
        return "align: sets x ceil(hypotheses / 64) exceeds " + std::to_string(SRK_ALIGN_MAX_WAVES_HOST) + ": split the batch";
    if (row_ptr[0] != 0) return "align: row_ptr[0] != 0";
    for (int32_t i = 0; i < n_sets; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) return "align: row_ptr decreases at set " + std::to_string(i);
    const int64_t O = row_ptr[n_sets];
    if (O > 0 && (!b || (!point && !a))) return "align: a NULL correspondence array";
    if (mapped) mapped->resize((size_t)O);
    for (int64_t o = 0; o < O; ++o) {
        if (point) {
            if (point[o] < 0 || point[o] >= n_points) return "align: the point of correspondence " + std::to_string(o) + " is beyond the map";
            if (mapped) (*mapped)[(size_t)o] = point_int ? (int32_t)point_int[point[o]] : point[o];
        } else if (!std::isfinite(a[3 * o]) || !std::isfinite(a[3 * o + 1]) || !std::isfinite(a[3 * o + 2]))
            return "align: a of correspondence " + std::to_string(o) + " is not finite";
        if (!std::isfinite(b[3 * o]) || !std::isfinite(b[3 * o + 1]) || !std::isfinite(b[3 * o + 2]))
            return "align: b of correspondence " + std::to_string(o) + " is not finite";
        if (q && (!(q[o] >= 0.0) || !std::isfinite(q[o]))) return "align: q of correspondence " + std::to_string(o) + " must be finite and not negative";
    }
    return std::string();
}

namespace {
// the wave's fixed tree over the lanes' sums: lane l adds lane l + d for d = 32, 16, .. 1; lane 0 ends with the total
void merge_lanes(double (*acc)[10], int width)
{
    for (int d = SRK_ALIGN_LANES / 2; d >= 1; d >>= 1)
        for (int l = 0; l < d; ++l)
            for (int e = 0; e < width; ++e) acc[l][e] += acc[l + d][e];
}

struct Walk {
    const std::vector<int64_t>& rank;
    const double* a;
    const double* b;
    const double* q;
    double tau2;
    double weight(int64_t k) const { return q ? q[rank[(size_t)k]] : 1.0; }
    const double* src(int64_t k) const { return a + 3 * rank[(size_t)k]; }
    const double* dst(int64_t k) const { return b + 3 * rank[(size_t)k]; }
    // the score of a model in ascending rank with one accumulator, its inlier count and the inliers' sum of r^2
    double score(const SrkAlignModel& m, int64_t& inl, double& ss) const
    {
        double sR[9], sc = 0.0;
        srk_align_scaled(m, sR);
        inl = 0;
        ss = 0.0;
        for (int64_t k = 0; k < (int64_t)rank.size(); ++k) {
            int in;
            double r2;
            sc += srk_align_term(sR, m.t, src(k), dst(k), weight(k), tau2, in, r2);
            inl += in;
            ss += in ? r2 : 0.0;
        }
        return sc;
    }
};
} // namespace

uint32_t srk_align_host_walk(int64_t n_obs, const double* a, const double* b, const double* q, const srk_align_options& opts, double* s, double R[9],
                             double t[3], double aligned[8], uint8_t* inlier_out, std::vector<double>* scores)
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    std::vector<int64_t> rank; // the gather: the weighted correspondences in ascending o
    for (int64_t o = 0; o < n_obs; ++o)
        if (!q || q[o] > 0.0) rank.push_back(o);
    const int64_t n = (int64_t)rank.size();
    const Walk w{ rank, a, b, q, opts.inlier_distance * opts.inlier_distance };
    SrkAlignModel cur;
    srk_align_identity(cur);
    *s = cur.s;
    for (int e = 0; e < 9; ++e) R[e] = cur.R[e];
    t[0] = t[1] = t[2] = 0.0;
    aligned[0] = aligned[3] = aligned[6] = aligned[7] = nan;
    aligned[1] = (double)n;
    aligned[2] = aligned[4] = aligned[5] = 0.0;
    if (inlier_out)
        for (int64_t o = 0; o < n_obs; ++o) inlier_out[o] = 0;
    if (scores) scores->assign((size_t)opts.hypotheses, inf);
    if (n < 3) return SRK_ALIGN_FEW_POINTS;
    double best = inf, best_ss = 0.0;
    int64_t best_inl = 0;
    int32_t best_h = -1, models = 0;
    for (int32_t h = 0; h < opts.hypotheses; ++h) {
        int64_t r[3];
        srk_align_sample(opts.seed, (uint32_t)h, n, r[0], r[1], r[2]);
        double a3[9], b3[9];
        for (int k = 0; k < 3; ++k)
            for (int c = 0; c < 3; ++c) {
                a3[3 * k + c] = w.src(r[k])[c];
                b3[3 * k + c] = w.dst(r[k])[c];
            }
        SrkAlignModel m;
        if (!srk_align_hypothesis(a3, b3, opts.with_scale, m)) continue;
        ++models;
        int64_t inl;
        double ss;
        const double sc = w.score(m, inl, ss);
        if (scores) (*scores)[(size_t)h] = sc;
        if (sc < best) { // an equal score stays with the smaller h
            best = sc;
            best_h = h;
            best_inl = inl;
            best_ss = ss;
            cur = m;
        }
    }
    aligned[4] = (double)models;
    if (best_h < 0) return SRK_ALIGN_NO_MODEL;
    int32_t rounds = 0;
    double gap = nan;
    for (int32_t round = 0; round < opts.refine_rounds; ++round) {
        double sR[9], acc[SRK_ALIGN_LANES][10];
        srk_align_scaled(cur, sR);
        int64_t count = 0;
        for (int l = 0; l < SRK_ALIGN_LANES; ++l) { // pass one: lane l takes ranks l, l + 64, ..
            for (int e = 0; e < 10; ++e) acc[l][e] = 0.0;
            for (int64_t k = l; k < n; k += SRK_ALIGN_LANES) {
                int in;
                double r2;
                srk_align_term(sR, cur.t, w.src(k), w.dst(k), w.weight(k), w.tau2, in, r2);
                if (in) {
                    srk_align_pass_one(acc[l], w.src(k), w.dst(k), w.weight(k));
                    ++count;
                }
            }
        }
        if (count < 3) break;
        merge_lanes(acc, 7);
        const double am[3] = { acc[0][1] / acc[0][0], acc[0][2] / acc[0][0], acc[0][3] / acc[0][0] };
        const double bm[3] = { acc[0][4] / acc[0][0], acc[0][5] / acc[0][0], acc[0][6] / acc[0][0] };
        for (int l = 0; l < SRK_ALIGN_LANES; ++l) { // pass two: the same walk, centred
            for (int e = 0; e < 10; ++e) acc[l][e] = 0.0;
            for (int64_t k = l; k < n; k += SRK_ALIGN_LANES) {
                int in;
                double r2;
                srk_align_term(sR, cur.t, w.src(k), w.dst(k), w.weight(k), w.tau2, in, r2);
                if (in) srk_align_pass_two(acc[l], w.src(k), w.dst(k), w.weight(k), am, bm);
            }
        }
        merge_lanes(acc, 10);
        SrkAlignModel cand;
        double g;
        if (!srk_align_closed_form(acc[0], acc[0][9], am, bm, opts.with_scale, cand, g)) break;
        int64_t inl;
        double ss;
        const double sc = w.score(cand, inl, ss);
        if (!(sc < best)) break; // only a strictly smaller score is accepted
        best = sc;
        best_inl = inl;
        best_ss = ss;
        cur = cand;
        gap = g;
        ++rounds;
    }
    *s = cur.s;
    for (int e = 0; e < 9; ++e) R[e] = cur.R[e];
    for (int e = 0; e < 3; ++e) t[e] = cur.t[e];
    aligned[0] = std::sqrt(best / (double)n);
    aligned[2] = (double)best_inl;
    aligned[3] = (double)best_h;
    aligned[5] = (double)rounds;
    aligned[6] = gap;
    aligned[7] = std::sqrt(best_ss / (double)best_inl);
    if (inlier_out) {
        double sR[9];
        srk_align_scaled(cur, sR);
        for (int64_t k = 0; k < n; ++k) {
            int in;
            double r2;
            srk_align_term(sR, cur.t, w.src(k), w.dst(k), w.weight(k), w.tau2, in, r2);
            inlier_out[rank[(size_t)k]] = (uint8_t)in;
        }
    }
    return 0;
}

void srk_align_revert(const srk_ba_normalizer& nrm, int32_t n, double* s, double* R, double* t)
{
    for (int32_t i = 0; i < n; ++i) {
        double* Q = R + 9 * (int64_t)i;
        double* tt = t + 3 * (int64_t)i;
        const double sc = s[i] * nrm.world_scale;
        double QR[9], QT[3];
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) QR[3 * r + c] = Q[3 * r] * nrm.R0[c] + Q[3 * r + 1] * nrm.R0[3 + c] + Q[3 * r + 2] * nrm.R0[6 + c];
            QT[r] = Q[3 * r] * nrm.T0[0] + Q[3 * r + 1] * nrm.T0[1] + Q[3 * r + 2] * nrm.T0[2];
        }
        for (int e = 0; e < 9; ++e) Q[e] = QR[e];
        for (int e = 0; e < 3; ++e) tt[e] += sc * QT[e];
        s[i] = sc;
    }
}

extern "C" {

void srk_align_default_options(srk_align_options* o)
{
    if (!o) return;
    o->hypotheses = 256;
    o->inlier_distance = 0.0; // no sensible default: the checks refuse it until the caller sets it
    o->seed = 1;
    o->with_scale = 1;
    o->refine_rounds = 2;
}

int srk_align_check_sets(int32_t n_sets, const int64_t* row_ptr, const int32_t* point, int64_t n_points, const double* a, const double* b, const double* q,
                         const srk_align_options* opts, const double* s, const double* R, const double* t, const double* aligned,
                         const uint32_t* status, const char** why)
{
    static thread_local std::string text;
    text = srk_align_check(n_sets, row_ptr, point, n_points, a, b, q, opts);
    if (text.empty() && n_sets > 0 && (!s || !R || !t || !aligned || !status)) text = "align: a NULL output array";
    if (why) *why = text.c_str();
    return text.empty() ? SRK_OK : SRK_E_ARGS;
}

int srk_align_host_set(int64_t n_obs, const double* a, const double* b, const double* q, const srk_align_options* opts, double* s, double* R, double* t,
                       double* aligned, uint8_t* inlier_out)
{
    if (n_obs < 0 || !s || !R || !t || !aligned) return SRK_E_ARGS;
    const int64_t row_ptr[2] = { 0, n_obs };
    if (!srk_align_check(1, row_ptr, nullptr, 0, a, b, q, opts).empty()) return SRK_E_ARGS;
    return (int)srk_align_host_walk(n_obs, a, b, q, srk_align_effective_options(opts), s, R, t, aligned, inlier_out);
}

int srk_similarity_apply(double s, const double* R, const double* t, int64_t n_points, double* X, int64_t n_frames, double* cam_R, double* cam_T)
{
    if (!R || !t || !(s > 0.0) || !std::isfinite(s) || n_points < 0 || n_frames < 0 || (n_points > 0 && !X) ||
        (n_frames > 0 && ((cam_R == nullptr) != (cam_T == nullptr))))
        return SRK_E_ARGS;
    if (X)
        for (int64_t i = 0; i < n_points; ++i) {
            double* x = X + 3 * i;
            const double v[3] = { x[0], x[1], x[2] };
            for (int r = 0; r < 3; ++r) x[r] = s * (R[3 * r] * v[0] + R[3 * r + 1] * v[1] + R[3 * r + 2] * v[2]) + t[r];
        }
    if (cam_R)
        for (int64_t j = 0; j < n_frames; ++j) { // x_cam = R_c X + T_c: R_c' = R_c R^T, T_c' = s T_c - R_c' t
            double* Rc = cam_R + 9 * j;
            double* Tc = cam_T + 3 * j;
            double N[9];
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) N[3 * r + c] = Rc[3 * r] * R[3 * c] + Rc[3 * r + 1] * R[3 * c + 1] + Rc[3 * r + 2] * R[3 * c + 2];
            for (int r = 0; r < 3; ++r) Tc[r] = s * Tc[r] - (N[3 * r] * t[0] + N[3 * r + 1] * t[1] + N[3 * r + 2] * t[2]);
            for (int e = 0; e < 9; ++e) Rc[e] = N[e];
        }
    return SRK_OK;
}

} // extern "C"
