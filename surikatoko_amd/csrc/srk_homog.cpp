// srk_homog.cpp -- the two-view homography, the host half: see srk_homog.hpp.  No HIP.
#include "srk_homog.hpp"
#include "srk_geom.hpp"
#include "srk_homog_math.hpp"

#include <cmath>
#include <limits>

static_assert(SRK_HOMOGRAPHY_FEW_POINTS == 1 && SRK_HOMOGRAPHY_NO_MODEL == 2, "srk_homog.hip writes the status bits as numbers");
static_assert(SRK_HOMOG_LANES_HOST == SRK_HOMOG_LANES, "a wave of srk_homog.hip holds 64 hypotheses");

srk_homography_options srk_homog_effective_options(const srk_homography_options* opts)
{
    if (opts) return *opts;
    srk_homography_options o;
    srk_homography_default_options(&o);
    return o;
}

namespace {
bool all_finite(const double* v, int64_t n)
{
    for (int64_t e = 0; e < n; ++e)
        if (!std::isfinite(v[e])) return false;
    return true;
}

std::string check_k(const double* K, int32_t count, const char* which)
{
    for (int32_t i = 0; i < count; ++i) {
        const double* k = K + 9 * (int64_t)i;
        if (!all_finite(k, 9)) return std::string("homography: ") + which + " of pair " + std::to_string(i) + " is not finite";
        double big = 0.0;
        for (int e = 0; e < 9; ++e) big = std::fmax(big, std::fabs(k[e]));
        // singular to rounding: the determinant is a sum of products of three entries
        if (!(std::fabs(srk_homog_det3(k)) > 1e-12 * big * big * big))
            return std::string("homography: ") + which + " of pair " + std::to_string(i) + " is singular";
    }
    return std::string();
}
} // namespace

std::string srk_homog_check(int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q, const double* K_a,
                            const double* K_b, int shared_k, const srk_homography_options* opts)
{
    if (n_pairs < 0) return "homography: a negative pair count";
    if (!row_ptr) return "homography: row_ptr is NULL";
    const srk_homography_options lo = srk_homog_effective_options(opts);
    if (lo.hypotheses < 1 || lo.hypotheses > SRK_HOMOG_MAX_HYPOTHESES_HOST)
        return "homography: hypotheses outside 1.." + std::to_string(SRK_HOMOG_MAX_HYPOTHESES_HOST);
    if (!(lo.inlier_pixels > 0.0) || !std::isfinite(lo.inlier_pixels)) return "homography: inlier_pixels must be finite and > 0";
    if (lo.refine_rounds < 0 || lo.refine_rounds > SRK_HOMOG_MAX_ROUNDS_HOST)
        return "homography: refine_rounds outside 0.." + std::to_string(SRK_HOMOG_MAX_ROUNDS_HOST);
    if ((int64_t)n_pairs * ((lo.hypotheses + SRK_HOMOG_LANES - 1) / SRK_HOMOG_LANES) > SRK_HOMOG_MAX_WAVES_HOST)
        return "homography: pairs x ceil(hypotheses / 64) exceeds " + std::to_string(SRK_HOMOG_MAX_WAVES_HOST) + ": split the batch";
    if (row_ptr[0] != 0) return "homography: row_ptr[0] != 0";
    for (int32_t i = 0; i < n_pairs; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) return "homography: row_ptr decreases at pair " + std::to_string(i);
    const int64_t O = row_ptr[n_pairs];
    if (O > 0 && (!uv_a || !uv_b)) return "homography: a NULL match array";
    if (n_pairs > 0 && (!K_a || !K_b)) return "homography: an intrinsics array is NULL";
    for (int64_t o = 0; o < O; ++o) {
        if (!all_finite(uv_a + 2 * o, 2)) return "homography: uv_a of match " + std::to_string(o) + " is not finite";
        if (!all_finite(uv_b + 2 * o, 2)) return "homography: uv_b of match " + std::to_string(o) + " is not finite";
        if (q && (!(q[o] >= 0.0) || !std::isfinite(q[o]))) return "homography: q of match " + std::to_string(o) + " must be finite and not negative";
    }
    const int32_t nk = shared_k ? (n_pairs > 0 ? 1 : 0) : n_pairs;
    std::string why = check_k(K_a, nk, "K_a");
    if (why.empty()) why = check_k(K_b, nk, "K_b");
    return why;
}

namespace {
// the wave's fixed tree over the lanes' sums: lane l adds lane l + d for d = 32, 16, .. 1; lane 0 ends with the total
void merge_lanes(double (*acc)[SRK_HOMOG_ACC], int width)
{
    for (int d = SRK_HOMOG_LANES / 2; d >= 1; d >>= 1)
        for (int l = 0; l < d; ++l)
            for (int e = 0; e < width; ++e) acc[l][e] += acc[l + d][e];
}

// the gathered strip of a pair: records {ua, va, ub, vb, q, 0, 0, 0} of the weighted matches in ascending o
struct Walk {
    std::vector<double> strip;
    std::vector<int64_t> rank;
    double f0, tau2;
    int64_t n() const { return (int64_t)rank.size(); }
    const double* rec(int64_t k) const { return strip.data() + SRK_HOMOG_STRIP * k; }
    // the score of a model in ascending rank with one accumulator, its inlier count and the inliers' sum of s
    double score(const SrkHomogModel& m, int64_t& inl, double& ss) const
    {
        double sc = 0.0;
        inl = 0;
        ss = 0.0;
        for (int64_t k = 0; k < n(); ++k) {
            int in;
            double s2;
            sc += srk_homog_term(m, rec(k), f0, tau2, in, s2);
            inl += in;
            ss += in ? s2 : 0.0;
        }
        return sc;
    }
};
} // namespace

uint32_t srk_homog_host_walk(int64_t n_obs, const double* uv_a, const double* uv_b, const double* q, const double* K_a, const double* K_b, double f0,
                             const srk_homography_options& opts, SrkHomogResult& out, uint8_t* inlier_out, std::vector<double>* scores)
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    Walk w;
    w.f0 = f0;
    w.tau2 = opts.inlier_pixels * opts.inlier_pixels;
    for (int64_t o = 0; o < n_obs; ++o) // the gather
        if (!q || q[o] > 0.0) {
            w.rank.push_back(o);
            const double e[SRK_HOMOG_STRIP] = { uv_a[2 * o], uv_a[2 * o + 1], uv_b[2 * o], uv_b[2 * o + 1], q ? q[o] : 1.0, 0.0, 0.0, 0.0 };
            w.strip.insert(w.strip.end(), e, e + SRK_HOMOG_STRIP);
        }
    const int64_t n = w.n();
    SrkHomogModel cur;
    srk_homog_identity(cur);
    out = SrkHomogResult();
    for (int e = 0; e < 9; ++e) out.G[e] = out.H[e] = cur.G[e];
    out.homog[0] = out.homog[3] = out.homog[6] = out.homog[7] = nan;
    out.homog[1] = (double)n;
    if (inlier_out)
        for (int64_t o = 0; o < n_obs; ++o) inlier_out[o] = 0;
    if (scores) scores->assign((size_t)opts.hypotheses, inf);
    if (n < 4) return SRK_HOMOGRAPHY_FEW_POINTS;
    double best = inf, best_ss = 0.0;
    int64_t best_inl = 0;
    int32_t best_h = -1, models = 0;
    for (int32_t h = 0; h < opts.hypotheses; ++h) {
        int64_t r[4];
        srk_homog_sample(opts.seed, (uint32_t)h, n, r[0], r[1], r[2], r[3]);
        double pa[12], pb[12];
        for (int k = 0; k < 4; ++k) {
            const double* e = w.rec(r[k]);
            pa[3 * k] = e[0], pa[3 * k + 1] = e[1], pa[3 * k + 2] = f0;
            pb[3 * k] = e[2], pb[3 * k + 1] = e[3], pb[3 * k + 2] = f0;
        }
        SrkHomogModel m;
        if (!srk_homog_hypothesis(pa, pb, m)) continue;
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
    out.homog[4] = (double)models;
    if (best_h < 0) return SRK_HOMOGRAPHY_NO_MODEL;
    int32_t rounds = 0;
    std::vector<double> lanes((size_t)SRK_HOMOG_LANES * SRK_HOMOG_ACC);
    double(*acc)[SRK_HOMOG_ACC] = reinterpret_cast<double(*)[SRK_HOMOG_ACC]>(lanes.data());
    for (int32_t round = 0; round < opts.refine_rounds; ++round) {
        int64_t count = 0;
        for (int l = 0; l < SRK_HOMOG_LANES; ++l) { // lane l takes ranks l, l + 64, ..
            for (int e = 0; e < SRK_HOMOG_ACC; ++e) acc[l][e] = 0.0;
            for (int64_t k = l; k < n; k += SRK_HOMOG_LANES) {
                int in;
                double s2;
                srk_homog_term(cur, w.rec(k), f0, w.tau2, in, s2);
                if (in) {
                    srk_homog_accumulate(acc[l], cur, w.rec(k), f0);
                    ++count;
                }
            }
        }
        if (count < 4) break;
        merge_lanes(acc, SRK_HOMOG_ACC);
        SrkHomogModel cand;
        if (!srk_homog_step(acc[0], cur, cand)) break;
        int64_t inl;
        double ss;
        const double sc = w.score(cand, inl, ss);
        if (!(sc < best)) break; // only a strictly smaller score is accepted
        best = sc;
        best_inl = inl;
        best_ss = ss;
        cur = cand;
        ++rounds;
    }
    // the decomposition of the returned model: the sign sum, the planes, the inliers ahead of each normal
    double Kai[9], Kbi[9], GK[9], Hraw[9];
    srk_homog_inv3(K_a, Kai);
    srk_homog_inv3(K_b, Kbi);
    srk_homog_mul3(cur.G, K_a, GK);
    srk_homog_mul3(Kbi, GK, Hraw);
    for (int l = 0; l < SRK_HOMOG_LANES; ++l) {
        acc[l][0] = 0.0;
        for (int64_t k = l; k < n; k += SRK_HOMOG_LANES) {
            int in;
            double s2, xa[3];
            srk_homog_term(cur, w.rec(k), f0, w.tau2, in, s2);
            if (in) acc[l][0] += srk_homog_sign_term(Kai, Kbi, Hraw, w.rec(k), f0, xa);
        }
    }
    merge_lanes(acc, 1);
    SrkHomogPlanes P;
    srk_homog_planes(Hraw, acc[0][0], P);
    int64_t ahead[2] = { 0, 0 };
    for (int64_t k = 0; k < n; ++k) { // counts: the order does not matter
        int in;
        double s2, xa[3];
        srk_homog_term(cur, w.rec(k), f0, w.tau2, in, s2);
        if (!in) continue;
        srk_homog_sign_term(Kai, Kbi, Hraw, w.rec(k), f0, xa);
        ahead[0] += srk_align_dot(P.N[0], xa) > 0.0;
        ahead[1] += srk_align_dot(P.N[1], xa) > 0.0;
    }
    srk_homog_finish(P, ahead, best_inl, out.R, out.T, out.N, out.front);
    for (int e = 0; e < 9; ++e) out.G[e] = cur.G[e], out.H[e] = P.H[e];
    out.n_poses = P.n_poses;
    out.homog[0] = std::sqrt(best / (double)n);
    out.homog[2] = (double)best_inl;
    out.homog[3] = (double)best_h;
    out.homog[5] = (double)rounds;
    out.homog[6] = P.gap;
    out.homog[7] = best_inl > 0 ? std::sqrt(best_ss / (double)best_inl) : 0.0; // a winner without inliers: nothing to average
    if (inlier_out)
        for (int64_t k = 0; k < n; ++k) {
            int in;
            double s2;
            srk_homog_term(cur, w.rec(k), f0, w.tau2, in, s2);
            inlier_out[w.rank[(size_t)k]] = (uint8_t)in;
        }
    return 0;
}

extern "C" {

void srk_homography_default_options(srk_homography_options* o)
{
    if (!o) return;
    o->hypotheses = 256;
    o->inlier_pixels = 6.0;
    o->seed = 1;
    o->refine_rounds = 4;
}

int srk_homography_check_pairs(int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q, const double* K_a,
                               const double* K_b, int shared_k, const srk_homography_options* opts, const char** why)
{
    static thread_local std::string text;
    try {
        text = srk_homog_check(n_pairs, row_ptr, uv_a, uv_b, q, K_a, K_b, shared_k, opts);
    } catch (const std::bad_alloc&) {
        return SRK_E_NOMEM;
    }
    if (why) *why = text.c_str();
    return text.empty() ? SRK_OK : SRK_E_ARGS;
}

int srk_homography_host_pair(int64_t n_obs, const double* uv_a, const double* uv_b, const double* q, const double* K_a, const double* K_b, double f0,
                             const srk_homography_options* opts, double* G, double* H, int32_t* n_poses, double* R, double* T, double* N,
                             int32_t* front, double* homog, uint8_t* inlier_out)
{
    try {
        if (n_obs < 0 || !G || !H || !n_poses || !R || !T || !N || !front || !homog || !std::isfinite(f0) || srk::is_close(0.0, f0)) return SRK_E_ARGS;
        const int64_t row_ptr[2] = { 0, n_obs };
        if (!srk_homog_check(1, row_ptr, uv_a, uv_b, q, K_a, K_b, 1, opts).empty()) return SRK_E_ARGS;
        SrkHomogResult out;
        const uint32_t st = srk_homog_host_walk(n_obs, uv_a, uv_b, q, K_a, K_b, f0, srk_homog_effective_options(opts), out, inlier_out);
        for (int e = 0; e < 9; ++e) G[e] = out.G[e], H[e] = out.H[e];
        for (int e = 0; e < 18; ++e) R[e] = out.R[e];
        for (int e = 0; e < 6; ++e) T[e] = out.T[e], N[e] = out.N[e];
        for (int e = 0; e < 8; ++e) homog[e] = out.homog[e];
        *n_poses = out.n_poses;
        front[0] = out.front[0], front[1] = out.front[1];
        return (int)st;
    } catch (const std::bad_alloc&) {
        return SRK_E_NOMEM;
    }
}

int srk_homography_decompose(const double* H_in, int64_t n, const double* x_a, const double* x_b, const double* q, double* H_out, double* R, double* T,
                             double* N, int32_t* front, double* gap)
{
    if (!H_in || n < 0 || (n > 0 && (!x_a || !x_b)) || !H_out || !R || !T || !N || !front || !gap) return SRK_E_ARGS;
    for (int e = 0; e < 9; ++e)
        if (!std::isfinite(H_in[e])) return SRK_E_ARGS;
    double sum = 0.0; // here in ascending order with one accumulator; the kernel's sum is lane-strided
    for (int64_t k = 0; k < n; ++k) {
        double hx[3];
        srk_homog_mulv(H_in, x_a + 3 * k, hx);
        sum += (q ? q[k] : 1.0) * srk_align_dot(x_b + 3 * k, hx);
    }
    SrkHomogPlanes P;
    srk_homog_planes(H_in, sum, P);
    int64_t ahead[2] = { 0, 0 };
    for (int64_t k = 0; k < n; ++k) {
        ahead[0] += srk_align_dot(P.N[0], x_a + 3 * k) > 0.0;
        ahead[1] += srk_align_dot(P.N[1], x_a + 3 * k) > 0.0;
    }
    bool finite = std::isfinite(P.gap); // H = 0 has no middle singular value: refused before anything is written
    for (int e = 0; e < 9; ++e) finite = finite && std::isfinite(P.H[e]);
    if (!finite) return SRK_E_ARGS;
    srk_homog_finish(P, ahead, n, R, T, N, front);
    for (int e = 0; e < 9; ++e) H_out[e] = P.H[e];
    *gap = P.gap;
    return P.n_poses;
}

} // extern "C"
