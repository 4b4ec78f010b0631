// srk_fund.cpp -- the two-view fundamental matrix, the host half: see srk_fund.hpp.  No HIP.
#include "srk_fund.hpp"
#include "srk_fund_math.hpp"
#include "srk_geom.hpp"

#include <cmath>
#include <limits>

static_assert(SRK_FUNDAMENTAL_FEW_POINTS == 1 && SRK_FUNDAMENTAL_NO_MODEL == 2, "srk_fund.hip writes the status bits as numbers");
static_assert(SRK_FUND_LANES_HOST == SRK_FUND_LANES, "a wave of srk_fund.hip holds 64 hypotheses");

srk_fundamental_options srk_fund_effective_options(const srk_fundamental_options* opts)
{
    if (opts) return *opts;
    srk_fundamental_options o;
    srk_fundamental_default_options(&o);
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

std::string srk_fund_check(int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                           const srk_fundamental_options* opts)
{
    if (n_pairs < 0) return "fundamental: a negative pair count";
    if (!row_ptr) return "fundamental: row_ptr is NULL";
    const srk_fundamental_options lo = srk_fund_effective_options(opts);
    if (lo.hypotheses < 1 || lo.hypotheses > SRK_FUND_MAX_HYPOTHESES_HOST)
        return "fundamental: hypotheses outside 1.." + std::to_string(SRK_FUND_MAX_HYPOTHESES_HOST);
    if (!(lo.inlier_pixels > 0.0) || !std::isfinite(lo.inlier_pixels)) return "fundamental: inlier_pixels must be finite and > 0";
    if (lo.refine_rounds < 0 || lo.refine_rounds > SRK_FUND_MAX_ROUNDS_HOST)
        return "fundamental: refine_rounds outside 0.." + std::to_string(SRK_FUND_MAX_ROUNDS_HOST);
    if ((int64_t)n_pairs * ((lo.hypotheses + SRK_FUND_LANES - 1) / SRK_FUND_LANES) > SRK_FUND_MAX_WAVES_HOST)
        return "fundamental: pairs x ceil(hypotheses / 64) exceeds " + std::to_string(SRK_FUND_MAX_WAVES_HOST) + ": split the batch";
    if (row_ptr[0] != 0) return "fundamental: row_ptr[0] != 0";
    for (int32_t i = 0; i < n_pairs; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) return "fundamental: row_ptr decreases at pair " + std::to_string(i);
    const int64_t O = row_ptr[n_pairs];
    if (O > 0 && (!uv_a || !uv_b)) return "fundamental: a NULL match array";
    for (int64_t o = 0; o < O; ++o) {
        if (!all_finite(uv_a + 2 * o, 2)) return "fundamental: uv_a of match " + std::to_string(o) + " is not finite";
        if (!all_finite(uv_b + 2 * o, 2)) return "fundamental: uv_b of match " + std::to_string(o) + " is not finite";
        if (q && (!(q[o] >= 0.0) || !std::isfinite(q[o]))) return "fundamental: q of match " + std::to_string(o) + " must be finite and not negative";
    }
    return std::string();
}

namespace {
// the wave's fixed tree over the lanes' sums: lane l adds lane l + d for d = 32, 16, .. 1; lane 0 ends with the total
void merge_lanes(double (*acc)[SRK_FUND_ACC])
{
    for (int d = SRK_FUND_LANES / 2; d >= 1; d >>= 1)
        for (int l = 0; l < d; ++l)
            for (int e = 0; e < SRK_FUND_ACC; ++e) acc[l][e] += acc[l + d][e];
}

// the gathered strip of a pair: records {ua, va, ub, vb, q, 0, 0, 0} of the weighted matches in ascending o
struct Walk {
    std::vector<double> strip;
    std::vector<int64_t> rank;
    double f0, tau2;
    int64_t n() const { return (int64_t)rank.size(); }
    const double* rec(int64_t k) const { return strip.data() + SRK_FUND_STRIP * k; }
    // the score of a model in ascending rank with one accumulator, its inlier count and the inliers' sum of s
    double score(const double* F, int64_t& inl, double& ss) const
    {
        double sc = 0.0;
        inl = 0;
        ss = 0.0;
        for (int64_t k = 0; k < n(); ++k) {
            int in;
            double s2;
            sc += srk_fund_term(F, rec(k), f0, tau2, in, s2);
            inl += in;
            ss += in ? s2 : 0.0;
        }
        return sc;
    }
    // the sums of a linearisation over the inliers of F: lane l takes ranks l, l + 64, .., the lanes merged in the fixed tree
    void sums(const SrkFundRep& cur, const double* F, double* total) const
    {
        SrkFundLin lin;
        srk_fund_linearise(cur, lin);
        std::vector<double> lanes((size_t)SRK_FUND_LANES * SRK_FUND_ACC, 0.0);
        double(*acc)[SRK_FUND_ACC] = reinterpret_cast<double(*)[SRK_FUND_ACC]>(lanes.data());
        for (int l = 0; l < SRK_FUND_LANES; ++l)
            for (int64_t k = l; k < n(); k += SRK_FUND_LANES) {
                int in;
                double s2;
                srk_fund_term(F, rec(k), f0, tau2, in, s2);
                if (in) srk_fund_accumulate(acc[l], lin, rec(k), f0);
            }
        merge_lanes(acc);
        for (int e = 0; e < SRK_FUND_ACC; ++e) total[e] = acc[0][e];
    }
};
} // namespace

uint32_t srk_fund_host_walk(int64_t n_obs, const double* uv_a, const double* uv_b, const double* q, double f0, const srk_fundamental_options& opts,
                            SrkFundResult& out, uint8_t* inlier_out, std::vector<double>* scores, std::vector<int32_t>* roots_out)
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    Walk w;
    w.f0 = f0;
    w.tau2 = opts.inlier_pixels * opts.inlier_pixels;
    for (int64_t o = 0; o < n_obs; ++o) // the gather
        if (!q || q[o] > 0.0) {
            w.rank.push_back(o);
            const double e[SRK_FUND_STRIP] = { uv_a[2 * o], uv_a[2 * o + 1], uv_b[2 * o], uv_b[2 * o + 1], q ? q[o] : 1.0, 0.0, 0.0, 0.0 };
            w.strip.insert(w.strip.end(), e, e + SRK_FUND_STRIP);
        }
    const int64_t n = w.n();
    SrkFundRep cur;
    srk_fund_identity(cur);
    out = SrkFundResult();
    for (int e = 0; e < 9; ++e) out.U[e] = cur.U[e], out.V[e] = cur.V[e];
    out.fund[0] = out.fund[3] = out.fund[5] = out.fund[8] = out.fund[10] = nan;
    out.fund[1] = (double)n;
    if (inlier_out)
        for (int64_t o = 0; o < n_obs; ++o) inlier_out[o] = 0;
    if (scores) scores->assign((size_t)opts.hypotheses, inf);
    if (roots_out) roots_out->assign((size_t)opts.hypotheses, -1);
    if (n < 8) return SRK_FUNDAMENTAL_FEW_POINTS;
    double best = inf, best_err8 = 0.0, Fh[9] = { 0 };
    int32_t best_h = -1, models = 0, best_roots = 0;
    const double if0 = 1.0 / f0;
    for (int32_t h = 0; h < opts.hypotheses; ++h) {
        int64_t r[8];
        srk_fund_sample(opts.seed, (uint32_t)h, n, r);
        double pa[21], pb[21];
        for (int k = 0; k < 7; ++k) {
            const double* e = w.rec(r[k]);
            pa[3 * k] = e[0] * if0, pa[3 * k + 1] = e[1] * if0, pa[3 * k + 2] = 1.0;
            pb[3 * k] = e[2] * if0, pb[3 * k + 1] = e[3] * if0, pb[3 * k + 2] = 1.0;
        }
        const double* e = w.rec(r[7]);
        const double e8[4] = { e[0], e[1], e[2], e[3] };
        double F[9], err8;
        int nroots;
        if (!srk_fund_hypothesis(pa, pb, e8, f0, F, err8, nroots)) continue;
        ++models;
        int64_t inl;
        double ss;
        const double sc = w.score(F, inl, ss);
        if (scores) (*scores)[(size_t)h] = sc;
        if (roots_out) (*roots_out)[(size_t)h] = nroots;
        if (sc < best) { // an equal score stays with the smaller h
            best = sc;
            best_h = h;
            best_err8 = err8;
            best_roots = nroots;
            for (int k = 0; k < 9; ++k) Fh[k] = F[k];
        }
    }
    out.fund[4] = (double)models;
    if (best_h < 0 || !srk_fund_represent(Fh, cur)) return SRK_FUNDAMENTAL_NO_MODEL;
    double F[9], acc[SRK_FUND_ACC] = { 0 }, ss;
    int64_t inl;
    srk_fund_build(cur, F);
    srk_fund_sign(cur, F); // the current model is always the signed one: the sums belong to the U that is returned
    best = w.score(F, inl, ss);
    double c = SRK_FUND_C0;
    int32_t accepted = 0, used = 0;
    bool fresh = true;
    for (int32_t attempt = 0; attempt < opts.refine_rounds; ++attempt) {
        if (inl < SRK_FUND_MIN_INLIERS) break;
        if (fresh) w.sums(cur, F, acc);
        fresh = false;
        if (!all_finite(acc, SRK_FUND_ACC)) break;
        ++used;
        double d[SRK_FUND_NV], Fc[9], sc = inf, css = 0.0;
        int64_t cinl = 0;
        SrkFundRep cand;
        const int stepped = srk_fund_lm_step(acc, c, d);
        if (stepped) {
            srk_fund_move(cur, d, cand);
            srk_fund_build(cand, Fc);
            sc = w.score(Fc, cinl, css);
        }
        const bool last = stepped && std::fabs(sc - best) <= SRK_FUND_STOP * best;
        if (stepped && sc < best) { // only a strictly smaller score is accepted
            best = sc;
            inl = cinl;
            ss = css;
            cur = cand;
            for (int e = 0; e < 9; ++e) F[e] = Fc[e];
            srk_fund_sign(cur, F);
            c /= 10.0;
            ++accepted;
            fresh = true;
        } else
            c *= 10.0;
        if (last) break;
    }
    if (fresh) w.sums(cur, F, acc); // the information at the result
    double A[SRK_FUND_NV][SRK_FUND_NV];
    srk_fund_full(acc, A);
    for (int a = 0; a < SRK_FUND_NV; ++a)
        for (int b = 0; b < SRK_FUND_NV; ++b) out.info[SRK_FUND_NV * a + b] = A[a][b];
    const double cond = srk_fund_cond1(A, nan);
    for (int e = 0; e < 9; ++e) out.F[e] = F[e], out.U[e] = cur.U[e], out.V[e] = cur.V[e];
    out.sigma = cur.sigma;
    out.fund[0] = std::sqrt(best / (double)n);
    out.fund[2] = (double)inl;
    out.fund[3] = (double)best_h;
    out.fund[5] = std::sqrt(best_err8);
    out.fund[6] = (double)accepted;
    out.fund[7] = (double)used;
    out.fund[8] = inl > 0 ? std::sqrt(ss / (double)inl) : 0.0; // a winner without inliers: nothing to average
    out.fund[9] = cur.sigma;
    out.fund[10] = cond;
    out.fund[11] = (double)best_roots;
    if (inlier_out)
        for (int64_t k = 0; k < n; ++k) {
            int in;
            double s2;
            srk_fund_term(F, w.rec(k), f0, w.tau2, in, s2);
            inlier_out[w.rank[(size_t)k]] = (uint8_t)in;
        }
    return 0;
}

extern "C" {

void srk_fundamental_default_options(srk_fundamental_options* o)
{
    if (!o) return;
    o->hypotheses = 256;
    o->inlier_pixels = 2.0;
    o->seed = 1;
    o->refine_rounds = 8;
}

int srk_fundamental_check_pairs(int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                                const srk_fundamental_options* opts, const char** why)
{
    static thread_local std::string text;
    try {
        text = srk_fund_check(n_pairs, row_ptr, uv_a, uv_b, q, opts);
    } catch (const std::bad_alloc&) {
        return SRK_E_NOMEM;
    }
    if (why) *why = text.c_str();
    return text.empty() ? SRK_OK : SRK_E_ARGS;
}

int srk_fundamental_host_pair(int64_t n_obs, const double* uv_a, const double* uv_b, const double* q, double f0, const srk_fundamental_options* opts,
                              double* F, double* U, double* V, double* sigma, double* fund, double* info, uint8_t* inlier_out)
{
    try {
        if (n_obs < 0 || !F || !U || !V || !sigma || !fund || !info || !std::isfinite(f0) || srk::is_close(0.0, f0)) return SRK_E_ARGS;
        const int64_t row_ptr[2] = { 0, n_obs };
        if (!srk_fund_check(1, row_ptr, uv_a, uv_b, q, opts).empty()) return SRK_E_ARGS;
        SrkFundResult out;
        const uint32_t st = srk_fund_host_walk(n_obs, uv_a, uv_b, q, f0, srk_fund_effective_options(opts), out, inlier_out);
        for (int e = 0; e < 9; ++e) F[e] = out.F[e], U[e] = out.U[e], V[e] = out.V[e];
        *sigma = out.sigma;
        for (int e = 0; e < 12; ++e) fund[e] = out.fund[e];
        for (int e = 0; e < 49; ++e) info[e] = out.info[e];
        return (int)st;
    } catch (const std::bad_alloc&) {
        return SRK_E_NOMEM;
    }
}

} // extern "C"
