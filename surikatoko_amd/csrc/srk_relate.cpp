// srk_relate.cpp -- two-view relative pose, the host half: see srk_relate.hpp.  No HIP.
#include "srk_relate.hpp"
#include "srk_relate_math.hpp"

#include <cmath>
#include <limits>

static_assert(SRK_RELATE_FEW_POINTS == 1 && SRK_RELATE_NO_MODEL == 2, "srk_relate.hip writes the status bits as numbers");
static_assert(SRK_RELATE_LANES_HOST == SRK_RELATE_LANES, "a wave of k_relate_score holds 64 hypotheses");

srk_relate_options srk_relate_effective_options(const srk_relate_options* opts)
{
    if (opts) return *opts;
    srk_relate_options o;
    srk_relate_default_options(&o);
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
        if (!all_finite(k, 9)) return std::string("relate: ") + which + " of pair " + std::to_string(i) + " is not finite";
        double big = 0.0;
        for (int e = 0; e < 9; ++e) big = std::fmax(big, std::fabs(k[e]));
        // singular to rounding: the determinant is a sum of products of three entries
        if (!(std::fabs(srk_relate_det3(k)) > 1e-12 * big * big * big)) return std::string("relate: ") + which + " of pair " + std::to_string(i) + " is singular";
    }
    return std::string();
}

// level D of the derivative chain: the brackets are the bound and the roots of level D - 1; interval k is lane k's on the device
template <int D> int level(const double* p, double bound, double* z, int n)
{
    double a[12], found[11];
    a[0] = -bound;
    for (int k = 0; k < n; ++k) a[k + 1] = z[k];
    a[n + 1] = bound;
    int m = 0;
    for (int k = 0; k <= n; ++k) {
        double root;
        if (srk_relate_interval<D>(p, a[k], a[k + 1], root)) found[m++] = root;
    }
    for (int k = 0; k < m; ++k) z[k] = found[k];
    return m;
}
} // namespace

std::string srk_relate_check(int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q, const double* K_a,
                             const double* K_b, int shared_k, const srk_relate_options* opts)
{
    if (n_pairs < 0) return "relate: a negative pair count";
    if (!row_ptr) return "relate: row_ptr is NULL";
    const srk_relate_options lo = srk_relate_effective_options(opts);
    if (lo.hypotheses < 1 || lo.hypotheses > SRK_RELATE_MAX_HYPOTHESES_HOST)
        return "relate: hypotheses outside 1.." + std::to_string(SRK_RELATE_MAX_HYPOTHESES_HOST);
    if (!(lo.inlier_pixels > 0.0) || !std::isfinite(lo.inlier_pixels)) return "relate: inlier_pixels must be finite and > 0";
    if ((int64_t)n_pairs * ((lo.hypotheses + SRK_RELATE_LANES - 1) / SRK_RELATE_LANES) > SRK_RELATE_MAX_WAVES_HOST)
        return "relate: pairs x ceil(hypotheses / 64) exceeds " + std::to_string(SRK_RELATE_MAX_WAVES_HOST) + ": split the batch";
    if (row_ptr[0] != 0) return "relate: row_ptr[0] != 0";
    for (int32_t i = 0; i < n_pairs; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) return "relate: row_ptr decreases at pair " + std::to_string(i);
    const int64_t O = row_ptr[n_pairs];
    if (O > 0 && (!uv_a || !uv_b)) return "relate: a NULL match array";
    if (n_pairs > 0 && (!K_a || !K_b)) return "relate: an intrinsics array is NULL";
    for (int64_t o = 0; o < O; ++o) {
        if (!all_finite(uv_a + 2 * o, 2)) return "relate: uv_a of match " + std::to_string(o) + " is not finite";
        if (!all_finite(uv_b + 2 * o, 2)) return "relate: uv_b of match " + std::to_string(o) + " is not finite";
        if (q && (!(q[o] >= 0.0) || !std::isfinite(q[o]))) return "relate: q of match " + std::to_string(o) + " must be finite and not negative";
    }
    const int32_t nk = shared_k ? (n_pairs > 0 ? 1 : 0) : n_pairs;
    std::string why = check_k(K_a, nk, "K_a");
    if (why.empty()) why = check_k(K_b, nk, "K_b");
    return why;
}

int srk_relate_host_hypothesis(const double* Kai, const double* Kbi, const double* uva, const double* uvb, double f0, double* rec, double* all_E)
{
    double xa[15], xb[15], N[36];
    for (int m = 0; m < 5; ++m) {
        srk_relate_ray(Kai, uva[2 * m], uva[2 * m + 1], f0, xa + 3 * m);
        srk_relate_ray(Kbi, uvb[2 * m], uvb[2 * m + 1], f0, xb + 3 * m);
    }
    srk_relate_nullspace(xa, xb, N);
    double rows[10][20];
    for (int r = 0; r < 10; ++r) srk_relate_row(N, r, rows[r]);
    // Gauss-Jordan on the left ten columns: the pivot of column c is the largest entry among the rows that own no column yet (an
    // equal entry: the smaller row), and that row owns c from then on
    bool used[10] = {};
    int owner[10];
    for (int c = 0; c < 10; ++c) {
        double best = -1.0;
        int p = -1;
        for (int l = 0; l < 10; ++l) {
            const double a = used[l] ? -1.0 : std::fabs(rows[l][c]);
            if (a > best) best = a, p = l;
        }
        if (p < 0)
            for (int l = 9; l >= 0; --l)
                if (!used[l]) p = l;
        const double inv = 1.0 / rows[p][c];
        double piv[20];
        for (int j = c; j < 20; ++j) piv[j] = rows[p][j] * inv;
        for (int l = 0; l < 10; ++l) {
            const double f = rows[l][c];
            for (int j = c; j < 20; ++j) rows[l][j] = l == p ? piv[j] : rows[l][j] - f * piv[j];
        }
        used[p] = true;
        owner[c] = p;
    }
    double bx[12], by[12], b1[15], p[11];
    srk_relate_bz(rows[owner[4]] + 10, rows[owner[5]] + 10, rows[owner[6]] + 10, rows[owner[7]] + 10, rows[owner[8]] + 10, rows[owner[9]] + 10, bx, by, b1);
    srk_relate_detb(bx, by, b1, p);
    const double bound = srk_relate_bound(p);
    double z[11];
    int n = 0;
    n = level<1>(p, bound, z, n);
    n = level<2>(p, bound, z, n);
    n = level<3>(p, bound, z, n);
    n = level<4>(p, bound, z, n);
    n = level<5>(p, bound, z, n);
    n = level<6>(p, bound, z, n);
    n = level<7>(p, bound, z, n);
    n = level<8>(p, bound, z, n);
    n = level<9>(p, bound, z, n);
    n = level<10>(p, bound, z, n);
    for (int e = 0; e < SRK_RELATE_HYP; ++e) rec[e] = 0.0;
    double best = std::numeric_limits<double>::infinity();
    for (int k = 0; k < n; ++k) { // ascending root: an equal error stays with the smaller one
        double E[9], F[9];
        srk_relate_model(N, bx, by, b1, z[k], E);
        srk_relate_fundamental(Kai, Kbi, E, F);
        const double e6 = srk_relate_sampson(F, uva[10], uva[11], uvb[10], uvb[11], f0);
        if (all_E)
            for (int e = 0; e < 9; ++e) all_E[9 * k + e] = E[e];
        if (std::isfinite(e6) && e6 < best) {
            best = e6;
            for (int e = 0; e < 9; ++e) rec[e] = F[e], rec[9 + e] = E[e];
            rec[18] = e6;
            rec[19] = 1.0;
        }
    }
    return n;
}

void srk_relate_poses_of(const double* E, double* R, double* T)
{
    double R1[9], R2[9], t[3];
    srk_relate_decompose(E, R1, R2, t);
    for (int k = 0; k < 4; ++k) {
        for (int e = 0; e < 9; ++e) R[9 * k + e] = k < 2 ? R1[e] : R2[e];
        for (int e = 0; e < 3; ++e) T[3 * k + e] = (k & 1) ? -t[e] : t[e];
    }
}

uint32_t srk_relate_host_pair_cpp(int64_t n_obs, const double* uv_a, const double* uv_b, const double* q, const double* K_a, const double* K_b,
                                  double f0, const srk_relate_options& opts, double R[9], double T[3], double E[9], double related[8],
                                  uint8_t* inlier_out, std::vector<double>* scores)
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    std::vector<int64_t> rank; // the gather: the weighted matches in ascending o
    for (int64_t o = 0; o < n_obs; ++o)
        if (!q || q[o] > 0.0) rank.push_back(o);
    const int64_t n = (int64_t)rank.size();
    const double tau2 = opts.inlier_pixels * opts.inlier_pixels;
    for (int e = 0; e < 9; ++e) R[e] = (e % 4 == 0) ? 1.0 : 0.0, E[e] = 0.0;
    T[0] = T[1] = T[2] = 0.0;
    related[0] = related[3] = related[5] = related[7] = nan;
    related[1] = (double)n;
    related[2] = related[4] = related[6] = 0.0;
    if (inlier_out)
        for (int64_t o = 0; o < n_obs; ++o) inlier_out[o] = 0;
    if (scores) scores->assign((size_t)opts.hypotheses, inf);
    if (n < 6) return SRK_RELATE_FEW_POINTS;
    double Kai[9], Kbi[9];
    srk_relate_inverse3(K_a, Kai);
    srk_relate_inverse3(K_b, Kbi);
    double best_rec[SRK_RELATE_HYP] = {};
    double best_score = inf;
    int32_t best_h = -1, best_inl = 0, models = 0;
    for (int32_t h = 0; h < opts.hypotheses; ++h) {
        int64_t r[6];
        srk_relate_sample(opts.seed, (uint32_t)h, n, r);
        double ua[12], ub[12], rec[SRK_RELATE_HYP];
        for (int k = 0; k < 6; ++k) {
            const int64_t o = rank[(size_t)r[k]];
            ua[2 * k] = uv_a[2 * o], ua[2 * k + 1] = uv_a[2 * o + 1];
            ub[2 * k] = uv_b[2 * o], ub[2 * k + 1] = uv_b[2 * o + 1];
        }
        srk_relate_host_hypothesis(Kai, Kbi, ua, ub, f0, rec, nullptr);
        if (rec[19] == 0.0) continue;
        ++models;
        double score = 0.0;
        int32_t inl = 0;
        for (int64_t k = 0; k < n; ++k) { // ascending rank, one accumulator
            const int64_t o = rank[(size_t)k];
            int in;
            score += srk_relate_term(rec, uv_a[2 * o], uv_a[2 * o + 1], uv_b[2 * o], uv_b[2 * o + 1], q ? q[o] : 1.0, f0, tau2, in);
            inl += in;
        }
        if (scores) (*scores)[(size_t)h] = score;
        if (score < best_score) { // an equal score stays with the smaller h
            best_score = score;
            best_h = h;
            best_inl = inl;
            for (int e = 0; e < SRK_RELATE_HYP; ++e) best_rec[e] = rec[e];
        }
    }
    related[4] = (double)models;
    if (best_h < 0) return SRK_RELATE_NO_MODEL;
    // the pick: the vote of the four poses over the inliers, lane l of the wave takes the ranks l, l + 64, ...
    double R1[9], R2[9], t[3];
    srk_relate_decompose(best_rec + 9, R1, R2, t);
    int32_t cnt[4][SRK_RELATE_LANES] = {};
    double ang[4][SRK_RELATE_LANES] = {};
    for (int64_t k = 0; k < n; ++k) {
        const int64_t o = rank[(size_t)k];
        const int l = (int)(k % SRK_RELATE_LANES);
        int in;
        srk_relate_term(best_rec, uv_a[2 * o], uv_a[2 * o + 1], uv_b[2 * o], uv_b[2 * o + 1], q ? q[o] : 1.0, f0, tau2, in);
        if (inlier_out) inlier_out[o] = (uint8_t)in;
        if (!in) continue;
        double a[3], b[3];
        srk_relate_ray(Kai, uv_a[2 * o], uv_a[2 * o + 1], f0, a);
        srk_relate_ray(Kbi, uv_b[2 * o], uv_b[2 * o + 1], f0, b);
        for (int c = 0; c < 4; ++c) {
            double angle;
            if (srk_relate_front(c < 2 ? R1 : R2, t, (c & 1) ? -1.0 : 1.0, a, b, angle)) {
                ++cnt[c][l];
                ang[c][l] += angle;
            }
        }
    }
    for (int d = SRK_RELATE_LANES / 2; d >= 1; d >>= 1) // the wave's tree
        for (int l = 0; l < d; ++l)
            for (int c = 0; c < 4; ++c) {
                cnt[c][l] += cnt[c][l + d];
                ang[c][l] += ang[c][l + d];
            }
    int c = 0;
    for (int k = 1; k < 4; ++k)
        if (cnt[k][0] > cnt[c][0]) c = k;
    for (int e = 0; e < 9; ++e) R[e] = c < 2 ? R1[e] : R2[e];
    for (int e = 0; e < 3; ++e) T[e] = (c & 1) ? -t[e] : t[e];
    srk_relate_essential(R, T, E);
    related[0] = std::sqrt(best_score / (double)n);
    related[2] = (double)best_inl;
    related[3] = (double)best_h;
    related[5] = std::sqrt(best_rec[18]);
    related[6] = (double)cnt[c][0];
    related[7] = ang[c][0] / (double)cnt[c][0];
    return 0;
}

extern "C" {

void srk_relate_default_options(srk_relate_options* o)
{
    if (!o) return;
    o->hypotheses = 256;
    o->inlier_pixels = 2.0;
    o->seed = 1;
}

int srk_relate_check_pairs(int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q, const double* K_a,
                           const double* K_b, int shared_k, const srk_relate_options* opts, const char** why)
{
    static thread_local std::string text;
    try {
        text = srk_relate_check(n_pairs, row_ptr, uv_a, uv_b, q, K_a, K_b, shared_k, opts);
    } catch (const std::bad_alloc&) {
        if (why) *why = "relate: out of host memory";
        return SRK_E_NOMEM;
    }
    if (why) *why = text.c_str();
    return text.empty() ? SRK_OK : SRK_E_ARGS;
}

int srk_relate_host_pair(int64_t n_obs, const double* uv_a, const double* uv_b, const double* q, const double* K_a, const double* K_b, double f0,
                         const srk_relate_options* opts, double* R, double* T, double* E, double* related, uint8_t* inlier_out)
{
    try {
        const int64_t row_ptr[2] = { 0, n_obs };
        if (n_obs < 0 || !R || !T || !E || !related || !std::isfinite(f0) || f0 == 0.0) return SRK_E_ARGS;
        if (!srk_relate_check(1, row_ptr, uv_a, uv_b, q, K_a, K_b, 1, opts).empty()) return SRK_E_ARGS;
        return (int)srk_relate_host_pair_cpp(n_obs, uv_a, uv_b, q, K_a, K_b, f0, srk_relate_effective_options(opts), R, T, E, related, inlier_out);
    } catch (const std::bad_alloc&) {
        return SRK_E_NOMEM;
    }
}

} // extern "C"
