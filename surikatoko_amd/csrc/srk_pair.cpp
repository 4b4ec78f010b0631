// srk_pair.cpp -- two-view pose refinement, the host half: see srk_pair.hpp.  No HIP.
#include "srk_pair.hpp"
#include "srk_pair_math.hpp"

#include <cmath>
#include <limits>

static_assert(SRK_PAIR_FEW_POINTS == 1 && SRK_PAIR_DEGENERATE == 2 && SRK_PAIR_NOT_CONVERGED == 8, "srk_pair_math.hpp writes the status bits as numbers");
static_assert(SRK_PAIR_LANES == 64, "a pair is one wave of srk_pair.hip");

srk_pair_options srk_pair_effective_options(const srk_pair_options* opts)
{
    if (opts) return *opts;
    srk_pair_options o;
    srk_pair_default_options(&o);
    return o;
}

namespace {
// the joint-prior setter's rule: orthogonal to 1e-9 and of determinant 1.  0 = a rotation, 1 / 2 = which it is not.
int rotation_defect(const double* z)
{
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double g = z[a] * z[b] + z[3 + a] * z[3 + b] + z[6 + a] * z[6 + b] - (a == b ? 1.0 : 0.0);
            if (std::fabs(g) > 1e-9) return 1;
        }
    return std::fabs(srk_relate_det3(z) - 1.0) > 1e-9 ? 2 : 0;
}
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
        if (!all_finite(k, 9)) return std::string("pair: ") + which + " of pair " + std::to_string(i) + " is not finite";
        double big = 0.0;
        for (int e = 0; e < 9; ++e) big = std::fmax(big, std::fabs(k[e]));
        // singular to rounding: the determinant is a sum of products of three entries (relate's rule)
        if (!(std::fabs(srk_relate_det3(k)) > 1e-12 * big * big * big)) return std::string("pair: ") + which + " of pair " + std::to_string(i) + " is singular";
    }
    return std::string();
}
} // namespace

std::string srk_pair_check_options(const srk_pair_options* opts, bool chained)
{
    if (!opts) return std::string();
    if (opts->attempts < 0 || opts->attempts > SRK_PAIR_MAX_ATTEMPTS_HOST) return "pair: attempts outside 0.." + std::to_string(SRK_PAIR_MAX_ATTEMPTS_HOST);
    if (!(opts->rel_change >= 0.0) || !std::isfinite(opts->rel_change)) return "pair: rel_change must be finite and not negative";
    if (opts->loss_kind < 0 || opts->loss_kind > 2) return "pair: loss_kind outside 0..2";
    if (opts->loss_kind != 0 && (!(opts->loss_delta_pixels > 0.0) || !std::isfinite(opts->loss_delta_pixels)))
        return "pair: a loss needs a finite loss_delta_pixels > 0";
    if (opts->inliers_only != 0 && opts->inliers_only != 1) return "pair: inliers_only must be 0 or 1";
    if (!chained && opts->inliers_only != 0) return "pair: inliers_only has no meaning without relate's inliers and must be 0";
    return std::string();
}

std::string srk_pair_check(int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q, const double* K_a,
                           const double* K_b, int shared_k, const double* R0, const double* T0, const srk_pair_options* opts)
{
    if (n_pairs < 0) return "pair: a negative pair count";
    if (n_pairs > SRK_PAIR_MAX_PAIRS_HOST) return "pair: too many pairs in one call";
    if (!row_ptr) return "pair: row_ptr is NULL";
    std::string why = srk_pair_check_options(opts, false);
    if (!why.empty()) return why;
    if (row_ptr[0] != 0) return "pair: row_ptr[0] != 0";
    for (int32_t i = 0; i < n_pairs; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) return "pair: row_ptr decreases at pair " + std::to_string(i);
    const int64_t O = row_ptr[n_pairs];
    if (O > 0 && (!uv_a || !uv_b)) return "pair: a NULL match array";
    if (n_pairs > 0 && (!K_a || !K_b)) return "pair: an intrinsics array is NULL";
    if (n_pairs > 0 && (!R0 || !T0)) return "pair: a NULL start pose array";
    for (int64_t o = 0; o < O; ++o) {
        if (!all_finite(uv_a + 2 * o, 2)) return "pair: uv_a of match " + std::to_string(o) + " is not finite";
        if (!all_finite(uv_b + 2 * o, 2)) return "pair: uv_b of match " + std::to_string(o) + " is not finite";
        if (q && (!(q[o] >= 0.0) || !std::isfinite(q[o]))) return "pair: q of match " + std::to_string(o) + " must be finite and not negative";
    }
    const int32_t nk = shared_k ? (n_pairs > 0 ? 1 : 0) : n_pairs;
    why = check_k(K_a, nk, "K_a");
    if (why.empty()) why = check_k(K_b, nk, "K_b");
    if (!why.empty()) return why;
    for (int32_t i = 0; i < n_pairs; ++i) {
        const double* r = R0 + 9 * (int64_t)i;
        const double* t = T0 + 3 * (int64_t)i;
        if (!all_finite(r, 9)) return "pair: R0 of pair " + std::to_string(i) + " is not finite";
        if (!all_finite(t, 3)) return "pair: T0 of pair " + std::to_string(i) + " is not finite";
        if (const int defect = rotation_defect(r))
            return "pair: R0 of pair " + std::to_string(i) + (defect == 1 ? " is not orthogonal to 1e-9" : " has determinant != 1");
        if (std::fabs(std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) - 1.0) > 1e-9) return "pair: T0 of pair " + std::to_string(i) + " is not a unit vector to 1e-9";
    }
    return std::string();
}

namespace {
// the sums of a pair at the pose p: every lane over its matches, then the tree down by 32, 16, 8, 4, 2, 1
SrkPairSums host_eval(const std::vector<int64_t> (&mine)[SRK_PAIR_LANES], const double* uv_a, const double* uv_b, const double* q, const double* kinv,
                      const SrkPairPose& p, double f0, int kind, double delta)
{
    SrkPairLin lin;
    srk_pair_linearise(kinv, p, lin);
    std::vector<SrkPairSums> s(SRK_PAIR_LANES);
    for (int l = 0; l < SRK_PAIR_LANES; ++l) {
        srk_pair_sums_zero(s[l]);
        for (int64_t o : mine[l]) srk_pair_obs(s[l], lin, uv_a[2 * o], uv_a[2 * o + 1], uv_b[2 * o], uv_b[2 * o + 1], f0, q ? q[o] : 1.0, kind, delta);
    }
    for (int d = SRK_PAIR_LANES / 2; d >= 1; d >>= 1)
        for (int l = 0; l < d; ++l) srk_pair_sums_add(s[l], s[l + d]);
    return s[0];
}
} // namespace

uint32_t srk_pair_host_pair_cpp(int64_t n_obs, const double* uv_a, const double* uv_b, const double* q, const double* K_a, const double* K_b,
                                double f0, const double* R0, const double* T0, const srk_pair_options& opts, double R[9], double T[3], double E[9],
                                double quality[6], double info[25], double basis[6], double* w_out, double* grad, std::vector<SrkPairAttempt>* log)
{
    std::vector<int64_t> mine[SRK_PAIR_LANES];
    int64_t n = 0;
    for (int64_t o = 0; o < n_obs; ++o)
        if (!q || q[o] > 0.0) mine[n++ % SRK_PAIR_LANES].push_back(o);
    const int kind = opts.loss_kind;
    const double delta = opts.loss_delta_pixels;
    double kinv[SRK_PAIR_KINV];
    srk_relate_inverse3(K_a, kinv);
    srk_relate_inverse3(K_b, kinv + 9);
    SrkPairPose cur;
    srk_pair_start_pose(R0, T0, 0, cur);
    SrkPairSums cs = host_eval(mine, uv_a, uv_b, q, kinv, cur, f0, kind, delta);
    int hit_cap = 0, used = 0;
    if (n >= SRK_PAIR_NV && opts.attempts > 0) {
        double c = SRK_RESECT_C0;
        hit_cap = 1;
        for (int32_t a = 0; a < opts.attempts; ++a) {
            double d[SRK_PAIR_NV];
            const int stepped = srk_pair_lm_step(cs, c, d);
            SrkPairPose cand = cur;
            SrkPairSums ns;
            srk_pair_sums_zero(ns);
            if (stepped) {
                srk_pair_move(cur, d, cand);
                ns = host_eval(mine, uv_a, uv_b, q, kinv, cand, f0, kind, delta);
            }
            const int verdict = srk_resect_judge(cs.E, ns.E, stepped, c, opts.rel_change);
            ++used;
            if (log) log->push_back({ verdict & 1, cs.E, stepped ? ns.E : std::numeric_limits<double>::quiet_NaN() });
            if (verdict & 1) {
                cur = cand;
                cs = ns;
            }
            if (verdict & 2) {
                hit_cap = 0;
                break;
            }
        }
    }
    int64_t front = 0;
    if (n >= SRK_PAIR_NV)
        for (int l = 0; l < SRK_PAIR_LANES; ++l)
            for (int64_t o : mine[l]) front += srk_pair_front(kinv, cur, uv_a[2 * o], uv_a[2 * o + 1], uv_b[2 * o], uv_b[2 * o + 1], f0);
    const uint32_t st = n >= SRK_PAIR_NV ? srk_pair_finish(cs, cur, n, front, f0, hit_cap, used, E, quality, info, basis) : srk_pair_few(cur, n, E, quality, info, basis);
    for (int e = 0; e < 9; ++e) R[e] = cur.R[e];
    for (int e = 0; e < 3; ++e) T[e] = cur.T[e];
    if (grad)
        for (int e = 0; e < SRK_PAIR_NV; ++e) grad[e] = cs.g[e];
    if (w_out) {
        double Ec[9], F[9];
        srk_relate_essential(cur.R, cur.T, Ec);
        srk_relate_fundamental(kinv, kinv + 9, Ec, F);
        for (int64_t o = 0; o < n_obs; ++o) {
            const double qo = q ? q[o] : 1.0;
            w_out[o] = qo > 0.0 ? srk_pair_weight(F, uv_a[2 * o], uv_a[2 * o + 1], uv_b[2 * o], uv_b[2 * o + 1], f0, qo, kind, delta) : 0.0;
        }
    }
    return st;
}

extern "C" {

void srk_pair_default_options(srk_pair_options* o)
{
    if (!o) return;
    o->attempts = 10;
    o->rel_change = 1e-9;
    o->loss_kind = 0;
    o->loss_delta_pixels = 0.0;
    o->inliers_only = 0;
}

int srk_pair_check_pairs(int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q, const double* K_a,
                         const double* K_b, int shared_k, const double* R0, const double* T0, const srk_pair_options* opts, const char** why)
{
    static thread_local std::string text;
    try {
        text = srk_pair_check(n_pairs, row_ptr, uv_a, uv_b, q, K_a, K_b, shared_k, R0, T0, opts);
    } catch (const std::bad_alloc&) {
        if (why) *why = "pair: out of host memory";
        return SRK_E_NOMEM;
    }
    if (why) *why = text.c_str();
    return text.empty() ? SRK_OK : SRK_E_ARGS;
}

int srk_pair_host_pair(int64_t n_obs, const double* uv_a, const double* uv_b, const double* q, const double* K_a, const double* K_b, double f0,
                       const double* R0, const double* T0, const srk_pair_options* opts, double* R, double* T, double* E, double* quality,
                       double* info, double* basis, double* w_out, double* grad, double* log, int32_t* log_count)
{
    try {
        const int64_t row_ptr[2] = { 0, n_obs };
        if (n_obs < 0 || !R || !T || !E || !quality || !info || !basis || !std::isfinite(f0) || f0 == 0.0) return SRK_E_ARGS;
        if (!srk_pair_check(1, row_ptr, uv_a, uv_b, q, K_a, K_b, 1, R0, T0, opts).empty()) return SRK_E_ARGS;
        std::vector<SrkPairAttempt> attempts;
        const uint32_t st = srk_pair_host_pair_cpp(n_obs, uv_a, uv_b, q, K_a, K_b, f0, R0, T0, srk_pair_effective_options(opts), R, T, E, quality, info,
                                                   basis, w_out, grad, &attempts);
        if (log)
            for (size_t a = 0; a < attempts.size(); ++a) {
                log[3 * a] = (double)attempts[a].accepted;
                log[3 * a + 1] = attempts[a].E_cur;
                log[3 * a + 2] = attempts[a].E_cand;
            }
        if (log_count) *log_count = (int32_t)attempts.size();
        return (int)st;
    } catch (const std::bad_alloc&) {
        return SRK_E_NOMEM;
    }
}

int srk_pair_factor(const double* R, const double* T, const double* info, const double* basis, double baseline, double* rel_R, double* rel_t,
                    double* info21)
{
    if (!R || !T || !info || !basis || !rel_R || !rel_t || !info21) return SRK_E_ARGS;
    if (!(baseline > 0.0) || !std::isfinite(baseline) || !all_finite(R, 9) || !all_finite(T, 3) || !all_finite(info, 25) || !all_finite(basis, 6))
        return SRK_E_ARGS;
    // Z = R^T, z = -lambda R^T T
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) rel_R[3 * a + b] = R[3 * b + a];
        rel_t[a] = -baseline * (R[a] * T[0] + R[3 + a] * T[1] + R[6 + a] * T[2]);
    }
    // M (5 x 6) = [[0, R^T], [-(1 / lambda) B^T R, B^T [T]x]] over [e_t; e_r]
    double M[5][6] = {};
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) M[a][3 + b] = R[3 * b + a];
    for (int j = 0; j < 2; ++j) {
        const double* bj = basis + 3 * j;
        for (int b = 0; b < 3; ++b) M[3 + j][b] = -(bj[0] * R[b] + bj[1] * R[3 + b] + bj[2] * R[6 + b]) / baseline;
        // b_j^T [T]x = (b_j x T)^T
        double c[3];
        srk_relate_cross(bj, T, c);
        for (int b = 0; b < 3; ++b) M[3 + j][3 + b] = c[b];
    }
    double IM[5][6]; // info M
    for (int a = 0; a < 5; ++a)
        for (int b = 0; b < 6; ++b) {
            double v = 0.0;
            for (int k = 0; k < 5; ++k) v += 0.5 * (info[5 * a + k] + info[5 * k + a]) * M[k][b];
            IM[a][b] = v;
        }
    int e = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) {
            double v = 0.0;
            for (int k = 0; k < 5; ++k) v += M[k][a] * IM[k][b];
            info21[e++] = v;
        }
    return SRK_OK;
}

} // extern "C"
