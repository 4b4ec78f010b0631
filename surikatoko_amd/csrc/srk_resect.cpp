// srk_resect.cpp -- batched camera resection, the host half: see srk_resect.hpp.  No HIP.
#include "srk_resect.hpp"
#include "srk_resect_math.hpp"

#include <cmath>

static_assert(SRK_RESECT_FEW_POINTS == 1 && SRK_RESECT_DEGENERATE == 2 && SRK_RESECT_BEHIND == 4 && SRK_RESECT_NOT_CONVERGED == 8,
              "srk_resect_math.hpp writes the status bits as numbers");
static_assert(SRK_RESECT_FRAMES_PER_WG_HOST * SRK_RESECT_LANES == 256, "a workgroup of srk_resect.hip has 256 lanes");

srk_resect_options srk_resect_effective_options(const srk_resect_options* opts)
{
    if (opts) return *opts;
    srk_resect_options o;
    srk_resect_default_options(&o);
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
    const double det = z[0] * (z[4] * z[8] - z[5] * z[7]) - z[1] * (z[3] * z[8] - z[5] * z[6]) + z[2] * (z[3] * z[7] - z[4] * z[6]);
    return std::fabs(det - 1.0) > 1e-9 ? 2 : 0;
}
bool all_finite(const double* v, int64_t n)
{
    for (int64_t e = 0; e < n; ++e)
        if (!std::isfinite(v[e])) return false;
    return true;
}
} // namespace

std::string srk_resect_check(int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv, const double* q, int64_t n_points,
                             const double* X, const double* K, int shared_k, const double* R0, const double* T0, const srk_resect_options* opts,
                             const int64_t* point_int, std::vector<int32_t>* mapped)
{
    if (n_frames < 0) return "resect: a negative frame count";
    if (n_frames > SRK_RESECT_MAX_FRAMES_HOST) return "resect: too many frames in one call";
    if (n_points < 0 || n_points > 2147483647LL) return "resect: the landmark count is outside 0..2^31 - 1";
    if (!row_ptr) return "resect: row_ptr is NULL";
    if (opts) {
        if (opts->attempts < 0 || opts->attempts > SRK_RESECT_MAX_ATTEMPTS_HOST) return "resect: attempts outside 0.." + std::to_string(SRK_RESECT_MAX_ATTEMPTS_HOST);
        if (!(opts->rel_change >= 0.0) || !std::isfinite(opts->rel_change)) return "resect: rel_change must be finite and not negative";
        if (opts->loss_kind < 0 || opts->loss_kind > 2) return "resect: loss_kind outside 0..2";
        if (opts->loss_kind != 0 && (!(opts->loss_delta_pixels > 0.0) || !std::isfinite(opts->loss_delta_pixels)))
            return "resect: a loss needs a finite loss_delta_pixels > 0";
    }
    if (row_ptr[0] != 0) return "resect: row_ptr[0] != 0";
    for (int32_t i = 0; i < n_frames; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) return "resect: row_ptr decreases at frame " + std::to_string(i);
    const int64_t O = row_ptr[n_frames];
    if (O > 0 && (!point || !uv)) return "resect: a NULL observation array";
    if (n_frames > 0 && (!K || !R0 || !T0)) return "resect: a NULL pose or intrinsics array";
    if (mapped) mapped->resize((size_t)O);
    for (int64_t o = 0; o < O; ++o) {
        if (point[o] < 0 || point[o] >= n_points) return "resect: the point of observation " + std::to_string(o) + " is out of range";
        if (mapped) (*mapped)[(size_t)o] = point_int ? (int32_t)point_int[point[o]] : point[o];
        if (!std::isfinite(uv[2 * o]) || !std::isfinite(uv[2 * o + 1])) return "resect: uv of observation " + std::to_string(o) + " is not finite";
        if (q && (!(q[o] >= 0.0) || !std::isfinite(q[o]))) return "resect: q of observation " + std::to_string(o) + " must be finite and not negative";
    }
    if (X)
        for (int64_t i = 0; i < n_points; ++i)
            if (!all_finite(X + 3 * i, 3)) return "resect: landmark " + std::to_string(i) + " is not finite";
    for (int32_t i = 0; i < (shared_k ? (n_frames > 0 ? 1 : 0) : n_frames); ++i)
        if (!all_finite(K + 9 * (int64_t)i, 9)) return "resect: K of frame " + std::to_string(i) + " is not finite";
    for (int32_t i = 0; i < n_frames; ++i) {
        if (!all_finite(R0 + 9 * (int64_t)i, 9)) return "resect: R0 of frame " + std::to_string(i) + " is not finite";
        if (!all_finite(T0 + 3 * (int64_t)i, 3)) return "resect: T0 of frame " + std::to_string(i) + " is not finite";
        if (const int defect = rotation_defect(R0 + 9 * (int64_t)i))
            return "resect: R0 of frame " + std::to_string(i) + (defect == 1 ? " is not orthogonal to 1e-9" : " has determinant != 1");
    }
    return std::string();
}

void srk_resect_normalize_poses(const srk_ba_normalizer& nrm, int32_t n, const double* R, const double* T, double* Rn, double* Tn)
{
    const double s = nrm.world_scale;
    for (int32_t j = 0; j < n; ++j) { // NormalizeRT of the scene normalisation
        const double* r = R + 9 * (int64_t)j;
        double RR[9], u[3];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) RR[3 * a + b] = r[3 * a] * nrm.R0[3 * b] + r[3 * a + 1] * nrm.R0[3 * b + 1] + r[3 * a + 2] * nrm.R0[3 * b + 2];
        for (int a = 0; a < 3; ++a) u[a] = RR[3 * a] * nrm.T0[0] + RR[3 * a + 1] * nrm.T0[1] + RR[3 * a + 2] * nrm.T0[2];
        for (int a = 0; a < 3; ++a) Tn[3 * (int64_t)j + a] = (T[3 * (int64_t)j + a] - u[a]) * s;
        for (int e = 0; e < 9; ++e) Rn[9 * (int64_t)j + e] = RR[e];
    }
}

void srk_resect_revert_poses(const srk_ba_normalizer& nrm, int32_t n, double* R, double* T, double* info, double* quality)
{
    const double s = nrm.world_scale;
    const double* R0 = nrm.R0;
    for (int32_t j = 0; j < n; ++j) {
        if (R && T) { // RevertRT of the scene normalisation
            double* r = R + 9 * (int64_t)j;
            double* t = T + 3 * (int64_t)j;
            double RR[9], u[3];
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) RR[3 * a + b] = r[3 * a] * R0[b] + r[3 * a + 1] * R0[3 + b] + r[3 * a + 2] * R0[6 + b];
            for (int a = 0; a < 3; ++a) u[a] = r[3 * a] * nrm.T0[0] + r[3 * a + 1] * nrm.T0[1] + r[3 * a + 2] * nrm.T0[2];
            for (int a = 0; a < 3; ++a) t[a] = t[a] / s + u[a];
            for (int e = 0; e < 9; ++e) r[e] = RR[e];
        }
        if (quality) quality[6 * (int64_t)j + 4] /= s; // the smallest depth (NaN stays NaN), whatever cond_1 is
        if (info) { // 3 x 3 blocks: f R0^T B R0 with f = s per translation index, then symmetrised
            double* L = info + 36 * (int64_t)j;
            for (int bi = 0; bi < 2; ++bi)
                for (int bj = 0; bj < 2; ++bj) {
                    double B[9], U[9];
                    for (int a = 0; a < 3; ++a)
                        for (int c = 0; c < 3; ++c) B[3 * a + c] = L[(3 * bi + a) * 6 + 3 * bj + c];
                    for (int a = 0; a < 3; ++a)
                        for (int c = 0; c < 3; ++c) {
                            double v = 0;
                            for (int k = 0; k < 3; ++k)
                                for (int l = 0; l < 3; ++l) v += R0[3 * k + a] * B[3 * k + l] * R0[3 * l + c];
                            U[3 * a + c] = v;
                        }
                    const double f = (bi ? 1.0 : s) * (bj ? 1.0 : s);
                    for (int a = 0; a < 3; ++a)
                        for (int c = 0; c < 3; ++c) L[(3 * bi + a) * 6 + 3 * bj + c] = f * U[3 * a + c];
                }
            for (int r = 0; r < 6; ++r)
                for (int c = r + 1; c < 6; ++c) L[r * 6 + c] = L[c * 6 + r] = 0.5 * (L[r * 6 + c] + L[c * 6 + r]);
            if (quality && !std::isnan(quality[6 * (int64_t)j + 3])) {
                double A[6][6];
                for (int r = 0; r < 6; ++r)
                    for (int c = 0; c < 6; ++c) A[r][c] = L[r * 6 + c];
                quality[6 * (int64_t)j + 3] = srk_resect_cond1(A);
            }
        }
    }
}

namespace {
// the sums of a frame under the pack p: every lane over its observations, then the tree down by 32, 16, 8, 4, 2, 1
SrkResectSums host_eval(const std::vector<int64_t> (&mine)[SRK_RESECT_LANES], const int32_t* point, const double* uv, const double* q,
                        const double* X, const double* p, double f0, int kind, double delta)
{
    std::vector<SrkResectSums> s(SRK_RESECT_LANES);
    for (int l = 0; l < SRK_RESECT_LANES; ++l) {
        srk_resect_sums_zero(s[l]);
        for (int64_t o : mine[l]) srk_resect_obs(s[l], p, X + 3 * (int64_t)point[o], uv[2 * o], uv[2 * o + 1], f0, q ? q[o] : 1.0, kind, delta);
    }
    for (int d = SRK_RESECT_LANES / 2; d >= 1; d >>= 1)
        for (int l = 0; l < d; ++l) srk_resect_sums_add(s[l], s[l + d]);
    return s[0];
}
} // namespace

uint32_t srk_resect_host_frame(int64_t n_obs, const int32_t* point, const double* uv, const double* q, const double* X, const double* K,
                               const double* R0, const double* T0, double f0, const srk_resect_options& opts, double R[9], double T[3],
                               double quality[6], double info[36], double* w_out, std::vector<int>* log)
{
    std::vector<int64_t> mine[SRK_RESECT_LANES];
    int64_t n = 0;
    for (int64_t o = 0; o < n_obs; ++o)
        if (!q || q[o] > 0.0) mine[n++ % SRK_RESECT_LANES].push_back(o);
    const int kind = opts.loss_kind;
    const double delta = opts.loss_delta_pixels;
    SrkResectPose cur;
    srk_resect_start_pose(R0, T0, cur);
    double p[SRK_RESECT_PACK];
    srk_resect_pack_pose(cur, K, p);
    SrkResectSums cs = host_eval(mine, point, uv, q, X, p, f0, kind, delta);
    int hit_cap = 0, used = 0;
    if (n >= 3 && opts.attempts > 0) {
        double c = SRK_RESECT_C0;
        hit_cap = 1;
        for (int32_t a = 0; a < opts.attempts; ++a) {
            double d[6];
            const int stepped = srk_resect_lm_step(cs, c, d);
            SrkResectPose cand = cur;
            SrkResectSums ns;
            srk_resect_sums_zero(ns);
            if (stepped) {
                srk_resect_move(cur, d, cand);
                srk_resect_pack_pose(cand, K, p);
                ns = host_eval(mine, point, uv, q, X, p, f0, kind, delta);
            }
            const int verdict = srk_resect_judge(cs.E, ns.E, stepped, c, opts.rel_change);
            ++used;
            if (log) log->push_back(verdict & 1);
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
    const uint32_t st = n >= 3 ? srk_resect_finish(cs, n, f0, hit_cap, used, quality, info) : srk_resect_few(n, quality, info);
    for (int e = 0; e < 9; ++e) R[e] = cur.R[e];
    for (int e = 0; e < 3; ++e) T[e] = cur.T[e];
    if (w_out) {
        srk_resect_pack_pose(cur, K, p);
        for (int64_t o = 0; o < n_obs; ++o) {
            const double qo = q ? q[o] : 1.0;
            w_out[o] = qo > 0.0 ? srk_resect_weight(p, X + 3 * (int64_t)point[o], uv[2 * o], uv[2 * o + 1], f0, qo, kind, delta) : 0.0;
        }
    }
    return st;
}

extern "C" {

void srk_resect_default_options(srk_resect_options* o)
{
    if (!o) return;
    o->attempts = 10;
    o->rel_change = 1e-9;
    o->loss_kind = 0;
    o->loss_delta_pixels = 0.0;
}

int srk_resect_check_frames(int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv, const double* q, int64_t n_points,
                            const double* X, const double* K, int shared_k, const double* R0, const double* T0, const srk_resect_options* opts,
                            const char** why)
{
    static thread_local std::string text;
    text = srk_resect_check(n_frames, row_ptr, point, uv, q, n_points, X, K, shared_k, R0, T0, opts);
    if (text.empty() && n_points > 0 && !X) text = "resect: the landmark array is NULL";
    if (why) *why = text.c_str();
    return text.empty() ? SRK_OK : SRK_E_ARGS;
}

int srk_resect_revert(const srk_ba_normalizer* nrm, int32_t n, double* R, double* T, double* info)
{
    if (!nrm || n < 0 || !(nrm->world_scale > 0) || !std::isfinite(nrm->world_scale) || ((R == nullptr) != (T == nullptr))) return SRK_E_ARGS;
    srk_resect_revert_poses(*nrm, n, R, T, info);
    return SRK_OK;
}

} // extern "C"
