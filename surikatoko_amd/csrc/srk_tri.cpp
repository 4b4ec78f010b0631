// srk_tri.cpp -- batched triangulation, the host half: see srk_tri.hpp.  No HIP.
#include "srk_tri.hpp"
#include "srk_tri_math.hpp"

#include <cmath>

static_assert(SRK_TRI_FEW_VIEWS == 1 && SRK_TRI_DEGENERATE == 2 && SRK_TRI_BEHIND == 4 && SRK_TRI_LOW_PARALLAX == 8 && SRK_TRI_NOT_CONVERGED == 16,
              "srk_tri_math.hpp and srk_tri.hip write the status bits as numbers");
static_assert(SRK_TRI_TRACKS_PER_WG_HOST * SRK_TRI_GROUP == 256, "a workgroup of srk_tri.hip has 256 lanes");

srk_tri_options srk_tri_effective_options(const srk_tri_options* opts)
{
    if (opts) return *opts;
    srk_tri_options o;
    o.refine_attempts = 0;
    o.refine_rel_change = 0.0;
    o.min_parallax_deg = 0.0;
    return o;
}

std::string srk_tri_check(int64_t n_tracks, const int64_t* row_ptr, const int32_t* frame, const double* uv, const double* q, int32_t n_frames,
                          const srk_tri_options* opts)
{
    if (n_tracks < 0) return "triangulate: a negative track count";
    if (n_tracks > SRK_TRI_MAX_TRACKS_HOST) return "triangulate: too many tracks in one call";
    if (n_frames < 1) return "triangulate: need at least one frame";
    if (!row_ptr) return "triangulate: row_ptr is NULL";
    if (opts) {
        if (opts->refine_attempts < 0 || opts->refine_attempts > SRK_TRI_MAX_REFINE_ATTEMPTS_HOST)
            return "triangulate: refine_attempts outside 0.." + std::to_string(SRK_TRI_MAX_REFINE_ATTEMPTS_HOST);
        if (!(opts->refine_rel_change >= 0.0) || !std::isfinite(opts->refine_rel_change)) return "triangulate: refine_rel_change must be finite and not negative";
        if (!(opts->min_parallax_deg >= 0.0) || !std::isfinite(opts->min_parallax_deg)) return "triangulate: min_parallax_deg must be finite and not negative";
    }
    if (row_ptr[0] != 0) return "triangulate: row_ptr[0] != 0";
    for (int64_t i = 0; i < n_tracks; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) return "triangulate: row_ptr decreases at track " + std::to_string(i);
    const int64_t O = row_ptr[n_tracks];
    if (O > 0 && (!frame || !uv)) return "triangulate: a NULL observation array";
    for (int64_t o = 0; o < O; ++o) {
        if (frame[o] < 0 || frame[o] >= n_frames) return "triangulate: the frame of observation " + std::to_string(o) + " is out of range";
        if (!std::isfinite(uv[2 * o]) || !std::isfinite(uv[2 * o + 1])) return "triangulate: uv of observation " + std::to_string(o) + " is not finite";
        if (q && (!(q[o] >= 0.0) || !std::isfinite(q[o]))) return "triangulate: q of observation " + std::to_string(o) + " must be finite and not negative";
    }
    return std::string();
}

void srk_tri_map_frames(int64_t n_obs, const int32_t* frame, const int32_t* frame_int, std::vector<int32_t>& out)
{
    out.resize((size_t)n_obs);
    for (int64_t o = 0; o < n_obs; ++o) out[(size_t)o] = frame_int ? frame_int[frame[o]] : frame[o];
}

void srk_tri_host_pack(int32_t n_frames, const double* cam_R, const double* cam_T, const double* K, int shared_k, std::vector<double>& pack)
{
    pack.resize((size_t)SRK_TRI_PACK * (size_t)n_frames);
    for (int32_t j = 0; j < n_frames; ++j)
        srk_tri_pack_frame(cam_R + 9 * (int64_t)j, cam_T + 3 * (int64_t)j, shared_k ? K : K + 9 * (int64_t)j, &pack[(size_t)SRK_TRI_PACK * (size_t)j]);
}

namespace {
// the sums of a track at X: every lane over its observations, then the tree ((0 1)(2 3))((4 5)(6 7))
SrkTriSums host_eval(const std::vector<int64_t> (&mine)[SRK_TRI_GROUP], const int32_t* frame, const double* uv, const double* q, const double* pack,
                     double f0, const double X[3], const double* ray0)
{
    SrkTriSums s[SRK_TRI_GROUP];
    for (int l = 0; l < SRK_TRI_GROUP; ++l) {
        srk_tri_sums_zero(s[l]);
        for (int64_t o : mine[l]) {
            const double* p = pack + (int64_t)SRK_TRI_PACK * frame[o];
            srk_tri_eval_obs(s[l], p, uv[2 * o], uv[2 * o + 1], f0, q ? q[o] : 1.0, X);
            if (ray0) {
                double ray[3];
                srk_tri_ray(p, uv[2 * o], uv[2 * o + 1], f0, ray);
                s[l].max_angle = std::fmax(s[l].max_angle, srk_tri_angle(ray0, ray));
            }
        }
    }
    for (int d = 1; d < SRK_TRI_GROUP; d <<= 1)
        for (int l = 0; l + d < SRK_TRI_GROUP; l += 2 * d) srk_tri_sums_add(s[l], s[l + d]);
    return s[0];
}
} // namespace

uint32_t srk_tri_host_track(int64_t n_obs, const int32_t* frame, const double* uv, const double* q, const double* pack, double f0,
                            const srk_tri_options& opts, double X[3], double quality[4])
{
    std::vector<int64_t> mine[SRK_TRI_GROUP];
    int64_t nw = 0;
    for (int64_t o = 0; o < n_obs; ++o)
        if (!q || q[o] > 0.0) mine[nw++ % SRK_TRI_GROUP].push_back(o);
    if (nw < 2) {
        X[0] = X[1] = X[2] = quality[0] = quality[2] = NAN;
        quality[1] = 0.0;
        quality[3] = (double)nw;
        return SRK_TRI_FEW_VIEWS;
    }
    SrkTriFactor f[SRK_TRI_GROUP];
    for (int l = 0; l < SRK_TRI_GROUP; ++l) {
        srk_tri_factor_zero(f[l]);
        for (int64_t o : mine[l]) srk_tri_fold_obs(f[l], pack + (int64_t)SRK_TRI_PACK * frame[o], uv[2 * o], uv[2 * o + 1], f0, q ? std::sqrt(q[o]) : 1.0);
    }
    for (int d = 1; d < SRK_TRI_GROUP; d <<= 1)
        for (int l = 0; l + d < SRK_TRI_GROUP; l += 2 * d) srk_tri_merge(f[l], f[l + d]);
    double ray0[3];
    {
        const int64_t o = mine[0][0];
        srk_tri_ray(pack + (int64_t)SRK_TRI_PACK * frame[o], uv[2 * o], uv[2 * o + 1], f0, ray0);
    }
    const int solved = srk_tri_solve(f[0], X);
    SrkTriSums cur = host_eval(mine, frame, uv, q, pack, f0, X, ray0);
    int hit_cap = 0;
    if (opts.refine_attempts > 0 && solved) {
        double c = 1e-4;
        hit_cap = 1;
        for (int32_t a = 0; a < opts.refine_attempts; ++a) {
            double d[3] = { 0, 0, 0 }, Xn[3];
            const int stepped = srk_tri_lm_step(cur, c, d);
            for (int e = 0; e < 3; ++e) Xn[e] = X[e] + d[e];
            SrkTriSums cand;
            srk_tri_sums_zero(cand);
            if (stepped) cand = host_eval(mine, frame, uv, q, pack, f0, Xn, nullptr);
            if (srk_tri_lm_judge(cur, cand, stepped, X, Xn, c, opts.refine_rel_change)) {
                hit_cap = 0;
                break;
            }
        }
    }
    return srk_tri_finish(f[0], cur, solved, nw, opts.min_parallax_deg, hit_cap, quality);
}

extern "C" {

void srk_tri_default_options(srk_tri_options* o)
{
    if (!o) return;
    o->refine_attempts = 10;
    o->refine_rel_change = 1e-9;
    o->min_parallax_deg = 0.0;
}

int srk_tri_check_tracks(int64_t n_tracks, const int64_t* row_ptr, const int32_t* frame, const double* uv, const double* q, int32_t n_frames,
                         const srk_tri_options* opts, const char** why)
{
    static thread_local std::string text;
    text = srk_tri_check(n_tracks, row_ptr, frame, uv, q, n_frames, opts);
    if (why) *why = text.c_str();
    return text.empty() ? SRK_OK : SRK_E_ARGS;
}

int srk_tri_revert_points(const srk_ba_normalizer* nrm, int64_t n, double* X)
{
    if (!nrm || n < 0 || (n > 0 && !X)) return SRK_E_ARGS;
    const double is = 1.0 / nrm->world_scale;
    for (int64_t i = 0; i < n; ++i) { // the point map of srk_ba_revert_normalization
        const double t[3] = { X[3 * i] * is - nrm->T0[0], X[3 * i + 1] * is - nrm->T0[1], X[3 * i + 2] * is - nrm->T0[2] };
        for (int a = 0; a < 3; ++a) X[3 * i + a] = nrm->R0[a] * t[0] + nrm->R0[3 + a] * t[1] + nrm->R0[6 + a] * t[2];
    }
    return SRK_OK;
}

} // extern "C"
