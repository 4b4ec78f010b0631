// srk_factors.cpp -- the host arithmetic of the factor settings (srk_factors.hpp).  No HIP header: built with the host compiler
// alone by tests/cpp/test_factor_tables.cpp, and shared by both libraries as srk_plan.o is.
#include "srk_factors.hpp"
#include "srk_geom.hpp"

#include <algorithm>
#include <cmath>
#include <map>
#include <set>
#include <utility>

void srk_symmetrise(double* L, int64_t n)
{
    for (int64_t r = 0; r < n; ++r)
        for (int64_t c = r + 1; c < n; ++c) L[r * n + c] = L[c * n + r] = 0.5 * (L[r * n + c] + L[c * n + r]);
}
const double* SrkJPriorSetting::info_of(size_t g) const
{
    int64_t at = 0;
    for (size_t q = 0; q < g; ++q) {
        const int64_t k = ptr[q + 1] - ptr[q];
        at += 36 * k * k;
    }
    return info.data() + at;
}

// ------------------------------------------------------------------ checks

std::string srk_setting_conflict(const char* family, bool set, bool groups, int world)
{
    if (!set) return {};
    if (groups) return std::string(family) + ": not available with intrinsic groups";
    if (world > 1) return std::string(family) + ": not available with more than one rank";
    return {};
}

bool srk_info_psd(double* A, int64_t n)
{
    double m = 0;
    for (int64_t e = 0; e < n * n; ++e) m = std::max(m, std::fabs(A[e]));
    if (m == 0) return true;
    for (int64_t k = 0; k < n; ++k) {
        int64_t p = k;
        for (int64_t i = k + 1; i < n; ++i)
            if (A[(n + 1) * i] > A[(n + 1) * p]) p = i;
        if (A[(n + 1) * p] <= 1e-12 * m) {
            for (int64_t i = k; i < n; ++i)
                for (int64_t j = k; j < n; ++j)
                    if (i == j ? A[(n + 1) * i] < -1e-12 * m : std::fabs(A[n * i + j]) > 1e-11 * m) return false;
            return true;
        }
        for (int64_t j = 0; j < n; ++j) std::swap(A[n * k + j], A[n * p + j]);
        for (int64_t i = 0; i < n; ++i) std::swap(A[n * i + k], A[n * i + p]);
        for (int64_t i = k + 1; i < n; ++i) {
            const double f = A[n * i + k] / A[(n + 1) * k];
            for (int64_t j = k + 1; j < n; ++j) A[n * i + j] -= f * A[n * k + j];
        }
    }
    return true;
}

// a finite 3 x 3 matrix z as a rotation: orthogonal to 1e-9 and of determinant 1.  0 = it is, 1 / 2 = which it is not.
static int rotation_defect(const double* z)
{
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double g = z[a] * z[b] + z[3 + a] * z[3 + b] + z[6 + a] * z[6 + b] - (a == b ? 1.0 : 0.0);
            if (std::fabs(g) > 1e-9) return 1;
        }
    const double det = z[0] * (z[4] * z[8] - z[5] * z[7]) - z[1] * (z[3] * z[8] - z[5] * z[6]) + z[2] * (z[3] * z[7] - z[4] * z[6]);
    return std::fabs(det - 1.0) > 1e-9 ? 2 : 0;
}
// ... as a static text that starts with the prefix (a string literal: the callers hand these texts out through the C ABI)
#define SRK_CHECK_ROTATION(prefix, z)                                                          \
    if (const int defect_ = rotation_defect(z))                                                \
        return defect_ == 1 ? prefix " is not orthogonal to 1e-9" : prefix " has determinant != 1"

const char* srk_check_prior_values(int64_t n, const double* pos, const double* info)
{
    for (int64_t i = 0; i < n; ++i) {
        for (int e = 0; e < 3; ++e)
            if (!std::isfinite(pos[3 * i + e])) return "position priors: a position is not finite";
        const double* l = info + 6 * i;
        double m = 0;
        for (int e = 0; e < 6; ++e) {
            if (!std::isfinite(l[e])) return "position priors: an information matrix is not finite";
            m = std::max(m, std::fabs(l[e]));
        }
        // positive semi-definite: every principal minor >= 0 (up to the rounding of a rank-deficient matrix)
        const double xx = l[0], xy = l[1], xz = l[2], yy = l[3], yz = l[4], zz = l[5];
        const double t2 = 1e-12 * m * m, t3 = 1e-12 * m * m * m;
        const double det = xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz) + xz * (xy * yz - yy * xz);
        if (xx < 0 || yy < 0 || zz < 0 || xx * yy - xy * xy < -t2 || xx * zz - xz * xz < -t2 || yy * zz - yz * yz < -t2 || det < -t3)
            return "position priors: an information matrix is not positive semi-definite";
    }
    return nullptr;
}

const char* srk_check_relpose(int32_t n, const int32_t* fa, const int32_t* fb, const double* R, const double* t, const double* info)
{
    for (int32_t i = 0; i < n; ++i) {
        if (fa[i] < 0 || fb[i] < 0) return "relative-pose factors: negative frame index";
        if (fa[i] == fb[i]) return "relative-pose factors: a factor needs two different frames";
        if (i > 0) {
            const int32_t lo0 = std::min(fa[i - 1], fb[i - 1]), hi0 = std::max(fa[i - 1], fb[i - 1]);
            const int32_t lo1 = std::min(fa[i], fb[i]), hi1 = std::max(fa[i], fb[i]);
            if (lo0 == lo1 && hi0 == hi1) return "relative-pose factors: a pair of frames is given twice";
            if (lo1 < lo0 || (lo1 == lo0 && hi1 < hi0)) return "relative-pose factors: pairs must be sorted by (min, max) of their frames";
        }
        const double* z = R + 9 * (int64_t)i;
        for (int e = 0; e < 9; ++e)
            if (!std::isfinite(z[e])) return "relative-pose factors: a rotation is not finite";
        for (int e = 0; e < 3; ++e)
            if (!std::isfinite(t[3 * (int64_t)i + e])) return "relative-pose factors: a translation is not finite";
        SRK_CHECK_ROTATION("relative-pose factors: a measured rotation", z);
        double A[36];
        int k = 0;
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c, ++k) {
                const double v = info[21 * (int64_t)i + k];
                if (!std::isfinite(v)) return "relative-pose factors: an information matrix is not finite";
                A[6 * r + c] = A[6 * c + r] = v;
            }
        if (!srk_info_psd(A, 6)) return "relative-pose factors: an information matrix is not positive semi-definite";
    }
    return nullptr;
}

const char* srk_check_jprior(int32_t n_sets, const int32_t* set_ptr, const int32_t* frame, const double* lin_R, const double* lin_C,
                             const double* mean, const double* info, int keep_gauge)
{
    if (keep_gauge != 0 && keep_gauge != 1) return "joint pose priors: keep_gauge must be 0 or 1";
    if (set_ptr[0] != 0) return "joint pose priors: set_ptr must start at 0";
    int64_t at = 0;
    std::map<int32_t, std::vector<int32_t>> sets_of; // frame -> the sets that hold it
    for (int32_t g = 0; g < n_sets; ++g) {
        const int64_t k = (int64_t)set_ptr[g + 1] - set_ptr[g], n = 6 * k;
        if (k < 1 || k > SRK_JP_MAX_FRAMES_HOST) return "joint pose priors: a set holds 1 to 16 frames";
        for (int64_t i = 0; i < k; ++i) {
            const int64_t q = set_ptr[g] + i;
            if (frame[q] < 0) return "joint pose priors: negative frame index";
            if (i > 0 && frame[q - 1] >= frame[q]) return "joint pose priors: the frames of a set must be strictly ascending";
            const double* z = lin_R + 9 * q;
            for (int e = 0; e < 9; ++e)
                if (!std::isfinite(z[e])) return "joint pose priors: a linearisation rotation is not finite";
            for (int e = 0; e < 3; ++e)
                if (!std::isfinite(lin_C[3 * q + e])) return "joint pose priors: a linearisation centre is not finite";
            for (int e = 0; mean && e < 6; ++e)
                if (!std::isfinite(mean[6 * q + e])) return "joint pose priors: a mean is not finite";
            SRK_CHECK_ROTATION("joint pose priors: a linearisation rotation", z);
            // two sets may share one frame: every coupling block of the system then has one owner among the sets
            std::vector<int32_t>& in = sets_of[frame[q]];
            for (int32_t other : in)
                for (int64_t i2 = 0; i2 < i; ++i2) {
                    const std::vector<int32_t>& in2 = sets_of[frame[set_ptr[g] + i2]];
                    if (std::find(in2.begin(), in2.end(), other) != in2.end()) return "joint pose priors: two sets share more than one frame";
                }
            in.push_back(g);
        }
        const double* L = info + at;
        double m = 0;
        for (int64_t e = 0; e < n * n; ++e) {
            if (!std::isfinite(L[e])) return "joint pose priors: an information matrix is not finite";
            m = std::max(m, std::fabs(L[e]));
        }
        std::vector<double> A((size_t)(n * n));
        for (int64_t r = 0; r < n; ++r)
            for (int64_t c = 0; c < n; ++c) {
                if (std::fabs(L[r * n + c] - L[c * n + r]) > 1e-12 * m) return "joint pose priors: an information matrix is not symmetric to 1e-12 of its largest entry";
                A[(size_t)(r * n + c)] = 0.5 * (L[r * n + c] + L[c * n + r]);
            }
        if (!srk_info_psd(A.data(), n)) return "joint pose priors: an information matrix is not positive semi-definite";
        at += n * n;
    }
    return nullptr;
}

// ------------------------------------------------------------------ the settings through a normaliser

extern "C" {

// position priors through a normaliser: pos_n = s (R0 pos + T0), L_n = R0 L R0^T / s^2, so that
// (x_n - pos_n)^T L_n (x_n - pos_n) = (x - pos)^T L (x - pos) for x_n = s (R0 x + T0)
int srk_ba_normalize_position_priors(const srk_ba_normalizer* nrm, int64_t n, const double* pos, const double* info,
                                     double* pos_out, double* info_out)
{
    if (!nrm || n < 0 || (pos != nullptr) != (pos_out != nullptr) || (info != nullptr) != (info_out != nullptr)) return SRK_E_ARGS;
    const double s = nrm->world_scale, is2 = 1.0 / (s * s);
    const double* R = nrm->R0;
    for (int64_t i = 0; pos && i < n; ++i) {
        double y[3];
        srk::se3_apply(nrm->R0, nrm->T0, pos + 3 * i, y);
        for (int e = 0; e < 3; ++e) pos_out[3 * i + e] = y[e] * s;
    }
    for (int64_t i = 0; info && i < n; ++i) {
        const double* l = info + 6 * i;
        const double L[9] = { l[0], l[1], l[2], l[1], l[3], l[4], l[2], l[4], l[5] };
        double RL[9], o[9];
        srk::mat3_mul(R, L, RL);
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) o[3 * a + b] = (RL[3 * a] * R[3 * b] + RL[3 * a + 1] * R[3 * b + 1] + RL[3 * a + 2] * R[3 * b + 2]) * is2;
        double* q = info_out + 6 * i; // the symmetric part: both triangles carry the same sum up to rounding
        q[0] = o[0]; q[1] = 0.5 * (o[1] + o[3]); q[2] = 0.5 * (o[2] + o[6]);
        q[3] = o[4]; q[4] = 0.5 * (o[5] + o[7]); q[5] = o[8];
    }
    return SRK_OK;
}

// relative-pose factors through a normaliser.  A relative pose is invariant under R0 and T0 and scales with s:
// z_n = s z, L_tt / s^2, L_tr / s, L_rr as it is, so that [e_t; e_r]^T L [e_t; e_r] is the same number in both worlds
int srk_ba_normalize_relative_pose_factors(const srk_ba_normalizer* nrm, int32_t n, const double* rel_t, const double* info,
                                           double* rel_t_out, double* info_out)
{
    if (!nrm || n < 0 || (rel_t != nullptr) != (rel_t_out != nullptr) || (info != nullptr) != (info_out != nullptr)) return SRK_E_ARGS;
    const double s = nrm->world_scale, is = 1.0 / s;
    for (int64_t i = 0; rel_t && i < 3 * (int64_t)n; ++i) rel_t_out[i] = s * rel_t[i];
    for (int64_t i = 0; info && i < n; ++i) {
        int k = 0;
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c, ++k) info_out[21 * i + k] = info[21 * i + k] * (r < 3 ? is : 1.0) * (c < 3 ? is : 1.0);
    }
    return SRK_OK;
}

// joint pose priors through a normaliser.  With X_n = s (R0 X + T0): Cbar_n = s (R0 Cbar + T0), Rbar_n = Rbar R0^T,
// and the residual of a frame maps as r_n = D r, D = diag(s R0, R0), so m_n = D m and L_n = D^-T L D^-1 keep the energy: block
// (i, j) of L_n is G L_ij G^T with G = diag(R0 / s, R0).  The inverse of the map srk_ba_revert_covariances applies.
int srk_ba_normalize_joint_pose_priors(const srk_ba_normalizer* nrm, int32_t n_sets, const int32_t* set_ptr, const double* lin_R,
                                       const double* lin_C, const double* mean, const double* info, double* lin_R_out,
                                       double* lin_C_out, double* mean_out, double* info_out)
{
    if (!nrm || n_sets < 0 || (n_sets > 0 && !set_ptr) || (lin_R != nullptr) != (lin_R_out != nullptr) ||
        (lin_C != nullptr) != (lin_C_out != nullptr) || (mean != nullptr) != (mean_out != nullptr) || (info != nullptr) != (info_out != nullptr))
        return SRK_E_ARGS;
    for (int32_t g = 0; g < n_sets; ++g)
        if (set_ptr[g + 1] < set_ptr[g] || set_ptr[0] != 0) return SRK_E_ARGS;
    const double s = nrm->world_scale, is = 1.0 / s;
    const double* R0 = nrm->R0;
    const int64_t nq = n_sets > 0 ? set_ptr[n_sets] : 0;
    double R0t[9];
    srk::mat3_tr(R0, R0t);
    for (int64_t q = 0; q < nq; ++q) {
        if (lin_R) srk::mat3_mul(lin_R + 9 * q, R0t, lin_R_out + 9 * q);
        if (lin_C) {
            double y[3];
            srk::se3_apply(R0, nrm->T0, lin_C + 3 * q, y);
            for (int e = 0; e < 3; ++e) lin_C_out[3 * q + e] = s * y[e];
        }
        if (mean) {
            double y[3];
            srk::mat3_vec(R0, mean + 6 * q, y);
            for (int e = 0; e < 3; ++e) mean_out[6 * q + e] = s * y[e];
            srk::mat3_vec(R0, mean + 6 * q + 3, mean_out + 6 * q + 3);
        }
    }
    int64_t at = 0;
    for (int32_t g = 0; info && g < n_sets; ++g) {
        const int64_t k = set_ptr[g + 1] - set_ptr[g], n = 6 * k;
        const double* L = info + at;
        double* o = info_out + at;
        for (int64_t bi = 0; bi < 2 * k; ++bi)     // 3 x 3 blocks: even = translation, odd = rotation
            for (int64_t bj = 0; bj < 2 * k; ++bj) {
                double B[9], RB[9], RBR[9];
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) B[3 * a + b] = L[(3 * bi + a) * n + 3 * bj + b];
                srk::mat3_mul(R0, B, RB);
                srk::mat3_mul(RB, R0t, RBR);
                const double f = ((bi & 1) ? 1.0 : is) * ((bj & 1) ? 1.0 : is);
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) o[(3 * bi + a) * n + 3 * bj + b] = f * RBR[3 * a + b];
            }
        srk_symmetrise(o, n); // both triangles carry the same sum up to rounding
        at += n * n;
    }
    return SRK_OK;
}

} // extern "C"

// ------------------------------------------------------------------ selection before the plan

static bool all_zero(const double* v, int64_t n)
{
    bool off = true;
    for (int64_t e = 0; e < n; ++e) off = off && v[e] == 0.0;
    return off;
}
// whether the 6 x 6 block (slot i, slot j) of a set's information matrix (n = 6 k rows) has a non-zero entry
static bool jp_block_nonzero(const double* L, int64_t n, int32_t i, int32_t j)
{
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c)
            if (L[(6 * i + r) * n + 6 * j + c] != 0.0) return true;
    return false;
}

std::string srk_select_factors(const SrkConstSetting& cst, const SrkPriorSetting& pri, const SrkRelPoseSetting& rp, const SrkJPriorSetting& jp,
                               int64_t N, int32_t M, SrkFactorSelection& sel)
{
    using std::to_string;
    sel = SrkFactorSelection{};
    if (cst.set) {
        if (!cst.frames.empty() && (int64_t)cst.frames.size() != (int64_t)M)
            return "constant blocks: set for " + to_string(cst.frames.size()) + " frames, the scene has " + to_string(M);
        if (!cst.points.empty() && (int64_t)cst.points.size() != N)
            return "constant blocks: set for " + to_string(cst.points.size()) + " landmarks, the scene has " + to_string(N);
    }
    if (pri.set) {
        if (!pri.pt_idx.empty() && pri.pt_idx.back() >= N)
            return "position priors: landmark index " + to_string(pri.pt_idx.back()) + ", the scene has " + to_string(N) + " landmarks";
        if (!pri.fr_idx.empty() && pri.fr_idx.back() >= M)
            return "position priors: frame index " + to_string(pri.fr_idx.back()) + ", the scene has " + to_string(M) + " frames";
    }
    for (size_t k = 0; rp.set && k < rp.a.size(); ++k) {
        if (rp.a[k] >= M || rp.b[k] >= M)
            return "relative-pose factors: frame index " + to_string(std::max(rp.a[k], rp.b[k])) + ", the scene has " + to_string(M) + " frames";
        if (all_zero(&rp.info[21 * k], 21)) continue;
        sel.rp_act.push_back((int32_t)k);
        sel.rel_a.push_back(rp.a[k]);
        sel.rel_b.push_back(rp.b[k]);
    }
    if (jp.set) {
        sel.jp_pptr.push_back(0);
        std::set<std::pair<int32_t, int32_t>> seen;
        for (size_t k = 0; k < sel.rel_a.size(); ++k) seen.insert({ std::min(sel.rel_a[k], sel.rel_b[k]), std::max(sel.rel_a[k], sel.rel_b[k]) });
        for (size_t g = 0; g + 1 < jp.ptr.size(); ++g) {
            const int32_t q0 = jp.ptr[g], k = jp.ptr[g + 1] - q0;
            const int32_t* fr = &jp.frame[(size_t)q0];
            if (fr[k - 1] >= M) return "joint pose priors: frame index " + to_string(fr[k - 1]) + ", the scene has " + to_string(M) + " frames";
            const double* L = jp.info_of(g);
            if (all_zero(L, 36 * (int64_t)k * k)) continue;
            sel.jp_act.push_back((int32_t)g);
            for (int32_t i = 1; i < k; ++i)
                for (int32_t j = 0; j < i; ++j)
                    if (jp_block_nonzero(L, 6 * k, i, j)) {
                        sel.jp_pslot.push_back((i << 8) | j);
                        if (seen.insert({ fr[j], fr[i] }).second) {
                            sel.rel_a.push_back(fr[j]);
                            sel.rel_b.push_back(fr[i]);
                        }
                    }
            sel.jp_pptr.push_back((int32_t)sel.jp_pslot.size());
        }
    }
    return {};
}

// ------------------------------------------------------------------ table builders

static int32_t internal_frame(const SrkPlanKept& plan, int32_t j) { return plan.frame_int.empty() ? j : plan.frame_int[(size_t)j]; }
// the place in S of entry (0, 0) of the block that couples the pose variables of two frames: row = first pose variable of the
// frame with the larger internal index, column = that of the other
static int64_t couple_target(const SrkFactorDims& d, int32_t f1, int32_t f2)
{
    const int64_t t0 = 4 - (10 - d.fv); // first pose variable of a frame
    const int64_t hi = std::max(f1, f2), lo = std::min(f1, f2);
    return (d.fv * hi + t0) * d.ld + d.fv * lo + t0;
}
// entries that each sit on one internal frame -> the frames with entries (ascending), and per frame its entries in entry order
static void frame_incidence(int32_t M, const std::vector<int32_t>& frame_of, std::vector<int32_t>& list, std::vector<int32_t>& ptr,
                            std::vector<int32_t>& ent)
{
    std::vector<int32_t> cnt((size_t)M, 0), at((size_t)M, -1);
    for (int32_t f : frame_of) ++cnt[(size_t)f];
    list.clear();
    ptr.assign(1, 0);
    for (int32_t j = 0; j < M; ++j)
        if (cnt[(size_t)j]) {
            at[(size_t)j] = (int32_t)list.size();
            list.push_back(j);
            ptr.push_back(ptr.back() + cnt[(size_t)j]);
        }
    ent.resize(frame_of.size());
    std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
    for (size_t e = 0; e < frame_of.size(); ++e) ent[(size_t)fill[(size_t)at[(size_t)frame_of[e]]]++] = (int32_t)e;
}

std::vector<int64_t> srk_observation_places(const SrkPlanKept& plan, int64_t N, int64_t O)
{
    std::vector<int64_t> at((size_t)O);
    for (int64_t i = 0; i < N; ++i) { // landmark perm, observation rank inside the landmark
        const int64_t oi = plan.row_ptr_int[(size_t)i], ou = plan.row_ptr_user[(size_t)plan.perm[(size_t)i]];
        const int64_t cnt = plan.row_ptr_int[(size_t)i + 1] - oi;
        for (int64_t a = 0; a < cnt; ++a) at[(size_t)(ou + a)] = oi + (plan.obs_rank.empty() ? a : plan.obs_rank[(size_t)(ou + a)]);
    }
    return at;
}

// in the internal order, and the frame-major copy beside it
SrkInfoTables srk_build_information(const SrkInfoSetting& s, const SrkPlanKept& plan, const SrkFactorDims& d)
{
    SrkInfoTables t;
    if (s.q.empty() || d.O == 0) return t;
    t.q.resize((size_t)d.O);
    t.qf.resize(plan.fobs_of.size());
    const std::vector<int64_t> at = srk_observation_places(plan, d.N, d.O);
    for (int64_t o = 0; o < d.O; ++o) t.q[(size_t)at[(size_t)o]] = s.q[(size_t)o];
    for (size_t o = 0; o < t.qf.size(); ++o) t.qf[(size_t)plan.fobs_of[o]] = t.q[o];
    t.on = true;
    return t;
}

SrkConstTables srk_build_constant(const SrkConstSetting& s, const SrkPlanKept& plan, const SrkFactorDims& d)
{
    SrkConstTables t;
    if (!s.set) return t;
    if (!s.points.empty())
        for (int64_t i = 0; i < d.N; ++i)
            if (s.points[(size_t)plan.perm[(size_t)i]]) t.pts.push_back((int32_t)i);
    if (!s.frames.empty()) {
        t.frame_int.assign((size_t)d.M, 0);
        for (int32_t j = 0; j < d.M; ++j)
            if (s.frames[(size_t)j]) t.frame_int[(size_t)internal_frame(plan, j)] = 1;
        for (int32_t j = 0; j < d.M; ++j)
            if (t.frame_int[(size_t)j]) t.frames.push_back(j);
    }
    return t;
}

// one kind of position prior: the entries of the setting by ascending internal index (to_setting[internal index] = place in the
// setting, -1 = none), switched-off ones left out (an all-zero information matrix: the sums, and their bits, are those of the
// setting without it); the values as SoA planes over the list (SrkPrior)
static void prior_list(const std::vector<int64_t>& to_setting, const std::vector<double>& info_user, const std::vector<double>& pos,
                       const std::vector<double>& info, std::vector<int32_t>& list, std::vector<double>& val)
{
    std::vector<size_t> at;
    for (size_t i = 0; i < to_setting.size(); ++i) {
        const int64_t k = to_setting[i];
        if (k < 0 || all_zero(&info_user[6 * (size_t)k], 6)) continue;
        list.push_back((int32_t)i);
        at.push_back((size_t)k);
    }
    const size_t n = at.size();
    val.resize(9 * n);
    for (size_t i = 0; i < n; ++i) {
        for (int e = 0; e < 3; ++e) val[(size_t)e * n + i] = pos[3 * at[i] + (size_t)e];
        for (int e = 0; e < 6; ++e) val[(size_t)(3 + e) * n + i] = info[6 * at[i] + (size_t)e];
    }
}
SrkPriorTables srk_build_priors(const SrkPriorSetting& s, const srk_ba_normalizer& nrm, const SrkPlanKept& plan, const SrkFactorDims& d)
{
    SrkPriorTables t;
    if (!s.set) return t;
    const size_t np = s.pt_idx.size(), nf = s.fr_idx.size();
    std::vector<double> pn(3 * np), ln(6 * np), cn(3 * nf), fn(6 * nf);
    if (np) srk_ba_normalize_position_priors(&nrm, (int64_t)np, s.pt_pos.data(), s.pt_info.data(), pn.data(), ln.data());
    if (nf) srk_ba_normalize_position_priors(&nrm, (int64_t)nf, s.fr_pos.data(), s.fr_info.data(), cn.data(), fn.data());
    if (np) {
        std::vector<int64_t> user((size_t)d.N, -1), slot((size_t)d.N); // caller's landmark -> its place in the setting; internal -> the same
        for (size_t k = 0; k < np; ++k) user[(size_t)s.pt_idx[k]] = (int64_t)k;
        for (int64_t i = 0; i < d.N; ++i) slot[(size_t)i] = user[(size_t)plan.perm[(size_t)i]];
        prior_list(slot, s.pt_info, pn, ln, t.pt_list, t.pt_val);
    }
    if (nf) {
        std::vector<int64_t> slot((size_t)d.M, -1); // internal frame -> its place in the setting
        for (size_t k = 0; k < nf; ++k) slot[(size_t)internal_frame(plan, s.fr_idx[k])] = (int64_t)k;
        prior_list(slot, s.fr_info, cn, fn, t.fr_list, t.fr_val);
    }
    return t;
}

SrkRelPoseTables srk_build_relpose(const SrkRelPoseSetting& s, const SrkFactorSelection& sel, const srk_ba_normalizer& nrm,
                                   const SrkPlanKept& plan, const SrkFactorDims& d)
{
    SrkRelPoseTables t;
    const size_t n = sel.rp_act.size();
    if (n == 0) return t;
    std::vector<double> tn(s.t.size()), ln(s.info.size());
    srk_ba_normalize_relative_pose_factors(&nrm, (int32_t)s.a.size(), s.t.data(), s.info.data(), tn.data(), ln.data());
    t.fa.resize(n); t.fb.resize(n); t.tgt.resize(n);
    t.val.resize((size_t)SRK_RP_PLANES_HOST * n);
    std::vector<int32_t> ends(2 * n); // entry 2 * factor + side, as fr_ent names it
    for (size_t i = 0; i < n; ++i) {
        const size_t k = (size_t)sel.rp_act[i];
        ends[2 * i] = t.fa[i] = internal_frame(plan, s.a[k]);
        ends[2 * i + 1] = t.fb[i] = internal_frame(plan, s.b[k]);
        for (int e = 0; e < 9; ++e) t.val[(size_t)e * n + i] = s.R[9 * k + (size_t)e];
        for (int e = 0; e < 3; ++e) t.val[(size_t)(9 + e) * n + i] = tn[3 * k + (size_t)e];
        for (int e = 0; e < 21; ++e) t.val[(size_t)(12 + e) * n + i] = ln[21 * k + (size_t)e];
        t.tgt[i] = couple_target(d, t.fa[i], t.fb[i]);
    }
    frame_incidence(d.M, ends, t.fr_list, t.fr_ptr, t.fr_ent); // factor order inside every frame's list
    return t;
}

SrkJPriorTables srk_build_jprior(const SrkJPriorSetting& s, const SrkFactorSelection& sel, const srk_ba_normalizer& nrm,
                                 const SrkPlanKept& plan, const SrkFactorDims& d)
{
    SrkJPriorTables t;
    const size_t ns = sel.jp_act.size();
    if (ns == 0) return t;
    std::vector<double> Rn(s.R.size()), Cn(s.C.size()), mn(s.mean.size()), Ln(s.info.size());
    srk_ba_normalize_joint_pose_priors(&nrm, (int32_t)s.ptr.size() - 1, s.ptr.data(), s.R.data(), s.C.data(), s.mean.data(), s.info.data(),
                                       Rn.data(), Cn.data(), mn.data(), Ln.data());
    t.ptr.assign(1, 0);
    t.pptr.assign(1, 0);
    for (size_t a = 0; a < ns; ++a) {
        const size_t g = (size_t)sel.jp_act[a];
        const int32_t q0 = s.ptr[g], k = s.ptr[g + 1] - q0;
        const int64_t n = 6 * (int64_t)k;
        const double* L = Ln.data() + (s.info_of(g) - s.info.data());
        t.iptr.push_back((int64_t)t.info.size());
        t.info.insert(t.info.end(), L, L + n * n);
        for (int32_t i = 0; i < k; ++i) {
            const size_t q = (size_t)(q0 + i);
            t.frame.push_back(internal_frame(plan, s.frame[q]));
            t.lin.insert(t.lin.end(), &Rn[9 * q], &Rn[9 * q] + 9);
            t.lin.insert(t.lin.end(), &Cn[3 * q], &Cn[3 * q] + 3);
            t.mean.insert(t.mean.end(), &mn[6 * q], &mn[6 * q] + 6);
        }
        const int32_t* fr = t.frame.data() + t.ptr.back();
        for (int32_t p = sel.jp_pptr[a]; p < sel.jp_pptr[a + 1]; ++p) {
            const int32_t ps = sel.jp_pslot[(size_t)p], i = ps >> 8, j = ps & 255;
            t.pslot.push_back(ps);
            t.tgt.push_back(couple_target(d, fr[i], fr[j]));
            t.pair_a.push_back(std::min(fr[i], fr[j]));
            t.pair_b.push_back(std::max(fr[i], fr[j]));
        }
        t.ptr.push_back(t.ptr.back() + k);
        t.pptr.push_back((int32_t)t.pslot.size());
    }
    frame_incidence(d.M, t.frame, t.fr_list, t.fr_ptr, t.fr_ent); // set order inside every frame's list
    return t;
}

// ------------------------------------------------------------------ residuals in the caller's units

// the centre C = -R^T T of frame j
static void centre(const double* R, const double* T, int32_t j, double* C)
{
    const double* r = R + 9 * (size_t)j;
    const double* t = T + 3 * (size_t)j;
    for (int e = 0; e < 3; ++e) C[e] = -(r[e] * t[0] + r[3 + e] * t[1] + r[6 + e] * t[2]);
}
// Log of a rotation matrix as the kernels take it (rp_log of k_relpose_error, k_jprior_error): must stay in step with theirs,
// the path near pi (cosine below -0.9: the axis from the symmetric part) included
static void so3_log(const double* M, double* w)
{
    const double v[3] = { 0.5 * (M[7] - M[5]), 0.5 * (M[2] - M[6]), 0.5 * (M[3] - M[1]) };
    const double s2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], sn = std::sqrt(s2), cs = 0.5 * (M[0] + M[4] + M[8] - 1.0);
    if (cs < -0.9) {
        double a[3];
        if (M[0] >= M[4] && M[0] >= M[8]) { a[0] = M[0] - cs; a[1] = 0.5 * (M[3] + M[1]); a[2] = 0.5 * (M[6] + M[2]); }
        else if (M[4] >= M[8]) { a[0] = 0.5 * (M[1] + M[3]); a[1] = M[4] - cs; a[2] = 0.5 * (M[7] + M[5]); }
        else { a[0] = 0.5 * (M[2] + M[6]); a[1] = 0.5 * (M[5] + M[7]); a[2] = M[8] - cs; }
        const double t = std::atan2(sn, cs);
        const double f = (a[0] * v[0] + a[1] * v[1] + a[2] * v[2] < 0 ? -t : t) / std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        for (int c = 0; c < 3; ++c) w[c] = f * a[c];
        return;
    }
    const double f = (sn < 1e-4 && cs > 0) ? 1.0 + s2 / 6.0 + 3.0 * s2 * s2 / 40.0 : std::atan2(sn, cs) / sn;
    for (int c = 0; c < 3; ++c) w[c] = f * v[c];
}

void srk_prior_residuals(const SrkPriorApplied& s, const double* pts, const double* R, const double* T, double* d_points, double* d_frames)
{
    for (size_t k = 0; d_points && k < s.pt_idx.size(); ++k)
        for (int e = 0; e < 3; ++e) d_points[3 * k + e] = pts[(size_t)(3 * s.pt_idx[k] + e)] - s.pt_pos[3 * k + e];
    for (size_t k = 0; d_frames && k < s.fr_idx.size(); ++k) {
        double C[3];
        centre(R, T, s.fr_idx[k], C);
        for (int e = 0; e < 3; ++e) d_frames[3 * k + e] = C[e] - s.fr_pos[3 * k + e];
    }
}

void srk_relpose_residuals(const SrkRelPoseApplied& s, const double* R, const double* T, double* r_out)
{
    for (size_t k = 0; k < s.a.size(); ++k) {
        const double* ra = R + 9 * (size_t)s.a[k];
        const double* rb = R + 9 * (size_t)s.b[k];
        const double* Z = &s.R[9 * k];
        double Ca[3], Cb[3], Pm[9], M[9];
        centre(R, T, s.a[k], Ca);
        centre(R, T, s.b[k], Cb);
        double* e = r_out + 6 * k;
        for (int r = 0; r < 3; ++r)
            e[r] = ra[3 * r] * (Cb[0] - Ca[0]) + ra[3 * r + 1] * (Cb[1] - Ca[1]) + ra[3 * r + 2] * (Cb[2] - Ca[2]) - s.t[3 * k + (size_t)r];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Pm[3 * r + c] = ra[3 * r] * rb[3 * c] + ra[3 * r + 1] * rb[3 * c + 1] + ra[3 * r + 2] * rb[3 * c + 2];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) M[3 * r + c] = Z[r] * Pm[c] + Z[3 + r] * Pm[3 + c] + Z[6 + r] * Pm[6 + c];
        so3_log(M, e + 3);
    }
}

void srk_jprior_residuals(const SrkJPriorApplied& s, const double* R, const double* T, double* r_out)
{
    for (size_t q = 0; q < s.frame.size(); ++q) {
        const double* r = R + 9 * (size_t)s.frame[q];
        const double* Rb = &s.R[9 * q];
        double* e = r_out + 6 * q;
        double M[9];
        centre(R, T, s.frame[q], e);
        for (int c = 0; c < 3; ++c) e[c] -= s.C[3 * q + (size_t)c];
        for (int a = 0; a < 3; ++a) // M = R^T Rbar
            for (int b = 0; b < 3; ++b) M[3 * a + b] = r[a] * Rb[b] + r[3 + a] * Rb[3 + b] + r[6 + a] * Rb[6 + b];
        so3_log(M, e + 3);
        for (int c = 0; c < 6; ++c) e[c] -= s.mean[6 * q + (size_t)c];
    }
}

// ------------------------------------------------------------------ Gauss-Newton terms of one factor / one set
// The marginalisation prior adds these on the host to the sum the device formed.  Poses in the normalised world, Log as above
// and the inverse Jacobians on the kernels' series and thresholds (rp_jk of srk_ba_kernels.hip): must stay in step with theirs.

// the coefficient of [phi]x^2 in the inverse Jacobians of SO(3) at the squared angle t2
static double so3_jk(double t2)
{
    if (t2 < 1e-6) return 1.0 / 12.0 + t2 / 720.0;
    const double t = std::sqrt(t2);
    if (t2 >= 2.25) return 1.0 / t2 - 1.0 / (2.0 * t * std::tan(0.5 * t));
    return 1.0 / t2 - (1.0 + std::cos(t)) / (2.0 * t * std::sin(t));
}
// I + sg [p]x / 2 + k [p]x^2: the inverse right Jacobian (sg = +1) or the inverse left Jacobian (sg = -1) at p
static void so3_jinv(const double p[3], double sg, double J[9])
{
    const double t2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2], k = so3_jk(t2), h = 0.5 * sg;
    J[0] = 1.0 + k * (p[0] * p[0] - t2); J[1] = -h * p[2] + k * p[0] * p[1]; J[2] = h * p[1] + k * p[0] * p[2];
    J[3] = h * p[2] + k * p[0] * p[1]; J[4] = 1.0 + k * (p[1] * p[1] - t2); J[5] = -h * p[0] + k * p[1] * p[2];
    J[6] = -h * p[1] + k * p[0] * p[2]; J[7] = h * p[0] + k * p[1] * p[2]; J[8] = 1.0 + k * (p[2] * p[2] - t2);
}
// H = J^T L J (n x n) and g = J^T L e from J [rows][n], L [rows][rows], e [rows]
static void gn_terms(int rows, int n, const double* J, const double* L, const double* e, double* H, double* g)
{
    std::vector<double> LJ((size_t)rows * n, 0.0), Le((size_t)rows, 0.0);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < rows; ++c) {
            const double l = L[r * rows + c];
            if (l == 0) continue;
            Le[(size_t)r] += l * e[c];
            for (int v = 0; v < n; ++v) LJ[(size_t)r * n + v] += l * J[c * n + v];
        }
    for (int a = 0; a < n; ++a) {
        double s = 0;
        for (int r = 0; r < rows; ++r) s += J[r * n + a] * Le[(size_t)r];
        g[a] = s;
        for (int v = 0; v < n; ++v) {
            double h = 0;
            for (int r = 0; r < rows; ++r) h += J[r * n + a] * LJ[(size_t)r * n + v];
            H[a * n + v] = h;
        }
    }
}

void srk_relpose_terms(const double* Ra, const double* Ta, const double* Rb, const double* Tb, const double* Z, const double* z,
                       const double* L, double* H, double* g)
{
    double Ca[3], Cb[3], d[3], e[6], Pm[9], M[9], Ji[9];
    centre(Ra, Ta, 0, Ca);
    centre(Rb, Tb, 0, Cb);
    for (int c = 0; c < 3; ++c) d[c] = Cb[c] - Ca[c];
    for (int r = 0; r < 3; ++r) e[r] = Ra[3 * r] * d[0] + Ra[3 * r + 1] * d[1] + Ra[3 * r + 2] * d[2] - z[r];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Pm[3 * r + c] = Ra[3 * r] * Rb[3 * c] + Ra[3 * r + 1] * Rb[3 * c + 1] + Ra[3 * r + 2] * Rb[3 * c + 2];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) M[3 * r + c] = Z[r] * Pm[c] + Z[3 + r] * Pm[3 + c] + Z[6 + r] * Pm[6 + c];
    so3_log(M, e + 3);
    so3_jinv(e + 3, 1.0, Ji);
    // [-R_a, R_a [d]x, R_a, 0; 0, -Jr^-1 R_b, 0, Jr^-1 R_b] over [T_a W_a T_b W_b]
    const double dx[9] = { 0.0, -d[2], d[1], d[2], 0.0, -d[0], -d[1], d[0], 0.0 };
    double J[72] = {};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            J[12 * r + c] = -Ra[3 * r + c];
            J[12 * r + 3 + c] = Ra[3 * r] * dx[c] + Ra[3 * r + 1] * dx[3 + c] + Ra[3 * r + 2] * dx[6 + c];
            J[12 * r + 6 + c] = Ra[3 * r + c];
            const double jr = Ji[3 * r] * Rb[c] + Ji[3 * r + 1] * Rb[3 + c] + Ji[3 * r + 2] * Rb[6 + c];
            J[12 * (3 + r) + 3 + c] = -jr;
            J[12 * (3 + r) + 9 + c] = jr;
        }
    gn_terms(6, 12, J, L, e, H, g);
}

void srk_jprior_terms(int32_t k, const double* R, const double* T, const double* lin, const double* mean, const double* L, double* H, double* g)
{
    const int n = 6 * k;
    std::vector<double> J((size_t)n * n, 0.0), e((size_t)n);
    for (int32_t q = 0; q < k; ++q) {
        const double* r = R + 9 * (size_t)q;
        const double* Rb = lin + 12 * (size_t)q;
        double M[9], Ji[9], rr[6];
        centre(R, T, q, rr);
        for (int c = 0; c < 3; ++c) rr[c] -= Rb[9 + c];
        for (int a = 0; a < 3; ++a) // M = R^T Rbar
            for (int b = 0; b < 3; ++b) M[3 * a + b] = r[a] * Rb[b] + r[3 + a] * Rb[3 + b] + r[6 + a] * Rb[6 + b];
        so3_log(M, rr + 3);
        so3_jinv(rr + 3, -1.0, Ji);
        for (int c = 0; c < 6; ++c) e[(size_t)(6 * q + c)] = rr[c] - mean[6 * q + c];
        for (int a = 0; a < 3; ++a) {
            J[(size_t)(6 * q + a) * n + 6 * q + a] = 1.0;
            for (int b = 0; b < 3; ++b) J[(size_t)(6 * q + 3 + a) * n + 6 * q + 3 + b] = Ji[3 * a + b];
        }
    }
    gn_terms(n, n, J.data(), L, e.data(), H, g);
}
