// srk_factors.hpp -- the factor settings (observation information, constant blocks, position priors, relative-pose factors, joint
// pose priors): what a setter stores, the checks of its values, what the next upload selects and the tables it builds for the
// device, and the residuals in the caller's units.  Host only: no HIP, so all of it can be checked on a machine without a GPU
// (tests/cpp/test_factor_tables.cpp).  srk_ba_host.hip allocates and copies what the builders return.
#pragma once
#include "../../include/srk_ba.h"
#include "srk_limits.hpp"
#include "srk_plan.hpp"

#include <stdint.h>
#include <string>
#include <vector>

#define SRK_RP_PLANES_HOST 33 // must match SRK_RP_PLANES of srk_dev.hpp (srk_ba_host.hip asserts it)

// ---- the settings: what a setter stores, in the caller's numbering and world coordinates, kept across uploads and
// srk_ba_reset_scene; and per family with residual calls the snapshot "what the resident scene was uploaded with"
struct SrkInfoSetting { // srk_ba_set_observation_information
    std::vector<double> q; // the caller's observation order, empty = none
};
struct SrkConstSetting { // srk_ba_set_constant_blocks (section 13): flags, either may be empty = none of that kind
    bool set = false;
    int keep_gauge = 1;
    std::vector<uint8_t> frames, points;
};
struct SrkPriorSetting { // srk_ba_set_position_priors (section 14)
    bool set = false;
    int keep_gauge = 1;
    std::vector<int64_t> pt_idx;
    std::vector<int32_t> fr_idx;
    std::vector<double> pt_pos, pt_info, fr_pos, fr_info;
};
struct SrkRelPoseSetting { // srk_ba_set_relative_pose_factors (section 15)
    bool set = false;
    std::vector<int32_t> a, b;
    std::vector<double> R, t, info;
};
struct SrkJPriorSetting { // srk_ba_set_joint_pose_priors (section 18): info symmetrised, mean zeros where none was given
    bool set = false;
    int keep_gauge = 1;
    std::vector<int32_t> ptr, frame;
    std::vector<double> R, C, mean, info;
    const double* info_of(size_t g) const; // the information matrix of set g: dense row-major, 6 k rows
};
// The snapshots hold indices and values the residuals are made of, not the information matrices: a change of information alone
// after an upload does not refuse the residual calls.  take() at an upload (a cleared setting is empty vectors), is() in the guard
// of a residual call.
struct SrkPriorApplied {
    std::vector<int64_t> pt_idx;
    std::vector<int32_t> fr_idx;
    std::vector<double> pt_pos, fr_pos;
    void take(const SrkPriorSetting& s) { pt_idx = s.pt_idx, fr_idx = s.fr_idx, pt_pos = s.pt_pos, fr_pos = s.fr_pos; }
    bool is(const SrkPriorSetting& s) const { return pt_idx == s.pt_idx && fr_idx == s.fr_idx && pt_pos == s.pt_pos && fr_pos == s.fr_pos; }
};
struct SrkRelPoseApplied {
    bool set = false;
    std::vector<int32_t> a, b;
    std::vector<double> R, t;
    void take(const SrkRelPoseSetting& s) { set = s.set, a = s.a, b = s.b, R = s.R, t = s.t; }
    bool is(const SrkRelPoseSetting& s) const { return set == s.set && a == s.a && b == s.b && R == s.R && t == s.t; }
};
struct SrkJPriorApplied {
    bool set = false;
    std::vector<int32_t> ptr, frame;
    std::vector<double> R, C, mean;
    void take(const SrkJPriorSetting& s) { set = s.set, ptr = s.ptr, frame = s.frame, R = s.R, C = s.C, mean = s.mean; }
    bool is(const SrkJPriorSetting& s) const { return set == s.set && ptr == s.ptr && frame == s.frame && R == s.R && C == s.C && mean == s.mean; }
};

// ---- the checks of the setters: NULL when fine, else a static text
const char* srk_check_prior_values(int64_t n, const double* pos, const double* info);
const char* srk_check_relpose(int32_t n, const int32_t* fa, const int32_t* fb, const double* R, const double* t, const double* info);
const char* srk_check_jprior(int32_t n_sets, const int32_t* set_ptr, const int32_t* frame, const double* lin_R, const double* lin_C,
                             const double* mean, const double* info, int keep_gauge);
// positive semi-definite n x n (full symmetric A, destroyed): elimination with diagonal pivoting; every pivot must be >= 0 up to
// the rounding of a rank-deficient matrix, and once the largest remaining diagonal entry is ~0 so must be everything left
bool srk_info_psd(double* A, int64_t n);
void srk_symmetrise(double* L, int64_t n); // the symmetric part of a dense row-major n x n matrix, in place
// A setting of the named family ("constant blocks", "position priors", "relative-pose factors", "joint pose priors") masks or
// adds to the 10- or 6-variable system of one rank: the fold of shared intrinsics and the exchange of the ranks' partial sums
// can follow later.  The text of the refusal, empty when fine.
std::string srk_setting_conflict(const char* family, bool set, bool groups, int world);

// ---- before the plan: the settings against the scene's counts, the switched-on factors and sets (an all-zero information matrix
// is left out, plan included, so that the run has the bits of the run without it) and the pairs of frames the planner must see
struct SrkFactorSelection {
    std::vector<int32_t> rp_act, jp_act; // the switched-on factors and sets: place in the setting
    std::vector<int32_t> rel_a, rel_b;   // SrkPlanOptions::rel_a / rel_b: the factors' pairs, then the sets' coupled pairs that are
                                         // not among them, each unordered pair once; caller's numbering
    std::vector<int32_t> jp_pptr, jp_pslot; // per active set its coupled slot pairs (slot i << 8) | slot j, i > j: those whose 6 x 6
                                            // block of the stored L is not all zeros (the normaliser maps a zero block to zeros)
};
// the text of the refusal, empty when fine
std::string srk_select_factors(const SrkConstSetting& cst, const SrkPriorSetting& pri, const SrkRelPoseSetting& rp, const SrkJPriorSetting& jp,
                               int64_t N, int32_t M, SrkFactorSelection& sel);

// ---- after the plan: the tables of the resident scene, in the layouts srk_dev.hpp documents.  Landmarks through the internal
// order (perm), frames through the renumbering (frame_int), values through the normaliser of the upload.
struct SrkFactorDims { int64_t N; int32_t M; int64_t O; int fv; int64_t ld; }; // fv: variables of a frame (10, or 6), ld: leading dimension of S
// [caller's observation] = its place in the internal order (srk_ba_observation_weights and _residuals map back through it)
std::vector<int64_t> srk_observation_places(const SrkPlanKept& plan, int64_t N, int64_t O);
struct SrkInfoTables {
    bool on = false;
    std::vector<double> q, qf; // internal order; frame-major order of fobs_* (two-kernel derivative path only)
};
struct SrkConstTables {
    std::vector<int32_t> pts, frames; // constant landmarks (internal order) and internal frames, ascending
    std::vector<uint8_t> frame_int;   // kept on the handle: the frames' flags by internal index
};
struct SrkPriorTables {
    std::vector<int32_t> pt_list, fr_list;
    std::vector<double> pt_val, fr_val; // [9][n]
};
struct SrkRelPoseTables {
    std::vector<int32_t> fa, fb; // kept on the handle as well: the internal frames of the active factors
    std::vector<double> val;     // [SRK_RP_PLANES_HOST][n]
    std::vector<int32_t> fr_list, fr_ptr, fr_ent;
    std::vector<int64_t> tgt;
};
struct SrkJPriorTables {
    std::vector<int32_t> ptr, frame, pptr, pslot, fr_list, fr_ptr, fr_ent;
    std::vector<int64_t> iptr, tgt;
    std::vector<double> lin, mean, info;
    std::vector<int32_t> pair_a, pair_b; // kept on the handle: the coupled pairs (lo, hi), internal numbering
};
SrkInfoTables srk_build_information(const SrkInfoSetting& s, const SrkPlanKept& plan, const SrkFactorDims& d);
SrkConstTables srk_build_constant(const SrkConstSetting& s, const SrkPlanKept& plan, const SrkFactorDims& d);
SrkPriorTables srk_build_priors(const SrkPriorSetting& s, const srk_ba_normalizer& nrm, const SrkPlanKept& plan, const SrkFactorDims& d);
SrkRelPoseTables srk_build_relpose(const SrkRelPoseSetting& s, const SrkFactorSelection& sel, const srk_ba_normalizer& nrm,
                                   const SrkPlanKept& plan, const SrkFactorDims& d);
SrkJPriorTables srk_build_jprior(const SrkJPriorSetting& s, const SrkFactorSelection& sel, const srk_ba_normalizer& nrm,
                                 const SrkPlanKept& plan, const SrkFactorDims& d);

// ---- residuals in the caller's units, from a downloaded scene (the caller's world coordinates) and the snapshot of its upload.
// The SO(3) logarithm is the kernels' (k_relpose_error, k_jprior_error): series below sin = 1e-4 at a positive cosine, the axis
// from the symmetric part at a cosine below -0.9 (valid up to and at pi), atan2 over the antisymmetric part else.
void srk_prior_residuals(const SrkPriorApplied& s, const double* pts, const double* R, const double* T, double* d_points /* [n][3] or NULL */,
                         double* d_frames /* [n][3] or NULL */);
void srk_relpose_residuals(const SrkRelPoseApplied& s, const double* R, const double* T, double* r_out /* [n][6] */);
void srk_jprior_residuals(const SrkJPriorApplied& s, const double* R, const double* T, double* r_out /* [slots][6] */);

// ---- the Gauss-Newton terms of one factor / one set at given poses (srk_ba_marginalization_prior adds them on the host; DESIGN.md
// section 20): H = J^T L J and g = J^T L e, WITHOUT the factor 2 of the device's sums, over the pose variables [Tx Ty Tz Wx Wy Wz]
// of the frames.  Poses (R world -> camera, T) and values in one coordinate system (the device tables' normalised world).  The
// same Log, inverse-Jacobian series and thresholds as the kernels (k_relpose_add, k_jprior_form).
// one relative-pose factor between frames a and b: Z [9], z [3], L [36] full symmetric; H [144] (a's six variables first), g [12]
void srk_relpose_terms(const double* Ra, const double* Ta, const double* Rb, const double* Tb, const double* Z, const double* z,
                       const double* L, double* H, double* g);
// one joint set over k frames: R [k][9], T [k][3] the frames' poses, lin [k][12] (Rbar, Cbar), mean [6 k], L [(6 k)^2]; H [(6 k)^2], g [6 k]
void srk_jprior_terms(int32_t k, const double* R, const double* T, const double* lin, const double* mean, const double* L, double* H, double* g);
