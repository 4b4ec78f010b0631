// srk_marg.hpp -- marginalisation priors (srk_ba_marginalization_prior), the host half: the plan of a call
// (checks, slots, selected landmarks, involved factors), the dense elimination of the dropped frames and the map of a result
// back into the caller's coordinates.  Host only: no HIP, so all of it can be checked on a machine without a GPU
// (tests/cpp/test_marg_plan.cpp).  srk_ba_host.hip allocates and copies what a plan holds; the kernels are in srk_marg.hip.
#pragma once
#include "../../include/srk_ba.h"
#include "srk_limits.hpp"

#include <stdint.h>
#include <string>
#include <vector>

// the resident scene as the plan reads it: the CSR in the internal order, the information of the observations, the maps between
// the caller's numbering and the internal one, and the switched-on factor settings (internal frames / landmarks)
struct SrkMargScene {
    int64_t N = 0;
    int32_t M = 0;
    const int64_t* row_ptr = nullptr;    // [N + 1] internal landmark order
    const int32_t* obs_frame = nullptr;  // [O] internal frames
    const double* q = nullptr;           // [O] information in the internal order, NULL = all 1
    const int64_t* perm = nullptr;       // [N] perm[internal landmark] = caller's index
    const int32_t* frame_int = nullptr;  // [M] caller's frame -> internal, NULL = the same
    const int32_t* frame_user = nullptr; // [M] internal frame -> caller's, NULL = the same
    int64_t n_pt_priors = 0;
    const int32_t* pt_prior = nullptr;   // landmarks with a position prior, internal order, ascending
    int32_t n_fr_priors = 0;
    const int32_t* fr_prior = nullptr;   // internal frames with a centre prior, ascending
    int32_t n_rp = 0;
    const int32_t *rp_a = nullptr, *rp_b = nullptr; // internal frames of the switched-on relative-pose factors
    int32_t n_sets = 0;
    const int32_t *set_ptr = nullptr, *set_frame = nullptr; // the switched-on joint sets: slots and their internal frames
    bool constant_blocks = false, intrinsic_groups = false, multi_rank = false;
};

struct SrkMargPlan {
    int32_t d = 0, k = 0;                 // dropped and kept frames; slots = d + k, D first, then K ascending in the caller's numbering
    std::vector<int32_t> kept;            // [k] caller's numbering
    std::vector<int32_t> slot_frame;      // [d + k] internal frame of each slot
    std::vector<int32_t> frame_slot;      // [M] slot of an internal frame, -1 = none
    // the selected landmarks (at least two weighted observations each), ascending in the internal order
    std::vector<int32_t> lm;              // internal landmark
    std::vector<int64_t> lm_row;          // first row of its SRK_MARG_ROWS rows in the dense strip
    std::vector<int64_t> lm_stage;        // first of its observations' staging rows (one per observation, weighted or not)
    std::vector<int32_t> lm_prior;        // place of its position prior in the prior list, -1 = none
    int64_t n_rows = 0, n_stage = 0;      // rows of the strip, staging rows
    int64_t n_single = 0;                 // landmarks of P left out: fewer than two weighted observations
    // per slot, the staging rows of its weighted observations in landmark order: the order of the second pass's sums
    std::vector<int32_t> slot_ptr;        // [d + k + 1]
    std::vector<int64_t> slot_ent;
    std::vector<int32_t> fr_priors;       // places in the frame-prior list of the priors on centres of D
    std::vector<int32_t> factors, sets;   // the involved relative-pose factors and joint sets: places in the switched-on lists
    int32_t ldz() const { return (6 * (d + k) + 1 + 15) / 16 * 16; }
};

// The plan of a call, or the text of its refusal (empty = fine).  drop [nd] and points [np] in the caller's numbering, strictly
// ascending.  A refused call leaves an empty plan.
std::string srk_marg_plan(const SrkMargScene& sc, int32_t nd, const int32_t* drop, int64_t np, const int64_t* points, SrkMargPlan& plan);

// Dense elimination.  A [(6 n)^2] symmetric row-major and b [6 n] over n = d + k slots, D first:
//   Lam = A_KK - A_KD A_DD^-1 A_DK (symmetrised), eta = b_K - A_KD A_DD^-1 b_D, Lam m = -eta.
// A_DD is eliminated with diagonal pivoting and the threshold of srk_info_psd (a pivot <= 1e-12 max |A_DD| is not positive:
// returns 1, nothing written).  m is the basic solution of the same pivoted elimination of Lam: pivots <= 1e-12 max |Lam| are
// skipped and their components are zero.  defect = |Lam m + eta|_inf / |eta|_inf (0 when eta is zero).  Returns 0, or 1.
int srk_marg_dense(const double* A, const double* b, int32_t d, int32_t k, double* Lam, double* eta, double* m, double* defect);

// The inverse of srk_ba_normalize_joint_pose_priors' map on one set of k frames, in place; any array may be NULL:
//   Rbar = Rbar_n R0, Cbar = R0^T (Cbar_n / s - T0), Lam = D^T Lam_n D, eta = D^T eta_n, m = D^-1 m_n, D = diag(s R0, R0).
void srk_marg_revert(const srk_ba_normalizer& nrm, int32_t k, double* lin_R, double* lin_C, double* Lam, double* eta, double* m);
