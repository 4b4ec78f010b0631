// srk_pair.hpp -- two-view pose refinement (srk_refine_pairs, srk_relate_frames_refined), the host half: the
// option defaults, the argument checks, a walk of one pair on the host in the kernel's own order of operations and the map from a
// refined pair to a relative-pose factor.  Host only: no HIP, so all of it can be checked on a machine without a GPU
// (tests/cpp/test_pair_host.cpp).  srk_ba_host.hip allocates and copies; the kernels are in srk_pair.hip.
#pragma once
#include "../../include/srk_ba.h"
#include "srk_limits.hpp"

#include <stdint.h>
#include <string>
#include <vector>

#define SRK_PAIR_MAX_ATTEMPTS_HOST 64
#define SRK_PAIR_MAX_PAIRS_HOST (1 << 22)

// the options a call runs with: opts NULL = the defaults
srk_pair_options srk_pair_effective_options(const srk_pair_options* opts);

// The checks of the options alone, or the text of the refusal (empty = fine).  chained: the call is srk_relate_frames_refined, where
// inliers_only may be 1.
std::string srk_pair_check_options(const srk_pair_options* opts, bool chained);

// The checks of srk_refine_pairs, or the text of its refusal (empty = fine).  Every index the kernel will follow is looked at here.
std::string srk_pair_check(int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q, const double* K_a,
                           const double* K_b, int shared_k, const double* R0, const double* T0, const srk_pair_options* opts);

// one attempt of a walk: whether it was accepted, E_pair before it and at the moved pose (NaN when the factorisation failed)
struct SrkPairAttempt {
    int accepted;
    double E_cur, E_cand;
};

// One pair on the host, statement for statement what its 64 lanes do on the device (the same deal of the weighted matches, the
// same merge tree, the same loop; only the contraction of multiply-adds and the last bits of sqrt, sin, cos and log1p may differ).
// uv_a, uv_b, q, w_out: the pair's own matches.  grad (may be NULL): g [5] at the result.  log (may be NULL): one entry per attempt.
// Returns the status bits.
uint32_t srk_pair_host_pair_cpp(int64_t n_obs, const double* uv_a, const double* uv_b, const double* q, const double* K_a, const double* K_b,
                                double f0, const double* R0, const double* T0, const srk_pair_options& opts, double R[9], double T[3], double E[9],
                                double quality[6], double info[25], double basis[6], double* w_out, double* grad = nullptr,
                                std::vector<SrkPairAttempt>* log = nullptr);
