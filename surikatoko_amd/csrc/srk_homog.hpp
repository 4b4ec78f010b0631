// srk_homog.hpp -- the two-view homography (srk_relate_homography), the host half: the option defaults, the
// argument checks, a walk of one pair on the host in the kernels' own order of operations, and the decomposition on its own.
// Host only: no HIP, so all of it can be checked on a machine without a GPU (tests/cpp/test_homog_host.cpp).  srk_ba_host.hip
// allocates and copies; the kernels are in srk_homog.hip.
#pragma once
#include "../../include/srk_ba.h"
#include "srk_limits.hpp"

#include <stdint.h>
#include <string>
#include <vector>

// the options a call runs with: opts NULL = the defaults
srk_homography_options srk_homog_effective_options(const srk_homography_options* opts);

// The checks of a call, or the text of its refusal (empty = fine).  Every index the kernels will follow is looked at here.
std::string srk_homog_check(int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q, const double* K_a,
                            const double* K_b, int shared_k, const srk_homography_options* opts);

// the outputs of one pair
struct SrkHomogResult {
    double G[9], H[9], R[18], T[6], N[6], homog[8];
    int32_t n_poses, front[2];
};

// One pair on the host, statement for statement what the kernels do (the ranks of the weighted matches, every hypothesis' sample,
// model and score in ascending rank order, the pick, the rounds with the lanes' strided sums merged in the wave's tree, the
// decomposition with its two passes over the inliers; only the contraction of multiply-adds and the last bits of sqrt may differ).
// scores (may be NULL) receives every hypothesis' score.  Returns the status bits.
uint32_t srk_homog_host_walk(int64_t n_obs, const double* uv_a, const double* uv_b, const double* q, const double* K_a, const double* K_b, double f0,
                             const srk_homography_options& opts, SrkHomogResult& out, uint8_t* inlier_out, std::vector<double>* scores = nullptr);
