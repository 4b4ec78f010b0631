// srk_align.hpp -- map alignment (srk_align_points, srk_ba_align), the host half: the option defaults, the
// argument checks, a walk of one set on the host in the kernels' own order of operations, and the maps between the normalised
// scene's similarity and the caller's.  Host only: no HIP, so all of it can be checked on a machine without a GPU
// (tests/cpp/test_align_host.cpp).  srk_ba_host.hip allocates and copies; the kernels are in srk_align.hip.
#pragma once
#include "../../include/srk_ba.h"
#include "srk_limits.hpp"

#include <stdint.h>
#include <string>
#include <vector>

// the options a call runs with: opts NULL = the defaults (which the checks refuse: inlier_distance has none)
srk_align_options srk_align_effective_options(const srk_align_options* opts);

// The checks of a call, or the text of its refusal (empty = fine).  Every index the kernels will follow is looked at here.  With
// point != NULL the sources are landmarks of a map of n_points (srk_ba_align; a may then be NULL) and point_int (caller's landmark
// -> internal, or NULL) is applied inside the loop that checks point[], into `mapped` when that is not NULL.
std::string srk_align_check(int32_t n_sets, const int64_t* row_ptr, const int32_t* point, int64_t n_points, const double* a, const double* b,
                            const double* q, const srk_align_options* opts, const int64_t* point_int = nullptr, std::vector<int32_t>* mapped = nullptr);

// One set on the host, statement for statement what the kernels do (the ranks of the weighted correspondences, every hypothesis'
// sample, triad and score in ascending rank order, the pick, the rounds of local optimisation with the lanes' strided sums merged
// in the wave's tree; only the contraction of multiply-adds and the last bits of sqrt may differ).  scores (may be NULL) receives
// every hypothesis' score.  Returns the status bits.
uint32_t srk_align_host_walk(int64_t n_obs, const double* a, const double* b, const double* q, const srk_align_options& opts, double* s, double R[9],
                             double t[3], double aligned[8], uint8_t* inlier_out, std::vector<double>* scores = nullptr);

// the similarity found in the normalised scene (X_n = s_n (R0 X + T0)) as a map of the caller's coordinates, in place:
// (sigma s_n, Q R0, sigma s_n Q T0 + tau)
void srk_align_revert(const srk_ba_normalizer& nrm, int32_t n, double* s, double* R, double* t);
