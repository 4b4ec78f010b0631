// srk_locate.hpp -- resection without a start pose (srk_locate_frames, srk_ba_locate), the host half: the
// option defaults, the argument checks and a walk of one frame on the host in the kernels' own order of operations.  Host only:
// no HIP, so all of it can be checked on a machine without a GPU (tests/cpp/test_locate_host.cpp).  srk_ba_host.hip allocates and
// copies; the kernels are in srk_locate.hip.
#pragma once
#include "../../include/srk_ba.h"
#include "srk_limits.hpp"

#include <stdint.h>
#include <string>
#include <vector>

// the options a call runs with: opts NULL = the defaults
srk_locate_options srk_locate_effective_options(const srk_locate_options* opts);

// The checks of a call, or the text of its refusal (empty = fine).  Every index the kernels will follow is looked at here.  X may
// be NULL (srk_ba_locate: the landmarks are the resident scene's); point_int (caller's landmark -> internal, or NULL) is applied
// inside the loop that checks point[], into `mapped` when that is not NULL.  refine NULL = no refinement.
std::string srk_locate_check(int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv, const double* q, int64_t n_points,
                             const double* X, const double* K, int shared_k, const srk_locate_options* opts, const srk_resect_options* refine,
                             const int64_t* point_int = nullptr, std::vector<int32_t>* mapped = nullptr);

// One frame on the host, statement for statement what the kernels do (the ranks of the weighted observations, every hypothesis'
// sample, P3P and choice, its score summed in ascending rank order, the pick; only the contraction of multiply-adds and the last
// bits of sqrt, cbrt, cos and acos may differ).  point, uv, q, inlier_out: the frame's own observations.  scores (may be NULL)
// receives every hypothesis' score.  Returns the status bits.
uint32_t srk_locate_host_frame(int64_t n_obs, const int32_t* point, const double* uv, const double* q, const double* X, const double* K,
                               double f0, const srk_locate_options& opts, double R[9], double T[3], double located[6], uint8_t* inlier_out,
                               std::vector<double>* scores = nullptr);

// P3P alone, for the tests: the poses of the landmarks X [3][3] seen at the pixels uv [3][2], every real root (no depth test, no
// fourth point).  R [4][9], T [4][3], ok [4]; returns the number of poses.
int srk_locate_p3p_all(const double* K, double f0, const double* X, const double* uv, double* R, double* T, int* ok);
