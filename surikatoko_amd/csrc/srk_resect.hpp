// srk_resect.hpp -- batched camera resection (srk_resect_frames, srk_ba_resect), the host half: the option
// defaults, the argument checks, the map of start poses into and of results out of the normalised coordinates and a walk of one
// frame on the host in the kernel's own order of operations.  Host only: no HIP, so all of it can be checked on a machine without
// a GPU (tests/cpp/test_resect_host.cpp).  srk_ba_host.hip allocates and copies; the kernels are in srk_resect.hip.
#pragma once
#include "../../include/srk_ba.h"
#include "srk_limits.hpp"

#include <stdint.h>
#include <string>
#include <vector>

// the options a call runs with: opts NULL = the defaults
srk_resect_options srk_resect_effective_options(const srk_resect_options* opts);

// The checks of a call, or the text of its refusal (empty = fine).  Every index the kernel will follow is looked at here.  X may
// be NULL (srk_ba_resect: the landmarks are the resident scene's); point_int (caller's landmark -> internal, or NULL) is applied
// inside the loop that checks point[], into `mapped` when that is not NULL.
std::string srk_resect_check(int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv, const double* q, int64_t n_points,
                             const double* X, const double* K, int shared_k, const double* R0, const double* T0, const srk_resect_options* opts,
                             const int64_t* point_int = nullptr, std::vector<int32_t>* mapped = nullptr);

// start poses into the normalised coordinates: R_n = R R0^T, T_n = s (T - R_n T0); and results back: R = R_n R0, T = T_n / s +
// R_n T0, info = D^T info_n D with D = diag(s R0, R0) (the inverse of what srk_ba_revert_covariances does to a pose covariance).
// Any array may be NULL.  With quality [n][6] (srk_ba_resect), its two entries that depend on the coordinates follow: cond_1 is taken
// again from the mapped info (the Jacobi scaling absorbs the scale, not the rotation R0; a frame whose cond_1 is NaN -- FEW_POINTS,
// DEGENERATE -- keeps the NaN) and the smallest depth is divided by s on every frame, a DEGENERATE one included.
void srk_resect_normalize_poses(const srk_ba_normalizer& nrm, int32_t n, const double* R, const double* T, double* Rn, double* Tn);
void srk_resect_revert_poses(const srk_ba_normalizer& nrm, int32_t n, double* R, double* T, double* info, double* quality = nullptr);

// One frame on the host, statement for statement what its 64 lanes do on the device (the same deal of the weighted observations,
// the same merge tree, the same loop; only the contraction of multiply-adds and the last bits of sin, cos and log1p may differ).
// point, uv, q, w_out: the frame's own observations.  log (may be NULL) receives one entry per attempt: 1 accepted, 0 rejected.
// Returns the status bits.
uint32_t srk_resect_host_frame(int64_t n_obs, const int32_t* point, const double* uv, const double* q, const double* X, const double* K,
                               const double* R0, const double* T0, double f0, const srk_resect_options& opts, double R[9], double T[3],
                               double quality[6], double info[36], double* w_out, std::vector<int>* log = nullptr);
