// srk_pair_dev.hpp -- the kernels of two-view pose refinement (srk_pair.hip).  Every pointer is a device
// pointer; the host side (srk_pair.cpp) has checked every index before anything is launched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// kinv [n_pairs][SRK_PAIR_KINV]: the inverses of the pairs' intrinsics (K_a, K_b [n_pairs][9], or [9] when shared_k)
void srk_launch_pair_pack(hipStream_t s, int32_t n_pairs, const double* K_a, const double* K_b, int shared_k, double* kinv);
// qe [O] = q (NULL = 1) times the inlier flags of relate's winner
void srk_launch_pair_mask(hipStream_t s, int64_t n_obs, const double* q, const uint8_t* inlier, double* qe);
// The pairs, one wave each.  q NULL = all 1.  attempts 0 = evaluate only.  related_status NULL, or relate's status words: a pair
// with a non-zero word starts from (I, (1, 0, 0)) whatever R0, T0 hold.  R [n][9], T [n][3], E [n][9], quality [n][6], info [n][25],
// basis [n][6], status [n]; w_out [O] or NULL.
void srk_launch_pair_refine(hipStream_t s, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                            const double* kinv, const double* R0, const double* T0, const uint32_t* related_status, double f0, int32_t attempts,
                            double rel_change, int32_t loss_kind, double loss_delta, double* R, double* T, double* E, double* quality, double* info,
                            double* basis, uint32_t* status, double* w_out);
