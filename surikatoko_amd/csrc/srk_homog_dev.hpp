// srk_homog_dev.hpp -- the kernels of the two-view homography (srk_homog.hip).  Every pointer is a device
// pointer; the host side (srk_homog.cpp) has checked every index before anything is launched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The pairs' weighted matches (q > 0; q NULL = all) compacted in ascending order into strip [O][SRK_HOMOG_STRIP] at
// row_ptr[i] + rank: uv_a, uv_b, q.  count [n_pairs] receives the number of weighted matches.  One wave per pair.
void srk_launch_homog_gather(hipStream_t s, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                             double* strip, int64_t* count);
// One lane per (pair, hypothesis), a wave = 64 hypotheses of one pair: the sample, the four-point model, then the score over the
// pair's strip; the wave's best into slots [n_pairs][waves][SRK_HOMOG_SLOT], waves = ceil(hypotheses / 64).
void srk_launch_homog_score(hipStream_t s, int32_t n_pairs, int32_t hypotheses, uint64_t seed, double tau, double f0, const int64_t* row_ptr,
                            const double* strip, const int64_t* count, double* slots);
// Per pair: the best of its waves' slots in ascending wave order, up to refine_rounds rounds of local optimisation over the strip,
// the decomposition, then G, H [n][9], n_poses [n], R [n][2][9], T, N [n][2][3], front [n][2], homog [n][8], status [n]; inlier_out
// [O] or NULL, from one pass over the pair's matches at the final model.  K_a, K_b [n][9], or [9] with shared_k.  One wave per pair.
void srk_launch_homog_pick(hipStream_t s, int32_t n_pairs, int32_t hypotheses, double tau, double f0, int32_t refine_rounds, const int64_t* row_ptr,
                           const double* uv_a, const double* uv_b, const double* q, const double* strip, const int64_t* count, const double* K_a,
                           const double* K_b, int shared_k, const double* slots, double* G, double* H, int32_t* n_poses, double* R, double* T, double* N,
                           int32_t* front, double* homog, uint32_t* status, uint8_t* inlier_out);
