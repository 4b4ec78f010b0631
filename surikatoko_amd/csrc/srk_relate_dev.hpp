// srk_relate_dev.hpp -- the kernels of two-view relative pose (srk_relate.hip).  Every pointer is a device
// pointer; the host side (srk_relate.cpp) has checked every index before anything is launched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The pairs' weighted matches (q > 0; q NULL = all) compacted in ascending order into strip [O][SRK_RELATE_STRIP] at
// row_ptr[i] + rank: uv_a, uv_b, q, the match's number in its pair.  count [n_pairs] receives the number of weighted matches.  One
// wave per pair.
void srk_launch_relate_gather(hipStream_t s, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                              double* strip, int64_t* count);
// 16 lanes per (pair, hypothesis): the sample, the five-point solve and the choice by the sixth match into
// hyp [n_pairs][hypotheses][SRK_RELATE_HYP].
void srk_launch_relate_solve(hipStream_t s, int32_t n_pairs, int32_t hypotheses, uint64_t seed, double f0, const int64_t* row_ptr, const double* strip,
                             const int64_t* count, const double* K_a, const double* K_b, int shared_k, double* hyp);
// One lane per (pair, hypothesis), a wave = 64 hypotheses of one pair: the score over the pair's strip; the wave's best into
// slots [n_pairs][waves][SRK_RELATE_SLOT], waves = ceil(hypotheses / 64).
void srk_launch_relate_score(hipStream_t s, int32_t n_pairs, int32_t hypotheses, double tau, double f0, const int64_t* row_ptr, const double* strip,
                             const int64_t* count, const double* hyp, double* slots);
// Per pair: the best of its waves' slots in ascending wave order, the decomposition of the winner and the vote of its four poses
// over the pair's inliers; R [n][9], T [n][3], E [n][9], related [n][8], status [n]; inlier_out [O] or NULL.  One wave per pair.
void srk_launch_relate_pick(hipStream_t s, int32_t n_pairs, int32_t hypotheses, double tau, double f0, const int64_t* row_ptr, const double* q,
                            const double* strip, const int64_t* count, const double* K_a, const double* K_b, int shared_k, const double* hyp,
                            const double* slots, double* R, double* T, double* E, double* related, uint32_t* status, uint8_t* inlier_out);
