// srk_fund_dev.hpp -- the kernels of the two-view fundamental matrix (srk_fund.hip).  Every pointer is a
// device pointer; the host side (srk_fund.cpp) has checked every index before anything is launched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The pairs' weighted matches (q > 0; q NULL = all) compacted in ascending order into strip [O][SRK_FUND_STRIP] at
// row_ptr[i] + rank: uv_a, uv_b, q.  count [n_pairs] receives the number of weighted matches.  One wave per pair.
void srk_launch_fund_gather(hipStream_t s, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                            double* strip, int64_t* count);
// One lane per (pair, hypothesis): the sample and the seven-point model into hyp [n_pairs][hypotheses][SRK_FUND_HYP].
void srk_launch_fund_solve(hipStream_t s, int32_t n_pairs, int32_t hypotheses, uint64_t seed, double f0, const int64_t* row_ptr, const double* strip,
                           const int64_t* count, double* hyp);
// One lane per (pair, hypothesis), a wave = 64 hypotheses of one pair: the score over the pair's strip; the wave's best into slots
// [n_pairs][waves][SRK_FUND_SLOT], waves = ceil(hypotheses / 64).
void srk_launch_fund_score(hipStream_t s, int32_t n_pairs, int32_t hypotheses, double tau, double f0, const int64_t* row_ptr, const double* strip,
                           const int64_t* count, const double* hyp, double* slots);
// Per pair: the best of its waves' slots in ascending wave order, the representation, up to refine_rounds attempts over the strip,
// then F, U, V [n][9], sigma [n], fund [n][12], info [n][49], status [n]; inlier_out [O] or NULL, from one pass over the pair's
// matches at the final model.  One wave per pair.
void srk_launch_fund_pick(hipStream_t s, int32_t n_pairs, int32_t hypotheses, double tau, double f0, int32_t refine_rounds, const int64_t* row_ptr,
                          const double* uv_a, const double* uv_b, const double* q, const double* strip, const int64_t* count, const double* hyp,
                          const double* slots, double* F, double* U, double* V, double* sigma, double* fund, double* info, uint32_t* status,
                          uint8_t* inlier_out);
