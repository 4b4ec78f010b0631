// srk_locate_dev.hpp -- the kernels of resection without a start pose (srk_locate.hip).  Every pointer is a
// device pointer; the host side (srk_locate.cpp) has checked every index before anything is launched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The frames' weighted observations (q > 0; q NULL = all) compacted in ascending order into strip [O][SRK_LOCATE_STRIP] at
// row_ptr[i] + rank: X[point[o]], uv, q.  count [n_frames] receives the number of weighted observations.  One wave per frame.
void srk_launch_locate_gather(hipStream_t s, int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv, const double* q,
                              const double* X, double* strip, int64_t* count);
// One lane per (frame, hypothesis), a wave = 64 hypotheses of one frame: the sample, P3P and the choice by the fourth point, then
// the score over the frame's strip; the wave's best into slots [n_frames][waves][SRK_LOCATE_SLOT], waves = ceil(hypotheses / 64).
void srk_launch_locate_score(hipStream_t s, int32_t n_frames, int32_t hypotheses, uint64_t seed, double tau, double f0, const int64_t* row_ptr,
                             const double* strip, const int64_t* count, const double* K, int shared_k, double* slots);
// Per frame: the best of its waves' slots in ascending wave order; R [n][9], T [n][3], located [n][6], status [n]; inlier_out [O]
// or NULL, from one pass over the frame's observations at the located pose.  One wave per frame.
void srk_launch_locate_pick(hipStream_t s, int32_t n_frames, int32_t hypotheses, double tau, double f0, const int64_t* row_ptr, const int32_t* point,
                            const double* uv, const double* q, const double* X, const double* K, int shared_k, const int64_t* count,
                            const double* slots, double* R, double* T, double* located, uint32_t* status, uint8_t* inlier_out);
