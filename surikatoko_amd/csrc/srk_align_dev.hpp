// srk_align_dev.hpp -- the kernels of map alignment (srk_align.hip).  Every pointer is a device pointer; the
// host side (srk_align.cpp) has checked every index before anything is launched.  The source of correspondence o is a[o], or
// with point != NULL the landmark a[point[o]].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The sets' weighted correspondences (q > 0; q NULL = all) compacted in ascending order into strip [O][SRK_ALIGN_STRIP] at
// row_ptr[i] + rank: a, b, q.  count [n_sets] receives the number of weighted correspondences.  One wave per set.
void srk_launch_align_gather(hipStream_t s, int32_t n_sets, const int64_t* row_ptr, const int32_t* point, const double* a, const double* b,
                             const double* q, double* strip, int64_t* count);
// One lane per (set, hypothesis), a wave = 64 hypotheses of one set: the sample, the triad, then the score over the set's strip;
// the wave's best into slots [n_sets][waves][SRK_ALIGN_SLOT], waves = ceil(hypotheses / 64).
void srk_launch_align_score(hipStream_t s, int32_t n_sets, int32_t hypotheses, uint64_t seed, double tau, int with_scale, const int64_t* row_ptr,
                            const double* strip, const int64_t* count, double* slots);
// Per set: the best of its waves' slots in ascending wave order, up to refine_rounds rounds of local optimisation over the strip,
// then scale [n], R [n][9], t [n][3], aligned [n][8], status [n]; inlier_out [O] or NULL, from one pass over the set's
// correspondences at the final model.  One wave per set.
void srk_launch_align_pick(hipStream_t s, int32_t n_sets, int32_t hypotheses, double tau, int with_scale, int32_t refine_rounds, const int64_t* row_ptr,
                           const int32_t* point, const double* a, const double* b, const double* q, const double* strip, const int64_t* count,
                           const double* slots, double* scale, double* R, double* t, double* aligned, uint32_t* status, uint8_t* inlier_out);
