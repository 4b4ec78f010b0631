// srk_resect_dev.hpp -- the kernels of batched camera resection (srk_resect.hip).  Every pointer is a
// device pointer; the host side (srk_resect.cpp) has checked every index before anything is launched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// pack [n_frames][SRK_RESECT_PACK] from the frames' start poses and intrinsics (K [n_frames][9], or [9] when shared_k)
void srk_launch_resect_pack(hipStream_t s, int32_t n_frames, const double* R0, const double* T0, const double* K, int shared_k, double* pack);
// The frames, one wave each.  q NULL = all 1.  attempts 0 = evaluate only.  X [n_points][3].  R [n][9], T [n][3], quality [n][6],
// info [n][36], status [n]; w_out [O] or NULL.
void srk_launch_resect_frames(hipStream_t s, int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv, const double* q,
                              const double* X, const double* K, int shared_k, const double* R0, const double* T0, const double* pack, double f0,
                              int32_t attempts, double rel_change, int32_t loss_kind, double loss_delta, double* R, double* T, double* quality,
                              double* info, uint32_t* status, double* w_out);
