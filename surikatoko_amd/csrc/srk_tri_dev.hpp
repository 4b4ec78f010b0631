// srk_tri_dev.hpp -- the kernels of batched triangulation (srk_tri.hip).  Every pointer is a device
// pointer; the host side (srk_tri.cpp) has checked every index before anything is launched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// pack [n_frames][SRK_TRI_PACK] from the frames' inverse poses and intrinsics (K [n_frames][9], or [9] when shared_k)
void srk_launch_tri_pack(hipStream_t s, int32_t n_frames, const double* cam_R, const double* cam_T, const double* K, int shared_k, double* pack);
// The tracks, SRK_TRI_GROUP lanes each.  q NULL = all 1.  refine_attempts 0 = the linear result.  X [n_tracks][3],
// quality [n_tracks][4], status [n_tracks].
void srk_launch_tri_tracks(hipStream_t s, int64_t n_tracks, const int64_t* row_ptr, const int32_t* frame, const double* uv, const double* q,
                           const double* pack, double f0, int32_t refine_attempts, double refine_rel_change, double min_parallax_deg,
                           double* X, double* quality, uint32_t* status);
