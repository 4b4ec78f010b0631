// srk_tri.hpp -- batched triangulation (srk_triangulate_tracks, srk_ba_triangulate), the host half: the
// option defaults, the argument checks, the map of a result out of the normalised coordinates and a walk of one track on the
// host in the kernel's own order of operations.  Host only: no HIP, so all of it can be checked on a machine without a GPU
// (tests/cpp/test_tri_host.cpp).  srk_ba_host.hip allocates and copies; the kernels are in srk_tri.hip.
#pragma once
#include "../../include/srk_ba.h"
#include "srk_limits.hpp"

#include <stdint.h>
#include <string>
#include <vector>

// the options a call runs with: opts NULL = linear only
srk_tri_options srk_tri_effective_options(const srk_tri_options* opts);

// The checks of a call, or the text of its refusal (empty = fine).  Every index the kernel will follow is looked at here.
std::string srk_tri_check(int64_t n_tracks, const int64_t* row_ptr, const int32_t* frame, const double* uv, const double* q, int32_t n_frames,
                          const srk_tri_options* opts);

// frame[o] through the handle's frame order (frame_int[caller's frame] = internal frame, NULL = the same), after srk_tri_check
void srk_tri_map_frames(int64_t n_obs, const int32_t* frame, const int32_t* frame_int, std::vector<int32_t>& out);

// One track on the host, statement for statement what its SRK_TRI_GROUP lanes do on the device (the same deal of the weighted
// observations, the same merge tree, the same refinement loop; only the contraction of multiply-adds may differ).  pack
// [n_frames][SRK_TRI_PACK] from srk_tri_host_pack.  Returns the status bits.
void srk_tri_host_pack(int32_t n_frames, const double* cam_R, const double* cam_T, const double* K, int shared_k, std::vector<double>& pack);
uint32_t srk_tri_host_track(int64_t n_obs, const int32_t* frame, const double* uv, const double* q, const double* pack, double f0,
                            const srk_tri_options& opts, double X[3], double quality[4]);
