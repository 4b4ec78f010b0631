// srk_plan.hpp -- the scene planner: everything srk_ba_upload_scene decides about a scene before a byte reaches the device --
// the internal frame and landmark order, the Schur runs, the long-track items, the derivative tasks, the deterministic-mode
// tables and the fall-back lists.  Host only: no HIP, so the tables can be checked on a machine without a GPU
// (tests/cpp/test_scene_plan.cpp).  srk_ba_host.hip allocates and copies what a plan holds.
#pragma once
#include "srk_limits.hpp"

#include <functional>
#include <stdint.h>
#include <vector>

// the caller's scene, points and cameras already normalised, K expanded to one matrix per frame
struct SrkSceneIn {
    int64_t N;
    int32_t M;
    const int64_t* row_ptr;
    const int32_t* obs_frame;
    const double* obs_uv;
    const double *pts, *camR, *camT, *K;
};

struct SrkPlanOptions {
    bool fixed_k = false, deterministic = false, schur_fp32 = false;
    int jac_mode = -1;         // srk_ba_set_jacobian_mode
    int frame_order_mode = -1; // srk_ba_set_frame_reordering
    const std::vector<int32_t>* frame_order = nullptr; // srk_ba_set_frame_order: M entries, or NULL / empty = none
    bool multi_rank = false;   // shards of one scene: no reordering of its own, no covisibility of its own
    int cus = 256;             // compute units of the device
    int run_split = 0;         // development build: SRK_SCHUR_RUN_SPLIT (0 = the model decides)
    bool no_long = false;      // development build: SRK_SCHUR_NO_LONG
    // relative-pose factors (srk_ba_set_relative_pose_factors): the pairs of frames they tie, caller's numbering, switched-off
    // factors left out.  Edges of the graph the renumbering looks at, and entries of min_cv like a shared landmark.
    const int32_t* rel_a = nullptr;
    const int32_t* rel_b = nullptr;
    int64_t n_rel = 0;
};

// What later calls read of a plan.  The handle (srk_ba) derives from this and keeps it when the tables are on the device.
struct SrkPlanKept {
    // landmarks are stored sorted by frame list (internal order); perm[internal] = caller's pnt_ind
    std::vector<int64_t> perm, row_ptr_user, row_ptr_int;
    // Frames may be stored in another order than the caller's (srk_frame_reorder: unordered image sets, loop
    // closures).  Both empty = the caller's order.  frame_int[caller's frame] = internal index, frame_user = its inverse;
    // obs_rank[caller's observation] = its place inside its landmark's internal (re-sorted) observation list.
    std::vector<int32_t> frame_int, frame_user, obs_rank;
    bool frame_order_supplied = false; // the scene uses the supplied frame order
    std::vector<int64_t> fobs_of;      // two-kernel derivative path only: [internal observation] = its place in the frame-major copy
    std::vector<int32_t> min_cv;       // [M] smallest frame sharing a landmark (or a relative-pose factor) with frame j
    int64_t max_frame_obs = 0;
    int64_t n_cal_list = 0;
    int64_t n_long_items = 0, n_long_runs = 0;
    int64_t n_groups = 0, n_groups_wide = 0, n_groups_mid = 0, n_generic = 0;
    int64_t n_mm_uniform = 0, n_mm_ragged = 0; // runs the MFMA kernel takes (<= SRK_WS_NF_HOST frames), by kind
    bool jac_fused = false; // every 1024-observation workgroup touches < SRK_JF_SLOTS_HOST consecutive frames
    bool jac_runs = false;  // run-based derivative kernel: the tasks are long enough to pay and every workgroup's frame window fits
    bool jac_runs_masked = false; // the tasks are pieces of runs over UNIONS of frame lists (ragged tracks)
    // the derivative kernel's OWN runs (round 4): when a scene holds tracks over more than SRK_GRP_MAXNF_HOST frames the Schur
    // kernels' runs do not cover every landmark; runs over unions of <= 32 frames (one mask word) built for the derivative kernel
    // alone do, as long as no track is longer than that
    bool jr_own_runs = false;
    int32_t jr_tasks = 0, jr_min_nf = 64;
    bool det_active = false; // the scene runs deterministically (every landmark through k_jac_runs / k_schur_mm)
    int32_t ds_n_pairs = 0;
    int long_fb = SRK_LONG_FB_HOST; // frames per block of k_schur_long's pairs: 8, or 16 when the scene has enough of them
};

// + the tables that only travel to the device (srk_dev.hpp describes their layout beside the launchers that read them)
struct SrkScenePlan : SrkPlanKept {
    int32_t g0 = 0, g1 = 1; // internal indices of the caller's frames 0 and 1
    // the scene in the internal order (row_ptr is SrkPlanKept::row_ptr_int)
    std::vector<double> pts, camR, camT, K, obs_uv, fobs_uv;
    std::vector<int64_t> col_ptr, lg_obs_off;
    std::vector<int32_t> obs_frame, obs_pt, fobs_pt, wg_jmin;
    std::vector<int32_t> grp_first, grp_count, grp_nf, grp_frames, gen_list, cal_list, long_cand; // long_cand: tracks too long for grp_*
    std::vector<uint8_t> obs_slot;
    std::vector<uint32_t> pt_mask, jd_mask;
    std::vector<int32_t> lg_item, lg_np, lg_nf, lg_pts, lg_frames, lg_obs;
    std::vector<int32_t> jr_first, jr_count, jr_jmin, jr_group, jd_first, jd_count, jd_nf, jd_frames;
    std::vector<int32_t> dj_ptr, dj_ent, ds_pair_ptr, ds_pair_fa, ds_pair_fb, ds_pair_ent, ds_f_ptr, ds_f_ent;
};

// stage: called with a name after each stage of the work (the upload's SRK_DEBUG=1 trace), may be empty
void srk_plan_scene(const SrkSceneIn& in, const SrkPlanOptions& opt, SrkScenePlan& plan,
                    const std::function<void(const char*)>& stage);

// Returns true and fills to_int[caller's frame] = internal index when renumbering the frames pays.  mode: SrkPlanOptions::frame_order_mode.
// rel_a / rel_b: n_rel more pairs of frames (relative-pose factors) that count as covisible.
bool srk_frame_reorder(int mode, int64_t N, int32_t M, const int64_t* row_ptr, const int32_t* obs_frame, std::vector<int32_t>& to_int,
                       const int32_t* rel_a = nullptr, const int32_t* rel_b = nullptr, int64_t n_rel = 0);

bool srk_debug(); // SRK_DEBUG=1: plan and per-attempt traces on stderr
