// srk_ba_host.hip -- host side of libsrk_ba.so: the C ABI of include/srk_ba.h, the gauge normalisation, the
// device-resident Levenberg-Marquardt loop (two attempt slots: the next damping factor runs speculatively beside the
// current one), the nested-dissection plan of the reduced camera system and the buffer management.
//
// Mirrors whigg/surikatoko cpp_impl/suriko-engine/src/bundle-adj-kanatani.cpp:
//   ComputeInplace :617-718, ComputeOnNormalizedWorld :720-893 (LM control), SceneNormalizer :123-333.
// There is NO CPU fallback: every compute call needs a HIP device and fails loudly (SRK_E_DEVICE) without one.
#include "../../include/srk_ba.h"
#include "srk_dev.hpp"
#include "srk_cov.hpp"
#include "srk_geom.hpp"
#include "srk_plan.hpp"
#include "srk_factors.hpp"
#include "srk_marg.hpp"
#include "srk_marg_dev.hpp"
#include "srk_tri.hpp"
#include "srk_tri_dev.hpp"
#include "srk_tri_math.hpp"
#include "srk_resect.hpp"
#include "srk_resect_dev.hpp"
#include "srk_resect_math.hpp"
#include "srk_align.hpp"
#include "srk_align_dev.hpp"
#include "srk_align_math.hpp"
#include "srk_homog.hpp"
#include "srk_homog_dev.hpp"
#include "srk_homog_math.hpp"
#include "srk_fund.hpp"
#include "srk_fund_dev.hpp"
#include "srk_fund_math.hpp"
#include "srk_locate.hpp"
#include "srk_locate_dev.hpp"
#include "srk_locate_math.hpp"
#include "srk_relate.hpp"
#include "srk_relate_dev.hpp"
#include "srk_relate_math.hpp"
#include "srk_pair.hpp"
#include "srk_pair_dev.hpp"
#include "srk_pair_math.hpp"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <numeric>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <iterator>
#include <map>
#include <memory>
#include <set>
#include <vector>
#include <unordered_set>
#include <thread>

namespace {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

// one event pair around the last launch of a pass (profile level >= 1), created on first use
struct TimedPass { hipEvent_t ev[2]{}; bool timed = false; };
// The factor settings, one struct per family (srk_factors.hpp has the host half): what the setter stored, the snapshot of the last
// upload, the host tables kept from it, the device tables (srk_dev.hpp: SrkLoss, SrkPrior, SrkRelPose, SrkJointPrior) and the
// timed passes.  All counts 0 = none of the family's passes is launched.
struct InfoFamily {
    SrkInfoSetting set;
    bool on = false; // the resident scene runs with it
    enum { Q, QF, NBUF };
    DevBuf buf[NBUF];
};
struct ConstFamily { // section 13
    SrkConstSetting set;
    std::vector<uint8_t> frame_int; // the frames' flags by internal index (SRK_BUF_GRAD, the covariances)
    enum { PTS, FRAMES, NBUF };
    DevBuf buf[NBUF];
    int64_t n_pts = 0;
    int32_t n_frames = 0;
    TimedPass pass[2]; // k_const_points, k_const_frames
};
struct PriorFamily { // section 14
    SrkPriorSetting set;
    SrkPriorApplied app;
    enum { PT_LIST, PT_VAL, FR_LIST, FR_VAL, NBUF };
    DevBuf buf[NBUF];
    int64_t n_pts = 0;
    int32_t n_frames = 0;
    TimedPass pass[2]; // k_prior_add, k_prior_error
};
struct RelPoseFamily { // section 15
    SrkRelPoseSetting set;
    SrkRelPoseApplied app;
    std::vector<int32_t> int_a, int_b; // the internal frames of the active factors (srk_ba_set_covisibility)
    enum { FA, FB, VAL, FR_LIST, FR_PTR, FR_ENT, TGT, CPL, NBUF };
    DevBuf buf[NBUF];
    int32_t n = 0, n_frames = 0;
    TimedPass pass[3]; // k_relpose_add, k_relpose_couple, k_relpose_error
};
struct JPriorFamily { // section 18
    SrkJPriorSetting set;
    SrkJPriorApplied app;
    std::vector<int32_t> pair_a, pair_b; // the coupled pairs (lo, hi) in the internal numbering (srk_ba_set_covisibility)
    enum { PTR, FRAME, LIN, MEAN, IPTR, INFO, PPTR, PSLOT, TGT, FR_LIST, FR_PTR, FR_ENT, BLK, CPL, NBUF };
    DevBuf buf[NBUF];
    int32_t n = 0, n_pairs = 0, n_frames = 0;
    TimedPass pass[3]; // k_jprior_form + k_jprior_add, k_jprior_couple, k_jprior_error
};
static_assert(SRK_RP_PLANES_HOST == SRK_RP_PLANES, "srk_factors.hpp and srk_dev.hpp disagree about the planes of a relative-pose factor");

} // namespace

#define SRK_FUSION_RETRIES 3
#define SRK_SLOTS 3 // attempt slots: two on one GPU (speculative pairs), up to three with several ranks (one damping factor each)
struct srk_ba : SrkPlanKept { // (the base: what the last upload's plan decided, srk_plan.hpp)
    int device = 0;
    int cus = 256; // compute units of the device
    bool own_stream = true;
    std::string last_error;

    // scene
    bool have_scene = false;
    SrkDims d{};
    double f0 = 0;
    srk_ba_normalizer nrm{};
    bool normalized_on_upload = false;

    // device buffers
    DevBuf pts[SRK_SLOTS + 1], camR[SRK_SLOTS + 1], camT[SRK_SLOTS + 1], K, cam[SRK_SLOTS + 1]; // the current scene + one trial scene per attempt slot
    DevBuf pts0, camR0, camT0; // copy of the uploaded (normalised) scene for srk_ba_reset_scene
    DevBuf row_ptr, obs_frame, obs_pt, obs_uv, col_ptr, fobs_pt, fobs_uv;
    DevBuf W, Vg, Ug, scratch;
    int frame_order_mode = -1; // srk_ba_set_frame_reordering: -1 automatic, 0 never, 1 whenever the ordering differs from the caller's
    std::vector<int32_t> frame_order_given; // srk_ba_set_frame_order: the numbering to use (several ranks: the same on every rank)
    DevBuf grp_first, grp_count, grp_nf, grp_frames, obs_slot, pt_mask, gen_list, wg_jmin;
    DevBuf cal_list;      // fixed intrinsics: the landmarks outside the runs k_schur_mm takes (per-landmark kernel)
    // long tracks (more than SRK_GRP_MAXNF_HOST frames): runs over frame-block pairs, k_schur_long
    DevBuf lg_item, lg_np, lg_nf, lg_pts, lg_frames, lg_obs_off, lg_obs;
    DevBuf sc_pts, sc_R, sc_T, sc_K, sc_cam, sc_frame, sc_pt, sc_uv, sc_partial, sc_out; // standalone scoring path
    // run-based Jacobian kernel (k_jac_runs): tasks = pieces of runs of landmarks with identical frame lists
    DevBuf jr_first, jr_count, jr_jmin, jr_group;
    DevBuf jd_nf, jd_frames, jd_mask; // the derivative kernel's OWN runs (SrkPlanKept::jr_own_runs)
    // deterministic mode (srk_ba_set_deterministic; srk_dev.hpp: SrkDetJac / SrkDetSchur): index tables of the ordered second
    // passes and the derivative kernel's staging buffer (the Schur kernel's are per attempt slot)
    bool deterministic = false;       // asked for (takes effect at the next upload)
    DevBuf dj_ptr, dj_ent, dj_stage, ds_pair_ptr, ds_pair_fa, ds_pair_fb, ds_pair_ent, ds_f_ptr, ds_f_ent;
    int jac_mode = -1;      // -1 = automatic, 0 = never k_jac_runs, 1 = whenever possible (srk_ba_set_jacobian_mode)
    // skyline of the reduced camera system (see k_env_zero): host + device copies
    std::vector<int64_t> env_col_h, env_off_h, row_end_h, col_begin_h;
    DevBuf env_col, env_off, band_col, band_off;
    int64_t env_packed = 0, band_packed = 0; // doubles inside the factorisation skyline / the pre-factorisation band
    bool use_envelope = true;
    // chunked solve of a banded system (srk_chol.hip): plan + its buffers
    bool use_chunks = true;
    // Everything one LM attempt writes lives in an attempt slot: the reduced camera system and its solver plan, the
    // corrections, the trial scene, the status words, and the stream it runs on.  Two slots let the loop run the next
    // damping factor speculatively beside the current one (the solve is a latency chain that leaves the chip idle).
    struct Attempt {
        DevBuf S, rhs, wy, dc, acc, dx, err_partial, info, dinv, packed, sync_flags;
        DevBuf irr; // [0] count + landmarks the SYRK form of k_schur_mm hands back to the per-landmark inverse path
        DevBuf det_stage, det_rhs; // deterministic mode: the runs' staged sums (SrkDetSchur)
        DevBuf Ssh, rsh, ysh, dcsh, dinvsh, Tsh; // shared intrinsics: the folded system P^T S P, its rhs, solve scratch, P^T dc
        SrkChunkPlan plan;
        SrkCholSync sync;            // in-launch hand-offs of the fused outer-step kernel (srk_chol.hip: k_step256)
        std::vector<DevBuf> plan_bufs;
        std::vector<char> plan_zeroed;   // plan_bufs[i] is a matrix / vector that must be zero outside what a solve writes
        std::vector<std::unique_ptr<SrkChunkPlan>> plan_children; // plans of the nested separator systems
        std::vector<int64_t> plan_sig;   // what the plan was built for (build_chunk_plan keeps it when the next scene's skyline is the same)
        SrkSolveProf solve_prof;     // event pairs / flops of the last profiled solve
        double* host_back = nullptr; // pinned: {error, solver info, point-update info} of one attempt
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
        hipEvent_t ev_a = nullptr, ev_b = nullptr; // cross-stream hand-offs of the damping-parallel schedule
        double* err_dst = nullptr;   // {error, solver info, point-update info} of this slot: 8 doubles inside srk_ba::status_all
        int trial = 1;               // index of this slot's trial scene buffers
        int slot = 0;                // its index in att (slot 1's all-reduces take comm2 when there is one: exchange)
        bool allocated = false;
    };
    Attempt att[SRK_SLOTS];
    hipStream_t main_stream = nullptr; // = att[0].stream
    hipEvent_t ev_jac = nullptr;       // derivatives done (the second slot's stream waits for it)
    bool speculate = true;             // single rank, instrumentation off: run two damping factors side by side
    int cur = 0; // index of the current scene buffers

    // multi-GPU exchange
    srk_allreduce_fn allreduce = nullptr;
    void* allreduce_ctx = nullptr;
    int rank = 0, world = 1;
    // native exchange: RCCL (librccl.so, loaded on first use) all-reduces on the stream of the attempt that needs them --
    // no host round trip, no Python.  comm_owned: created by srk_ba_rccl_init (destroyed with the handle).
    ncclComm_t comm = nullptr;
    bool comm_owned = false;
    // a second communicator for the second attempt slot (srk_ba_rccl_init_second): with it the speculative pairs stay on
    // with several ranks -- each slot's all-reduces run on its own stream AND its own communicator, so the two slots'
    // collectives never share a communicator's queue.  Without it (or with the all-reduce callback, which blocks the
    // host) pairs stay on as well when spec_multi allows: the callback serialises the exchanges on the host.
    ncclComm_t comm2 = nullptr;
    bool spec_multi = true; // SRK_MULTI_SPECULATION=0: one attempt at a time with several ranks
    // Damping-parallel schedule (world >= 2): an iteration's attempts c, 10c, 100c are built by every rank on its
    // shard, band k is REDUCED to rank k, rank k solves factor k and broadcasts its corrections, every rank scores all of
    // them.  All collectives of that schedule go through ONE communicator on ONE stream (comm_stream) in one program order.
    bool dp_schedule = true;          // srk_ba_set_multi_schedule(h, 0): the round-2 schedule (all-reduce, redundant solves)
    bool dp_force = false;            // srk_ba_set_multi_schedule(h, 2): the schedule at world size 1 as well (three slots, every
                                      // collective issued; all one GPU can rehearse of the native path)
    // The native form of that schedule (groups of ncclReduce / ncclBroadcast rooted at different ranks on one communicator)
    // has never run on more than one GPU in this repository's tests: its FIRST round on a handle checks itself against plain
    // all-reduces of checksums (dp_selfcheck below); a mismatch or an RCCL error switches the handle to the all-reduce schedule.
    bool dp_verified = false;         // the first native round passed its self-check
    bool dp_selfcheck_failed = false; // ... or did not: the handle runs the all-reduce schedule (srk_ba_multi_schedule: 3)
    DevBuf dp_chk;                    // scratch of the self-check: [512] partial sums, [2] checksum, [16] all-reduce staging
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_comm = nullptr;
    DevBuf status_all;                // [SRK_SLOTS][8] doubles: the slots' {error, solver info, point-update info}
    double* dp_back = nullptr;        // pinned copy of status_all
    int64_t seen_global = -1; // observation count over all ranks of the uploaded scene (-1 = not yet exchanged)

    // timing
    hipEvent_t ev[16]{};
    std::vector<hipEvent_t> chol_ev;
    bool schur_fp32 = false; // opt-in mixed precision: fp32 run sums in the grouped Schur kernel
    bool store_f32 = false;  // opt-in: the point-frame blocks W are STORED as float (next upload); arithmetic stays fp64
    bool fixed_k = false;    // opt-in: calibrated BA, six pose variables per frame (next upload; srk_ba_set_fixed_intrinsics)
    // opt-in: shared intrinsics (srk_ba_set_intrinsic_groups, next upload).  igroup_user[caller's frame]
    // = group, empty = off.  The uploaded scene: shk_G groups (0 = off), every scene buffer set with its own K (Ks[w]: the
    // trial K of an attempt lives with its trial scene), the frames' groups and members in the internal order
    std::vector<int32_t> igroup_user;
    int32_t igroup_n = 0;
    int32_t shk_G = 0;
    int64_t shk_ncols = 0, shk_ldb = 0;
    DevBuf Ks[SRK_SLOTS + 1], shk_grp, shk_lo, shk_hi, shk_mptr, shk_mem, shk_env;
    std::vector<int32_t> shk_grp_h, shk_first; // [M] group of each internal frame; [G] the first internal frame of each group
    // the closed-form frame derivatives are those of the error only when K(2,2) = f0: with groups the
    // device K of frame j is the caller's K times f0 / K(2,2) (the same projections); shk_k22_user[j] = the caller's K(2,2)
    std::vector<double> shk_k22_user;
    std::vector<int64_t> shk_row_end, shk_col_begin; // skyline of the compact pose system (host, for the solve)
    int loss_kind = SRK_LOSS_NONE; // opt-in: robust loss (srk_ba_set_robust_loss); takes effect at the next optimise / phase call
    double loss_delta_pix = 0;     // its scale in pixels; the kernels get delta / f0 (robust_loss below)
    // opt-in: the factor settings, each kept across uploads and srk_ba_reset_scene and applied by the next upload
    InfoFamily obs_info;
    ConstFamily cst;
    PriorFamily pri;
    RelPoseFamily rp;
    JPriorFamily jp;
    SrkFactorSelection sel; // what the last upload switched on of them (the planner has seen sel.rel_a / rel_b)
    int profile_level = 0; // 0 = no events, 1 = phase events (report.ms_*), 2 = + event pairs around the MFMA updates
    bool chol_fused = true; // the solve's outer steps as one launch each (k_step256); srk_ba_set_solver_fusion
    // what the caller asked for.  A hand-off timeout switches chol_fused off for the rest of that call; the next upload /
    // optimise call switches it back on (a timeout is a scheduling event: another process on the GPU, a debugger) until the
    // handle has seen SRK_FUSION_RETRIES of them -- then the unfused sequence stays, and srk_ba_solver_sync_timeouts says so.
    bool chol_fused_wanted = true;
    int fusion_rearms_left = 3; // SRK_FUSION_RETRIES
    int64_t sync_timeouts = 0; // solves repeated with the unfused kernels after a hand-off timed out
    struct IterLog { int32_t attempts; double ms, err, factor; };
    std::vector<IterLog> iter_log; // the accepted iterations of the last optimise call (srk_ba_iteration_log)
    int last_slot = 0;     // attempt slot of the last judged attempt (what SRK_BUF_RCS / RHS / CORRECTIONS download)
    double last_hessian_factor = 0;
    bool lean_resets = false; // srk_ba_optimize: no per-attempt memsets (see phase_solve)
    // A failed factorisation (non-positive / non-finite pivot) leaves NaNs in the slot's system and chunk matrices, also
    // OUTSIDE the parts the next attempt rewrites (k_panel's dead rows: 0 * NaN).  The flag makes the next entry point
    // re-zero every slot's system and plan buffers (clear_poison) before anything is computed from them.
    bool poisoned = false;
    // marginal covariances (srk_ba_phase_covariance): the right-hand sides Y of the forward substitution and
    // the small tables of a call, grown lazily; cov_batch_cols: srk_ba_set_covariance_batch (0 = as many columns as fit 256 MB);
    // cov_pt_frame0: the first internal frame of every internal landmark, fetched at the first call after an upload
    DevBuf cov_Y, cov_grp, cov_blk, cov_out, cov_free, cov_colb;
    DevBuf cov_pairs; // the pair table of a batch of cross-covariances (section 17)
    int64_t cov_batch_cols = 0;
    std::vector<int32_t> cov_pt_frame0;
    // marginalisation priors (srk_ba_marginalization_prior): the tables of a call's plan, the dense strip Z,
    // the observations' staging rows, the chunks' partial Gram products and the result, grown lazily; two event pairs (the strip
    // and the frames' sums; the Gram product and its reduction), created at the first call; mg_obs_frame: the frames of the
    // observations in the internal order, fetched at the first call after an upload
    enum { MG_LM, MG_LM_STAGE, MG_LM_PRIOR, MG_FRAME_SLOT, MG_SLOT_PTR, MG_SLOT_ENT, MG_Z, MG_STAGE, MG_SKIP, MG_US, MG_PART, MG_OUT, MG_NBUF };
    DevBuf mg[MG_NBUF];
    hipEvent_t mg_ev[4]{};
    std::vector<int32_t> mg_obs_frame;
    // batched triangulation (srk_triangulate_tracks, srk_ba_triangulate): the tracks, the caller's poses, the
    // frames' packs and the results of a call, grown lazily
    enum { TRI_ROW, TRI_FRAME, TRI_UV, TRI_Q, TRI_R, TRI_T, TRI_K, TRI_PACK, TRI_X, TRI_QUAL, TRI_STATUS, TRI_NBUF };
    DevBuf tri[TRI_NBUF];
    hipEvent_t tri_ev[2]{}; // around the two kernels of a call, created at the first call
    double tri_ms = 0;      // their device time in the last call (srk_ba_triangulate_kernel_ms)
    // batched camera resection (srk_resect_frames, srk_ba_resect): the frames' observations, the caller's
    // landmarks, intrinsics and start poses, the packs and the results, grown lazily
    enum { RS_ROW, RS_POINT, RS_UV, RS_Q, RS_X, RS_K, RS_R0, RS_T0, RS_PACK, RS_R, RS_T, RS_QUAL, RS_INFO, RS_STATUS, RS_W, RS_NBUF };
    DevBuf rs[RS_NBUF];
    hipEvent_t rs_ev[2]{}; // around the two kernels of a call, created at the first call
    double rs_ms = 0;      // their device time in the last call (srk_ba_resect_kernel_ms)
    // resection without a start pose (srk_locate_frames, srk_ba_locate): the gathered strip, the frames'
    // weighted counts, the waves' slots and the located outputs, grown lazily.  The observations, intrinsics and every buffer of
    // the refinement are the resection's (rs): the located poses are written into RS_R0 / RS_T0, where its kernels read their starts
    enum { LC_STRIP, LC_COUNT, LC_SLOTS, LC_LOCATED, LC_LSTATUS, LC_INL, LC_NBUF };
    DevBuf lc[LC_NBUF];
    hipEvent_t lc_ev[4]{};           // the call, and the hypothesis-and-score kernel inside it; created at the first call
    double lc_ms = 0, lc_score_ms = 0; // srk_ba_locate_kernel_ms, srk_ba_locate_score_ms
    // two-view relative pose (srk_relate_frames): the pairs' matches and intrinsics, the gathered strip, the
    // pairs' weighted counts, the hypotheses' records, the waves' slots and the outputs, grown lazily
    enum { RL_ROW, RL_UVA, RL_UVB, RL_Q, RL_KA, RL_KB, RL_STRIP, RL_COUNT, RL_HYP, RL_SLOTS, RL_R, RL_T, RL_E, RL_RELATED, RL_STATUS, RL_INL, RL_NBUF };
    DevBuf rl[RL_NBUF];
    hipEvent_t rl_ev[4]{};           // the call, and the score kernel inside it; created at the first call
    double rl_ms = 0, rl_score_ms = 0; // srk_ba_relate_kernel_ms, srk_ba_relate_score_ms
    // map alignment (srk_align_points, srk_ba_align): the sets' correspondences, the gathered strip, the sets'
    // weighted counts, the waves' slots and the outputs, grown lazily
    enum { AL_ROW, AL_POINT, AL_A, AL_B, AL_Q, AL_STRIP, AL_COUNT, AL_SLOTS, AL_S, AL_R, AL_T, AL_ALIGNED, AL_STATUS, AL_INL, AL_NBUF };
    DevBuf al[AL_NBUF];
    hipEvent_t al_ev[4]{};           // the call, and the hypothesis-and-score kernel inside it; created at the first call
    double al_ms = 0, al_score_ms = 0; // srk_ba_align_kernel_ms, srk_ba_align_score_ms
    // two-view pose refinement (srk_refine_pairs, srk_relate_frames_refined): the pairs' matches, intrinsics
    // and start poses of srk_refine_pairs (the chained call reads relate's buffers instead), the inverses of K, the product of q
    // with the inlier flags and the outputs, grown lazily
    enum { PR_ROW, PR_UVA, PR_UVB, PR_Q, PR_KA, PR_KB, PR_R0, PR_T0, PR_KINV, PR_QE, PR_R, PR_T, PR_E, PR_QUAL, PR_INFO, PR_BASIS, PR_STATUS, PR_W, PR_NBUF };
    DevBuf pr[PR_NBUF];
    hipEvent_t pr_ev[2]{}; // around the refinement's kernels, created at the first call
    double pr_ms = 0;      // their device time in the last call (srk_ba_pair_kernel_ms)
    // two-view homography (srk_relate_homography): the pairs' matches and intrinsics, the gathered strip, the
    // pairs' weighted counts, the waves' slots and the outputs, grown lazily
    enum { HG_ROW, HG_UVA, HG_UVB, HG_Q, HG_KA, HG_KB, HG_STRIP, HG_COUNT, HG_SLOTS, HG_G, HG_H, HG_POSES, HG_R, HG_T, HG_N, HG_FRONT, HG_HOMOG, HG_STATUS, HG_INL, HG_NBUF };
    DevBuf hg[HG_NBUF];
    hipEvent_t hg_ev[4]{};           // the call, and the hypothesis-and-score kernel inside it; created at the first call
    double hg_ms = 0, hg_score_ms = 0; // srk_ba_homography_kernel_ms, srk_ba_homography_score_ms
    // two-view fundamental matrix (srk_relate_uncalibrated): the pairs' matches, the gathered strip, the pairs'
    // weighted counts, the hypotheses' records, the waves' slots and the outputs, grown lazily
    enum { FD_ROW, FD_UVA, FD_UVB, FD_Q, FD_STRIP, FD_COUNT, FD_HYP, FD_SLOTS, FD_F, FD_U, FD_V, FD_SIGMA, FD_FUND, FD_INFO, FD_STATUS, FD_INL, FD_NBUF };
    DevBuf fd[FD_NBUF];
    hipEvent_t fd_ev[5]{};           // the call, the score kernel and the solve kernel inside it; created at the first call
    double fd_ms = 0, fd_score_ms = 0, fd_solve_ms = 0; // srk_ba_fundamental_kernel_ms, _score_ms, _solve_ms
};

// librccl.so is opened on first use: the library itself carries no link-time dependency on it (a single-GPU caller
// never needs it), and a Python caller keeps torch's own copy to itself
namespace {
struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
    bool rooted = false; // Reduce / Broadcast / GroupStart / GroupEnd resolved (else they are emulated by all-reduces)
};
RcclApi& rccl()
{
    static RcclApi api = [] {
        RcclApi a;
        const char* names[] = { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" };
        for (const char* n : names)
            if ((a.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL)) != nullptr) break;
        if (!a.lib) return a;
        a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(a.lib, "ncclGetUniqueId"));
        a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(a.lib, "ncclCommInitRank"));
        a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(a.lib, "ncclCommDestroy"));
        a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(dlsym(a.lib, "ncclAllReduce"));
        a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(a.lib, "ncclGetErrorString"));
        a.Reduce = reinterpret_cast<decltype(a.Reduce)>(dlsym(a.lib, "ncclReduce"));
        a.Broadcast = reinterpret_cast<decltype(a.Broadcast)>(dlsym(a.lib, "ncclBroadcast"));
        a.GroupStart = reinterpret_cast<decltype(a.GroupStart)>(dlsym(a.lib, "ncclGroupStart"));
        a.GroupEnd = reinterpret_cast<decltype(a.GroupEnd)>(dlsym(a.lib, "ncclGroupEnd"));
        a.rooted = a.Reduce && a.Broadcast && a.GroupStart && a.GroupEnd;
        a.ok = a.GetUniqueId && a.CommInitRank && a.CommDestroy && a.AllReduce && a.GetErrorString;
        return a;
    }();
    return api;
}
} // namespace

#define HIPCHK(h, expr)                                                                              \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess) {                                                                      \
            (h)->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);                     \
            return SRK_E_DEVICE;                                                                     \
        }                                                                                            \
    } while (0)

static int dev_alloc(srk_ba* h, DevBuf& b, size_t bytes)
{
    if (bytes == 0) bytes = 8;
    if (b.p && b.bytes >= bytes) return SRK_OK;
    if (b.p) {
        hipFree(b.p);
        b.p = nullptr;
        b.bytes = 0;
    }
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) {
        h->last_error = std::string("hipMalloc: ") + hipGetErrorString(e);
        b.p = nullptr;
        return e == hipErrorOutOfMemory ? SRK_E_NOMEM : SRK_E_DEVICE;
    }
    b.bytes = bytes;
    return SRK_OK;
}
static void dev_free(DevBuf& b)
{
    if (b.p) hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}
static void release(DevBuf* b, int nb, TimedPass* p, int np) // the device tables and event pairs of a family of factor settings
{
    for (int i = 0; i < nb; ++i) dev_free(b[i]);
    for (int k = 0; k < np; ++k)
        for (hipEvent_t& e : p[k].ev)
            if (e) hipEventDestroy(e);
}
template <typename T> static T* P(const DevBuf& b) { return reinterpret_cast<T*>(b.p); }

extern "C" {

int srk_ba_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

srk_ba* srk_ba_create(int device_id)
{
    int n = srk_ba_device_count();
    if (n <= 0 || device_id < 0 || device_id >= n) {
        fprintf(stderr, "srk_ba_create: no usable HIP device (count=%d, requested=%d); there is no CPU fallback\n", n,
                device_id);
        return nullptr;
    }
    if (hipSetDevice(device_id) != hipSuccess) return nullptr;
    srk_ba* h = new srk_ba();
    h->device = device_id;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0) h->cus = prop.multiProcessorCount;
    if (hipStreamCreate(&h->main_stream) != hipSuccess) {
        delete h;
        return nullptr;
    }
#ifdef SRK_DEV // development switches (tools/): the default build reads no environment but SRK_DEBUG (the trace)
    if (const char* e = getenv("SRK_CHOL_FUSED")) h->chol_fused = h->chol_fused_wanted = e[0] != '0'; // the unfused launch sequence
    if (const char* e = getenv("SRK_MULTI_SPECULATION")) h->spec_multi = e[0] != '0';
    if (const char* e = getenv("SRK_MULTI_SCHEDULE")) {
        h->dp_schedule = std::strcmp(e, "allreduce") != 0;
        h->dp_force = std::strcmp(e, "dp_force") == 0;
    }
#endif
    h->att[0].stream = h->main_stream;
    bool ok = hipEventCreateWithFlags(&h->ev_jac, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&h->ev_comm, hipEventDisableTiming) == hipSuccess &&
              hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking) == hipSuccess &&
              hipHostMalloc(reinterpret_cast<void**>(&h->dp_back), 64 * SRK_SLOTS, hipHostMallocDefault) == hipSuccess &&
              hipMalloc(&h->status_all.p, 64 * SRK_SLOTS) == hipSuccess;
    if (ok) h->status_all.bytes = 64 * SRK_SLOTS, ok = hipMemset(h->status_all.p, 0, 64 * SRK_SLOTS) == hipSuccess;
    for (int sl = 0; sl < SRK_SLOTS; ++sl) {
        auto& a = h->att[sl];
        a.slot = sl;
        a.trial = sl + 1;
        a.err_dst = ok ? P<double>(h->status_all) + 8 * sl : nullptr;
        if (sl > 0) ok = ok && hipStreamCreateWithFlags(&a.stream, hipStreamNonBlocking) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&a.done, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&a.ev_a, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&a.ev_b, hipEventDisableTiming) == hipSuccess &&
             hipHostMalloc(reinterpret_cast<void**>(&a.host_back), 64, hipHostMallocDefault) == hipSuccess;
    }
    for (auto& e : h->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    if (!ok) {
        delete h;
        return nullptr;
    }
    return h;
}

void srk_ba_destroy(srk_ba* h)
{
    if (!h) return;
    hipSetDevice(h->device);
    if (h->main_stream) hipStreamSynchronize(h->main_stream);
    for (int sl = 1; sl < SRK_SLOTS; ++sl)
        if (h->att[sl].stream) hipStreamSynchronize(h->att[sl].stream);
    if (h->comm_stream) hipStreamSynchronize(h->comm_stream);
    if (h->comm2) rccl().CommDestroy(h->comm2); // the second slot's communicator is always owned by the handle
    if (h->comm && h->comm_owned) rccl().CommDestroy(h->comm);
    h->comm = h->comm2 = nullptr;
    for (int w = 0; w < SRK_SLOTS + 1; ++w)
        for (DevBuf* b : { &h->pts[w], &h->camR[w], &h->camT[w], &h->cam[w], &h->Ks[w] }) dev_free(*b);
    dev_free(h->status_all);
    if (h->dp_back) hipHostFree(h->dp_back);
    DevBuf* all[] = { &h->K, &h->pts0, &h->camR0, &h->camT0, &h->row_ptr,
                      &h->obs_frame, &h->obs_pt, &h->obs_uv, &h->col_ptr, &h->fobs_pt, &h->fobs_uv, &h->W, &h->Vg, &h->Ug,
                      &h->scratch, &h->grp_first, &h->grp_count, &h->grp_nf, &h->grp_frames, &h->obs_slot, &h->pt_mask,
                      &h->gen_list, &h->cal_list, &h->env_col, &h->env_off, &h->wg_jmin, &h->band_col, &h->band_off,
                      &h->dj_ptr, &h->dj_ent, &h->dj_stage, &h->ds_pair_ptr, &h->ds_pair_fa, &h->ds_pair_fb, &h->ds_pair_ent, &h->ds_f_ptr, &h->ds_f_ent,
                      &h->jd_nf, &h->jd_frames, &h->jd_mask,
                      &h->jr_first, &h->jr_count, &h->jr_jmin, &h->jr_group, &h->lg_item, &h->lg_np, &h->lg_nf, &h->lg_pts, &h->lg_frames,
                      &h->lg_obs_off, &h->lg_obs, &h->shk_grp, &h->shk_lo, &h->shk_hi, &h->shk_mptr, &h->shk_mem, &h->shk_env, &h->dp_chk,
                      &h->cov_Y, &h->cov_grp, &h->cov_blk, &h->cov_out, &h->cov_free, &h->cov_colb, &h->cov_pairs };
    for (DevBuf* b : all) dev_free(*b);
    for (DevBuf& b : h->mg) dev_free(b);
    for (DevBuf& b : h->tri) dev_free(b);
    for (DevBuf& b : h->rs) dev_free(b);
    for (DevBuf& b : h->lc) dev_free(b);
    for (DevBuf& b : h->rl) dev_free(b);
    for (DevBuf& b : h->al) dev_free(b);
    for (DevBuf& b : h->pr) dev_free(b);
    for (DevBuf& b : h->hg) dev_free(b);
    for (hipEvent_t& e : h->hg_ev)
        if (e) hipEventDestroy(e);
    for (DevBuf& b : h->fd) dev_free(b);
    for (hipEvent_t& e : h->fd_ev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t& e : h->pr_ev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t& e : h->al_ev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t& e : h->rl_ev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t& e : h->lc_ev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t& e : h->rs_ev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t& e : h->tri_ev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t& e : h->mg_ev)
        if (e) hipEventDestroy(e);
    for (auto& a : h->att) {
        for (DevBuf* b : { &a.S, &a.rhs, &a.wy, &a.dc, &a.acc, &a.dx, &a.err_partial, &a.info, &a.dinv, &a.packed, &a.sync_flags, &a.irr, &a.det_stage, &a.det_rhs,
                          &a.Ssh, &a.rsh, &a.ysh, &a.dcsh, &a.dinvsh, &a.Tsh }) dev_free(*b);
        for (DevBuf& b : a.plan_bufs) dev_free(b);
        if (a.host_back) hipHostFree(a.host_back);
        if (a.done) hipEventDestroy(a.done);
        if (a.ev_a) hipEventDestroy(a.ev_a);
        if (a.ev_b) hipEventDestroy(a.ev_b);
    }
    for (DevBuf* b : { &h->sc_pts, &h->sc_R, &h->sc_T, &h->sc_K, &h->sc_cam, &h->sc_frame, &h->sc_pt, &h->sc_uv, &h->sc_partial, &h->sc_out })
        dev_free(*b);
    for (auto& e : h->ev)
        if (e) hipEventDestroy(e);
    for (auto& e : h->chol_ev) hipEventDestroy(e);
    if (h->ev_jac) hipEventDestroy(h->ev_jac);
    release(h->obs_info.buf, InfoFamily::NBUF, nullptr, 0);
    release(h->cst.buf, ConstFamily::NBUF, h->cst.pass, 2);
    release(h->pri.buf, PriorFamily::NBUF, h->pri.pass, 2);
    release(h->rp.buf, RelPoseFamily::NBUF, h->rp.pass, 3);
    release(h->jp.buf, JPriorFamily::NBUF, h->jp.pass, 3);
    if (h->ev_comm) hipEventDestroy(h->ev_comm);
    if (h->comm_stream) hipStreamDestroy(h->comm_stream);
    for (int sl = 1; sl < SRK_SLOTS; ++sl)
        if (h->att[sl].stream) hipStreamDestroy(h->att[sl].stream);
    if (h->own_stream && h->main_stream) hipStreamDestroy(h->main_stream);
    delete h;
}

const char* srk_ba_last_error(const srk_ba* h) { return h ? h->last_error.c_str() : "null handle"; }

const char* srk_ba_status_string(int status)
{
    switch (status) {
    case SRK_STATUS_ABS_ERR_THRESHOLD: return "abs err threshold";
    case SRK_STATUS_SMALL_ERR_CHANGE: return "small relative err change";
    case SRK_STATUS_HESSIAN_OVERFLOW: return "hessian overflow";
    case SRK_STATUS_ERR_CONVERGED: return "err converged to limit value";
    case SRK_STATUS_MAX_ITERATIONS: return "max iterations";
    case SRK_STATUS_DEVICE_ERROR: return "device error";
    default: return "";
    }
}

int srk_ba_set_stream(srk_ba* h, void* hip_stream)
{
    if (!h) return SRK_E_ARGS;
    hipSetDevice(h->device);
    if (h->main_stream) hipStreamSynchronize(h->main_stream);
    if (h->own_stream && h->main_stream) hipStreamDestroy(h->main_stream);
    h->main_stream = h->att[0].stream = reinterpret_cast<hipStream_t>(hip_stream);
    h->own_stream = false;
    return SRK_OK;
}

// landmark shards must agree on the frame numbering: each rank's own renumbering (made from its shard at upload) would not
static bool exchange_after_reordered_upload(srk_ba* h, int world_size)
{
    if (world_size < 2 || !h->have_scene || h->frame_int.empty() || h->frame_order_supplied) return false;
    h->last_error = "the uploaded scene's frames were renumbered for one rank; configure the exchange before the upload";
    return true;
}

// fixed intrinsics (srk_ba_set_fixed_intrinsics) are built for one rank, fp64 storage and fp64 Schur sums, not deterministic
// mode: the combination is refused by whichever call makes it (a setter, or the upload).  Returns the text, or NULL when fine.
static const char* fixed_k_conflict(bool fixed_k, bool deterministic, bool store_f32, bool schur_fp32, int world)
{
    if (!fixed_k) return nullptr;
    if (deterministic) return "fixed intrinsics: not available in deterministic mode";
    if (store_f32) return "fixed intrinsics: not available with f32 storage of the point-frame blocks";
    if (schur_fp32) return "fixed intrinsics: not available with fp32 Schur accumulation";
    if (world > 1) return "fixed intrinsics: not available with more than one rank";
    return nullptr;
}
// shared intrinsics (srk_ba_set_intrinsic_groups) extend the 10-variable fp64 system of one rank: refused in the same way
static const char* groups_conflict(bool groups, bool fixed_k, bool store_f32, bool schur_fp32, int world)
{
    if (!groups) return nullptr;
    if (fixed_k) return "intrinsic groups: not available with fixed intrinsics";
    if (store_f32) return "intrinsic groups: not available with f32 storage of the point-frame blocks";
    if (schur_fp32) return "intrinsic groups: not available with fp32 Schur accumulation";
    if (world > 1) return "intrinsic groups: not available with more than one rank";
    return nullptr;
}
static bool refuse_modes(srk_ba* h, bool fixed_k, bool deterministic, bool store_f32, bool schur_fp32, int world, bool groups)
{
    const char* c = fixed_k_conflict(fixed_k, deterministic, store_f32, schur_fp32, world);
    if (!c) c = groups_conflict(groups, fixed_k, store_f32, schur_fp32, world);
    std::string e = c ? c : "";
    if (e.empty()) e = srk_setting_conflict("constant blocks", h->cst.set.set, groups, world);
    if (e.empty()) e = srk_setting_conflict("position priors", h->pri.set.set, groups, world);
    if (e.empty()) e = srk_setting_conflict("relative-pose factors", h->rp.set.set, groups, world);
    if (e.empty()) e = srk_setting_conflict("joint pose priors", h->jp.set.set, groups, world);
    if (!e.empty()) h->last_error = e;
    return !e.empty();
}

int srk_ba_set_allreduce(srk_ba* h, srk_allreduce_fn fn, void* ctx, int rank, int world_size)
{
    if (!h || world_size < 1 || rank < 0 || rank >= world_size) return SRK_E_ARGS;
    if (refuse_modes(h, h->fixed_k, h->deterministic, h->store_f32, h->schur_fp32, world_size, !h->igroup_user.empty())) return SRK_E_ARGS;
    if (exchange_after_reordered_upload(h, world_size)) return SRK_E_STATE;
    // either exchange replaces the other: exchange() prefers a communicator, so a callback set after srk_ba_rccl_init
    // would never be called unless the communicators are detached here
    if (h->comm || h->comm2) {
        hipSetDevice(h->device);
        if (h->main_stream) hipStreamSynchronize(h->main_stream);
        for (int sl = 1; sl < SRK_SLOTS; ++sl)
            if (h->att[sl].stream) hipStreamSynchronize(h->att[sl].stream);
        if (h->comm_stream) hipStreamSynchronize(h->comm_stream);
        if (h->comm2) rccl().CommDestroy(h->comm2);
        if (h->comm && h->comm_owned) rccl().CommDestroy(h->comm);
        h->comm = h->comm2 = nullptr;
        h->comm_owned = false;
    }
    h->allreduce = fn;
    h->allreduce_ctx = ctx;
    h->rank = rank;
    h->world = world_size;
    h->seen_global = -1;
    return SRK_OK;
}

// ---- native RCCL exchange
int srk_ba_rccl_get_unique_id(void* id128)
{
    if (!id128 || !rccl().ok) return SRK_E_DEVICE;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId");
    return rccl().GetUniqueId(reinterpret_cast<ncclUniqueId*>(id128)) == ncclSuccess ? SRK_OK : SRK_E_DEVICE;
}
static int rccl_attach(srk_ba* h, ncclComm_t comm, bool owned, int rank, int world_size)
{
    if (refuse_modes(h, h->fixed_k, h->deterministic, h->store_f32, h->schur_fp32, world_size, !h->igroup_user.empty())) {
        if (owned) rccl().CommDestroy(comm);
        return SRK_E_ARGS;
    }
    if (exchange_after_reordered_upload(h, world_size)) {
        if (owned) rccl().CommDestroy(comm);
        return SRK_E_STATE;
    }
    if (h->comm && h->comm_owned) rccl().CommDestroy(h->comm);
    if (h->comm2) rccl().CommDestroy(h->comm2);
    h->comm2 = nullptr;
    h->comm = comm;
    h->comm_owned = owned;
    h->allreduce = nullptr;
    h->allreduce_ctx = nullptr;
    h->rank = rank;
    h->world = world_size;
    h->seen_global = -1;
    return SRK_OK;
}
int srk_ba_rccl_init(srk_ba* h, const void* id128, int rank, int world_size)
{
    if (!h || !id128 || world_size < 1 || rank < 0 || rank >= world_size) return SRK_E_ARGS;
    if (!rccl().ok) { h->last_error = "librccl.so could not be loaded"; return SRK_E_DEVICE; }
    HIPCHK(h, hipSetDevice(h->device));
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof id);
    ncclComm_t comm = nullptr;
    ncclResult_t r = rccl().CommInitRank(&comm, world_size, id, rank);
    if (r != ncclSuccess) { h->last_error = std::string("ncclCommInitRank: ") + rccl().GetErrorString(r); return SRK_E_DEVICE; }
    return rccl_attach(h, comm, true, rank, world_size);
}
// collective, after srk_ba_rccl_init: a second communicator (its own ncclUniqueId) for the second attempt slot
int srk_ba_rccl_init_second(srk_ba* h, const void* id128)
{
    if (!h || !id128) return SRK_E_ARGS;
    if (!h->comm || !rccl().ok) { h->last_error = "srk_ba_rccl_init_second: srk_ba_rccl_init comes first"; return SRK_E_STATE; }
    HIPCHK(h, hipSetDevice(h->device));
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof id);
    ncclComm_t comm = nullptr;
    ncclResult_t r = rccl().CommInitRank(&comm, h->world, id, h->rank);
    if (r != ncclSuccess) { h->last_error = std::string("ncclCommInitRank (second): ") + rccl().GetErrorString(r); return SRK_E_DEVICE; }
    if (h->comm2) rccl().CommDestroy(h->comm2);
    h->comm2 = comm;
    return SRK_OK;
}
int srk_ba_rccl_set_comm(srk_ba* h, void* nccl_comm, int rank, int world_size)
{
    if (!h || world_size < 1 || rank < 0 || rank >= world_size) return SRK_E_ARGS;
    if (nccl_comm && !rccl().ok) { h->last_error = "librccl.so could not be loaded"; return SRK_E_DEVICE; }
    return rccl_attach(h, reinterpret_cast<ncclComm_t>(nccl_comm), false, rank, world_size);
}

// ------------------------------------------------------------------ host normalisation (bundle-adj-kanatani.cpp:123-333)

int srk_ba_check_world_is_normalized(int32_t M, const double* cam_R, const double* cam_T, double t1y, int32_t comp)
{
    if (M < 2 || !cam_R || !cam_T || comp < 0 || comp > 2) return 0; // :291-292
    const double atol = 1e-3;                                           // :297
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            if (!srk::is_close(r == c ? 1.0 : 0.0, cam_R[3 * r + c], atol, atol)) return 0; // :299 IsIdentity
    if (srk::norm3(cam_T) >= atol) return 0;                                                  // :308-309
    double Ri[9], Ti[3];
    srk::se3_inv(cam_R + 9, cam_T + 3, Ri, Ti);                                               // :320
    return srk::is_close(t1y, std::fabs(Ti[comp]), atol) ? 1 : 0;                             // :323
}

int srk_ba_normalize_scene(int64_t N, double* pts, int32_t M, double* cam_R, double* cam_T, double t1y, int32_t comp,
                           srk_ba_normalizer* out)
{
    if (M < 2 || comp < 0 || comp > 2 || !out || !cam_R || !cam_T || (N > 0 && !pts)) return 0;
    // cam0_from1 = SE3AFromB(cam0, cam1)  (:208, obs-geom.cpp:141-150)
    double R1i[9], T1i[3], v[3], T01[3];
    srk::se3_inv(cam_R + 9, cam_T + 3, R1i, T1i);
    srk::mat3_vec(cam_R, T1i, v);
    for (int i = 0; i < 3; ++i) T01[i] = v[i] + cam_T[i];
    double shift = T01[comp];
    if (srk::is_close(0.0, shift, 1e-5)) return 0; // :215-217 (the lone third argument is rtol)
    double s = t1y / std::fabs(shift);             // :219
    std::memcpy(out->R0, cam_R, sizeof out->R0);
    std::memcpy(out->T0, cam_T, sizeof out->T0);
    out->world_scale = s;
    double R0t[9];
    srk::mat3_tr(out->R0, R0t);
    for (int32_t j = 0; j < M; ++j) { // NormalizeRT :143-162
        double RR[9], u[3];
        srk::mat3_mul(cam_R + 9 * (int64_t)j, R0t, RR);
        srk::mat3_vec(RR, out->T0, u);
        for (int i = 0; i < 3; ++i) cam_T[3 * (int64_t)j + i] = (cam_T[3 * (int64_t)j + i] - u[i]) * s;
        std::memcpy(cam_R + 9 * (int64_t)j, RR, sizeof RR);
    }
    for (int64_t i = 0; i < N; ++i) { // :179-199
        double y[3];
        srk::se3_apply(out->R0, out->T0, pts + 3 * i, y);
        pts[3 * i] = y[0] * s;
        pts[3 * i + 1] = y[1] * s;
        pts[3 * i + 2] = y[2] * s;
    }
    return 1;
}

void srk_ba_revert_normalization(int64_t N, double* pts, int32_t M, double* cam_R, double* cam_T,
                                 const srk_ba_normalizer* nrm)
{
    double s = nrm->world_scale;
    double R0t[9];
    srk::mat3_tr(nrm->R0, R0t);
    for (int64_t i = 0; i < N; ++i) { // :187-191
        double is = 1 / s;
        double t[3] = { pts[3 * i] * is - nrm->T0[0], pts[3 * i + 1] * is - nrm->T0[1], pts[3 * i + 2] * is - nrm->T0[2] };
        srk::mat3_vec(R0t, t, pts + 3 * i);
    }
    for (int32_t j = 0; j < M; ++j) { // RevertRT :164-177
        double RR[9], u[3];
        double* R = cam_R + 9 * (int64_t)j;
        double* T = cam_T + 3 * (int64_t)j;
        srk::mat3_mul(R, nrm->R0, RR);
        srk::mat3_vec(R, nrm->T0, u);
        for (int i = 0; i < 3; ++i) T[i] = T[i] / s + u[i];
        std::memcpy(R, RR, sizeof RR);
    }
}

} // extern "C"

// ------------------------------------------------------------------ scene upload

static int validate_scene(srk_ba* h, double f0, int64_t N, const double* pts, int32_t M, const double* cam_R,
                          const double* cam_T, const double* K, const int64_t* row_ptr, const int32_t* obs_frame,
                          const double* obs_uv, int32_t min_frames = 2)
{
    if (!h) return SRK_E_ARGS;
    // CHECK(!IsClose(0, f0)) (:420)
    if (srk::is_close(0.0, f0)) { h->last_error = "f0 must not be ~0"; return SRK_E_ARGS; }
    if (M < min_frames) { h->last_error = min_frames > 1 ? "need at least two frames" : "need at least one frame"; return SRK_E_ARGS; }
    if (N < 0 || !cam_R || !cam_T || !K || !row_ptr) { h->last_error = "null scene array"; return SRK_E_ARGS; }
    if (N > 0 && !pts) { h->last_error = "null points"; return SRK_E_ARGS; }
    if (N > 2147483000LL) { h->last_error = "too many points for int32 indices"; return SRK_E_ARGS; }
    if (row_ptr[0] != 0) { h->last_error = "obs_row_ptr[0] != 0"; return SRK_E_ARGS; }
    int64_t O = row_ptr[N];
    if (O > 0 && (!obs_frame || !obs_uv)) { h->last_error = "null observation arrays"; return SRK_E_ARGS; }
    for (int64_t i = 0; i < N; ++i) {
        if (row_ptr[i + 1] < row_ptr[i]) { h->last_error = "obs_row_ptr not monotone"; return SRK_E_ARGS; }
        for (int64_t o = row_ptr[i]; o < row_ptr[i + 1]; ++o) {
            int32_t j = obs_frame[o];
            if (j < 0 || j >= M) { h->last_error = "obs_frame out of range"; return SRK_E_ARGS; }
            if (o > row_ptr[i] && obs_frame[o - 1] >= j) {
                h->last_error = "obs_frame must be strictly ascending inside a point";
                return SRK_E_ARGS;
            }
        }
    }
    return SRK_OK;
}

static double* kbuf(srk_ba* h, int w);
static int compute_cam_packs(srk_ba* h, int which)
{
    srk_launch_cam_pack(h->main_stream, h->d.M, P<double>(h->camR[which]), P<double>(h->camT[which]), kbuf(h, which),
                        h->f0, P<double>(h->cam[which]));
    HIPCHK(h, hipGetLastError());
    return SRK_OK;
}

// Chunked solve plan: P chunks of the variable range separated by P-1 separators at least as wide as the
// bandwidth (so chunks are decoupled).  The separator system is block tridiagonal in units of sepw, so it is chunked
// again (cuts aligned to those blocks) by a child plan: nested dissection of a banded system, every level one batch.
//
// Cost model, in units of one 256-column outer step of the blocked Cholesky (~0.17 ms on MI355X): a chunked level
// pays its longest chunk (border rows make a step ~10% dearer), a fixed overhead for gather / reduce / scatter,
// and the cost of its separator system.
static double plan_cost(int64_t ld, int64_t sepw, int64_t unit, int* best_P)
{
    const double n256 = (double)(ld / SRK_CHOL_NB);
    double best = n256;
    int bp = 0;
    for (int p = 2; p <= SRK_MAX_CHUNKS; ++p) {
        const int64_t interior = ld - sepw * (p - 1);
        if (interior < (int64_t)p * sepw) break; // every chunk at least one separator wide
        const int64_t units = interior / unit;
        const int64_t longest = ((units + p - 1) / p) * unit;
        const double cst = 1.1 * (double)((longest + SRK_CHOL_NB - 1) / SRK_CHOL_NB) + 0.6 + plan_cost(sepw * (p - 1), sepw, sepw, nullptr);
        if (cst < best - 1e-9) best = cst, bp = p;
    }
    if (best_P) *best_P = bp;
    return best;
}

// row_end (per 256 block, multiple of 128) / col_begin (per 64 tile): the skyline of the system to be chunked
static int make_plan(srk_ba* h, srk_ba::Attempt& a, hipStream_t s, SrkChunkPlan& pl, int64_t ld, int64_t sepw, int64_t unit,
                     const std::vector<int64_t>& row_end, const std::vector<int64_t>& col_begin)
{
    pl.P = 0;
    int P = 0;
    plan_cost(ld, sepw, unit, &P);
    if (P < 2) return SRK_OK;
    const int64_t interior = ld - sepw * (P - 1);
    const int64_t blocks = interior / unit; // ld, sepw are multiples of unit
    if (srk_debug())
        fprintf(stderr, "srk_ba chunk plan: system %lld -> %d chunks of <= %lld + %d separators of %lld\n", (long long)ld, P,
                (long long)(((blocks + P - 1) / P) * unit), P - 1, (long long)sepw);
    pl.sepw = sepw;
    pl.lds = sepw * (P - 1);
    std::vector<int64_t> sep_start((size_t)(P - 1));
    int64_t pos = 0;
    auto alloc = [&](size_t bytes, bool zero) -> void* {
        a.plan_bufs.emplace_back();
        a.plan_zeroed.push_back(zero ? 1 : 0);
        if (dev_alloc(h, a.plan_bufs.back(), bytes) != SRK_OK) return nullptr;
        if (zero) hipMemsetAsync(a.plan_bufs.back().p, 0, bytes, s);
        return a.plan_bufs.back().p;
    };
    for (int c = 0; c < P; ++c) {
        int64_t nb = blocks / P + (c < blocks % P ? 1 : 0);
        pl.a[c] = pos;
        pl.n[c] = nb * unit;
        pl.ldc[c] = pl.n[c] + 2 * sepw;
        pos += pl.n[c];
        if (c < P - 1) {
            sep_start[(size_t)c] = pos;
            pos += sepw;
        }
        const int64_t nc = pl.n[c], ldc = pl.ldc[c];
        pl.Ac[c] = (double*)alloc((size_t)(8 * ldc * ldc), true);
        pl.wc[c] = (double*)alloc((size_t)(8 * ldc), true);
        pl.yc[c] = (double*)alloc((size_t)(8 * ldc), true);
        pl.xc[c] = (double*)alloc((size_t)(8 * ldc), true);
        pl.dinvc[c] = (double*)alloc((size_t)(8 * 64 * ldc), false);
        if (!pl.Ac[c] || !pl.wc[c] || !pl.yc[c] || !pl.xc[c] || !pl.dinvc[c]) return SRK_E_NOMEM;
        pl.row_end[c].assign((size_t)(nc / SRK_CHOL_NB), 0);
        for (int64_t K = 0; K < nc / SRK_CHOL_NB; ++K) {
            int64_t rg = row_end[(size_t)(pl.a[c] / SRK_CHOL_NB + K)] - pl.a[c];
            pl.row_end[c][(size_t)K] = std::min<int64_t>(std::max<int64_t>(rg, SRK_CHOL_NB * (K + 1)), nc);
        }
        pl.col_begin[c].assign((size_t)(nc / 64), 0);
        for (int64_t q = 0; q < nc / 64; ++q)
            pl.col_begin[c][(size_t)q] = std::max<int64_t>(col_begin[(size_t)(pl.a[c] / 64 + q)] - pl.a[c], 0);
    }
    const int64_t lds = pl.lds;
    pl.Cs = (double*)alloc((size_t)(8 * lds * lds), true);
    pl.ws = (double*)alloc((size_t)(8 * lds), true);
    pl.ys = (double*)alloc((size_t)(8 * lds), true);
    pl.xs = (double*)alloc((size_t)(8 * lds), true);
    pl.dinvs = (double*)alloc((size_t)(8 * 64 * lds), false);
    pl.d_sep_start = (int64_t*)alloc((size_t)(8 * (P - 1)), false);
    pl.d_sep_env = (int64_t*)alloc((size_t)(8 * (lds / 128)), false);
    if (!pl.Cs || !pl.ws || !pl.ys || !pl.xs || !pl.dinvs || !pl.d_sep_start || !pl.d_sep_env) return SRK_E_NOMEM;
    HIPCHK(h, hipMemcpyAsync(pl.d_sep_start, sep_start.data(), (size_t)(8 * (P - 1)), hipMemcpyHostToDevice, s));
    // separators only couple with their neighbours (through the chunk between them): block tridiagonal skyline
    pl.s_row_end.assign((size_t)(lds / SRK_CHOL_NB), 0);
    for (int64_t K = 0; K < lds / SRK_CHOL_NB; ++K) {
        int64_t c = (SRK_CHOL_NB * K) / sepw;
        pl.s_row_end[(size_t)K] = std::min<int64_t>(lds, (c + 2) * sepw);
    }
    pl.s_col_begin.assign((size_t)(lds / 64), 0);
    for (int64_t q = 0; q < lds / 64; ++q) {
        int64_t c = (64 * q) / sepw;
        pl.s_col_begin[(size_t)q] = std::max<int64_t>(c - 1, 0) * sepw;
    }
    std::vector<int64_t> sep_env((size_t)(lds / 128));
    for (int64_t t = 0; t < lds / 128; ++t) sep_env[(size_t)t] = pl.s_col_begin[(size_t)(2 * t)];
    HIPCHK(h, hipMemcpyAsync(pl.d_sep_env, sep_env.data(), (size_t)(8 * (lds / 128)), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));
    // the separator system, chunked again when that shortens its chain
    a.plan_children.emplace_back(new SrkChunkPlan());
    SrkChunkPlan* child = a.plan_children.back().get();
    int rc = make_plan(h, a, s, *child, lds, sepw, sepw, pl.s_row_end, pl.s_col_begin);
    if (rc != SRK_OK) return rc;
    pl.child = child->P >= 2 ? child : nullptr;
    pl.P = P;
    return SRK_OK;
}

static int build_chunk_plan(srk_ba* h, srk_ba::Attempt& a, hipStream_t s)
{
    const SrkDims& d = h->d;
    SrkChunkPlan& pl = a.plan;
    // the same skyline as the plan in place was built for (a scene uploaded again, the next call of a caller that adjusts the
    // same tracks): keep plan and buffers -- freeing and allocating them again costs ~9 ms a slot at 1000 frames -- and
    // bring the buffers that must be zero outside what a solve writes back to zero
    std::vector<int64_t> sig = { d.ld, d.fv, h->use_envelope ? 1 : 0, h->use_chunks ? 1 : 0, h->shk_G };
    sig.insert(sig.end(), h->min_cv.begin(), h->min_cv.end());
    if (!a.plan_sig.empty() && sig == a.plan_sig) {
        for (size_t i = 0; i < a.plan_bufs.size(); ++i)
            if (a.plan_zeroed[i]) HIPCHK(h, hipMemsetAsync(a.plan_bufs[i].p, 0, a.plan_bufs[i].bytes, s));
        return SRK_OK;
    }
    a.plan_sig = sig;
    pl.P = 0;
    pl.child = nullptr;
    for (DevBuf& b : a.plan_bufs) dev_free(b);
    a.plan_bufs.clear();
    a.plan_zeroed.clear();
    a.plan_children.clear();
    if (!h->use_envelope || !h->use_chunks || h->shk_G > 0) return SRK_OK; // shared intrinsics: one chain with the border
    int64_t maxdist = 0;
    for (int32_t j = 0; j < d.M; ++j) maxdist = std::max<int64_t>(maxdist, d.fv * (int64_t)(j - h->min_cv[(size_t)j]) + d.fv - 1);
    // separators at least one bandwidth wide, in units of the 256-column outer panel (k_bwd_border stages 2 sepw values)
    const int64_t sepw = (maxdist + SRK_CHOL_NB - 1) / SRK_CHOL_NB * SRK_CHOL_NB;
    if (sepw > SRK_MAX_SEPW) return SRK_OK;
    const int rc = make_plan(h, a, s, pl, d.ld, sepw, SRK_CHOL_NB, h->row_end_h, h->col_begin_h);
    if (rc != SRK_OK) a.plan_sig.clear();
    return rc;
}

// Skyline of the RCS from the covisibility (min_cv[j] = smallest frame index sharing a landmark with frame j), for fv
// variables a frame and the padded size ld.  All quantities are aligned to the solver's blocking: env_col multiples of 256,
// row_end multiples of 128.
static void make_skyline(const srk_ba* h, int fv, int64_t ld, std::vector<int64_t>& env_col, std::vector<int64_t>& row_end,
                         std::vector<int64_t>& col_begin)
{
    const int64_t nt = ld / 128, nk = ld / SRK_CHOL_NB, n64 = ld / 64;
    const int32_t M = h->d.M;
    env_col.assign((size_t)nt, 0);
    for (int64_t t = 0; t < nt; ++t) {
        int64_t r0 = 128 * t, r1 = 128 * t + 127;
        int64_t fc = r0; // padding rows and the diagonal itself
        if (h->use_envelope) {
            for (int64_t j = r0 / fv; j <= r1 / fv && j < M; ++j) fc = std::min<int64_t>(fc, fv * (int64_t)h->min_cv[(size_t)j]);
        } else {
            fc = 0;
        }
        env_col[(size_t)t] = (fc / SRK_CHOL_NB) * SRK_CHOL_NB;
    }
    row_end.assign((size_t)nk, 0);
    for (int64_t K = 0; K < nk; ++K) {
        int64_t last = -1;
        for (int64_t t = nt - 1; t >= 0; --t)
            if (env_col[(size_t)t] <= SRK_CHOL_NB * K) { last = t; break; }
        int64_t re = 128 * (last + 1);
        re = std::max<int64_t>(re, SRK_CHOL_NB * (K + 1));
        row_end[(size_t)K] = std::min<int64_t>(re, ld);
    }
    col_begin.assign((size_t)n64, 0);
    for (int64_t q = 0; q < n64; ++q) col_begin[(size_t)q] = env_col[(size_t)(q / 2)];
}

static int build_envelope(srk_ba* h)
{
    const SrkDims& d = h->d;
    const int64_t nt = d.ld / 128;
    make_skyline(h, d.fv, d.ld, h->env_col_h, h->row_end_h, h->col_begin_h);
    h->env_off_h.assign((size_t)nt + 1, 0);
    for (int64_t t = 0; t < nt; ++t)
        h->env_off_h[(size_t)t + 1] = h->env_off_h[(size_t)t] + 128 * (128 * (t + 1) - h->env_col_h[(size_t)t]);
    h->env_packed = h->env_off_h[(size_t)nt];
    int rc;
    if ((rc = dev_alloc(h, h->env_col, (size_t)(8 * nt))) != SRK_OK) return rc;
    if ((rc = dev_alloc(h, h->env_off, (size_t)(8 * (nt + 1)))) != SRK_OK) return rc;
    HIPCHK(h, hipMemcpyAsync(h->env_col.p, h->env_col_h.data(), (size_t)(8 * nt), hipMemcpyHostToDevice, h->main_stream));
    HIPCHK(h, hipMemcpyAsync(h->env_off.p, h->env_off_h.data(), (size_t)(8 * (nt + 1)), hipMemcpyHostToDevice, h->main_stream));
    // exchange format of the assembled system (landmark shards): the exact pre-factorisation band of every row
    {
        std::vector<int64_t> bc((size_t)d.ld), bo((size_t)d.ld + 1, 0);
        for (int64_t r = 0; r < d.ld; ++r) {
            int64_t c0 = r; // padding rows: the diagonal only
            if (r < d.fv * (int64_t)d.M) c0 = h->use_envelope ? d.fv * (int64_t)h->min_cv[(size_t)(r / d.fv)] : 0;
            bc[(size_t)r] = c0;
            bo[(size_t)r + 1] = bo[(size_t)r] + (r - c0 + 1);
        }
        h->band_packed = bo[(size_t)d.ld];
        if ((rc = dev_alloc(h, h->band_col, (size_t)(8 * d.ld))) != SRK_OK) return rc;
        if ((rc = dev_alloc(h, h->band_off, (size_t)(8 * (d.ld + 1)))) != SRK_OK) return rc;
        HIPCHK(h, hipMemcpyAsync(h->band_col.p, bc.data(), (size_t)(8 * d.ld), hipMemcpyHostToDevice, h->main_stream));
        HIPCHK(h, hipMemcpyAsync(h->band_off.p, bo.data(), (size_t)(8 * (d.ld + 1)), hipMemcpyHostToDevice, h->main_stream));
        HIPCHK(h, hipStreamSynchronize(h->main_stream)); // bc / bo are locals
    }
    for (int sl = 0; sl < SRK_SLOTS; ++sl) { // every allocated attempt slot: its own zeroed system and solver plan
        if (!h->att[sl].allocated) continue;
        HIPCHK(h, hipMemsetAsync(h->att[sl].S.p, 0, (size_t)(8 * d.ld * d.ld), h->main_stream)); // outside the skyline stays 0
        HIPCHK(h, hipStreamSynchronize(h->main_stream));
        rc = build_chunk_plan(h, h->att[sl], h->main_stream); // plan buffers of slot sl, allocated and zeroed on the main stream
        if (rc != SRK_OK) return rc;
    }
    return SRK_OK;
}

// Shared intrinsics: the compact pose skyline, the coupled-frame ranges and group members the fold
// reads, and every attempt slot's folded system.  After build_envelope (min_cv, the 10-variable plan).
static int build_shared_k(srk_ba* h)
{
    const SrkDims& d = h->d;
    const int32_t M = d.M, G = h->shk_G;
    const int64_t ncols = (6 * (int64_t)M + SRK_CHOL_NB - 1) / SRK_CHOL_NB * SRK_CHOL_NB, ldb = ncols + 2 * SRK_SHK_BORDER;
    h->shk_ncols = ncols;
    h->shk_ldb = ldb;
    std::vector<int64_t> env;
    make_skyline(h, 6, ncols, env, h->shk_row_end, h->shk_col_begin);
    // S10 block (f, f') may be non-zero iff the frames share a landmark: min_cv[f'] <= f for f <= f', min_cv[f] <= f' above
    std::vector<int32_t> lo(h->min_cv), hi((size_t)M, 0), mptr((size_t)G + 1, 0), mem((size_t)M);
    for (int32_t f = 0; f < M; ++f) hi[(size_t)h->min_cv[(size_t)f]] = std::max(hi[(size_t)h->min_cv[(size_t)f]], f);
    for (int32_t f = 0; f < M; ++f) hi[(size_t)f] = std::max({ hi[(size_t)f], f, f > 0 ? hi[(size_t)f - 1] : 0 });
    for (int32_t f = 0; f < M; ++f) ++mptr[(size_t)h->shk_grp_h[(size_t)f] + 1];
    for (int32_t g = 0; g < G; ++g) mptr[(size_t)g + 1] += mptr[(size_t)g];
    {
        std::vector<int32_t> fill(mptr.begin(), mptr.end() - 1);
        for (int32_t f = 0; f < M; ++f) mem[(size_t)fill[(size_t)h->shk_grp_h[(size_t)f]]++] = f;
    }
    h->shk_first.assign((size_t)G, 0);
    for (int32_t g = 0; g < G; ++g) h->shk_first[(size_t)g] = mem[(size_t)mptr[(size_t)g]];
    int rc;
    if ((rc = dev_alloc(h, h->shk_grp, 4 * (size_t)M)) != SRK_OK) return rc;
    if ((rc = dev_alloc(h, h->shk_lo, 4 * (size_t)M)) != SRK_OK) return rc;
    if ((rc = dev_alloc(h, h->shk_hi, 4 * (size_t)M)) != SRK_OK) return rc;
    if ((rc = dev_alloc(h, h->shk_mptr, 4 * ((size_t)G + 1))) != SRK_OK) return rc;
    if ((rc = dev_alloc(h, h->shk_mem, 4 * (size_t)M)) != SRK_OK) return rc;
    if ((rc = dev_alloc(h, h->shk_env, 8 * env.size())) != SRK_OK) return rc;
    hipStream_t s = h->main_stream;
    HIPCHK(h, hipMemcpyAsync(h->shk_grp.p, h->shk_grp_h.data(), 4 * (size_t)M, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(h->shk_lo.p, lo.data(), 4 * (size_t)M, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(h->shk_hi.p, hi.data(), 4 * (size_t)M, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(h->shk_mptr.p, mptr.data(), 4 * ((size_t)G + 1), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(h->shk_mem.p, mem.data(), 4 * (size_t)M, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(h->shk_env.p, env.data(), 8 * env.size(), hipMemcpyHostToDevice, s));
    for (auto& a : h->att) {
        if (!a.allocated) continue;
        if ((rc = dev_alloc(h, a.Ssh, (size_t)(8 * ldb * ldb))) != SRK_OK) return rc;
        if ((rc = dev_alloc(h, a.rsh, (size_t)(8 * ldb))) != SRK_OK) return rc;
        if ((rc = dev_alloc(h, a.ysh, (size_t)(16 * ldb))) != SRK_OK) return rc; // w (a copy of rhs_sh), y
        if ((rc = dev_alloc(h, a.dcsh, (size_t)(8 * ldb))) != SRK_OK) return rc;
        if ((rc = dev_alloc(h, a.dinvsh, (size_t)(8 * 64 * ldb))) != SRK_OK) return rc;
        if ((rc = dev_alloc(h, a.Tsh, (size_t)(8 * 16 * (int64_t)G * M))) != SRK_OK) return rc;
        // outside what the fold writes (the skyline, the live border rows) the system stays zero
        HIPCHK(h, hipMemsetAsync(a.Ssh.p, 0, (size_t)(8 * ldb * ldb), s));
        HIPCHK(h, hipMemsetAsync(a.ysh.p, 0, (size_t)(16 * ldb), s));
        HIPCHK(h, hipMemsetAsync(a.dcsh.p, 0, (size_t)(8 * ldb), s));
    }
    HIPCHK(h, hipStreamSynchronize(s)); // host tables go out of scope
    return SRK_OK;
}

static SrkShk shk_args(const srk_ba* h, const srk_ba::Attempt& a)
{
    SrkShk k;
    k.M = h->d.M;
    k.G = h->shk_G;
    k.ld10 = h->d.ld;
    k.ncols = h->shk_ncols;
    k.ldb = h->shk_ldb;
    k.grp = P<int32_t>(h->shk_grp);
    k.cpl_lo = P<int32_t>(h->shk_lo);
    k.cpl_hi = P<int32_t>(h->shk_hi);
    k.mem_ptr = P<int32_t>(h->shk_mptr);
    k.mem = P<int32_t>(h->shk_mem);
    k.env_sh = P<int64_t>(h->shk_env);
    k.T = P<double>(a.Tsh);
    return k;
}
// the intrinsics of scene buffer set w: its own copy with shared intrinsics (the trial K of an attempt), else the uploaded K
static double* kbuf(srk_ba* h, int w) { return h->shk_G > 0 ? P<double>(h->Ks[w]) : P<double>(h->K); }

static void rearm_fusion(srk_ba* h);
// per-observation information q (the caller's order) against a scene's CSR rows: every value finite and >= 0, one per
// observation, and no landmark left with fewer than two observations of positive information (its 3 x 3 block would be singular)
static int check_information(srk_ba* h, const char* who, const double* q, int64_t count, int64_t N, const int64_t* row_ptr)
{
    if (count != row_ptr[N]) {
        h->last_error = std::string(who) + ": the observation information holds " + std::to_string(count) + " values, the scene " +
                        std::to_string(row_ptr[N]) + " observations";
        return SRK_E_ARGS;
    }
    for (int64_t o = 0; o < count; ++o)
        if (!(std::isfinite(q[o]) && q[o] >= 0)) {
            h->last_error = std::string(who) + ": observation information must be finite and not negative (observation " + std::to_string(o) + ")";
            return SRK_E_ARGS;
        }
    for (int64_t i = 0; i < N; ++i) {
        const int64_t cnt = row_ptr[i + 1] - row_ptr[i];
        int64_t pos = 0;
        for (int64_t o = row_ptr[i]; o < row_ptr[i + 1]; ++o) pos += q[o] > 0 ? 1 : 0;
        if (pos < std::min<int64_t>(cnt, 2)) {
            h->last_error = std::string(who) + ": observation information leaves landmark " + std::to_string(i) +
                            " with fewer than two observations of positive information";
            return SRK_E_ARGS;
        }
    }
    return SRK_OK;
}
// ---- the factor settings -> the device tables of the resident scene: srk_factors.cpp builds them, upload_tables allocates and
// copies.  A table: bytes from src (or zeros) in a buffer of max(bytes, at_least) bytes; nothing at all when that is 0.
struct TableUp { DevBuf* buf; const void* src; size_t bytes, at_least; bool zero; };
template <typename T> static TableUp table_of(DevBuf& b, const std::vector<T>& v, size_t at_least = 0)
{
    return { &b, v.data(), sizeof(T) * v.size(), at_least, false };
}
static TableUp zeros_of(DevBuf& b, size_t bytes) { return { &b, nullptr, bytes, 0, true }; }
static int upload_tables(srk_ba* h, std::initializer_list<TableUp> tables)
{
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->main_stream;
    int rc;
    for (const TableUp& u : tables) {
        const size_t size = std::max(u.bytes, u.at_least);
        if (size == 0) continue;
        if ((rc = dev_alloc(h, *u.buf, size)) != SRK_OK) return rc;
        if (u.zero) HIPCHK(h, hipMemsetAsync(u.buf->p, 0, size, s));
        else if (u.bytes) HIPCHK(h, hipMemcpyAsync(u.buf->p, u.src, u.bytes, hipMemcpyHostToDevice, s));
    }
    HIPCHK(h, hipStreamSynchronize(s)); // the staging vectors go out of scope; every attempt stream starts behind this call
    return SRK_OK;
}
static SrkFactorDims factor_dims(const srk_ba* h) { return { h->d.N, h->d.M, h->d.O, h->d.fv, h->d.ld }; }

static int apply_information(srk_ba* h)
{
    InfoFamily& f = h->obs_info;
    f.on = false;
    const SrkInfoTables t = srk_build_information(f.set, *h, factor_dims(h));
    if (!t.on) return SRK_OK;
    const int rc = upload_tables(h, { table_of(f.buf[f.Q], t.q), table_of(f.buf[f.QF], t.qf) });
    f.on = rc == SRK_OK;
    return rc;
}
static int apply_constant_blocks(srk_ba* h)
{
    ConstFamily& f = h->cst;
    f.n_pts = 0;
    f.n_frames = 0;
    f.frame_int.clear();
    if (!f.set.set) return SRK_OK;
    SrkConstTables t = srk_build_constant(f.set, *h, factor_dims(h));
    f.frame_int.swap(t.frame_int);
    const int rc = upload_tables(h, { table_of(f.buf[f.PTS], t.pts), table_of(f.buf[f.FRAMES], t.frames) });
    if (rc != SRK_OK) return rc;
    f.n_pts = (int64_t)t.pts.size();
    f.n_frames = (int32_t)t.frames.size();
    return SRK_OK;
}
static int apply_position_priors(srk_ba* h)
{
    PriorFamily& f = h->pri;
    f.n_pts = 0;
    f.n_frames = 0;
    f.app.take(f.set);
    if (!f.set.set) return SRK_OK;
    const SrkPriorTables t = srk_build_priors(f.set, h->nrm, *h, factor_dims(h));
    const int rc = upload_tables(h, { table_of(f.buf[f.PT_LIST], t.pt_list), table_of(f.buf[f.PT_VAL], t.pt_val),
                                      table_of(f.buf[f.FR_LIST], t.fr_list), table_of(f.buf[f.FR_VAL], t.fr_val) });
    if (rc != SRK_OK) return rc;
    f.n_pts = (int64_t)t.pt_list.size();
    f.n_frames = (int32_t)t.fr_list.size();
    return SRK_OK;
}
static int apply_relative_pose_factors(srk_ba* h)
{
    RelPoseFamily& f = h->rp;
    f.n = f.n_frames = 0;
    f.int_a.clear(); f.int_b.clear();
    f.app.take(f.set);
    SrkRelPoseTables t = srk_build_relpose(f.set, h->sel, h->nrm, *h, factor_dims(h));
    const size_t n = t.fa.size();
    if (n == 0) return SRK_OK;
    const int rc = upload_tables(h, { table_of(f.buf[f.FA], t.fa), table_of(f.buf[f.FB], t.fb), table_of(f.buf[f.VAL], t.val),
                                      table_of(f.buf[f.FR_LIST], t.fr_list), table_of(f.buf[f.FR_PTR], t.fr_ptr),
                                      table_of(f.buf[f.FR_ENT], t.fr_ent), table_of(f.buf[f.TGT], t.tgt), zeros_of(f.buf[f.CPL], 8 * 36 * n) });
    if (rc != SRK_OK) return rc;
    f.int_a.swap(t.fa);
    f.int_b.swap(t.fb);
    f.n = (int32_t)n;
    f.n_frames = (int32_t)t.fr_list.size();
    return SRK_OK;
}
static int apply_joint_pose_priors(srk_ba* h)
{
    JPriorFamily& f = h->jp;
    f.n = f.n_pairs = f.n_frames = 0;
    for (TimedPass& p : f.pass) p.timed = false;
    f.pair_a.clear(); f.pair_b.clear();
    f.app.take(f.set);
    SrkJPriorTables t = srk_build_jprior(f.set, h->sel, h->nrm, *h, factor_dims(h));
    const size_t nq = t.frame.size(), np = t.pslot.size();
    if (nq == 0) return SRK_OK;
    f.pair_a.swap(t.pair_a);
    f.pair_b.swap(t.pair_b);
    const int rc = upload_tables(h, { table_of(f.buf[f.PTR], t.ptr, 8), table_of(f.buf[f.FRAME], t.frame, 8), table_of(f.buf[f.LIN], t.lin, 8),
                                      table_of(f.buf[f.MEAN], t.mean, 8), table_of(f.buf[f.IPTR], t.iptr, 8), table_of(f.buf[f.INFO], t.info, 8),
                                      table_of(f.buf[f.PPTR], t.pptr, 8), table_of(f.buf[f.PSLOT], t.pslot, 8), table_of(f.buf[f.TGT], t.tgt, 8),
                                      table_of(f.buf[f.FR_LIST], t.fr_list, 8), table_of(f.buf[f.FR_PTR], t.fr_ptr, 8),
                                      table_of(f.buf[f.FR_ENT], t.fr_ent, 8), zeros_of(f.buf[f.BLK], 8 * 42 * nq),
                                      zeros_of(f.buf[f.CPL], 8 * 36 * std::max<size_t>(np, 1)) });
    if (rc != SRK_OK) return rc;
    f.n = (int32_t)t.iptr.size();
    f.n_pairs = (int32_t)np;
    f.n_frames = (int32_t)t.fr_list.size();
    return SRK_OK;
}

// the lists of the resident scene for the kernels: NULL without switched-on entries, so that none of a family's passes is launched
static const SrkPrior* position_priors(const srk_ba* h, SrkPrior& p)
{
    const PriorFamily& f = h->pri;
    if (f.n_pts == 0 && f.n_frames == 0) return nullptr;
    p = SrkPrior{ P<int32_t>(f.buf[f.PT_LIST]), P<double>(f.buf[f.PT_VAL]), f.n_pts, P<int32_t>(f.buf[f.FR_LIST]), P<double>(f.buf[f.FR_VAL]), f.n_frames };
    return &p;
}
static const SrkRelPose* relpose_factors(const srk_ba* h, SrkRelPose& p)
{
    const RelPoseFamily& f = h->rp;
    if (f.n == 0) return nullptr;
    p = SrkRelPose{ P<int32_t>(f.buf[f.FA]), P<int32_t>(f.buf[f.FB]), P<double>(f.buf[f.VAL]), f.n, P<int32_t>(f.buf[f.FR_LIST]),
                    P<int32_t>(f.buf[f.FR_PTR]), P<int32_t>(f.buf[f.FR_ENT]), f.n_frames, P<int64_t>(f.buf[f.TGT]), P<double>(f.buf[f.CPL]) };
    return &p;
}
static const SrkJointPrior* joint_priors(const srk_ba* h, SrkJointPrior& p)
{
    const JPriorFamily& f = h->jp;
    if (f.n == 0) return nullptr;
    p = SrkJointPrior{ f.n, P<int32_t>(f.buf[f.PTR]), P<int32_t>(f.buf[f.FRAME]), P<double>(f.buf[f.LIN]), P<double>(f.buf[f.MEAN]),
                       P<int64_t>(f.buf[f.IPTR]), P<double>(f.buf[f.INFO]), P<int32_t>(f.buf[f.PPTR]), P<int32_t>(f.buf[f.PSLOT]),
                       P<int64_t>(f.buf[f.TGT]), f.n_pairs, P<double>(f.buf[f.BLK]), P<double>(f.buf[f.CPL]), P<int32_t>(f.buf[f.FR_LIST]),
                       P<int32_t>(f.buf[f.FR_PTR]), P<int32_t>(f.buf[f.FR_ENT]), f.n_frames };
    return &p;
}

// ---- the timed passes (profile level >= 1; the *_pass_ms calls read them)
static bool pass_events(TimedPass& p)
{
    for (hipEvent_t& e : p.ev)
        if (!e && hipEventCreate(&e) != hipSuccess) return false;
    return true;
}
// a launch between the two events of its pass
template <typename Launch> static int timed_launch(srk_ba* h, TimedPass& p, hipStream_t s, Launch launch)
{
    const bool timed = h->profile_level >= 1 && pass_events(p);
    if (timed) HIPCHK(h, hipEventRecord(p.ev[0], s));
    launch();
    if (timed) HIPCHK(h, hipEventRecord(p.ev[1], s));
    p.timed = timed;
    HIPCHK(h, hipGetLastError());
    return SRK_OK;
}
// for srk_launch_error, which records the pair around a family's pass itself: the pair, or NULL when the pass is not timed
static const hipEvent_t* error_pass_events(srk_ba* h, TimedPass& p, bool launched)
{
    if (!launched) return nullptr;
    p.timed = h->profile_level >= 1 && pass_events(p);
    return p.timed ? p.ev : nullptr;
}
// the milliseconds of a family's n passes, 0 where a pass was not timed (every slot's stream has drained first)
static int pass_ms(srk_ba* h, const TimedPass* pass, int n, double* const* out)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->main_stream));
    for (int sl = 1; sl < SRK_SLOTS; ++sl)
        if (h->att[sl].stream) HIPCHK(h, hipStreamSynchronize(h->att[sl].stream));
    for (int k = 0; k < n; ++k) {
        float ms = 0;
        if (pass[k].timed && hipEventElapsedTime(&ms, pass[k].ev[0], pass[k].ev[1]) != hipSuccess) ms = 0;
        if (out[k]) *out[k] = pass[k].timed ? (double)ms : 0.0;
    }
    return SRK_OK;
}

// ---- shared by the entry points of the factor settings
// a pass on its own (a family's energy, the observations' weights or residuals): nb partial sums and the n_out results behind them
// in a buffer of the call's own; launch(stream, partials, results) starts the pass, the results come back to out
template <typename Launch> static int error_pass(srk_ba* h, int32_t nb, int64_t n_out, double* out, Launch launch)
{
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->main_stream;
    HIPCHK(h, hipStreamSynchronize(s));
    DevBuf part;
    int rc = dev_alloc(h, part, 8 * ((size_t)nb + (size_t)n_out));
    if (rc != SRK_OK) return rc;
    launch(s, P<double>(part), P<double>(part) + nb);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, P<double>(part) + nb, 8 * (size_t)n_out, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    dev_free(part);
    HIPCHK(h, e);
    return SRK_OK;
}
// a setter of the named family against the modes already set
static bool refuse_setting(srk_ba* h, const char* family)
{
    const std::string e = srk_setting_conflict(family, true, !h->igroup_user.empty(), h->world);
    if (!e.empty()) h->last_error = e;
    return !e.empty();
}
template <typename T> static void copy_out(T* dst, const std::vector<T>& v)
{
    if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(T));
}
// the resident scene in the caller's world coordinates, for the residual calls
struct WorldScene {
    std::vector<double> pts, R, T;
    int rc;
    explicit WorldScene(srk_ba* h) : pts((size_t)(3 * h->d.N)), R((size_t)(9 * (int64_t)h->d.M)), T((size_t)(3 * (int64_t)h->d.M)),
                                     rc(srk_ba_download_scene(h, pts.data(), R.data(), T.data(), 1)) {}
};
static int upload_scene_impl(srk_ba* h, double f0, int64_t N, const double* pts_in, int32_t M,
                             const double* cam_R_in, const double* cam_T_in, const double* K_in, int shared_k,
                             const int64_t* row_ptr, const int32_t* obs_frame, const double* obs_uv,
                             int already_normalized);
// (the upload allocates host vectors and starts sorting threads: nothing of that may leave through the C ABI as an exception)
extern "C" int srk_ba_upload_scene(srk_ba* h, double f0, int64_t N, const double* pts_in, int32_t M,
                                   const double* cam_R_in, const double* cam_T_in, const double* K_in, int shared_k,
                                   const int64_t* row_ptr, const int32_t* obs_frame, const double* obs_uv,
                                   int already_normalized)
{
    try {
        return upload_scene_impl(h, f0, N, pts_in, M, cam_R_in, cam_T_in, K_in, shared_k, row_ptr, obs_frame, obs_uv, already_normalized);
    } catch (const std::bad_alloc&) {
        if (h) h->last_error = "upload: out of host memory", h->have_scene = false;
        return SRK_E_NOMEM;
    } catch (const std::exception& e) {
        if (h) h->last_error = std::string("upload: ") + e.what(), h->have_scene = false;
        return SRK_E_DEVICE;
    } catch (...) {
        if (h) h->last_error = "upload: unknown exception", h->have_scene = false;
        return SRK_E_DEVICE;
    }
}
static int upload_scene_impl(srk_ba* h, double f0, int64_t N, const double* pts_in, int32_t M,
                             const double* cam_R_in, const double* cam_T_in, const double* K_in, int shared_k,
                             const int64_t* row_ptr, const int32_t* obs_frame, const double* obs_uv,
                             int already_normalized)
{
    auto t_stage = std::chrono::steady_clock::now();
    auto stage = [&](const char* what) { // SRK_DEBUG=1: where the host time of an upload goes
        if (!srk_debug()) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "srk_ba upload: %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_stage).count());
        t_stage = now;
    };
    int rc = validate_scene(h, f0, N, pts_in, M, cam_R_in, cam_T_in, K_in, row_ptr, obs_frame, obs_uv);
    if (rc != SRK_OK) return rc;
    if (refuse_modes(h, h->fixed_k, h->deterministic, h->store_f32, h->schur_fp32, h->world, !h->igroup_user.empty())) return SRK_E_ARGS;
    if (!h->obs_info.set.q.empty() &&
        check_information(h, "upload", h->obs_info.set.q.data(), (int64_t)h->obs_info.set.q.size(), N, row_ptr) != SRK_OK)
        return SRK_E_ARGS;
    // the settings against this scene, the switched-on factors and sets, and their pairs for the planner (srk_factors.cpp)
    const std::string refused = srk_select_factors(h->cst.set, h->pri.set, h->rp.set, h->jp.set, N, M, h->sel);
    if (!refused.empty()) { h->last_error = refused; return SRK_E_ARGS; }
    rearm_fusion(h);
    stage("validate");
    HIPCHK(h, hipSetDevice(h->device));
    h->have_scene = false;
    h->seen_global = -1;
    int64_t O = row_ptr[N];
    std::vector<double> pts(pts_in, pts_in + 3 * N), camR(cam_R_in, cam_R_in + 9 * (int64_t)M),
        camT(cam_T_in, cam_T_in + 3 * (int64_t)M);
    h->normalized_on_upload = false;
    if (!already_normalized) {
        // unity_t1_comp_ind_ = 1, unity_t1_comp_value_ = 1.0 (bundle-adj-kanatani.h:131-132); :680-682
        if (!srk_ba_normalize_scene(N, pts.data(), M, camR.data(), camT.data(), 1.0, 1, &h->nrm)) {
            h->last_error = "scene cannot be normalised (cam0->cam1 translation component ~ 0)";
            return 1; // reference: ComputeInplace returns false, status string stays empty
        }
        h->normalized_on_upload = true;
    } else {
        std::memset(&h->nrm, 0, sizeof h->nrm);
        h->nrm.R0[0] = h->nrm.R0[4] = h->nrm.R0[8] = 1;
        h->nrm.world_scale = 1;
    }
    std::vector<double> Kexp(9 * (int64_t)M);
    for (int32_t j = 0; j < M; ++j) std::memcpy(&Kexp[9 * (int64_t)j], shared_k ? K_in : K_in + 9 * (int64_t)j, 72);
    h->shk_G = 0;
    if (!h->igroup_user.empty()) { // shared intrinsics: one K per group, so every frame of a group must carry the same one
        if ((int64_t)h->igroup_user.size() != (int64_t)M) { h->last_error = "intrinsic groups: set for another number of frames"; return SRK_E_ARGS; }
        std::vector<int32_t> first((size_t)h->igroup_n, -1);
        for (int32_t j = 0; j < M; ++j) {
            int32_t& f = first[(size_t)h->igroup_user[(size_t)j]];
            if (f < 0) f = j;
            else if (std::memcmp(&Kexp[9 * (size_t)f], &Kexp[9 * (size_t)j], 72) != 0) {
                h->last_error = "intrinsic groups: the frames of a group carry different intrinsics";
                return SRK_E_ARGS;
            }
        }
        // K in the convention the closed-form derivatives assume, K(2,2) = f0 (the same projections); the K step then
        // follows the derivatives of the error in every unit of K
        h->shk_k22_user.assign((size_t)M, 0.0);
        for (int32_t j = 0; j < M; ++j) {
            double* k = &Kexp[9 * (size_t)j];
            if (!(std::isfinite(k[8]) && k[8] != 0.0)) { h->last_error = "intrinsic groups: K(2,2) must be finite and non-zero"; return SRK_E_ARGS; }
            h->shk_k22_user[(size_t)j] = k[8];
            const double s = f0 / k[8];
            for (int e = 0; e < 8; ++e) k[e] *= s;
            k[8] = f0;
        }
    }

    if (!h->frame_order_given.empty() && (int64_t)h->frame_order_given.size() != (int64_t)M) { h->last_error = "the supplied frame order is for another number of frames"; return SRK_E_ARGS; }
    // ---- the plan (srk_plan.cpp, host only): the internal frame and landmark order, the runs, tasks and tables of every kernel
    SrkPlanOptions opt{ h->fixed_k, h->deterministic, h->schur_fp32, h->jac_mode, h->frame_order_mode, &h->frame_order_given,
                        h->allreduce || h->comm /* multi_rank */, h->cus };
#ifdef SRK_DEV
    if (const char* e = getenv("SRK_SCHUR_RUN_SPLIT")) opt.run_split = std::max(1, std::min(16, atoi(e))); // development: fixed cut
    opt.no_long = getenv("SRK_SCHUR_NO_LONG") != nullptr; // development: everything through the per-landmark kernel
#endif
    opt.rel_a = h->sel.rel_a.data();
    opt.rel_b = h->sel.rel_b.data();
    opt.n_rel = (int64_t)h->sel.rel_a.size();
    SrkScenePlan plan;
    srk_plan_scene({ N, M, row_ptr, obs_frame, obs_uv, pts.data(), camR.data(), camT.data(), Kexp.data() }, opt, plan, stage);
    if (!h->igroup_user.empty()) {
        h->shk_G = h->igroup_n;
        h->shk_grp_h.assign((size_t)M, 0);
        for (int32_t j = 0; j < M; ++j) h->shk_grp_h[(size_t)j] = h->igroup_user[(size_t)(plan.frame_user.empty() ? j : plan.frame_user[(size_t)j])];
    }
    SrkDims d{};
    d.N = N;
    d.M = M;
    d.O = O;
    d.Os = ((O + 63) / 64) * 64;
    if (d.Os == 0) d.Os = 64;
    d.Ns = ((N + 63) / 64) * 64;
    if (d.Ns == 0) d.Ns = 64;
    d.fv = h->fixed_k ? 6 : 10;
    d.ld = ((d.fv * (int64_t)M + SRK_CHOL_NB - 1) / SRK_CHOL_NB) * SRK_CHOL_NB;
    d.comp = 1;
    d.g0 = plan.g0;
    d.g1 = plan.g1;
    // a setting without the reference's gauge: no frame index matches, so srk_is_fixed_var is false for every variable.  The
    // constant blocks' masking passes are then the only source of identity rows besides the padding;
    // position priors, or joint pose priors as the caller asserts, fix the similarity (sections 14 and 18)
    if ((h->cst.set.set && !h->cst.set.keep_gauge) || (h->pri.set.set && !h->pri.set.keep_gauge) || (h->jp.set.set && !h->jp.set.keep_gauge)) d.g0 = d.g1 = -1;
    d.w_f32 = h->store_f32 ? 1 : 0;
    h->d = d;
    h->f0 = f0;
    h->cov_pt_frame0.clear();
    h->mg_obs_frame.clear();

    // ---- the device buffers of the scene, each named once: allocated in this order, then filled from its host source (if any)
    struct Up { DevBuf& buf; const void* src; size_t bytes; }; // src NULL: nothing to copy
    std::vector<Up> up;
    auto add = [&](DevBuf& b, const void* src, int64_t bytes) { up.push_back({ b, src, (size_t)bytes }); };
    auto tab = [&](DevBuf& b, const auto& v, size_t at_least = 0) { add(b, v.empty() ? nullptr : v.data(), (int64_t)(sizeof(v[0]) * std::max(v.size(), at_least))); };
    // several ranks, damping-parallel schedule: one slot per damping factor of a round (at most three)
    // (srk_ba_set_speculation(h, 0) = strictly one attempt at a time, with several ranks as well: one slot, hence the
    // all-reduce schedule without pairs)
    const int n_slots = (opt.multi_rank && h->dp_schedule && h->speculate && (h->world >= 2 || h->dp_force))
                            ? (h->dp_force ? SRK_SLOTS : std::min(SRK_SLOTS, h->world))
                            : (h->speculate ? 2 : 1);
    for (int w = 0; w <= n_slots; ++w) { // the current scene (from the plan) and one trial scene per attempt slot
        add(h->pts[w], w ? nullptr : plan.pts.data(), 24 * N);
        add(h->camR[w], w ? nullptr : plan.camR.data(), 72 * (int64_t)M);
        add(h->camT[w], w ? nullptr : plan.camT.data(), 24 * (int64_t)M);
        add(h->cam[w], nullptr, 8 * SRK_CAM_PACK * (int64_t)M);
        if (h->shk_G > 0) add(h->Ks[w], w ? nullptr : plan.K.data(), 72 * (int64_t)M);
    }
    tab(h->pts0, plan.pts); tab(h->camR0, plan.camR); tab(h->camT0, plan.camT); tab(h->K, plan.K);
    tab(h->row_ptr, plan.row_ptr_int); tab(h->obs_frame, plan.obs_frame); tab(h->obs_pt, plan.obs_pt); tab(h->obs_uv, plan.obs_uv);
    tab(h->col_ptr, plan.col_ptr); tab(h->fobs_pt, plan.fobs_pt); tab(h->fobs_uv, plan.fobs_uv);
    add(h->W, nullptr, (d.w_f32 ? 4 : 8) * SRK_WF_PLANES * d.Os); // the 21 rank-2 factors of every point-frame block, fp64 or (opt-in) float
    add(h->Vg, nullptr, 8 * 9 * d.Ns);
    add(h->Ug, nullptr, 8 * SRK_UGS(d.fv) * (int64_t)M); // the frame sums: 65 a frame, 27 with fixed intrinsics
    bool new_flags[SRK_SLOTS] = {};
    for (int sl = 0; sl < SRK_SLOTS; ++sl) {
        srk_ba::Attempt& a = h->att[sl];
        a.allocated = sl < n_slots;
        if (!a.allocated) continue;
        if (plan.det_active) {
            add(a.det_stage, nullptr, 8 * (int64_t)SRK_DET_STRIDE * plan.n_groups);
            add(a.det_rhs, nullptr, 8 * (int64_t)SRK_DET_LD * plan.n_groups);
        }
        add(a.S, nullptr, 8 * d.ld * d.ld);
        add(a.rhs, nullptr, 8 * d.ld);
        add(a.wy, nullptr, 8 * 2 * d.ld);
        add(a.dc, nullptr, 8 * d.ld);
        add(a.acc, nullptr, 8 * 3 * d.Ns + 64);
        add(a.dx, nullptr, 24 * N);
        // (position priors: their partial sums sit behind the observation partials of either error kernel)
        add(a.err_partial, nullptr, 8 * (std::max<int64_t>(1024, srk_error_partials_staged(d)) +
                                         (h->pri.set.set ? srk_prior_partials((int64_t)h->pri.set.pt_idx.size(), (int64_t)h->pri.set.fr_idx.size()) : 0) +
                                         srk_relpose_partials((int64_t)h->sel.rp_act.size()) + srk_jprior_partials((int64_t)h->sel.jp_act.size())));
        add(a.info, nullptr, 64);
        add(a.dinv, nullptr, 8 * 64 * d.ld);
        add(a.irr, nullptr, 4 * (N + 2));
        new_flags[sl] = !a.sync_flags.p; // flag words of the fused outer-step kernel: zeroed ONCE (they hold launch epochs)
        if (new_flags[sl]) add(a.sync_flags, nullptr, 4 * SRK_SYNC_WORDS);
    }
    tab(h->cal_list, plan.cal_list);
    tab(h->grp_first, plan.grp_first); tab(h->grp_count, plan.grp_count); tab(h->grp_nf, plan.grp_nf); tab(h->grp_frames, plan.grp_frames);
    tab(h->obs_slot, plan.obs_slot); tab(h->pt_mask, plan.pt_mask); tab(h->gen_list, plan.gen_list);
    tab(h->lg_item, plan.lg_item); tab(h->lg_np, plan.lg_np); tab(h->lg_nf, plan.lg_nf); tab(h->lg_pts, plan.lg_pts);
    tab(h->lg_frames, plan.lg_frames); tab(h->lg_obs_off, plan.lg_obs_off); tab(h->lg_obs, plan.lg_obs);
    tab(h->wg_jmin, plan.wg_jmin);
    if (plan.jac_runs) {
        tab(h->jr_first, plan.jr_first); tab(h->jr_count, plan.jr_count); tab(h->jr_jmin, plan.jr_jmin);
        if (plan.jac_runs_masked) tab(h->jr_group, plan.jr_group);
    }
    if (plan.det_active) {
        tab(h->dj_ptr, plan.dj_ptr); tab(h->dj_ent, plan.dj_ent, 1);
        add(h->dj_stage, nullptr, 8 * (int64_t)SRK_UG * 64 * (int64_t)plan.jr_first.size());
        tab(h->ds_pair_ptr, plan.ds_pair_ptr); tab(h->ds_pair_fa, plan.ds_pair_fa, 1); tab(h->ds_pair_fb, plan.ds_pair_fb, 1); tab(h->ds_pair_ent, plan.ds_pair_ent, 1);
        tab(h->ds_f_ptr, plan.ds_f_ptr); tab(h->ds_f_ent, plan.ds_f_ent, 1);
    }
    if (plan.jr_own_runs) {
        tab(h->jd_nf, plan.jd_nf); tab(h->jd_frames, plan.jd_frames); tab(h->jd_mask, plan.jd_mask);
    }
    for (const Up& u : up)
        if ((rc = dev_alloc(h, u.buf, u.bytes)) != SRK_OK) return rc;
    hipStream_t s = h->main_stream;
    stage("device allocations");
    for (const Up& u : up)
        if (u.src && u.bytes > 0) HIPCHK(h, hipMemcpyAsync(u.buf.p, u.src, u.bytes, hipMemcpyHostToDevice, s));
    for (int sl = 0; sl < SRK_SLOTS; ++sl) {
        srk_ba::Attempt& a = h->att[sl];
        if (!a.allocated) continue;
        HIPCHK(h, hipMemsetAsync(a.irr.p, 0, 4, s));
        if (new_flags[sl]) HIPCHK(h, hipMemset(a.sync_flags.p, 0, 4 * SRK_SYNC_WORDS));
        a.sync.flags = P<unsigned>(a.sync_flags);
        a.sync.fused = h->chol_fused;
        HIPCHK(h, hipMemsetAsync(a.dc.p, 0, 8 * d.ld, s));
        HIPCHK(h, hipMemsetAsync(a.dx.p, 0, 24 * N > 0 ? 24 * N : 8, s));
    }
    h->cur = 0;
    for (int sl = 0; sl < SRK_SLOTS; ++sl) h->att[sl].trial = sl + 1;
    rc = compute_cam_packs(h, 0);
    if (rc != SRK_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(s)); // the plan's tables go out of scope
    // what later calls read of the plan stays with the handle (copied, not moved: the handle's vectors keep their storage from
    // upload to upload, and the planner's allocations come and go as a block)
    static_cast<SrkPlanKept&>(*h) = plan;
    stage("host-to-device copies");
    rc = build_envelope(h);
    if (rc != SRK_OK) return rc;
    if (h->shk_G > 0) {
        if ((rc = build_shared_k(h)) != SRK_OK) return rc;
    } else {
        for (auto& a : h->att)
            for (DevBuf* b : { &a.Ssh, &a.rsh, &a.ysh, &a.dcsh, &a.dinvsh, &a.Tsh }) dev_free(*b);
    }
    stage("skyline, solver plans");
    if ((rc = apply_information(h)) != SRK_OK) return rc;
    if ((rc = apply_constant_blocks(h)) != SRK_OK) return rc;
    if ((rc = apply_position_priors(h)) != SRK_OK) return rc;
    if ((rc = apply_relative_pose_factors(h)) != SRK_OK) return rc;
    if ((rc = apply_joint_pose_priors(h)) != SRK_OK) return rc;
    h->have_scene = true;
    return SRK_OK;
}


// entry of an upload / optimise call: the fused outer steps again after an earlier call's hand-off timeout (see chol_fused_wanted).
// Every rank of a sharded run counts the same timeouts (the status words are exchanged), so all re-arm together.
static void rearm_fusion(srk_ba* h)
{
    if (!h->chol_fused_wanted || h->chol_fused || h->fusion_rearms_left <= 0) return;
    --h->fusion_rearms_left;
    h->chol_fused = true;
    for (auto& a : h->att) a.sync.fused = true;
}
// a hand-off of the fused solve timed out: the unfused launch sequence for the rest of this call (see chol_fused_wanted)
static void fusion_off(srk_ba* h)
{
    ++h->sync_timeouts;
    h->chol_fused = false;
    for (auto& a : h->att) a.sync.fused = false;
}

// after a failed solve: every slot's system and zero-initialised plan buffers back to zeros (see srk_ba::poisoned)
static int clear_poison(srk_ba* h)
{
    if (!h->poisoned) return SRK_OK;
    const SrkDims& d = h->d;
    for (auto& a : h->att) {
        if (!a.allocated) continue;
        HIPCHK(h, hipStreamSynchronize(a.stream));
        HIPCHK(h, hipMemsetAsync(a.S.p, 0, (size_t)(8 * d.ld * d.ld), h->main_stream));
        HIPCHK(h, hipMemsetAsync(a.rhs.p, 0, (size_t)(8 * d.ld), h->main_stream));
        HIPCHK(h, hipMemsetAsync(a.wy.p, 0, (size_t)(16 * d.ld), h->main_stream));
        HIPCHK(h, hipMemsetAsync(a.dc.p, 0, (size_t)(8 * d.ld), h->main_stream));
        HIPCHK(h, hipMemsetAsync(a.dx.p, 0, d.N > 0 ? (size_t)(24 * d.N) : 8, h->main_stream));
        HIPCHK(h, hipMemsetAsync(a.info.p, 0, 4, h->main_stream));
        HIPCHK(h, hipMemsetAsync(a.acc.p, 0, (size_t)(8 * 3 * d.Ns + 64), h->main_stream));
        if (h->shk_G > 0) {
            const size_t ldb = (size_t)h->shk_ldb;
            HIPCHK(h, hipMemsetAsync(a.Ssh.p, 0, 8 * ldb * ldb, h->main_stream));
            HIPCHK(h, hipMemsetAsync(a.rsh.p, 0, 8 * ldb, h->main_stream));
            HIPCHK(h, hipMemsetAsync(a.ysh.p, 0, 16 * ldb, h->main_stream));
            HIPCHK(h, hipMemsetAsync(a.dcsh.p, 0, 8 * ldb, h->main_stream));
        }
        for (size_t i = 0; i < a.plan_bufs.size(); ++i)
            if (a.plan_zeroed[i]) HIPCHK(h, hipMemsetAsync(a.plan_bufs[i].p, 0, a.plan_bufs[i].bytes, h->main_stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->main_stream));
    h->poisoned = false;
    return SRK_OK;
}

// a per-frame array of `w` doubles per frame, just downloaded in the internal frame order -> the caller's order
static void frames_to_user(const srk_ba* h, double* a, int w)
{
    if (h->frame_int.empty()) return;
    const int32_t M = h->d.M;
    std::vector<double> tmp(a, a + (size_t)w * (size_t)M);
    for (int32_t j = 0; j < M; ++j) std::memcpy(a + (size_t)w * (size_t)j, &tmp[(size_t)w * (size_t)h->frame_int[(size_t)j]], (size_t)(8 * w));
}

extern "C" int srk_ba_reset_scene(srk_ba* h)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->main_stream;
    for (int sl = 1; sl < SRK_SLOTS; ++sl) HIPCHK(h, hipStreamSynchronize(h->att[sl].stream)); // a speculative attempt may still read the current scene
    {
        int rcp = clear_poison(h);
        if (rcp != SRK_OK) return rcp;
    }
    h->cur = 0;
    for (int sl = 0; sl < SRK_SLOTS; ++sl) h->att[sl].trial = sl + 1;
    if (h->d.N > 0) HIPCHK(h, hipMemcpyAsync(h->pts[0].p, h->pts0.p, 24 * h->d.N, hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemcpyAsync(h->camR[0].p, h->camR0.p, 72 * (int64_t)h->d.M, hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemcpyAsync(h->camT[0].p, h->camT0.p, 24 * (int64_t)h->d.M, hipMemcpyDeviceToDevice, s));
    if (h->shk_G > 0) HIPCHK(h, hipMemcpyAsync(h->Ks[0].p, h->K.p, 72 * (int64_t)h->d.M, hipMemcpyDeviceToDevice, s)); // the uploaded K
    return compute_cam_packs(h, 0);
}

extern "C" int srk_ba_download_scene(srk_ba* h, double* pts, double* cam_R, double* cam_T, int revert)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->main_stream;
    int c = h->cur;
    std::vector<double> tmp((size_t)(3 * h->d.N));
    if (h->d.N > 0) HIPCHK(h, hipMemcpyAsync(tmp.data(), h->pts[c].p, 24 * h->d.N, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(cam_R, h->camR[c].p, 72 * (int64_t)h->d.M, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(cam_T, h->camT[c].p, 24 * (int64_t)h->d.M, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    frames_to_user(h, cam_R, 9);
    frames_to_user(h, cam_T, 3);
    for (int64_t i = 0; i < h->d.N; ++i) std::memcpy(pts + 3 * h->perm[(size_t)i], &tmp[(size_t)(3 * i)], 24);
    if (revert && h->normalized_on_upload) srk_ba_revert_normalization(h->d.N, pts, h->d.M, cam_R, cam_T, &h->nrm); // :706
    return SRK_OK;
}

// ------------------------------------------------------------------ phases

static int exchange(srk_ba* h, srk_ba::Attempt& a, double* dev_ptr, int64_t count)
{
    if (h->comm) { // RCCL on this attempt's stream: ordered behind the kernels that filled the buffer, nothing waits on the host
        ncclComm_t comm = (a.slot == 1 && h->comm2) ? h->comm2 : h->comm; // the second slot's own communicator
        ncclResult_t r = rccl().AllReduce(dev_ptr, dev_ptr, (size_t)count, ncclDouble, ncclSum, comm, a.stream);
        if (r != ncclSuccess) {
            h->last_error = std::string("ncclAllReduce: ") + rccl().GetErrorString(r);
            return SRK_E_DEVICE;
        }
        return SRK_OK;
    }
    if (!h->allreduce) return SRK_OK;
    // the hook reduces on its own (RCCL) stream: everything queued on ours must have landed first, and the hook
    // returns only after the reduced values are visible
    HIPCHK(h, hipStreamSynchronize(a.stream));
    int rc = h->allreduce(h->allreduce_ctx, dev_ptr, count);
    if (rc != 0) {
        h->last_error = "allreduce hook failed";
        return SRK_E_DEVICE;
    }
    return SRK_OK;
}

// ---- collectives of the damping-parallel schedule (world >= 2).  A group = the same operation for the slots k = 0 .. G-1
// (root of slot k: k % world), issued by every rank in the same program order.  Natively: ONE communicator on ONE stream
// (comm_stream) -- the group waits for each slot's producer stream, runs as one ncclGroup (the rooted operations of
// different roots share the links), and each slot's stream waits for it; nothing waits on the host.  With the callback
// (gloo rehearsals, a caller's own transport) only a sum is available: a reduce is an all-reduce whose result the other
// ranks ignore, a broadcast an all-reduce of a buffer the other ranks zeroed; the callback blocks the host.
enum { SRK_COLL_ALLREDUCE = 0, SRK_COLL_REDUCE = 1, SRK_COLL_BCAST = 2 };
#define SRK_RETRY_ALLREDUCE 1000 // (internal) the damping-parallel round failed its self-check: the all-reduce schedule from here on
#ifdef SRK_DEV
static int g_dp_corrupt = 0; // test hook: the next self-check finds a mismatch at stage 1 (reduce) / 2 (broadcast)
extern "C" void srk_dbg_dp_corrupt(int stage) { g_dp_corrupt = stage; }
#endif
// {sum, sum of magnitudes} of a device buffer in a fixed order, to the host (blocking: first round of a handle only)
static int dp_checksum(srk_ba* h, hipStream_t st, const double* p, int64_t n, double out[2])
{
    int rc = dev_alloc(h, h->dp_chk, 8 * (512 + 2 + 16));
    if (rc != SRK_OK) return rc;
    srk_launch_checksum(st, p, n, P<double>(h->dp_chk), P<double>(h->dp_chk) + 512);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, P<double>(h->dp_chk) + 512, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return SRK_OK;
}
// sum over the ranks of n <= 16 host doubles through the communicator's plain all-reduce (blocking)
static int dp_allreduce_host(srk_ba* h, double* v, int n)
{
    int rc = dev_alloc(h, h->dp_chk, 8 * (512 + 2 + 16));
    if (rc != SRK_OK) return rc;
    double* stage = P<double>(h->dp_chk) + 514;
    HIPCHK(h, hipMemcpyAsync(stage, v, (size_t)(8 * n), hipMemcpyHostToDevice, h->comm_stream));
    ncclResult_t r = rccl().AllReduce(stage, stage, (size_t)n, ncclDouble, ncclSum, h->comm, h->comm_stream);
    if (r != ncclSuccess) { h->last_error = std::string("ncclAllReduce (self-check): ") + rccl().GetErrorString(r); return SRK_E_DEVICE; }
    HIPCHK(h, hipMemcpyAsync(v, stage, (size_t)(8 * n), hipMemcpyDeviceToHost, h->comm_stream));
    HIPCHK(h, hipStreamSynchronize(h->comm_stream));
    return SRK_OK;
}
static int coll_group(srk_ba* h, int op, int G, double* const* ptrs, const int64_t* counts)
{
    if (h->comm) {
        for (int k = 0; k < G; ++k) {
            HIPCHK(h, hipEventRecord(h->att[k].ev_a, h->att[k].stream));
            HIPCHK(h, hipStreamWaitEvent(h->comm_stream, h->att[k].ev_a, 0));
        }
        const bool rooted = rccl().rooted && op != SRK_COLL_ALLREDUCE;
        if (!rooted && op == SRK_COLL_BCAST)
            for (int k = 0; k < G; ++k)
                if (h->rank != k % h->world) HIPCHK(h, hipMemsetAsync(ptrs[k], 0, (size_t)(8 * counts[k]), h->comm_stream));
        ncclResult_t r = ncclSuccess;
        if (rooted) r = rccl().GroupStart();
        for (int k = 0; k < G && r == ncclSuccess; ++k) {
            const int root = k % h->world;
            if (rooted && op == SRK_COLL_REDUCE)
                r = rccl().Reduce(ptrs[k], ptrs[k], (size_t)counts[k], ncclDouble, ncclSum, root, h->comm, h->comm_stream);
            else if (rooted && op == SRK_COLL_BCAST)
                r = rccl().Broadcast(ptrs[k], ptrs[k], (size_t)counts[k], ncclDouble, root, h->comm, h->comm_stream);
            else
                r = rccl().AllReduce(ptrs[k], ptrs[k], (size_t)counts[k], ncclDouble, ncclSum, h->comm, h->comm_stream);
        }
        if (rooted) {
            ncclResult_t r2 = rccl().GroupEnd();
            if (r == ncclSuccess) r = r2;
        }
        if (r != ncclSuccess) {
            h->last_error = std::string("RCCL collective: ") + rccl().GetErrorString(r);
            return SRK_E_DEVICE;
        }
        HIPCHK(h, hipEventRecord(h->ev_comm, h->comm_stream));
        for (int k = 0; k < G; ++k) HIPCHK(h, hipStreamWaitEvent(h->att[k].stream, h->ev_comm, 0));
        return SRK_OK;
    }
    if (!h->allreduce) return SRK_OK;
    for (int k = 0; k < G; ++k) {
        hipStream_t st = h->att[k].stream;
        if (op == SRK_COLL_BCAST && h->rank != k % h->world) HIPCHK(h, hipMemsetAsync(ptrs[k], 0, (size_t)(8 * counts[k]), st));
        HIPCHK(h, hipStreamSynchronize(st));
        if (h->allreduce(h->allreduce_ctx, ptrs[k], counts[k]) != 0) {
            h->last_error = "allreduce hook failed";
            return SRK_E_DEVICE;
        }
    }
    return SRK_OK;
}

// with_status: {solver info, point-update finite flag (lives behind acc)} are packed next to the error scalar and
// summed over the ranks with it, so every rank takes the same accept / reject decision
// the robust loss and the observation information for the kernels (DESIGN.md sections 10, 12): NULL when neither is set, so
// the plain least-squares kernels run
static const SrkLoss* robust_loss(const srk_ba* h, SrkLoss& L)
{
    if (h->loss_kind == SRK_LOSS_NONE && !h->obs_info.on) return nullptr;
    L.kind = h->loss_kind;
    L.d = h->loss_delta_pix / h->f0;
    L.d2 = L.d * L.d;
    L.q = h->obs_info.on ? P<double>(h->obs_info.buf[InfoFamily::Q]) : nullptr;
    L.qf = h->obs_info.on && !h->fobs_of.empty() ? P<double>(h->obs_info.buf[InfoFamily::QF]) : nullptr;
    return &L;
}

static int phase_error(srk_ba* h, srk_ba::Attempt& a, int which, double* err_host, bool with_status = false, bool no_exchange = false)
{
    const SrkDims& d = h->d;
    hipStream_t s = a.stream;
    int32_t np = srk_error_partials(d);
    SrkLoss L;
    SrkPrior pr;
    const SrkPrior* prior = position_priors(h, pr); // the prior sums of the scene being scored
    SrkRelPose rpl;
    const SrkRelPose* relpose = relpose_factors(h, rpl); // the factor sum of the scene being scored
    SrkJointPrior jpl;
    const SrkJointPrior* jprior = joint_priors(h, jpl); // the joint pose priors' sum of the scene being scored
    // (one event pair for all attempt slots: with speculation on, the *_pass_ms calls report the attempt that recorded last)
    srk_launch_error(s, d, P<double>(h->pts[which]), P<double>(h->cam[which]), P<int32_t>(h->obs_frame),
                     P<int32_t>(h->obs_pt), P<double>(h->obs_uv), P<double>(a.err_partial), np, a.err_dst,
                     h->jac_fused ? P<int32_t>(h->wg_jmin) : nullptr, with_status ? P<int>(a.info) : nullptr,
                     with_status ? reinterpret_cast<int*>(reinterpret_cast<char*>(a.acc.p) + 8 * 3 * d.Ns) : nullptr,
                     robust_loss(h, L), prior, error_pass_events(h, h->pri.pass[1], prior != nullptr), relpose,
                     error_pass_events(h, h->rp.pass[2], relpose != nullptr), jprior, error_pass_events(h, h->jp.pass[2], jprior != nullptr));
    HIPCHK(h, hipGetLastError());
    int rc = no_exchange ? SRK_OK : exchange(h, a, a.err_dst, with_status ? 3 : 1);
    if (rc != SRK_OK) return rc;
    if (err_host) {
        HIPCHK(h, hipMemcpyAsync(err_host, a.err_dst, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
    }
    return SRK_OK;
}

static int phase_derivatives(srk_ba* h)
{
    const SrkDims& d = h->d;
    hipStream_t s = h->main_stream;
    int c = h->cur;
    HIPCHK(h, hipMemsetAsync(h->Vg.p, 0, 8 * 9 * d.Ns, s));
    HIPCHK(h, hipMemsetAsync(h->Ug.p, 0, 8 * SRK_UGS(d.fv) * (int64_t)d.M, s));
    if (h->profile_level >= 1) HIPCHK(h, hipEventRecord(h->ev[12], s));
    const SrkDetJac detj{ P<double>(h->dj_stage), P<int32_t>(h->dj_ptr), P<int32_t>(h->dj_ent) };
    SrkLoss Ls;
    const SrkLoss* L = robust_loss(h, Ls); // the IRLS weights, recomputed in every derivative pass
    if (h->jac_runs) {
        srk_launch_jac_runs(s, d, P<double>(h->pts[c]), P<double>(h->cam[c]), P<int64_t>(h->row_ptr), P<int32_t>(h->obs_frame),
                            P<double>(h->obs_uv), P<double>(h->W), P<double>(h->Vg), P<double>(h->Ug), P<int32_t>(h->jr_first),
                            P<int32_t>(h->jr_count), h->jr_tasks, P<int32_t>(h->jr_jmin),
                            h->jac_runs_masked ? P<int32_t>(h->jr_group) : nullptr,
                            h->jr_own_runs ? P<int32_t>(h->jd_nf) : P<int32_t>(h->grp_nf),
                            h->jr_own_runs ? P<int32_t>(h->jd_frames) : P<int32_t>(h->grp_frames),
                            h->jr_own_runs ? P<uint32_t>(h->jd_mask) : P<uint32_t>(h->pt_mask), h->det_active ? &detj : nullptr,
                            h->jr_own_runs ? SRK_JD_MAXNF_HOST : SRK_GRP_MAXNF_HOST, L);
        if (h->profile_level >= 1) HIPCHK(h, hipEventRecord(h->ev[13], s));
    } else if (h->jac_fused) {
        srk_launch_jac_fused(s, d, P<double>(h->pts[c]), P<double>(h->cam[c]), P<int32_t>(h->obs_frame),
                             P<int32_t>(h->obs_pt), P<double>(h->obs_uv), P<double>(h->W), P<double>(h->Vg),
                             P<double>(h->Ug), P<int32_t>(h->wg_jmin), L);
        if (h->profile_level >= 1) HIPCHK(h, hipEventRecord(h->ev[13], s));
    } else {
        srk_launch_jac_points(s, d, P<double>(h->pts[c]), P<double>(h->cam[c]), P<int32_t>(h->obs_frame),
                              P<int32_t>(h->obs_pt), P<double>(h->obs_uv), P<double>(h->W), P<double>(h->Vg), L);
        if (h->profile_level >= 1) HIPCHK(h, hipEventRecord(h->ev[13], s));
        srk_launch_jac_frames(s, d, h->max_frame_obs, P<double>(h->pts[c]), P<double>(h->cam[c]),
                              P<int64_t>(h->col_ptr), P<int32_t>(h->fobs_pt), P<double>(h->fobs_uv), P<double>(h->Ug), L);
    }
    HIPCHK(h, hipGetLastError());
    int rc;
    SrkPrior pr;
    if (const SrkPrior* prior = position_priors(h, pr)) // 2 L into the blocks, 2 L (x - xbar) into the gradients
        if ((rc = timed_launch(h, h->pri.pass[0], s, [&] { srk_launch_prior_add(s, d, P<double>(h->pts[c]), P<double>(h->cam[c]), *prior, P<double>(h->Vg), P<double>(h->Ug)); })) != SRK_OK) return rc;
    SrkRelPose rpl;
    if (const SrkRelPose* relpose = relpose_factors(h, rpl)) // the factors' terms into Ug, the coupling blocks aside
        if ((rc = timed_launch(h, h->rp.pass[0], s, [&] { srk_launch_relpose_add(s, d, P<double>(h->cam[c]), *relpose, P<double>(h->Ug)); })) != SRK_OK) return rc;
    SrkJointPrior jpl;
    if (const SrkJointPrior* jprior = joint_priors(h, jpl)) // the sets' terms into Ug, the coupling blocks aside
        if ((rc = timed_launch(h, h->jp.pass[0], s, [&] { srk_launch_jprior_add(s, d, P<double>(h->cam[c]), *jprior, P<double>(h->Ug)); })) != SRK_OK) return rc;
    if (h->cst.n_pts > 0) // constant landmarks: identity block, zero gradient, zero point-frame blocks
        if ((rc = timed_launch(h, h->cst.pass[0], s, [&] { srk_launch_const_points(s, d, P<int32_t>(h->cst.buf[ConstFamily::PTS]), h->cst.n_pts, P<int64_t>(h->row_ptr), P<double>(h->W), P<double>(h->Vg)); })) != SRK_OK) return rc;
    // landmark shards: Ug stays this rank's partial sum; it enters the reduced camera system before that is summed
    return SRK_OK;
}

static int phase_schur(srk_ba* h, srk_ba::Attempt& a, double c, bool local_only = false);
// the reduced camera system of this rank's landmarks, packed for an exchange: band + right-hand side behind it
static int schur_pack(srk_ba* h, srk_ba::Attempt& a)
{
    const SrkDims& d = h->d;
    hipStream_t s = a.stream;
    int rc;
    if ((rc = dev_alloc(h, a.packed, (size_t)(8 * (h->band_packed + d.ld)))) != SRK_OK) return rc;
    double* tail = P<double>(a.packed) + h->band_packed;
    srk_launch_band_pack(s, d.ld, P<int64_t>(h->band_col), P<int64_t>(h->band_off), P<double>(a.S), P<double>(a.packed), 0);
    HIPCHK(h, hipMemcpyAsync(tail, a.rhs.p, (size_t)(8 * d.ld), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipGetLastError());
    return SRK_OK;
}
static int schur_unpack(srk_ba* h, srk_ba::Attempt& a)
{
    const SrkDims& d = h->d;
    hipStream_t s = a.stream;
    double* tail = P<double>(a.packed) + h->band_packed;
    srk_launch_band_pack(s, d.ld, P<int64_t>(h->band_col), P<int64_t>(h->band_off), P<double>(a.S), P<double>(a.packed), 1);
    HIPCHK(h, hipMemcpyAsync(a.rhs.p, tail, (size_t)(8 * d.ld), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipGetLastError());
    return SRK_OK;
}
static int phase_schur(srk_ba* h, srk_ba::Attempt& a, double c, bool local_only)
{
    const SrkDims& d = h->d;
    hipStream_t s = a.stream;
    srk_launch_env_zero(s, d.ld, P<int64_t>(h->env_col), P<double>(a.S), P<double>(a.rhs), P<int32_t>(a.irr)); // S band, rhs, hand-back counter
    const SrkDetSchur dets{ P<double>(a.det_stage), P<double>(a.det_rhs), P<int32_t>(h->ds_pair_ptr), P<int32_t>(h->ds_pair_fa),
                            P<int32_t>(h->ds_pair_fb), P<int32_t>(h->ds_pair_ent), h->ds_n_pairs, P<int32_t>(h->ds_f_ptr), P<int32_t>(h->ds_f_ent) };
    // the runs of at most SRK_WS_NF_HOST frames through k_schur_mm (with fixed intrinsics on 6-wide blocks, which are built
    // neither for fp32 run sums nor for the deterministic mode: srk_dispatch_det, srk_launch_schur_grouped), the wider ones
    // through k_schur_grouped
    const bool cal = d.fv == 6;
    srk_launch_schur_grouped(s, d, c, P<int64_t>(h->row_ptr), P<int32_t>(h->obs_pt), P<uint8_t>(h->obs_slot),
                             P<uint32_t>(h->pt_mask), P<double>(h->W), P<double>(h->Vg), P<double>(a.S),
                             P<double>(a.rhs), P<int32_t>(h->grp_first), P<int32_t>(h->grp_count), P<int32_t>(h->grp_nf),
                             P<int32_t>(h->grp_frames), h->n_groups, h->n_groups_wide, h->n_groups_mid,
                             !cal && h->schur_fp32 ? 1 : 0, P<int32_t>(a.irr), h->n_mm_uniform, h->n_mm_ragged,
                             !cal && h->det_active ? &dets : nullptr);
    if (cal) {
        // fixed intrinsics: every other landmark through the per-landmark kernel
        srk_launch_schur(s, d, c, P<int64_t>(h->row_ptr), P<int32_t>(h->obs_frame), P<double>(h->W), P<double>(h->Vg),
                         P<double>(a.S), P<double>(a.rhs), P<int32_t>(h->cal_list), h->n_cal_list);
    } else {
        srk_launch_schur_long(s, d, c, P<double>(h->W), P<double>(h->Vg), P<double>(a.S), P<double>(a.rhs),
                              P<int32_t>(h->lg_item), h->n_long_items, P<int32_t>(h->lg_np), P<int32_t>(h->lg_nf), P<int32_t>(h->lg_pts),
                              P<int32_t>(h->lg_frames), P<int64_t>(h->lg_obs_off), P<int32_t>(h->lg_obs), h->long_fb);
        srk_launch_schur(s, d, c, P<int64_t>(h->row_ptr), P<int32_t>(h->obs_frame), P<double>(h->W), P<double>(h->Vg),
                         P<double>(a.S), P<double>(a.rhs), P<int32_t>(h->gen_list), h->n_generic);
    }
    HIPCHK(h, hipGetLastError());
    // G (frame blocks, damped) and the frame gradients are linear in this rank's landmarks as well, so they are added
    // before the exchange; the identity diagonal of fixed / padding variables comes from rank 0 alone
    srk_launch_assemble(s, d, c, P<double>(h->Ug), P<double>(a.S), P<double>(a.rhs), h->rank == 0 ? 1.0 : 0.0,
                        P<int64_t>(h->row_ptr), P<int32_t>(h->obs_frame), P<double>(h->W), P<double>(h->Vg), P<int32_t>(a.irr));
    HIPCHK(h, hipGetLastError());
    int rc;
    SrkRelPose rpl;
    if (const SrkRelPose* relpose = relpose_factors(h, rpl)) // the coupling blocks, before the constant frames are masked
        if ((rc = timed_launch(h, h->rp.pass[1], s, [&] { srk_launch_relpose_couple(s, d, *relpose, P<double>(a.S)); })) != SRK_OK) return rc;
    SrkJointPrior jpl;
    const SrkJointPrior* jprior = joint_priors(h, jpl);
    if (jprior && jprior->n_pairs > 0) // the sets' coupling blocks, before the constant frames are masked
        if ((rc = timed_launch(h, h->jp.pass[1], s, [&] { srk_launch_jprior_couple(s, d, *jprior, P<double>(a.S)); })) != SRK_OK) return rc;
    if (h->cst.n_frames > 0) // constant frames: identity rows and columns, zero rhs
        if ((rc = timed_launch(h, h->cst.pass[1], s, [&] { srk_launch_const_frames(s, d, P<int32_t>(h->cst.buf[ConstFamily::FRAMES]), h->cst.n_frames, P<int64_t>(h->env_col), P<double>(a.S), P<double>(a.rhs)); })) != SRK_OK) return rc;
    if (h->shk_G > 0) { // shared intrinsics: S_sh = P^T S10 P, rhs_sh = P^T rhs10 (one rank only)
        srk_launch_rcs_fold(s, shk_args(h, a), P<double>(a.S), P<double>(a.rhs), P<double>(a.Ssh), P<double>(a.rsh));
        HIPCHK(h, hipGetLastError());
    }
    h->last_hessian_factor = c;
    if ((h->allreduce || h->comm) && !local_only) { // landmark shards: ONE exchange per attempt; only the band travels, the rhs rides behind it
        int rc = schur_pack(h, a);
        if (rc == SRK_OK) rc = exchange(h, a, P<double>(a.packed), h->band_packed + d.ld);
        if (rc == SRK_OK) rc = schur_unpack(h, a);
        if (rc != SRK_OK) return rc;
    }
    return SRK_OK;
}

// one solve of the reduced camera system in the current mode; prof may be NULL
static int launch_solve(srk_ba* h, srk_ba::Attempt& a, SrkSolveProf* prof)
{
    const SrkDims& d = h->d;
    if (h->shk_G > 0) { // (rhs_sh stays for the downloads: the solve consumes a copy)
        const bool sky = h->use_envelope;
        double* w = P<double>(a.ysh);
        if (!(prof && prof->dry)) HIPCHK(h, hipMemcpyAsync(w, a.rsh.p, (size_t)(8 * h->shk_ldb), hipMemcpyDeviceToDevice, a.stream));
        srk_chol_solve_bordered(a.stream, h->shk_ncols, h->shk_ldb, P<double>(a.Ssh), w, w + h->shk_ldb,
                                P<double>(a.dcsh), P<double>(a.dinvsh), P<int>(a.info), sky ? h->shk_row_end.data() : nullptr,
                                sky ? h->shk_col_begin.data() : nullptr, 6 * (int64_t)d.M, 4 * (int64_t)h->shk_G, prof, &a.sync);
    } else if (a.plan.P >= 2)
        srk_chol_solve_chunked(a.stream, a.plan, d.ld, P<double>(a.S), P<double>(a.rhs), P<double>(a.dc),
                               P<int64_t>(h->env_col), P<int>(a.info), prof, &a.sync);
    else
        srk_chol_solve(a.stream, d.ld, P<double>(a.S), P<double>(a.rhs), P<double>(a.wy), P<double>(a.dc),
                       P<int>(a.info), h->row_end_h.data(), h->col_begin_h.data(), P<double>(a.dinv), prof, &a.sync, d.fv * (int64_t)d.M);
    return SRK_OK;
}

static int phase_solve(srk_ba* h, srk_ba::Attempt& a, bool profile)
{
    const SrkDims& d = h->d;
    // inside the LM loop the status words and the point accumulators are left cleared by the kernels that consume them
    // (k_error_final, k_point_update); the step-wise entry points clear them here
    if (!h->lean_resets) HIPCHK(h, hipMemsetAsync(a.info.p, 0, 4, a.stream));
    a.solve_prof = SrkSolveProf{};
    if (profile) {
        size_t need = (size_t)(2 * (2 * (d.ld / SRK_CHOL_NB) + 64)); // every level of a nested plan included
        while (h->chol_ev.size() < need) {
            hipEvent_t e;
            HIPCHK(h, hipEventCreate(&e));
            h->chol_ev.push_back(e);
        }
        a.solve_prof.ev = h->chol_ev.data();
        a.solve_prof.cap = h->chol_ev.size();
    }
    const int rc = launch_solve(h, a, profile ? &a.solve_prof : nullptr);
    if (rc != SRK_OK) return rc;
    HIPCHK(h, hipGetLastError());
    return SRK_OK;
}

static int read_info(srk_ba* h, srk_ba::Attempt& a, int* info_host)
{
    HIPCHK(h, hipMemcpyAsync(info_host, a.info.p, 4, hipMemcpyDeviceToHost, a.stream));
    HIPCHK(h, hipStreamSynchronize(a.stream));
    return SRK_OK;
}

static int phase_backsub_apply(srk_ba* h, srk_ba::Attempt& a, double c)
{
    const SrkDims& d = h->d;
    hipStream_t s = a.stream;
    int cur = h->cur, tr = a.trial;
    if (!h->lean_resets) HIPCHK(h, hipMemsetAsync(a.acc.p, 0, 8 * 3 * d.Ns + 64, s));
    if (h->shk_G > 0) // shared intrinsics: dc10 = P dc_sh, and the trial K of every frame
        srk_launch_rcs_expand(s, shk_args(h, a), P<double>(a.dcsh), P<double>(a.dc), kbuf(h, cur), kbuf(h, tr));
    srk_launch_backsub(s, d, c, P<int32_t>(h->obs_frame), P<int32_t>(h->obs_pt), P<double>(h->W), P<double>(h->Vg),
                       P<double>(a.dc), P<double>(a.acc), P<double>(h->pts[cur]), P<double>(h->pts[tr]),
                       P<double>(a.dx));
    HIPCHK(h, hipGetLastError());
    return SRK_OK;
}

static int phase_cam_apply(srk_ba* h, srk_ba::Attempt& a)
{
    int cur = h->cur, tr = a.trial;
    srk_launch_cam_apply(a.stream, h->d.M, P<double>(h->camR[cur]), P<double>(h->camT[cur]), P<double>(a.dc),
                         P<double>(h->camR[tr]), P<double>(h->camT[tr]), kbuf(h, tr), h->f0, P<double>(h->cam[tr]), h->d.fv);
    // constant frames: a zero correction does not return T bit for bit (it goes through R^T), so their trial pose is copied
    srk_launch_const_cam_keep(a.stream, P<int32_t>(h->cst.buf[ConstFamily::FRAMES]), h->cst.n_frames, P<double>(h->camR[cur]), P<double>(h->camT[cur]),
                              P<double>(h->cam[cur]), P<double>(h->camR[tr]), P<double>(h->camT[tr]), P<double>(h->cam[tr]));
    HIPCHK(h, hipGetLastError());
    return SRK_OK;
}

extern "C" {

int srk_ba_phase_error(srk_ba* h, double* err, int64_t* seen)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    HIPCHK(h, hipSetDevice(h->device));
    if (seen) *seen = h->d.O;
    return phase_error(h, h->att[0], h->cur, err);
}
int srk_ba_phase_derivatives(srk_ba* h)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    HIPCHK(h, hipSetDevice(h->device));
    int rc = phase_derivatives(h);
    if (rc != SRK_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(h->main_stream));
    return SRK_OK;
}
int srk_ba_phase_schur(srk_ba* h, double c)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    HIPCHK(h, hipSetDevice(h->device));
    srk_ba::Attempt& a = h->att[0]; // the staged calls always work on attempt slot 0
    h->last_slot = 0;
    int rc = clear_poison(h);
    if (rc != SRK_OK) return rc;
    rc = phase_schur(h, a, c);
    if (rc != SRK_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(a.stream));
    return SRK_OK;
}
int srk_ba_phase_solve(srk_ba* h)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    HIPCHK(h, hipSetDevice(h->device));
    srk_ba::Attempt& a = h->att[0];
    int rc = phase_solve(h, a, false);
    if (rc != SRK_OK) return rc;
    int info = 0;
    rc = read_info(h, a, &info);
    if (rc != SRK_OK) return rc;
    if (info && srk_debug()) fprintf(stderr, "srk_ba_phase_solve: info=%d (1 = pivot, 4 = non-finite solution, 8 = hand-off timeout of the fused solve)\n", info);
    if ((info & 8) && a.plan.P >= 2) {
        // a hand-off of the fused outer step timed out: a scheduling event, not a numerical failure.  The chunked solve works
        // on copies (the system itself is intact): the plan's buffers back to zero, fusion off for good, once more unfused.
        fusion_off(h);
        HIPCHK(h, hipStreamSynchronize(a.stream));
        for (size_t i = 0; i < a.plan_bufs.size(); ++i)
            if (a.plan_zeroed[i]) HIPCHK(h, hipMemsetAsync(a.plan_bufs[i].p, 0, a.plan_bufs[i].bytes, a.stream));
        HIPCHK(h, hipMemsetAsync(a.info.p, 0, 4, a.stream));
        rc = phase_solve(h, a, false);
        if (rc != SRK_OK) return rc;
        rc = read_info(h, a, &info);
        if (rc != SRK_OK) return rc;
    } else if (info & 8) {
        // (the single-chain / dense solve factorises the system in place: nothing to repeat from; the caller builds it again)
        fusion_off(h);
        h->last_error = "a hand-off of the fused solve timed out; the system was factorised in place: call srk_ba_phase_schur again "
                        "(the unfused launch sequence is selected from now on)";
    }
    if (info) h->poisoned = true;
    return info ? 1 : 0;
}
int srk_ba_phase_backsub(srk_ba* h, double c)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    HIPCHK(h, hipSetDevice(h->device));
    srk_ba::Attempt& a = h->att[0];
    int rc = phase_backsub_apply(h, a, c);
    if (rc != SRK_OK) return rc;
    rc = phase_cam_apply(h, a);
    if (rc != SRK_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(a.stream));
    return SRK_OK;
}
int srk_ba_phase_accept(srk_ba* h)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    std::swap(h->cur, h->att[0].trial); // slot 0's trial scene becomes current
    return SRK_OK;
}

} // extern "C"

// ------------------------------------------------------------------ marginal covariances

// the map of srk_ba_revert_covariances on one block: landmarks R0^T Sigma R0 / s^2; frames D Sigma D^T with
// D = diag(I (intrinsics, fv = 10 only), R0^T / s, R0^T)
static void cov_revert_frame(const srk_ba_normalizer& nrm, int fv, double* B)
{
    const int off = fv - 6;
    const double is = 1.0 / nrm.world_scale;
    double D[100] = {};
    for (int i = 0; i < off; ++i) D[i * fv + i] = 1.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            D[(off + a) * fv + off + b] = nrm.R0[3 * b + a] * is;
            D[(off + 3 + a) * fv + off + 3 + b] = nrm.R0[3 * b + a];
        }
    double T[100];
    for (int i = 0; i < fv; ++i)
        for (int j = 0; j < fv; ++j) {
            double v = 0;
            for (int k = 0; k < fv; ++k) v += D[i * fv + k] * B[k * fv + j];
            T[i * fv + j] = v;
        }
    for (int i = 0; i < fv; ++i)
        for (int j = i; j < fv; ++j) {
            double v = 0;
            for (int k = 0; k < fv; ++k) v += T[i * fv + k] * D[j * fv + k];
            B[i * fv + j] = B[j * fv + i] = v;
        }
}
static void cov_revert_point(const srk_ba_normalizer& nrm, double* B)
{
    const double is2 = 1.0 / (nrm.world_scale * nrm.world_scale);
    const double* R = nrm.R0;
    double T[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) T[3 * i + j] = R[i] * B[j] + R[3 + i] * B[3 + j] + R[6 + i] * B[6 + j]; // R0^T Sigma
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) B[3 * i + j] = B[3 * j + i] = (T[3 * i] * R[j] + T[3 * i + 1] * R[3 + j] + T[3 * i + 2] * R[6 + j]) * is2;
}

static int cov_check_args(srk_ba* h, int32_t nf, const int32_t* frames, const double* fb, int64_t np, const int64_t* points, const double* pb)
{
    if (nf < 0 || np < 0 || (nf > 0 && (!frames || !fb)) || (np > 0 && (!points || !pb))) {
        h->last_error = "covariance: a negative count, or a NULL array with a positive count";
        return SRK_E_ARGS;
    }
    if (h->world > 1 || h->allreduce || h->comm) { h->last_error = "covariance: more than one rank is not supported"; return SRK_E_ARGS; }
    if (h->shk_G > 0) { h->last_error = "covariance: intrinsic groups are not supported"; return SRK_E_ARGS; }
    for (int32_t k = 0; k < nf; ++k)
        if (frames[k] < 0 || frames[k] >= h->d.M) { h->last_error = "covariance: a frame index is out of range"; return SRK_E_ARGS; }
    for (int64_t k = 0; k < np; ++k)
        if (points[k] < 0 || points[k] >= h->d.N) { h->last_error = "covariance: a landmark index is out of range"; return SRK_E_ARGS; }
    return SRK_OK;
}

// the start the covariance calls share: slot 0's system (built by phase_schur at h->last_hessian_factor) is factorised in place;
// with want_selection the mask of the variables that move and the skyline go to the device; with want_points pt_int receives
// the internal index of every landmark of the caller (the first frame of every internal landmark is fetched at the first
// such call after an upload).  0 ok, 1 not positive definite, negative on error.
static int cov_prepare(srk_ba* h, bool want_selection, bool want_points, std::vector<int64_t>& pt_int)
{
    const SrkDims& d = h->d;
    srk_ba::Attempt& a = h->att[0];
    hipStream_t s = a.stream;
    const int fv = d.fv;
    const int64_t n_rows = fv * (int64_t)d.M;
    int rc;
    // the factor: the single-chain solve with a zero right-hand side and the unfused launch sequence, whatever the rcs mode
    HIPCHK(h, hipMemsetAsync(a.info.p, 0, 4, s));
    HIPCHK(h, hipMemsetAsync(a.rhs.p, 0, (size_t)(8 * d.ld), s));
    srk_chol_solve(s, d.ld, P<double>(a.S), P<double>(a.rhs), P<double>(a.wy), P<double>(a.dc), P<int>(a.info), h->row_end_h.data(),
                   h->col_begin_h.data(), P<double>(a.dinv), nullptr, nullptr, n_rows);
    HIPCHK(h, hipGetLastError());
    int info = 0;
    if ((rc = read_info(h, a, &info)) != SRK_OK) return rc;
    if (info) { h->poisoned = true; return 1; }
    if (!want_selection) return 0;

    // which variables move
    std::vector<uint8_t> free_var((size_t)d.ld, 0);
    {
        const int off = 10 - fv;
        const int64_t b0 = fv * (int64_t)d.g0, v1 = fv * (int64_t)d.g1 + 4 - off + d.comp;
        for (int64_t var = 0; var < n_rows; ++var) {
            const bool gauge = (var >= b0 + 4 - off && var <= b0 + 9 - off) || var == v1;
            const bool cst = !h->cst.frame_int.empty() && h->cst.frame_int[(size_t)(var / fv)];
            free_var[(size_t)var] = gauge || cst ? 0 : 1;
        }
    }
    if ((rc = dev_alloc(h, h->cov_free, (size_t)d.ld)) != SRK_OK) return rc;
    HIPCHK(h, hipMemcpyAsync(h->cov_free.p, free_var.data(), (size_t)d.ld, hipMemcpyHostToDevice, s));
    if ((rc = dev_alloc(h, h->cov_colb, (size_t)(8 * (d.ld / 64)))) != SRK_OK) return rc;
    HIPCHK(h, hipMemcpyAsync(h->cov_colb.p, h->col_begin_h.data(), (size_t)(8 * (d.ld / 64)), hipMemcpyHostToDevice, s));
    // landmarks: internal index and the first frame that sees them
    if (want_points) {
        if (h->cov_pt_frame0.empty()) {
            std::vector<int32_t> of((size_t)d.O);
            HIPCHK(h, hipMemcpyAsync(of.data(), h->obs_frame.p, (size_t)(4 * d.O), hipMemcpyDeviceToHost, s));
            HIPCHK(h, hipStreamSynchronize(s));
            h->cov_pt_frame0.assign((size_t)d.N, 0);
            for (int64_t i = 0; i < d.N; ++i) {
                int32_t f0 = d.M - 1;
                for (int64_t o = h->row_ptr_int[(size_t)i]; o < h->row_ptr_int[(size_t)i + 1]; ++o) f0 = std::min(f0, of[(size_t)o]);
                h->cov_pt_frame0[(size_t)i] = f0;
            }
        }
        pt_int.assign((size_t)d.N, 0);
        for (int64_t i = 0; i < d.N; ++i) pt_int[(size_t)h->perm[(size_t)i]] = i;
    }
    return 0;
}

// the column cap of a batch: Y [ld][columns] stays under 256 MB, or what srk_ba_set_covariance_batch asks for (at least floor)
static int64_t cov_max_cols(const srk_ba* h, int64_t floor)
{
    if (h->cov_batch_cols > 0) return std::max<int64_t>(floor, h->cov_batch_cols);
    return std::max<int64_t>(SRK_COV_CB, ((int64_t)256 << 20) / (8 * h->d.ld) / SRK_COV_CB * SRK_COV_CB);
}

// the blocks of the inverse of the system in slot 0 (built by phase_schur at h->last_hessian_factor); 0 ok, 1 not positive
// definite / non-finite, negative on error.  Arguments checked by the caller.
static int phase_covariance(srk_ba* h, int32_t nf, const int32_t* frames, double* frame_blocks, int64_t np, const int64_t* points,
                            double* point_blocks)
{
    const SrkDims& d = h->d;
    srk_ba::Attempt& a = h->att[0];
    hipStream_t s = a.stream;
    const int fv = d.fv;
    const double c = h->last_hessian_factor;
    const int64_t n_rows = fv * (int64_t)d.M;
    const int32_t n_tiles = (int32_t)((n_rows + 63) / 64);
    std::vector<int64_t> pt_int;
    int rc = cov_prepare(h, nf > 0 || np > 0, np > 0, pt_int);
    if (rc != 0 || (nf == 0 && np == 0)) return rc;
    int info = 0;
    // the selected blocks, sorted by their first non-zero row so that every column block starts late
    struct Sel { SrkCovGroup g; int64_t dst; };
    std::vector<Sel> sel;
    sel.reserve((size_t)(nf + np));
    for (int32_t k = 0; k < nf; ++k) {
        const int32_t f = h->frame_int.empty() ? frames[k] : h->frame_int[(size_t)frames[k]];
        sel.push_back(Sel{ SrkCovGroup{ f, 0, fv, (int32_t)(fv * (int64_t)f), 0 }, k });
    }
    std::vector<char> pt_zero((size_t)np, 0);
    for (int64_t k = 0; k < np; ++k) {
        if ((size_t)points[k] < h->cst.set.points.size() && h->cst.set.points[(size_t)points[k]]) { pt_zero[(size_t)k] = 1; continue; } // constant: a zero block
        const int64_t i = pt_int[(size_t)points[k]];
        sel.push_back(Sel{ SrkCovGroup{ i, 0, 3, (int32_t)(fv * (int64_t)h->cov_pt_frame0[(size_t)i]), 1 }, nf + k });
    }
    std::stable_sort(sel.begin(), sel.end(), [](const Sel& x, const Sel& y) { return x.g.first_row < y.g.first_row; });
    // batches of columns: Y [ld][ncp] stays under the byte cap
    const int64_t max_cols = cov_max_cols(h, 10);
    std::vector<double> res((size_t)(100 * sel.size()));
    std::vector<SrkCovGroup> grp;
    std::vector<int32_t> blk;
    for (size_t b0 = 0; b0 < sel.size();) {
        size_t b1 = b0;
        int64_t cols = 0;
        grp.clear();
        while (b1 < sel.size() && cols + sel[b1].g.ncols <= max_cols) {
            SrkCovGroup g = sel[b1].g;
            g.col0 = (int32_t)cols;
            cols += g.ncols;
            grp.push_back(g);
            ++b1;
        }
        const int64_t ncp = (cols + SRK_COV_CB - 1) / SRK_COV_CB * SRK_COV_CB;
        blk.assign((size_t)(ncp / SRK_COV_CB), n_tiles);
        for (const SrkCovGroup& g : grp)
            for (int64_t q = g.col0 / SRK_COV_CB; q <= (g.col0 + g.ncols - 1) / SRK_COV_CB; ++q)
                blk[(size_t)q] = std::min<int32_t>(blk[(size_t)q], g.first_row / 64);
        const int32_t ng = (int32_t)grp.size();
        if ((rc = dev_alloc(h, h->cov_Y, (size_t)(8 * d.ld * ncp))) != SRK_OK) return rc;
        if ((rc = dev_alloc(h, h->cov_grp, sizeof(SrkCovGroup) * grp.size())) != SRK_OK) return rc;
        if ((rc = dev_alloc(h, h->cov_blk, 4 * blk.size())) != SRK_OK) return rc;
        if ((rc = dev_alloc(h, h->cov_out, (size_t)(800 * ng))) != SRK_OK) return rc;
        HIPCHK(h, hipMemcpyAsync(h->cov_grp.p, grp.data(), sizeof(SrkCovGroup) * grp.size(), hipMemcpyHostToDevice, s));
        HIPCHK(h, hipMemcpyAsync(h->cov_blk.p, blk.data(), 4 * blk.size(), hipMemcpyHostToDevice, s));
        HIPCHK(h, hipMemsetAsync(h->cov_Y.p, 0, (size_t)(8 * 64 * (int64_t)n_tiles * ncp), s));
        HIPCHK(h, hipMemsetAsync(h->cov_out.p, 0, (size_t)(800 * ng), s));
        srk_launch_cov_rhs(s, d, c, P<SrkCovGroup>(h->cov_grp), ng, P<int64_t>(h->row_ptr), P<int32_t>(h->obs_frame), P<double>(h->W),
                           P<double>(h->Vg), P<uint8_t>(h->cov_free), P<double>(h->cov_Y), ncp, P<int>(a.info));
        srk_launch_cov_fwd(s, d.ld, P<double>(a.S), P<double>(a.dinv), P<int64_t>(h->cov_colb), n_tiles, P<int32_t>(h->cov_blk),
                           P<double>(h->cov_Y), ncp);
        srk_launch_cov_gram(s, d, c, P<SrkCovGroup>(h->cov_grp), ng, P<double>(h->Vg), P<double>(h->cov_Y), ncp, n_rows, P<double>(h->cov_out));
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(res.data() + 100 * b0, h->cov_out.p, (size_t)(800 * ng), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s)); // grp / blk are reused by the next batch
        b0 = b1;
    }
    if ((rc = read_info(h, a, &info)) != SRK_OK) return rc;
    if (info) return 1;
    for (size_t k = 0; k < sel.size(); ++k) {
        const int n = sel[k].g.ncols;
        for (int e = 0; e < n * n; ++e)
            if (!std::isfinite(res[100 * k + e])) return 1;
    }
    for (size_t k = 0; k < sel.size(); ++k) {
        const int n = sel[k].g.ncols;
        double* dst = sel[k].g.is_point ? point_blocks + 9 * (sel[k].dst - nf) : frame_blocks + (int64_t)fv * fv * sel[k].dst;
        std::memcpy(dst, res.data() + 100 * k, sizeof(double) * (size_t)(n * n));
    }
    for (int64_t k = 0; k < np; ++k)
        if (pt_zero[(size_t)k]) std::fill(point_blocks + 9 * k, point_blocks + 9 * k + 9, 0.0);
    return 0;
}

extern "C" {

int srk_ba_set_covariance_batch(srk_ba* h, int64_t max_columns)
{
    if (!h || max_columns < 0) return SRK_E_ARGS;
    h->cov_batch_cols = max_columns;
    return SRK_OK;
}

int srk_ba_phase_covariance(srk_ba* h, int32_t n_frames_sel, const int32_t* frames, double* frame_blocks, int64_t n_points_sel,
                            const int64_t* points, double* point_blocks)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    int rc = cov_check_args(h, n_frames_sel, frames, frame_blocks, n_points_sel, points, point_blocks);
    if (rc != SRK_OK) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    return phase_covariance(h, n_frames_sel, frames, frame_blocks, n_points_sel, points, point_blocks);
}

int srk_ba_revert_covariances(const srk_ba_normalizer* nrm, int frame_vars, int32_t n_frames, double* frame_cov, int64_t n_points,
                              double* point_cov)
{
    if (!nrm || (frame_vars != 6 && frame_vars != 10) || n_frames < 0 || n_points < 0 || (n_frames > 0 && !frame_cov) ||
        (n_points > 0 && !point_cov) || !(nrm->world_scale > 0) || !std::isfinite(nrm->world_scale))
        return SRK_E_ARGS;
    for (int32_t k = 0; k < n_frames; ++k) cov_revert_frame(*nrm, frame_vars, frame_cov + (int64_t)frame_vars * frame_vars * k);
    for (int64_t k = 0; k < n_points; ++k) cov_revert_point(*nrm, point_cov + 9 * k);
    return SRK_OK;
}

int srk_ba_covariances(srk_ba* h, double sigma_pixels, int32_t n_frames_sel, const int32_t* frames, double* frame_cov,
                       int64_t n_points_sel, const int64_t* points, double* point_cov, int caller_coordinates)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    if (!(sigma_pixels > 0) || !std::isfinite(sigma_pixels)) { h->last_error = "covariances: sigma_pixels must be finite and positive"; return SRK_E_ARGS; }
    int rc = cov_check_args(h, n_frames_sel, frames, frame_cov, n_points_sel, points, point_cov);
    if (rc != SRK_OK) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = clear_poison(h)) != SRK_OK) return rc;
    if ((rc = phase_derivatives(h)) != SRK_OK) return rc;
    h->last_slot = 0;
    if ((rc = phase_schur(h, h->att[0], 0.0)) != SRK_OK) return rc;
    rc = phase_covariance(h, n_frames_sel, frames, frame_cov, n_points_sel, points, point_cov);
    if (rc != 0) return rc;
    const int fv = h->d.fv;
    const double k = 2.0 * (sigma_pixels / h->f0) * (sigma_pixels / h->f0);
    for (int64_t e = 0; e < (int64_t)fv * fv * n_frames_sel; ++e) frame_cov[e] *= k;
    for (int64_t e = 0; e < 9 * n_points_sel; ++e) point_cov[e] *= k;
    if (caller_coordinates && h->normalized_on_upload) srk_ba_revert_covariances(&h->nrm, fv, n_frames_sel, frame_cov, n_points_sel, point_cov);
    return 0;
}

} // extern "C"

// ------------------------------------------------------------------ cross-covariances between blocks

// the pairs of a call in the caller's numbering: frame x frame [n][FV][FV] (rows a, columns b), landmark x frame [n][3][FV],
// landmark x landmark [n][3][3]
struct CovPairArgs {
    int64_t n_ff; const int32_t* ff_a; const int32_t* ff_b; double* ff_blocks;
    int64_t n_pf; const int64_t* pf_point; const int32_t* pf_frame; double* pf_blocks;
    int64_t n_pp; const int64_t* pp_a; const int64_t* pp_b; double* pp_blocks;
};

// D of a frame block, row-major fv x fv: diag(I (intrinsics, fv = 10 only), R0^T / s, R0^T); of a landmark block (fv = 0): R0^T / s
static void cov_cross_map(const srk_ba_normalizer& nrm, int fv, double* D)
{
    const double is = 1.0 / nrm.world_scale;
    const int n = fv ? fv : 3, off = fv ? fv - 6 : 0;
    std::fill(D, D + n * n, 0.0);
    for (int i = 0; i < off; ++i) D[i * n + i] = 1.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            D[(off + a) * n + off + b] = nrm.R0[3 * b + a] * is;
            if (fv) D[(off + 3 + a) * n + off + 3 + b] = nrm.R0[3 * b + a];
        }
}
// B (np x nq, row-major) <- Dp B Dq^T
static void cov_revert_cross(const double* Dp, int np, const double* Dq, int nq, double* B)
{
    double T[100];
    for (int i = 0; i < np; ++i)
        for (int j = 0; j < nq; ++j) {
            double v = 0;
            for (int k = 0; k < np; ++k) v += Dp[i * np + k] * B[k * nq + j];
            T[i * nq + j] = v;
        }
    for (int i = 0; i < np; ++i)
        for (int j = 0; j < nq; ++j) {
            double v = 0;
            for (int k = 0; k < nq; ++k) v += T[i * nq + k] * Dq[j * nq + k];
            B[i * nq + j] = v;
        }
}

static int cov_cross_check_args(srk_ba* h, const CovPairArgs& q)
{
    if (q.n_ff < 0 || q.n_pf < 0 || q.n_pp < 0 || (q.n_ff > 0 && (!q.ff_a || !q.ff_b || !q.ff_blocks)) ||
        (q.n_pf > 0 && (!q.pf_point || !q.pf_frame || !q.pf_blocks)) || (q.n_pp > 0 && (!q.pp_a || !q.pp_b || !q.pp_blocks))) {
        h->last_error = "cross-covariance: a negative count, or a NULL array with a positive count";
        return SRK_E_ARGS;
    }
    if (q.n_ff + q.n_pf + q.n_pp > INT32_MAX / 2) { h->last_error = "cross-covariance: too many pairs in one call"; return SRK_E_ARGS; }
    if (h->world > 1 || h->allreduce || h->comm) { h->last_error = "cross-covariance: more than one rank is not supported"; return SRK_E_ARGS; }
    if (h->shk_G > 0) { h->last_error = "cross-covariance: intrinsic groups are not supported"; return SRK_E_ARGS; }
    const auto bad_f = [&](int32_t f) { return f < 0 || f >= h->d.M; };
    const auto bad_p = [&](int64_t i) { return i < 0 || i >= h->d.N; };
    for (int64_t k = 0; k < q.n_ff; ++k)
        if (bad_f(q.ff_a[k]) || bad_f(q.ff_b[k])) { h->last_error = "cross-covariance: a frame index is out of range"; return SRK_E_ARGS; }
    for (int64_t k = 0; k < q.n_pf; ++k) {
        if (bad_p(q.pf_point[k])) { h->last_error = "cross-covariance: a landmark index is out of range"; return SRK_E_ARGS; }
        if (bad_f(q.pf_frame[k])) { h->last_error = "cross-covariance: a frame index is out of range"; return SRK_E_ARGS; }
    }
    for (int64_t k = 0; k < q.n_pp; ++k)
        if (bad_p(q.pp_a[k]) || bad_p(q.pp_b[k])) { h->last_error = "cross-covariance: a landmark index is out of range"; return SRK_E_ARGS; }
    return SRK_OK;
}

// the requested blocks of the inverse of the system in slot 0; 0 ok, 1 not positive definite / non-finite (outputs untouched),
// negative on error.  Arguments checked by the caller.  The blocks the pairs name are deduplicated; the pairs are sorted by
// (smaller first row, larger first row) and fill batches greedily so that both blocks of every pair of a batch lie in that
// batch's Y, each block once (a block may come back in a later batch); per batch k_cov_rhs, k_cov_fwd, k_cov_cross.
static int phase_cross_covariance(srk_ba* h, const CovPairArgs& q)
{
    const SrkDims& d = h->d;
    srk_ba::Attempt& a = h->att[0];
    hipStream_t s = a.stream;
    const int fv = d.fv;
    const double c = h->last_hessian_factor;
    const int64_t n_rows = fv * (int64_t)d.M;
    const int32_t n_tiles = (int32_t)((n_rows + 63) / 64);
    const int64_t n_all = q.n_ff + q.n_pf + q.n_pp;
    std::vector<int64_t> pt_int;
    int rc = cov_prepare(h, n_all > 0, q.n_pf + q.n_pp > 0, pt_int);
    if (rc != 0 || n_all == 0) return rc;

    // the distinct blocks (key: internal frame, or M + internal landmark); a constant landmark has none: its pairs are zero blocks
    std::vector<SrkCovGroup> blocks;
    std::map<int64_t, int32_t> block_of;
    const auto frame_block = [&](int32_t user) {
        const int32_t f = h->frame_int.empty() ? user : h->frame_int[(size_t)user];
        auto it = block_of.find(f);
        if (it != block_of.end()) return it->second;
        blocks.push_back(SrkCovGroup{ f, 0, fv, (int32_t)(fv * (int64_t)f), 0 });
        return block_of[f] = (int32_t)blocks.size() - 1;
    };
    const auto point_block = [&](int64_t user) {
        if ((size_t)user < h->cst.set.points.size() && h->cst.set.points[(size_t)user]) return (int32_t)-1;
        const int64_t i = pt_int[(size_t)user];
        auto it = block_of.find(d.M + i);
        if (it != block_of.end()) return it->second;
        blocks.push_back(SrkCovGroup{ i, 0, 3, (int32_t)(fv * (int64_t)h->cov_pt_frame0[(size_t)i]), 1 });
        return block_of[d.M + i] = (int32_t)blocks.size() - 1;
    };
    struct Pair { int32_t p, q, kind; int64_t dst, res; }; // kind 0 frame x frame, 1 landmark x frame, 2 landmark x landmark
    std::vector<Pair> pairs;
    pairs.reserve((size_t)n_all);
    for (int64_t k = 0; k < q.n_ff; ++k) pairs.push_back(Pair{ frame_block(q.ff_a[k]), frame_block(q.ff_b[k]), 0, k, -1 });
    for (int64_t k = 0; k < q.n_pf; ++k) {
        const int32_t p = point_block(q.pf_point[k]);
        if (p >= 0) pairs.push_back(Pair{ p, frame_block(q.pf_frame[k]), 1, k, -1 });
    }
    for (int64_t k = 0; k < q.n_pp; ++k) {
        const int32_t p = point_block(q.pp_a[k]), p2 = point_block(q.pp_b[k]);
        if (p >= 0 && p2 >= 0) pairs.push_back(Pair{ p, p2, 2, k, -1 });
    }
    const auto rows_of = [&](const Pair& x) {
        const int32_t rp = blocks[(size_t)x.p].first_row, rq = blocks[(size_t)x.q].first_row;
        return std::make_pair(std::min(rp, rq), std::max(rp, rq));
    };
    std::stable_sort(pairs.begin(), pairs.end(), [&](const Pair& x, const Pair& y) { return rows_of(x) < rows_of(y); });

    const int64_t max_cols = cov_max_cols(h, 20); // one pair of ten-variable frames always fits
    std::vector<double> res((size_t)(100 * pairs.size()));
    std::vector<int32_t> slot(blocks.size(), -1), members; // a block's place in the batch's group table
    std::vector<SrkCovGroup> grp;
    std::vector<SrkCovPair> tab;
    std::vector<int32_t> blk;
    for (size_t b0 = 0; b0 < pairs.size();) {
        size_t b1 = b0;
        int64_t cols = 0;
        members.clear();
        for (; b1 < pairs.size(); ++b1) {
            const Pair& x = pairs[b1];
            const int64_t need = (slot[(size_t)x.p] < 0 ? blocks[(size_t)x.p].ncols : 0) +
                                 (x.q != x.p && slot[(size_t)x.q] < 0 ? blocks[(size_t)x.q].ncols : 0);
            if (cols + need > max_cols) break; // (never the first pair of a batch: max_cols >= 20)
            for (int32_t m : { x.p, x.q })
                if (slot[(size_t)m] < 0) { slot[(size_t)m] = 0; members.push_back(m); }
            cols += need;
        }
        // the batch's blocks by first row, so that every column block of k_cov_fwd starts late
        std::stable_sort(members.begin(), members.end(), [&](int32_t x, int32_t y) { return blocks[(size_t)x].first_row < blocks[(size_t)y].first_row; });
        grp.clear();
        cols = 0;
        for (int32_t m : members) {
            SrkCovGroup g = blocks[(size_t)m];
            g.col0 = (int32_t)cols;
            cols += g.ncols;
            slot[(size_t)m] = (int32_t)grp.size();
            grp.push_back(g);
        }
        const int64_t ncp = (cols + SRK_COV_CB - 1) / SRK_COV_CB * SRK_COV_CB;
        blk.assign((size_t)(ncp / SRK_COV_CB), n_tiles);
        for (const SrkCovGroup& g : grp)
            for (int64_t cb = g.col0 / SRK_COV_CB; cb <= (g.col0 + g.ncols - 1) / SRK_COV_CB; ++cb)
                blk[(size_t)cb] = std::min<int32_t>(blk[(size_t)cb], g.first_row / 64);
        // the pair table by kind: one launch per shape
        tab.clear();
        int32_t n_kind[3] = { 0, 0, 0 };
        for (int kind = 0; kind < 3; ++kind)
            for (size_t k = b0; k < b1; ++k)
                if (pairs[k].kind == kind) {
                    pairs[k].res = (int64_t)(b0 + tab.size());
                    tab.push_back(SrkCovPair{ slot[(size_t)pairs[k].p], slot[(size_t)pairs[k].q] });
                    ++n_kind[kind];
                }
        const int32_t ng = (int32_t)grp.size(), npr = (int32_t)tab.size();
        if ((rc = dev_alloc(h, h->cov_Y, (size_t)(8 * d.ld * ncp))) != SRK_OK) return rc;
        if ((rc = dev_alloc(h, h->cov_grp, sizeof(SrkCovGroup) * grp.size())) != SRK_OK) return rc;
        if ((rc = dev_alloc(h, h->cov_blk, 4 * blk.size())) != SRK_OK) return rc;
        if ((rc = dev_alloc(h, h->cov_pairs, sizeof(SrkCovPair) * tab.size())) != SRK_OK) return rc;
        if ((rc = dev_alloc(h, h->cov_out, (size_t)(800 * (int64_t)npr))) != SRK_OK) return rc;
        HIPCHK(h, hipMemcpyAsync(h->cov_grp.p, grp.data(), sizeof(SrkCovGroup) * grp.size(), hipMemcpyHostToDevice, s));
        HIPCHK(h, hipMemcpyAsync(h->cov_blk.p, blk.data(), 4 * blk.size(), hipMemcpyHostToDevice, s));
        HIPCHK(h, hipMemcpyAsync(h->cov_pairs.p, tab.data(), sizeof(SrkCovPair) * tab.size(), hipMemcpyHostToDevice, s));
        HIPCHK(h, hipMemsetAsync(h->cov_Y.p, 0, (size_t)(8 * 64 * (int64_t)n_tiles * ncp), s));
        HIPCHK(h, hipMemsetAsync(h->cov_out.p, 0, (size_t)(800 * (int64_t)npr), s));
        srk_launch_cov_rhs(s, d, c, P<SrkCovGroup>(h->cov_grp), ng, P<int64_t>(h->row_ptr), P<int32_t>(h->obs_frame), P<double>(h->W),
                           P<double>(h->Vg), P<uint8_t>(h->cov_free), P<double>(h->cov_Y), ncp, P<int>(a.info));
        srk_launch_cov_fwd(s, d.ld, P<double>(a.S), P<double>(a.dinv), P<int64_t>(h->cov_colb), n_tiles, P<int32_t>(h->cov_blk),
                           P<double>(h->cov_Y), ncp);
        srk_launch_cov_cross(s, d, c, P<SrkCovGroup>(h->cov_grp), P<SrkCovPair>(h->cov_pairs), n_kind[0], n_kind[1], n_kind[2], P<double>(h->Vg),
                             P<double>(h->cov_Y), ncp, n_rows, P<double>(h->cov_out));
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(res.data() + 100 * b0, h->cov_out.p, (size_t)(800 * (int64_t)npr), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s)); // the tables are reused by the next batch
        for (int32_t m : members) slot[(size_t)m] = -1;
        b0 = b1;
    }
    int info = 0;
    if ((rc = read_info(h, a, &info)) != SRK_OK) return rc;
    if (info) return 1;
    const int shape[3][2] = { { fv, fv }, { 3, fv }, { 3, 3 } };
    for (const Pair& x : pairs)
        for (int e = 0; e < shape[x.kind][0] * shape[x.kind][1]; ++e)
            if (!std::isfinite(res[(size_t)(100 * x.res + e)])) return 1;
    // pairs with a constant landmark stay zero
    double* const outs[3] = { q.ff_blocks, q.pf_blocks, q.pp_blocks };
    const int64_t counts[3] = { q.n_ff, q.n_pf, q.n_pp };
    for (int kind = 0; kind < 3; ++kind)
        if (counts[kind] > 0) std::fill(outs[kind], outs[kind] + counts[kind] * shape[kind][0] * shape[kind][1], 0.0);
    for (const Pair& x : pairs) {
        const int n = shape[x.kind][0] * shape[x.kind][1];
        std::memcpy(outs[x.kind] + x.dst * n, res.data() + 100 * x.res, sizeof(double) * (size_t)n);
    }
    return 0;
}

// the derivative pass and the undamped system of the resident scene's current state in slot 0 (the convenience calls)
static int cov_build_undamped(srk_ba* h)
{
    int rc;
    if ((rc = clear_poison(h)) != SRK_OK) return rc;
    if ((rc = phase_derivatives(h)) != SRK_OK) return rc;
    h->last_slot = 0;
    return phase_schur(h, h->att[0], 0.0);
}

extern "C" {

int srk_ba_phase_cross_covariance(srk_ba* h, int64_t n_ff, const int32_t* ff_a, const int32_t* ff_b, double* ff_blocks, int64_t n_pf,
                                  const int64_t* pf_point, const int32_t* pf_frame, double* pf_blocks, int64_t n_pp, const int64_t* pp_a,
                                  const int64_t* pp_b, double* pp_blocks)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    const CovPairArgs q{ n_ff, ff_a, ff_b, ff_blocks, n_pf, pf_point, pf_frame, pf_blocks, n_pp, pp_a, pp_b, pp_blocks };
    int rc = cov_cross_check_args(h, q);
    if (rc != SRK_OK) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    return phase_cross_covariance(h, q);
}

int srk_ba_revert_cross_covariances(const srk_ba_normalizer* nrm, int frame_vars, int64_t n_ff, double* ff_blocks, int64_t n_pf,
                                    double* pf_blocks, int64_t n_pp, double* pp_blocks)
{
    if (!nrm || (frame_vars != 6 && frame_vars != 10) || n_ff < 0 || n_pf < 0 || n_pp < 0 || (n_ff > 0 && !ff_blocks) ||
        (n_pf > 0 && !pf_blocks) || (n_pp > 0 && !pp_blocks) || !(nrm->world_scale > 0) || !std::isfinite(nrm->world_scale))
        return SRK_E_ARGS;
    const int fv = frame_vars;
    double Df[100], Dp[9];
    cov_cross_map(*nrm, fv, Df);
    cov_cross_map(*nrm, 0, Dp);
    for (int64_t k = 0; k < n_ff; ++k) cov_revert_cross(Df, fv, Df, fv, ff_blocks + (int64_t)fv * fv * k);
    for (int64_t k = 0; k < n_pf; ++k) cov_revert_cross(Dp, 3, Df, fv, pf_blocks + (int64_t)3 * fv * k);
    for (int64_t k = 0; k < n_pp; ++k) cov_revert_cross(Dp, 3, Dp, 3, pp_blocks + 9 * k);
    return SRK_OK;
}

int srk_ba_cross_covariances(srk_ba* h, double sigma_pixels, int64_t n_ff, const int32_t* ff_a, const int32_t* ff_b, double* ff_cov,
                             int64_t n_pf, const int64_t* pf_point, const int32_t* pf_frame, double* pf_cov, int64_t n_pp,
                             const int64_t* pp_a, const int64_t* pp_b, double* pp_cov, int caller_coordinates)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    if (!(sigma_pixels > 0) || !std::isfinite(sigma_pixels)) { h->last_error = "cross-covariances: sigma_pixels must be finite and positive"; return SRK_E_ARGS; }
    const CovPairArgs q{ n_ff, ff_a, ff_b, ff_cov, n_pf, pf_point, pf_frame, pf_cov, n_pp, pp_a, pp_b, pp_cov };
    int rc = cov_cross_check_args(h, q);
    if (rc != SRK_OK) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = cov_build_undamped(h)) != SRK_OK) return rc;
    if ((rc = phase_cross_covariance(h, q)) != 0) return rc;
    const int fv = h->d.fv;
    const double k = 2.0 * (sigma_pixels / h->f0) * (sigma_pixels / h->f0);
    for (int64_t e = 0; e < (int64_t)fv * fv * n_ff; ++e) ff_cov[e] *= k;
    for (int64_t e = 0; e < (int64_t)3 * fv * n_pf; ++e) pf_cov[e] *= k;
    for (int64_t e = 0; e < 9 * n_pp; ++e) pp_cov[e] *= k;
    if (caller_coordinates && h->normalized_on_upload) {
        // a block with itself is mapped as srk_ba_revert_covariances maps it: exactly symmetric, the bits of srk_ba_covariances;
        // a block (a, b) with a > b is mapped as the transpose of (b, a), so that the two stay transposes of one another to the bit
        double Df[100], Dp[9];
        cov_cross_map(h->nrm, fv, Df);
        cov_cross_map(h->nrm, 0, Dp);
        const auto square = [](const double* D, int n, bool swapped, double* B) {
            const auto transpose = [&] {
                for (int i = 0; i < n; ++i)
                    for (int j = i + 1; j < n; ++j) std::swap(B[i * n + j], B[j * n + i]);
            };
            if (swapped) transpose();
            cov_revert_cross(D, n, D, n, B);
            if (swapped) transpose();
        };
        for (int64_t e = 0; e < n_ff; ++e) {
            double* B = ff_cov + (int64_t)fv * fv * e;
            if (ff_a[e] == ff_b[e]) cov_revert_frame(h->nrm, fv, B);
            else square(Df, fv, ff_a[e] > ff_b[e], B);
        }
        for (int64_t e = 0; e < n_pf; ++e) cov_revert_cross(Dp, 3, Df, fv, pf_cov + (int64_t)3 * fv * e);
        for (int64_t e = 0; e < n_pp; ++e) {
            if (pp_a[e] == pp_b[e]) cov_revert_point(h->nrm, pp_cov + 9 * e);
            else square(Dp, 3, pp_a[e] > pp_b[e], pp_cov + 9 * e);
        }
    }
    return 0;
}

int srk_ba_relative_pose_covariances(srk_ba* h, double sigma_pixels, int32_t n, const int32_t* frame_a, const int32_t* frame_b, double* cov)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    if (!(sigma_pixels > 0) || !std::isfinite(sigma_pixels)) { h->last_error = "relative-pose covariances: sigma_pixels must be finite and positive"; return SRK_E_ARGS; }
    if (n < 0 || (n > 0 && (!frame_a || !frame_b || !cov))) {
        h->last_error = "relative-pose covariances: a negative count, or a NULL array with a positive count";
        return SRK_E_ARGS;
    }
    for (int32_t k = 0; k < n; ++k)
        if (frame_a[k] >= 0 && frame_a[k] == frame_b[k]) { h->last_error = "relative-pose covariances: a pair names one frame twice"; return SRK_E_ARGS; }
    // one factorisation for all: the marginal of every frame named, once, then the cross block of every pair
    std::vector<int32_t> fa, fb;
    std::map<int32_t, int64_t> marg;
    for (int32_t k = 0; k < n; ++k)
        for (int32_t f : { frame_a[k], frame_b[k] })
            if (marg.emplace(f, (int64_t)fa.size()).second) { fa.push_back(f); fb.push_back(f); }
    fa.insert(fa.end(), frame_a, frame_a + n);
    fb.insert(fb.end(), frame_b, frame_b + n);
    const int fv = h->d.fv, off = fv - 6;
    const int64_t n_marg = (int64_t)marg.size();
    std::vector<double> blk((size_t)(fv * fv) * fa.size());
    const CovPairArgs q{ (int64_t)fa.size(), fa.data(), fb.data(), blk.data(), 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr };
    int rc = cov_cross_check_args(h, q);
    if (rc != SRK_OK) return rc;
    if (n == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = cov_build_undamped(h)) != SRK_OK) return rc;
    if ((rc = phase_cross_covariance(h, q)) != 0) return rc;
    // the resident scene's current poses (internal frame order)
    const int32_t M = h->d.M;
    std::vector<double> R(9 * (size_t)M), T(3 * (size_t)M);
    hipStream_t s = h->att[0].stream;
    HIPCHK(h, hipMemcpyAsync(R.data(), h->camR[h->cur].p, 72 * (int64_t)M, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(T.data(), h->camT[h->cur].p, 24 * (int64_t)M, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    const double kf = 2.0 * (sigma_pixels / h->f0) * (sigma_pixels / h->f0);
    const double is = h->normalized_on_upload ? 1.0 / h->nrm.world_scale : 1.0; // z scales with the world, Z does not; no R0 enters
    for (int32_t k = 0; k < n; ++k) {
        const int32_t ia = h->frame_int.empty() ? frame_a[k] : h->frame_int[(size_t)frame_a[k]];
        const int32_t ib = h->frame_int.empty() ? frame_b[k] : h->frame_int[(size_t)frame_b[k]];
        const double *Ra = &R[9 * (size_t)ia], *Rb = &R[9 * (size_t)ib];
        double Ca[3], Cb[3], dv[3], Rt[9];
        srk::se3_inv(Ra, &T[3 * (size_t)ia], Rt, Ca); // the centre C = -R^T T
        srk::se3_inv(Rb, &T[3 * (size_t)ib], Rt, Cb);
        for (int e = 0; e < 3; ++e) dv[e] = Cb[e] - Ca[e];
        const double dx[9] = { 0, -dv[2], dv[1], dv[2], 0, -dv[0], -dv[1], dv[0], 0 };
        double RaDx[9];
        srk::mat3_mul(Ra, dx, RaDx);
        // J = [J_a J_b] (6 x 12), J_a = [[-R_a, R_a [d]x], [0, -R_b]], J_b = [[R_a, 0], [0, R_b]]
        double J[6][12] = {};
        for (int r = 0; r < 3; ++r)
            for (int cc = 0; cc < 3; ++cc) {
                J[r][cc] = -Ra[3 * r + cc];
                J[r][3 + cc] = RaDx[3 * r + cc];
                J[3 + r][3 + cc] = -Rb[3 * r + cc];
                J[r][6 + cc] = Ra[3 * r + cc];
                J[3 + r][9 + cc] = Rb[3 * r + cc];
            }
        // the joint covariance of the two frames' pose variables (with ten variables a frame: its variables 4..9)
        const double* Saa = &blk[(size_t)(fv * fv) * (size_t)marg[frame_a[k]]];
        const double* Sbb = &blk[(size_t)(fv * fv) * (size_t)marg[frame_b[k]]];
        const double* Sab = &blk[(size_t)(fv * fv) * (size_t)(n_marg + k)];
        double Sg[12][12];
        for (int r = 0; r < 6; ++r)
            for (int cc = 0; cc < 6; ++cc) {
                Sg[r][cc] = Saa[(off + r) * fv + off + cc];
                Sg[6 + r][6 + cc] = Sbb[(off + r) * fv + off + cc];
                Sg[r][6 + cc] = Sg[6 + cc][r] = Sab[(off + r) * fv + off + cc];
            }
        double JS[6][12];
        for (int r = 0; r < 6; ++r)
            for (int cc = 0; cc < 12; ++cc) {
                double v = 0;
                for (int e = 0; e < 12; ++e) v += J[r][e] * Sg[e][cc];
                JS[r][cc] = v;
            }
        double* out = cov + 36 * (int64_t)k;
        for (int r = 0; r < 6; ++r)
            for (int cc = r; cc < 6; ++cc) {
                double v = 0;
                for (int e = 0; e < 12; ++e) v += JS[r][e] * J[cc][e];
                v *= kf * (r < 3 ? is : 1.0) * (cc < 3 ? is : 1.0); // tt / s^2, tr / s, rr
                out[6 * r + cc] = out[6 * cc + r] = v;
            }
    }
    return 0;
}

} // extern "C"

// ------------------------------------------------------------------ marginalisation priors

namespace {
// what a call carries from its plan to its result, in the variables of the resident (normalised) scene
struct MargCall {
    SrkMargPlan plan;
    std::vector<int32_t> set_ptr, set_frame; // the switched-on joint sets as the device holds them
    std::vector<double> R, T;                // the current poses, internal order
    std::vector<double> A0, b0, A1, b1;
    srk_ba_marg_report rep{};
};
template <typename T> int marg_fetch(srk_ba* h, hipStream_t s, const DevBuf& b, size_t n, std::vector<T>& out)
{
    out.assign(n, T());
    if (n == 0) return SRK_OK;
    HIPCHK(h, hipMemcpyAsync(out.data(), b.p, n * sizeof(T), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return SRK_OK;
}
template <typename T> int marg_put(srk_ba* h, hipStream_t s, DevBuf& b, const std::vector<T>& v)
{
    const int rc = dev_alloc(h, b, v.size() * sizeof(T));
    if (rc != SRK_OK || v.empty()) return rc;
    HIPCHK(h, hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return SRK_OK;
}
} // namespace

// the plan of a call: the checks and tables of srk_marg_plan on the resident scene.  The only device traffic is the download of
// small index tables (the observations' frames once per upload).
static int marg_plan(srk_ba* h, int32_t nd, const int32_t* drop, int64_t np, const int64_t* points, MargCall& mc)
{
    const SrkDims& d = h->d;
    hipStream_t s = h->main_stream;
    int rc;
    for (auto& a : h->att) // nothing of an earlier call is still writing the scene
        if (a.allocated && a.stream) HIPCHK(h, hipStreamSynchronize(a.stream));
    if (h->mg_obs_frame.empty() && d.O > 0 && (rc = marg_fetch(h, s, h->obs_frame, (size_t)d.O, h->mg_obs_frame)) != SRK_OK) return rc;
    SrkInfoTables qt;
    if (h->obs_info.on) qt = srk_build_information(h->obs_info.set, *h, factor_dims(h));
    std::vector<int32_t> pt_prior, fr_prior;
    if ((rc = marg_fetch(h, s, h->pri.buf[PriorFamily::PT_LIST], (size_t)h->pri.n_pts, pt_prior)) != SRK_OK) return rc;
    if ((rc = marg_fetch(h, s, h->pri.buf[PriorFamily::FR_LIST], (size_t)h->pri.n_frames, fr_prior)) != SRK_OK) return rc;
    if ((rc = marg_fetch(h, s, h->jp.buf[JPriorFamily::PTR], h->jp.n > 0 ? (size_t)h->jp.n + 1 : 0, mc.set_ptr)) != SRK_OK) return rc;
    if ((rc = marg_fetch(h, s, h->jp.buf[JPriorFamily::FRAME], h->jp.n > 0 ? (size_t)mc.set_ptr.back() : 0, mc.set_frame)) != SRK_OK) return rc;
    SrkMargScene sc;
    sc.N = d.N;
    sc.M = d.M;
    sc.row_ptr = h->row_ptr_int.data();
    sc.obs_frame = h->mg_obs_frame.data();
    sc.q = qt.on ? qt.q.data() : nullptr;
    sc.perm = h->perm.data();
    sc.frame_int = h->frame_int.empty() ? nullptr : h->frame_int.data();
    sc.frame_user = h->frame_user.empty() ? nullptr : h->frame_user.data();
    sc.n_pt_priors = (int64_t)pt_prior.size();
    sc.pt_prior = pt_prior.data();
    sc.n_fr_priors = (int32_t)fr_prior.size();
    sc.fr_prior = fr_prior.data();
    sc.n_rp = h->rp.n;
    sc.rp_a = h->rp.int_a.data();
    sc.rp_b = h->rp.int_b.data();
    sc.n_sets = h->jp.n;
    sc.set_ptr = mc.set_ptr.data();
    sc.set_frame = mc.set_frame.data();
    sc.constant_blocks = h->cst.n_pts > 0 || h->cst.n_frames > 0;
    sc.intrinsic_groups = h->shk_G > 0;
    sc.multi_rank = h->world > 1 || h->allreduce || h->comm;
    const std::string why = srk_marg_plan(sc, nd, drop, np, points, mc.plan);
    if (!why.empty()) { h->last_error = why; return SRK_E_ARGS; }
    return SRK_OK;
}

static int marg_kept_out(srk_ba* h, const MargCall& mc, int32_t kept_cap, int32_t* kept, int32_t* n_kept, bool write)
{
    if (kept && kept_cap < mc.plan.k) {
        h->last_error = "marginalization: " + std::to_string(mc.plan.k) + " kept frames do not fit kept_cap = " + std::to_string(kept_cap);
        return SRK_E_ARGS;
    }
    if (write) {
        copy_out(kept, mc.plan.kept);
        if (n_kept) *n_kept = mc.plan.k;
    }
    return SRK_OK;
}

// A0, b0: the two kernels and their second passes on the current scene
static int marg_device(srk_ba* h, MargCall& mc)
{
    const SrkDims& d = h->d;
    const SrkMargPlan& p = mc.plan;
    hipStream_t s = h->main_stream;
    const int32_t ns = p.d + p.k, ldz = p.ldz(), ncols = 6 * ns;
    const int64_t n_lm = (int64_t)p.lm.size(), n_rows = p.n_rows;
    // the row chunks of Z: 512 rows each (128 landmarks), at most 64 of them
    const int32_t n_chunks = (int32_t)std::min<int64_t>(64, (n_rows + 511) / 512);
    const int64_t rows_per_chunk = n_chunks > 0 ? ((n_rows + n_chunks - 1) / n_chunks + 15) / 16 * 16 : 0;
    int rc;
    DevBuf* g = h->mg;
    if ((rc = marg_put(h, s, g[srk_ba::MG_LM], p.lm)) != SRK_OK || (rc = marg_put(h, s, g[srk_ba::MG_LM_STAGE], p.lm_stage)) != SRK_OK ||
        (rc = marg_put(h, s, g[srk_ba::MG_LM_PRIOR], p.lm_prior)) != SRK_OK || (rc = marg_put(h, s, g[srk_ba::MG_FRAME_SLOT], p.frame_slot)) != SRK_OK ||
        (rc = marg_put(h, s, g[srk_ba::MG_SLOT_PTR], p.slot_ptr)) != SRK_OK || (rc = marg_put(h, s, g[srk_ba::MG_SLOT_ENT], p.slot_ent)) != SRK_OK)
        return rc;
    const size_t z_bytes = (size_t)(8 * n_rows * ldz), st_bytes = (size_t)(8 * p.n_stage * SRK_MARG_STAGE);
    const size_t out_doubles = (size_t)ncols * ncols + (size_t)ncols;
    if ((rc = dev_alloc(h, g[srk_ba::MG_Z], z_bytes)) != SRK_OK || (rc = dev_alloc(h, g[srk_ba::MG_STAGE], st_bytes)) != SRK_OK ||
        (rc = dev_alloc(h, g[srk_ba::MG_SKIP], (size_t)(4 * n_lm))) != SRK_OK || (rc = dev_alloc(h, g[srk_ba::MG_US], (size_t)(8 * 27 * ns))) != SRK_OK ||
        (rc = dev_alloc(h, g[srk_ba::MG_PART], (size_t)(8 * (int64_t)n_chunks * ldz * ldz))) != SRK_OK ||
        (rc = dev_alloc(h, g[srk_ba::MG_OUT], 8 * out_doubles)) != SRK_OK)
        return rc;
    for (hipEvent_t& e : h->mg_ev)
        if (!e) HIPCHK(h, hipEventCreate(&e));
    if (z_bytes) HIPCHK(h, hipMemsetAsync(g[srk_ba::MG_Z].p, 0, z_bytes, s));
    if (st_bytes) HIPCHK(h, hipMemsetAsync(g[srk_ba::MG_STAGE].p, 0, st_bytes, s));
    if (n_lm) HIPCHK(h, hipMemsetAsync(g[srk_ba::MG_SKIP].p, 0, (size_t)(4 * n_lm), s));
    SrkMargTables t{};
    t.n_lm = (int32_t)n_lm;
    t.n_slots = ns;
    t.ldz = ldz;
    t.lm = P<int32_t>(g[srk_ba::MG_LM]);
    t.lm_stage = P<int64_t>(g[srk_ba::MG_LM_STAGE]);
    t.lm_prior = P<int32_t>(g[srk_ba::MG_LM_PRIOR]);
    t.frame_slot = P<int32_t>(g[srk_ba::MG_FRAME_SLOT]);
    t.prior_val = P<double>(h->pri.buf[PriorFamily::PT_VAL]);
    t.n_priors = h->pri.n_pts;
    t.slot_ptr = P<int32_t>(g[srk_ba::MG_SLOT_PTR]);
    t.slot_ent = P<int64_t>(g[srk_ba::MG_SLOT_ENT]);
    SrkLoss Ls;
    const SrkLoss* L = robust_loss(h, Ls);
    const int c = h->cur;
    HIPCHK(h, hipEventRecord(h->mg_ev[0], s));
    srk_launch_marg_rows(s, d, P<double>(h->pts[c]), P<double>(h->cam[c]), P<int64_t>(h->row_ptr), P<int32_t>(h->obs_frame), P<double>(h->obs_uv), L,
                         t, P<double>(g[srk_ba::MG_Z]), P<double>(g[srk_ba::MG_STAGE]), P<int32_t>(g[srk_ba::MG_SKIP]));
    srk_launch_marg_frame_sums(s, t, P<double>(g[srk_ba::MG_STAGE]), P<double>(g[srk_ba::MG_US]));
    HIPCHK(h, hipEventRecord(h->mg_ev[1], s));
    HIPCHK(h, hipEventRecord(h->mg_ev[2], s));
    srk_launch_marg_gram(s, P<double>(g[srk_ba::MG_Z]), n_rows, ldz, n_chunks, rows_per_chunk, P<double>(g[srk_ba::MG_PART]));
    srk_launch_marg_reduce(s, P<double>(g[srk_ba::MG_PART]), n_chunks, ldz, ns, P<double>(g[srk_ba::MG_US]), P<double>(g[srk_ba::MG_OUT]),
                           P<double>(g[srk_ba::MG_OUT]) + (size_t)ncols * ncols);
    HIPCHK(h, hipEventRecord(h->mg_ev[3], s));
    HIPCHK(h, hipGetLastError());
    std::vector<double> out;
    std::vector<int32_t> skip;
    if ((rc = marg_fetch(h, s, g[srk_ba::MG_OUT], out_doubles, out)) != SRK_OK) return rc;
    if ((rc = marg_fetch(h, s, g[srk_ba::MG_SKIP], (size_t)n_lm, skip)) != SRK_OK) return rc;
    mc.A0.assign(out.begin(), out.begin() + (size_t)ncols * ncols);
    mc.b0.assign(out.begin() + (size_t)ncols * ncols, out.end());
    int64_t n_skip = 0;
    for (int32_t v : skip) n_skip += v ? 1 : 0;
    float ms0 = 0, ms1 = 0;
    HIPCHK(h, hipEventElapsedTime(&ms0, h->mg_ev[0], h->mg_ev[1]));
    HIPCHK(h, hipEventElapsedTime(&ms1, h->mg_ev[2], h->mg_ev[3]));
    mc.rep.landmarks_used = n_lm - n_skip;
    mc.rep.landmarks_skipped = p.n_single + n_skip;
    mc.rep.ms_rows = ms0;
    mc.rep.ms_gram = ms1;
    return SRK_OK;
}

// A1, b1 = A0, b0 plus the host's terms: the priors on centres of D, the relative-pose factors and the joint sets, at the current poses
static int marg_host_terms(srk_ba* h, MargCall& mc)
{
    const SrkDims& d = h->d;
    const SrkMargPlan& p = mc.plan;
    hipStream_t s = h->main_stream;
    const int64_t n = 6 * (int64_t)(p.d + p.k);
    const int c = h->cur;
    int rc;
    if ((rc = marg_fetch(h, s, h->camR[c], (size_t)(9 * d.M), mc.R)) != SRK_OK || (rc = marg_fetch(h, s, h->camT[c], (size_t)(3 * d.M), mc.T)) != SRK_OK) return rc;
    mc.A1 = mc.A0;
    mc.b1 = mc.b0;
    // H [m][m], g [m] over the pose variables of the listed internal frames, into A1, b1
    const auto scatter = [&](int32_t nf, const int32_t* frames, const double* H, const double* gv) {
        const int m = 6 * nf;
        for (int a = 0; a < m; ++a) {
            const int64_t ra = 6 * (int64_t)p.frame_slot[(size_t)frames[a / 6]] + a % 6;
            mc.b1[(size_t)ra] += gv[a];
            for (int b = 0; b < m; ++b) mc.A1[(size_t)(ra * n + 6 * (int64_t)p.frame_slot[(size_t)frames[b / 6]] + b % 6)] += H[a * m + b];
        }
    };
    if (!p.fr_priors.empty()) {
        std::vector<int32_t> list;
        std::vector<double> val;
        const size_t nf = (size_t)h->pri.n_frames;
        if ((rc = marg_fetch(h, s, h->pri.buf[PriorFamily::FR_LIST], nf, list)) != SRK_OK || (rc = marg_fetch(h, s, h->pri.buf[PriorFamily::FR_VAL], 9 * nf, val)) != SRK_OK) return rc;
        for (int32_t q : p.fr_priors) {
            const int32_t f = list[(size_t)q];
            const double* r = &mc.R[9 * (size_t)f];
            const double* t = &mc.T[3 * (size_t)f];
            double dx[3];
            for (int e = 0; e < 3; ++e) dx[e] = -(r[e] * t[0] + r[3 + e] * t[1] + r[6 + e] * t[2]) - val[(size_t)e * nf + (size_t)q];
            const double* v = val.data();
            const double L[9] = { v[3 * nf + q], v[4 * nf + q], v[5 * nf + q], v[4 * nf + q], v[6 * nf + q], v[7 * nf + q], v[5 * nf + q], v[7 * nf + q], v[8 * nf + q] };
            double H[36] = {}, gv[6] = {};
            for (int a = 0; a < 3; ++a) {
                gv[a] = L[3 * a] * dx[0] + L[3 * a + 1] * dx[1] + L[3 * a + 2] * dx[2];
                for (int b = 0; b < 3; ++b) H[6 * a + b] = L[3 * a + b];
            }
            scatter(1, &f, H, gv);
        }
    }
    if (!p.factors.empty()) {
        std::vector<double> val;
        const size_t nf = (size_t)h->rp.n;
        if ((rc = marg_fetch(h, s, h->rp.buf[RelPoseFamily::VAL], SRK_RP_PLANES * nf, val)) != SRK_OK) return rc;
        for (int32_t q : p.factors) {
            const int32_t fr[2] = { h->rp.int_a[(size_t)q], h->rp.int_b[(size_t)q] };
            double Z[9], z[3], L[36], H[144], gv[12];
            for (int e = 0; e < 9; ++e) Z[e] = val[(size_t)e * nf + (size_t)q];
            for (int e = 0; e < 3; ++e) z[e] = val[(size_t)(9 + e) * nf + (size_t)q];
            int k = 12;
            for (int r = 0; r < 6; ++r)
                for (int cc = r; cc < 6; ++cc, ++k) L[6 * r + cc] = L[6 * cc + r] = val[(size_t)k * nf + (size_t)q];
            srk_relpose_terms(&mc.R[9 * (size_t)fr[0]], &mc.T[3 * (size_t)fr[0]], &mc.R[9 * (size_t)fr[1]], &mc.T[3 * (size_t)fr[1]], Z, z, L, H, gv);
            scatter(2, fr, H, gv);
        }
    }
    if (!p.sets.empty()) {
        std::vector<double> lin, mean, info;
        std::vector<int64_t> iptr;
        const size_t nq = mc.set_frame.size();
        if ((rc = marg_fetch(h, s, h->jp.buf[JPriorFamily::LIN], 12 * nq, lin)) != SRK_OK || (rc = marg_fetch(h, s, h->jp.buf[JPriorFamily::MEAN], 6 * nq, mean)) != SRK_OK ||
            (rc = marg_fetch(h, s, h->jp.buf[JPriorFamily::IPTR], (size_t)h->jp.n, iptr)) != SRK_OK)
            return rc;
        int64_t n_info = 0;
        for (int32_t gq = 0; gq < h->jp.n; ++gq) {
            const int64_t k = mc.set_ptr[(size_t)gq + 1] - mc.set_ptr[(size_t)gq];
            n_info = std::max(n_info, iptr[(size_t)gq] + 36 * k * k);
        }
        if ((rc = marg_fetch(h, s, h->jp.buf[JPriorFamily::INFO], (size_t)n_info, info)) != SRK_OK) return rc;
        for (int32_t gq : p.sets) {
            const int32_t q0 = mc.set_ptr[(size_t)gq], k = mc.set_ptr[(size_t)gq + 1] - q0;
            std::vector<double> Rk((size_t)(9 * k)), Tk((size_t)(3 * k)), H((size_t)(36 * k * k)), gv((size_t)(6 * k));
            for (int32_t i = 0; i < k; ++i) {
                const size_t f = (size_t)mc.set_frame[(size_t)(q0 + i)];
                std::copy(&mc.R[9 * f], &mc.R[9 * f] + 9, &Rk[9 * (size_t)i]);
                std::copy(&mc.T[3 * f], &mc.T[3 * f] + 3, &Tk[3 * (size_t)i]);
            }
            srk_jprior_terms(k, Rk.data(), Tk.data(), &lin[12 * (size_t)q0], &mean[6 * (size_t)q0], &info[(size_t)iptr[(size_t)gq]], H.data(), gv.data());
            scatter(k, &mc.set_frame[(size_t)q0], H.data(), gv.data());
        }
    }
    for (int64_t r = 0; r < n; ++r) // (both triangles carry the same sums up to rounding)
        for (int64_t cc = r + 1; cc < n; ++cc) mc.A1[(size_t)(r * n + cc)] = mc.A1[(size_t)(cc * n + r)] = 0.5 * (mc.A1[(size_t)(r * n + cc)] + mc.A1[(size_t)(cc * n + r)]);
    mc.rep.factors = (int32_t)p.factors.size();
    mc.rep.sets = (int32_t)p.sets.size();
    mc.rep.frame_priors = (int32_t)p.fr_priors.size();
    return SRK_OK;
}

extern "C" {

int srk_ba_marginalization_plan(srk_ba* h, int32_t n_drop, const int32_t* drop, int64_t n_points, const int64_t* points, int32_t kept_cap,
                                int32_t* kept, srk_ba_marg_counts* counts)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    try {
        HIPCHK(h, hipSetDevice(h->device));
        MargCall mc;
        int rc = marg_plan(h, n_drop, drop, n_points, points, mc);
        if (rc != SRK_OK || (rc = marg_kept_out(h, mc, kept_cap, kept, nullptr, true)) != SRK_OK) return rc;
        const SrkMargPlan& p = mc.plan;
        if (counts)
            *counts = srk_ba_marg_counts{ p.d, p.k, (int64_t)p.lm.size(), p.n_single, p.n_stage, (int32_t)p.factors.size(), (int32_t)p.sets.size(),
                                          (int32_t)p.fr_priors.size() };
        return SRK_OK;
    } catch (const std::bad_alloc&) {
        h->last_error = "marginalization_plan: out of host memory";
        return SRK_E_NOMEM;
    }
}

int srk_ba_phase_marginalization(srk_ba* h, int32_t n_drop, const int32_t* drop, int64_t n_points, const int64_t* points, int32_t kept_cap,
                                 int32_t* kept, int32_t* n_kept, double* A0, double* b0, double* A1, double* b1, srk_ba_marg_report* report)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    try {
        HIPCHK(h, hipSetDevice(h->device));
        MargCall mc;
        int rc = marg_plan(h, n_drop, drop, n_points, points, mc);
        if (rc != SRK_OK || (rc = marg_kept_out(h, mc, kept_cap, kept, n_kept, false)) != SRK_OK) return rc;
        if ((rc = marg_device(h, mc)) != SRK_OK || (rc = marg_host_terms(h, mc)) != SRK_OK) return rc;
        marg_kept_out(h, mc, kept_cap, kept, n_kept, true);
        copy_out(A0, mc.A0);
        copy_out(b0, mc.b0);
        copy_out(A1, mc.A1);
        copy_out(b1, mc.b1);
        if (report) *report = mc.rep;
        return SRK_OK;
    } catch (const std::bad_alloc&) {
        h->last_error = "phase_marginalization: out of host memory";
        return SRK_E_NOMEM;
    }
}

int srk_ba_marginalization_prior(srk_ba* h, int32_t n_drop, const int32_t* drop, int64_t n_points, const int64_t* points, int32_t kept_cap,
                                 int32_t* kept, int32_t* n_kept, double* lin_R, double* lin_C, double* info, double* eta, double* mean,
                                 srk_ba_marg_report* report)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    try {
        HIPCHK(h, hipSetDevice(h->device));
        MargCall mc;
        int rc = marg_plan(h, n_drop, drop, n_points, points, mc);
        if (rc != SRK_OK || (rc = marg_kept_out(h, mc, kept_cap, kept, n_kept, false)) != SRK_OK) return rc;
        if ((rc = marg_device(h, mc)) != SRK_OK) return rc;
        const auto t0 = std::chrono::steady_clock::now();
        if ((rc = marg_host_terms(h, mc)) != SRK_OK) return rc;
        const SrkMargPlan& p = mc.plan;
        const size_t nk = 6 * (size_t)p.k;
        std::vector<double> Lam(nk * nk), et(nk), mn(nk), lr(9 * (size_t)p.k), lc(3 * (size_t)p.k);
        if (srk_marg_dense(mc.A1.data(), mc.b1.data(), p.d, p.k, Lam.data(), et.data(), mn.data(), &mc.rep.defect) != 0) {
            h->last_error = "marginalization: the block of the dropped frames is not positive definite";
            return 1;
        }
        for (int32_t i = 0; i < p.k; ++i) {
            const size_t f = (size_t)p.slot_frame[(size_t)(p.d + i)];
            const double* r = &mc.R[9 * f];
            const double* t = &mc.T[3 * f];
            std::copy(r, r + 9, &lr[9 * (size_t)i]);
            for (int e = 0; e < 3; ++e) lc[3 * (size_t)i + e] = -(r[e] * t[0] + r[3 + e] * t[1] + r[6 + e] * t[2]);
        }
        if (h->normalized_on_upload) srk_marg_revert(h->nrm, p.k, lr.data(), lc.data(), Lam.data(), et.data(), mn.data());
        mc.rep.ms_host = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        marg_kept_out(h, mc, kept_cap, kept, n_kept, true);
        copy_out(lin_R, lr);
        copy_out(lin_C, lc);
        copy_out(info, Lam);
        copy_out(eta, et);
        copy_out(mean, mn);
        if (report) *report = mc.rep;
        return SRK_OK;
    } catch (const std::bad_alloc&) {
        h->last_error = "marginalization_prior: out of host memory";
        return SRK_E_NOMEM;
    }
}

} // extern "C"

// ------------------------------------------------------------------ batched triangulation
// The checked tracks of a call to the device, the kernel over the given frames' poses (device pointers), the results back.
// frame: the frames as the pose arrays number them.
static int tri_run(srk_ba* h, double f0, int64_t n_tracks, const int64_t* row_ptr, const int32_t* frame, const double* uv, const double* q,
                   int32_t n_frames, const double* dR, const double* dT, const double* dK, int shared_k, const srk_tri_options& o, double* X,
                   double* quality, uint32_t* status)
{
    hipStream_t s = h->main_stream;
    const int64_t O = row_ptr[n_tracks];
    DevBuf* g = h->tri;
    int rc;
    struct { DevBuf* b; const void* src; size_t bytes; } up[] = {
        { &g[srk_ba::TRI_ROW], row_ptr, (size_t)(8 * (n_tracks + 1)) }, { &g[srk_ba::TRI_FRAME], frame, (size_t)(4 * O) },
        { &g[srk_ba::TRI_UV], uv, (size_t)(16 * O) },                   { &g[srk_ba::TRI_Q], q, q ? (size_t)(8 * O) : 0 },
    };
    for (auto& u : up) {
        if ((rc = dev_alloc(h, *u.b, u.bytes)) != SRK_OK) return rc;
        if (u.bytes) HIPCHK(h, hipMemcpyAsync(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice, s));
    }
    if ((rc = dev_alloc(h, g[srk_ba::TRI_PACK], (size_t)(8 * SRK_TRI_PACK * (int64_t)n_frames))) != SRK_OK ||
        (rc = dev_alloc(h, g[srk_ba::TRI_X], (size_t)(24 * n_tracks))) != SRK_OK || (rc = dev_alloc(h, g[srk_ba::TRI_QUAL], (size_t)(32 * n_tracks))) != SRK_OK ||
        (rc = dev_alloc(h, g[srk_ba::TRI_STATUS], (size_t)(4 * n_tracks))) != SRK_OK)
        return rc;
    for (hipEvent_t& e : h->tri_ev)
        if (!e) HIPCHK(h, hipEventCreate(&e));
    HIPCHK(h, hipEventRecord(h->tri_ev[0], s));
    srk_launch_tri_pack(s, n_frames, dR, dT, dK, shared_k, P<double>(g[srk_ba::TRI_PACK]));
    srk_launch_tri_tracks(s, n_tracks, P<int64_t>(g[srk_ba::TRI_ROW]), P<int32_t>(g[srk_ba::TRI_FRAME]), P<double>(g[srk_ba::TRI_UV]),
                          q ? P<double>(g[srk_ba::TRI_Q]) : nullptr, P<double>(g[srk_ba::TRI_PACK]), f0, o.refine_attempts, o.refine_rel_change,
                          o.min_parallax_deg, P<double>(g[srk_ba::TRI_X]), P<double>(g[srk_ba::TRI_QUAL]), P<uint32_t>(g[srk_ba::TRI_STATUS]));
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->tri_ev[1], s));
    HIPCHK(h, hipMemcpyAsync(X, g[srk_ba::TRI_X].p, (size_t)(24 * n_tracks), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(quality, g[srk_ba::TRI_QUAL].p, (size_t)(32 * n_tracks), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(status, g[srk_ba::TRI_STATUS].p, (size_t)(4 * n_tracks), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->tri_ev[0], h->tri_ev[1]));
    h->tri_ms = ms;
    return SRK_OK;
}

extern "C" double srk_ba_triangulate_kernel_ms(const srk_ba* h) { return h ? h->tri_ms : 0.0; }

extern "C" int srk_triangulate_tracks(srk_ba* h, double f0, int64_t n_tracks, const int64_t* row_ptr, const int32_t* frame, const double* uv,
                                      const double* q, int32_t n_frames, const double* cam_R, const double* cam_T, const double* K, int shared_k,
                                      const srk_tri_options* opts, double* X, double* quality, uint32_t* status)
{
    if (!h) return SRK_E_ARGS;
    try {
        std::string why = srk_tri_check(n_tracks, row_ptr, frame, uv, q, n_frames, opts);
        if (why.empty() && (!cam_R || !cam_T || !K)) why = "triangulate: a NULL pose or intrinsics array";
        if (why.empty() && (!std::isfinite(f0) || srk::is_close(0.0, f0))) why = "triangulate: f0 must be finite and not ~0";
        if (why.empty() && n_tracks > 0 && (!X || !quality || !status)) why = "triangulate: a NULL output array";
        if (!why.empty()) { h->last_error = why; return SRK_E_ARGS; }
        if (n_tracks == 0) return SRK_OK;
        HIPCHK(h, hipSetDevice(h->device));
        hipStream_t s = h->main_stream;
        DevBuf* g = h->tri;
        int rc;
        struct { DevBuf* b; const void* src; size_t bytes; } up[] = {
            { &g[srk_ba::TRI_R], cam_R, (size_t)(72 * (int64_t)n_frames) }, { &g[srk_ba::TRI_T], cam_T, (size_t)(24 * (int64_t)n_frames) },
            { &g[srk_ba::TRI_K], K, (size_t)(72 * (int64_t)(shared_k ? 1 : n_frames)) },
        };
        for (auto& u : up) {
            if ((rc = dev_alloc(h, *u.b, u.bytes)) != SRK_OK) return rc;
            HIPCHK(h, hipMemcpyAsync(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice, s));
        }
        return tri_run(h, f0, n_tracks, row_ptr, frame, uv, q, n_frames, P<double>(g[srk_ba::TRI_R]), P<double>(g[srk_ba::TRI_T]),
                       P<double>(g[srk_ba::TRI_K]), shared_k ? 1 : 0, srk_tri_effective_options(opts), X, quality, status);
    } catch (const std::bad_alloc&) {
        h->last_error = "triangulate: out of host memory";
        return SRK_E_NOMEM;
    }
}

extern "C" int srk_ba_triangulate(srk_ba* h, int64_t n_tracks, const int64_t* row_ptr, const int32_t* frame, const double* uv, const double* q,
                                  const srk_tri_options* opts, int revert_normalization, double* X, double* quality, uint32_t* status)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    try {
        std::string why;
        if (h->world > 1 || h->allreduce || h->comm) why = "triangulate: more than one rank is not supported";
        else if (h->shk_G > 0) why = "triangulate: intrinsic groups are not supported";
        else why = srk_tri_check(n_tracks, row_ptr, frame, uv, q, h->d.M, opts);
        if (why.empty() && n_tracks > 0 && (!X || !quality || !status)) why = "triangulate: a NULL output array";
        if (!why.empty()) { h->last_error = why; return SRK_E_ARGS; }
        if (n_tracks == 0) return SRK_OK;
        HIPCHK(h, hipSetDevice(h->device));
        for (auto& a : h->att) // nothing of an earlier call is still writing the scene
            if (a.allocated && a.stream) HIPCHK(h, hipStreamSynchronize(a.stream));
        std::vector<int32_t> fr;
        srk_tri_map_frames(row_ptr[n_tracks], frame, h->frame_int.empty() ? nullptr : h->frame_int.data(), fr);
        const int c = h->cur;
        const int rc = tri_run(h, h->f0, n_tracks, row_ptr, fr.data(), uv, q, h->d.M, P<double>(h->camR[c]), P<double>(h->camT[c]), kbuf(h, c), 0,
                               srk_tri_effective_options(opts), X, quality, status);
        if (rc != SRK_OK) return rc;
        if (revert_normalization && h->normalized_on_upload) srk_tri_revert_points(&h->nrm, n_tracks, X);
        return SRK_OK;
    } catch (const std::bad_alloc&) {
        h->last_error = "triangulate: out of host memory";
        return SRK_E_NOMEM;
    }
}

// ------------------------------------------------------------------ batched camera resection
// The checked frames of a call to the device, the two kernels over the given landmarks (a device pointer), the results back.
// point: the landmarks as dX numbers them.  K, R0, T0: host arrays in the coordinates of dX.
static int resect_run(srk_ba* h, double f0, int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv, const double* q,
                      const double* dX, const double* K, int shared_k, const double* R0, const double* T0, const srk_resect_options& o, double* R,
                      double* T, double* quality, double* info, uint32_t* status, double* w_out)
{
    hipStream_t s = h->main_stream;
    const int64_t O = row_ptr[n_frames], n = n_frames;
    DevBuf* g = h->rs;
    int rc;
    struct { DevBuf* b; const void* src; size_t bytes; } up[] = {
        { &g[srk_ba::RS_ROW], row_ptr, (size_t)(8 * (n + 1)) }, { &g[srk_ba::RS_POINT], point, (size_t)(4 * O) },
        { &g[srk_ba::RS_UV], uv, (size_t)(16 * O) },            { &g[srk_ba::RS_Q], q, q ? (size_t)(8 * O) : 0 },
        { &g[srk_ba::RS_K], K, (size_t)(72 * (shared_k ? 1 : n)) }, { &g[srk_ba::RS_R0], R0, (size_t)(72 * n) },
        { &g[srk_ba::RS_T0], T0, (size_t)(24 * n) },
    };
    for (auto& u : up) {
        if ((rc = dev_alloc(h, *u.b, u.bytes)) != SRK_OK) return rc;
        if (u.bytes) HIPCHK(h, hipMemcpyAsync(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice, s));
    }
    if ((rc = dev_alloc(h, g[srk_ba::RS_PACK], (size_t)(8 * SRK_RESECT_PACK * n))) != SRK_OK || (rc = dev_alloc(h, g[srk_ba::RS_R], (size_t)(72 * n))) != SRK_OK ||
        (rc = dev_alloc(h, g[srk_ba::RS_T], (size_t)(24 * n))) != SRK_OK || (rc = dev_alloc(h, g[srk_ba::RS_QUAL], (size_t)(48 * n))) != SRK_OK ||
        (rc = dev_alloc(h, g[srk_ba::RS_INFO], (size_t)(288 * n))) != SRK_OK || (rc = dev_alloc(h, g[srk_ba::RS_STATUS], (size_t)(4 * n))) != SRK_OK ||
        (rc = dev_alloc(h, g[srk_ba::RS_W], w_out ? (size_t)(8 * O) : 0)) != SRK_OK)
        return rc;
    for (hipEvent_t& e : h->rs_ev)
        if (!e) HIPCHK(h, hipEventCreate(&e));
    HIPCHK(h, hipEventRecord(h->rs_ev[0], s));
    srk_launch_resect_pack(s, n_frames, P<double>(g[srk_ba::RS_R0]), P<double>(g[srk_ba::RS_T0]), P<double>(g[srk_ba::RS_K]), shared_k,
                           P<double>(g[srk_ba::RS_PACK]));
    srk_launch_resect_frames(s, n_frames, P<int64_t>(g[srk_ba::RS_ROW]), P<int32_t>(g[srk_ba::RS_POINT]), P<double>(g[srk_ba::RS_UV]),
                             q ? P<double>(g[srk_ba::RS_Q]) : nullptr, dX, P<double>(g[srk_ba::RS_K]), shared_k, P<double>(g[srk_ba::RS_R0]),
                             P<double>(g[srk_ba::RS_T0]), P<double>(g[srk_ba::RS_PACK]), f0, o.attempts, o.rel_change, o.loss_kind,
                             o.loss_delta_pixels, P<double>(g[srk_ba::RS_R]), P<double>(g[srk_ba::RS_T]), P<double>(g[srk_ba::RS_QUAL]),
                             P<double>(g[srk_ba::RS_INFO]), P<uint32_t>(g[srk_ba::RS_STATUS]), w_out && O > 0 ? P<double>(g[srk_ba::RS_W]) : nullptr);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->rs_ev[1], s));
    HIPCHK(h, hipMemcpyAsync(R, g[srk_ba::RS_R].p, (size_t)(72 * n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(T, g[srk_ba::RS_T].p, (size_t)(24 * n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(quality, g[srk_ba::RS_QUAL].p, (size_t)(48 * n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(info, g[srk_ba::RS_INFO].p, (size_t)(288 * n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(status, g[srk_ba::RS_STATUS].p, (size_t)(4 * n), hipMemcpyDeviceToHost, s));
    if (w_out && O > 0) HIPCHK(h, hipMemcpyAsync(w_out, g[srk_ba::RS_W].p, (size_t)(8 * O), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->rs_ev[0], h->rs_ev[1]));
    h->rs_ms = ms;
    return SRK_OK;
}

extern "C" double srk_ba_resect_kernel_ms(const srk_ba* h) { return h ? h->rs_ms : 0.0; }

extern "C" int srk_resect_frames(srk_ba* h, double f0, int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv,
                                 const double* q, int64_t n_points, const double* X, const double* K, int shared_k, const double* R0,
                                 const double* T0, const srk_resect_options* opts, double* R, double* T, double* quality, double* info,
                                 uint32_t* status, double* w_out)
{
    if (!h) return SRK_E_ARGS;
    try {
        std::string why = srk_resect_check(n_frames, row_ptr, point, uv, q, n_points, X, K, shared_k, R0, T0, opts);
        if (why.empty() && n_points > 0 && !X) why = "resect: the landmark array is NULL";
        if (why.empty() && (!std::isfinite(f0) || srk::is_close(0.0, f0))) why = "resect: f0 must be finite and not ~0";
        if (why.empty() && n_frames > 0 && (!R || !T || !quality || !info || !status)) why = "resect: a NULL output array";
        if (!why.empty()) { h->last_error = why; return SRK_E_ARGS; }
        if (n_frames == 0) return SRK_OK;
        HIPCHK(h, hipSetDevice(h->device));
        DevBuf& gx = h->rs[srk_ba::RS_X];
        int rc;
        if ((rc = dev_alloc(h, gx, (size_t)(24 * n_points))) != SRK_OK) return rc;
        if (n_points > 0) HIPCHK(h, hipMemcpyAsync(gx.p, X, (size_t)(24 * n_points), hipMemcpyHostToDevice, h->main_stream));
        return resect_run(h, f0, n_frames, row_ptr, point, uv, q, P<double>(gx), K, shared_k ? 1 : 0, R0, T0, srk_resect_effective_options(opts), R, T,
                          quality, info, status, w_out);
    } catch (const std::bad_alloc&) {
        h->last_error = "resect: out of host memory";
        return SRK_E_NOMEM;
    }
}

extern "C" int srk_ba_resect(srk_ba* h, int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv, const double* q,
                             const double* K, int shared_k, const double* R0, const double* T0, const srk_resect_options* opts,
                             int revert_normalization, double* R, double* T, double* quality, double* info, uint32_t* status, double* w_out)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    try {
        std::string why;
        std::vector<int32_t> pt;
        if (h->world > 1 || h->allreduce || h->comm) why = "resect: more than one rank is not supported";
        else {
            std::vector<int64_t> pt_int((size_t)h->d.N); // the caller's landmark -> its place in the handle's landmark order
            for (int64_t i = 0; i < h->d.N; ++i) pt_int[(size_t)h->perm[(size_t)i]] = i;
            why = srk_resect_check(n_frames, row_ptr, point, uv, q, h->d.N, nullptr, K, shared_k, R0, T0, opts, pt_int.data(), &pt);
        }
        if (why.empty() && n_frames > 0 && (!R || !T || !quality || !info || !status)) why = "resect: a NULL output array";
        if (!why.empty()) { h->last_error = why; return SRK_E_ARGS; }
        if (n_frames == 0) return SRK_OK;
        HIPCHK(h, hipSetDevice(h->device));
        for (auto& a : h->att) // nothing of an earlier call is still writing the scene
            if (a.allocated && a.stream) HIPCHK(h, hipStreamSynchronize(a.stream));
        std::vector<double> Rn((size_t)(9 * (int64_t)n_frames)), Tn((size_t)(3 * (int64_t)n_frames));
        if (h->normalized_on_upload) srk_resect_normalize_poses(h->nrm, n_frames, R0, T0, Rn.data(), Tn.data());
        else {
            std::memcpy(Rn.data(), R0, Rn.size() * 8);
            std::memcpy(Tn.data(), T0, Tn.size() * 8);
        }
        const int rc = resect_run(h, h->f0, n_frames, row_ptr, pt.data(), uv, q, P<double>(h->pts[h->cur]), K, shared_k ? 1 : 0, Rn.data(), Tn.data(),
                                  srk_resect_effective_options(opts), R, T, quality, info, status, w_out);
        if (rc != SRK_OK) return rc;
        if (revert_normalization && h->normalized_on_upload) {
            std::vector<char> moved((size_t)n_frames);
            for (int32_t i = 0; i < n_frames; ++i)
                moved[(size_t)i] = std::memcmp(R + 9 * (int64_t)i, &Rn[(size_t)(9 * (int64_t)i)], 72) != 0 || std::memcmp(T + 3 * (int64_t)i, &Tn[(size_t)(3 * (int64_t)i)], 24) != 0;
            srk_resect_revert_poses(h->nrm, n_frames, R, T, info, quality);
            for (int32_t i = 0; i < n_frames; ++i) // a pose that did not move is the caller's start bit for bit, not its round trip
                if (!moved[(size_t)i]) {
                    std::memcpy(R + 9 * (int64_t)i, R0 + 9 * (int64_t)i, 72);
                    std::memcpy(T + 3 * (int64_t)i, T0 + 3 * (int64_t)i, 24);
                }
        }
        return SRK_OK;
    } catch (const std::bad_alloc&) {
        h->last_error = "resect: out of host memory";
        return SRK_E_NOMEM;
    }
}

// ------------------------------------------------------------------ resection without a start pose
// The checked frames of a call to the device, gather / hypotheses and scores / pick over the given landmarks (a device pointer),
// the refinement's two kernels from the located poses when asked for, the results back.  point: the landmarks as dX numbers them.
static int locate_run(srk_ba* h, double f0, int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv, const double* q,
                      const double* dX, const double* K, int shared_k, const srk_locate_options& lo, const srk_resect_options* refine, double* R,
                      double* T, double* located, uint32_t* located_status, uint8_t* inlier_out, double* quality, double* info, uint32_t* status,
                      double* w_out)
{
    hipStream_t s = h->main_stream;
    const int64_t O = row_ptr[n_frames], n = n_frames;
    const int64_t waves = (lo.hypotheses + SRK_LOCATE_LANES - 1) / SRK_LOCATE_LANES;
    DevBuf* g = h->rs;
    DevBuf* l = h->lc;
    int rc;
    struct { DevBuf* b; const void* src; size_t bytes; } up[] = {
        { &g[srk_ba::RS_ROW], row_ptr, (size_t)(8 * (n + 1)) }, { &g[srk_ba::RS_POINT], point, (size_t)(4 * O) },
        { &g[srk_ba::RS_UV], uv, (size_t)(16 * O) },            { &g[srk_ba::RS_Q], q, q ? (size_t)(8 * O) : 0 },
        { &g[srk_ba::RS_K], K, (size_t)(72 * (shared_k ? 1 : n)) },
    };
    for (auto& u : up) {
        if ((rc = dev_alloc(h, *u.b, u.bytes)) != SRK_OK) return rc;
        if (u.bytes) HIPCHK(h, hipMemcpyAsync(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice, s));
    }
    const bool want_w = refine && w_out && O > 0, want_inl = inlier_out && O > 0;
    if ((rc = dev_alloc(h, l[srk_ba::LC_STRIP], (size_t)(8 * SRK_LOCATE_STRIP * O))) != SRK_OK || (rc = dev_alloc(h, l[srk_ba::LC_COUNT], (size_t)(8 * n))) != SRK_OK ||
        (rc = dev_alloc(h, l[srk_ba::LC_SLOTS], (size_t)(8 * SRK_LOCATE_SLOT * n * waves))) != SRK_OK ||
        (rc = dev_alloc(h, l[srk_ba::LC_LOCATED], (size_t)(48 * n))) != SRK_OK || (rc = dev_alloc(h, l[srk_ba::LC_LSTATUS], (size_t)(4 * n))) != SRK_OK ||
        (rc = dev_alloc(h, l[srk_ba::LC_INL], want_inl ? (size_t)O : 0)) != SRK_OK || (rc = dev_alloc(h, g[srk_ba::RS_R0], (size_t)(72 * n))) != SRK_OK ||
        (rc = dev_alloc(h, g[srk_ba::RS_T0], (size_t)(24 * n))) != SRK_OK)
        return rc;
    if (refine &&
        ((rc = dev_alloc(h, g[srk_ba::RS_PACK], (size_t)(8 * SRK_RESECT_PACK * n))) != SRK_OK || (rc = dev_alloc(h, g[srk_ba::RS_R], (size_t)(72 * n))) != SRK_OK ||
         (rc = dev_alloc(h, g[srk_ba::RS_T], (size_t)(24 * n))) != SRK_OK || (rc = dev_alloc(h, g[srk_ba::RS_QUAL], (size_t)(48 * n))) != SRK_OK ||
         (rc = dev_alloc(h, g[srk_ba::RS_INFO], (size_t)(288 * n))) != SRK_OK || (rc = dev_alloc(h, g[srk_ba::RS_STATUS], (size_t)(4 * n))) != SRK_OK ||
         (rc = dev_alloc(h, g[srk_ba::RS_W], want_w ? (size_t)(8 * O) : 0)) != SRK_OK))
        return rc;
    for (hipEvent_t& e : h->lc_ev)
        if (!e) HIPCHK(h, hipEventCreate(&e));
    const int64_t* d_row = P<int64_t>(g[srk_ba::RS_ROW]);
    const int32_t* d_point = P<int32_t>(g[srk_ba::RS_POINT]);
    const double* d_uv = P<double>(g[srk_ba::RS_UV]);
    const double* d_q = q ? P<double>(g[srk_ba::RS_Q]) : nullptr;
    const double* d_K = P<double>(g[srk_ba::RS_K]);
    double* d_R0 = P<double>(g[srk_ba::RS_R0]);
    double* d_T0 = P<double>(g[srk_ba::RS_T0]);
    HIPCHK(h, hipEventRecord(h->lc_ev[0], s));
    srk_launch_locate_gather(s, n_frames, d_row, d_point, d_uv, d_q, dX, P<double>(l[srk_ba::LC_STRIP]), P<int64_t>(l[srk_ba::LC_COUNT]));
    HIPCHK(h, hipEventRecord(h->lc_ev[1], s));
    srk_launch_locate_score(s, n_frames, lo.hypotheses, lo.seed, lo.inlier_pixels, f0, d_row, P<double>(l[srk_ba::LC_STRIP]),
                            P<int64_t>(l[srk_ba::LC_COUNT]), d_K, shared_k, P<double>(l[srk_ba::LC_SLOTS]));
    HIPCHK(h, hipEventRecord(h->lc_ev[2], s));
    srk_launch_locate_pick(s, n_frames, lo.hypotheses, lo.inlier_pixels, f0, d_row, d_point, d_uv, d_q, dX, d_K, shared_k, P<int64_t>(l[srk_ba::LC_COUNT]),
                           P<double>(l[srk_ba::LC_SLOTS]), d_R0, d_T0, P<double>(l[srk_ba::LC_LOCATED]), P<uint32_t>(l[srk_ba::LC_LSTATUS]),
                           want_inl ? P<uint8_t>(l[srk_ba::LC_INL]) : nullptr);
    if (refine) { // the located poses never leave the device: they are the starts of the resection's own kernels
        srk_launch_resect_pack(s, n_frames, d_R0, d_T0, d_K, shared_k, P<double>(g[srk_ba::RS_PACK]));
        srk_launch_resect_frames(s, n_frames, d_row, d_point, d_uv, d_q, dX, d_K, shared_k, d_R0, d_T0, P<double>(g[srk_ba::RS_PACK]), f0,
                                 refine->attempts, refine->rel_change, refine->loss_kind, refine->loss_delta_pixels, P<double>(g[srk_ba::RS_R]),
                                 P<double>(g[srk_ba::RS_T]), P<double>(g[srk_ba::RS_QUAL]), P<double>(g[srk_ba::RS_INFO]),
                                 P<uint32_t>(g[srk_ba::RS_STATUS]), want_w ? P<double>(g[srk_ba::RS_W]) : nullptr);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->lc_ev[3], s));
    HIPCHK(h, hipMemcpyAsync(R, refine ? g[srk_ba::RS_R].p : g[srk_ba::RS_R0].p, (size_t)(72 * n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(T, refine ? g[srk_ba::RS_T].p : g[srk_ba::RS_T0].p, (size_t)(24 * n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(located, l[srk_ba::LC_LOCATED].p, (size_t)(48 * n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(located_status, l[srk_ba::LC_LSTATUS].p, (size_t)(4 * n), hipMemcpyDeviceToHost, s));
    if (want_inl) HIPCHK(h, hipMemcpyAsync(inlier_out, l[srk_ba::LC_INL].p, (size_t)O, hipMemcpyDeviceToHost, s));
    if (refine) {
        HIPCHK(h, hipMemcpyAsync(quality, g[srk_ba::RS_QUAL].p, (size_t)(48 * n), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemcpyAsync(info, g[srk_ba::RS_INFO].p, (size_t)(288 * n), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemcpyAsync(status, g[srk_ba::RS_STATUS].p, (size_t)(4 * n), hipMemcpyDeviceToHost, s));
        if (want_w) HIPCHK(h, hipMemcpyAsync(w_out, g[srk_ba::RS_W].p, (size_t)(8 * O), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(h, hipStreamSynchronize(s));
    float ms = 0, score_ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->lc_ev[0], h->lc_ev[3]));
    HIPCHK(h, hipEventElapsedTime(&score_ms, h->lc_ev[1], h->lc_ev[2]));
    h->lc_ms = ms;
    h->lc_score_ms = score_ms;
    return SRK_OK;
}

extern "C" double srk_ba_locate_kernel_ms(const srk_ba* h) { return h ? h->lc_ms : 0.0; }
extern "C" double srk_ba_locate_score_ms(const srk_ba* h) { return h ? h->lc_score_ms : 0.0; }

static std::string locate_outputs_missing(int32_t n_frames, const srk_resect_options* refine, const double* R, const double* T, const double* located,
                                          const uint32_t* located_status, const double* quality, const double* info, const uint32_t* status)
{
    if (n_frames > 0 && (!R || !T || !located || !located_status)) return "locate: a NULL output array";
    if (n_frames > 0 && refine && (!quality || !info || !status)) return "locate: a NULL output array of the refinement";
    return std::string();
}

extern "C" int srk_locate_frames(srk_ba* h, double f0, int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv,
                                 const double* q, int64_t n_points, const double* X, const double* K, int shared_k, const srk_locate_options* opts,
                                 const srk_resect_options* refine, double* R, double* T, double* located, uint32_t* located_status,
                                 uint8_t* inlier_out, double* quality, double* info, uint32_t* status, double* w_out)
{
    if (!h) return SRK_E_ARGS;
    try {
        std::string why = srk_locate_check(n_frames, row_ptr, point, uv, q, n_points, X, K, shared_k, opts, refine);
        if (why.empty() && n_points > 0 && !X) why = "locate: the landmark array is NULL";
        if (why.empty() && (!std::isfinite(f0) || srk::is_close(0.0, f0))) why = "locate: f0 must be finite and not ~0";
        if (why.empty()) why = locate_outputs_missing(n_frames, refine, R, T, located, located_status, quality, info, status);
        if (!why.empty()) { h->last_error = why; return SRK_E_ARGS; }
        if (n_frames == 0) return SRK_OK;
        HIPCHK(h, hipSetDevice(h->device));
        DevBuf& gx = h->rs[srk_ba::RS_X];
        int rc;
        if ((rc = dev_alloc(h, gx, (size_t)(24 * n_points))) != SRK_OK) return rc;
        if (n_points > 0) HIPCHK(h, hipMemcpyAsync(gx.p, X, (size_t)(24 * n_points), hipMemcpyHostToDevice, h->main_stream));
        return locate_run(h, f0, n_frames, row_ptr, point, uv, q, P<double>(gx), K, shared_k ? 1 : 0, srk_locate_effective_options(opts), refine, R, T,
                          located, located_status, inlier_out, quality, info, status, w_out);
    } catch (const std::bad_alloc&) {
        h->last_error = "locate: out of host memory";
        return SRK_E_NOMEM;
    }
}

extern "C" int srk_ba_locate(srk_ba* h, int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv, const double* q,
                             const double* K, int shared_k, const srk_locate_options* opts, const srk_resect_options* refine,
                             int revert_normalization, double* R, double* T, double* located, uint32_t* located_status, uint8_t* inlier_out,
                             double* quality, double* info, uint32_t* status, double* w_out)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    try {
        std::string why;
        std::vector<int32_t> pt;
        if (h->world > 1 || h->allreduce || h->comm) why = "locate: more than one rank is not supported";
        else {
            std::vector<int64_t> pt_int((size_t)h->d.N); // the caller's landmark -> its place in the handle's landmark order
            for (int64_t i = 0; i < h->d.N; ++i) pt_int[(size_t)h->perm[(size_t)i]] = i;
            why = srk_locate_check(n_frames, row_ptr, point, uv, q, h->d.N, nullptr, K, shared_k, opts, refine, pt_int.data(), &pt);
        }
        if (why.empty()) why = locate_outputs_missing(n_frames, refine, R, T, located, located_status, quality, info, status);
        if (!why.empty()) { h->last_error = why; return SRK_E_ARGS; }
        if (n_frames == 0) return SRK_OK;
        HIPCHK(h, hipSetDevice(h->device));
        for (auto& a : h->att) // nothing of an earlier call is still writing the scene
            if (a.allocated && a.stream) HIPCHK(h, hipStreamSynchronize(a.stream));
        const int rc = locate_run(h, h->f0, n_frames, row_ptr, pt.data(), uv, q, P<double>(h->pts[h->cur]), K, shared_k ? 1 : 0,
                                  srk_locate_effective_options(opts), refine, R, T, located, located_status, inlier_out, quality, info, status, w_out);
        if (rc != SRK_OK) return rc;
        if (revert_normalization && h->normalized_on_upload) {
            srk_resect_revert_poses(h->nrm, n_frames, R, T, refine ? info : nullptr, refine ? quality : nullptr);
            if (!refine)
                for (int32_t i = 0; i < n_frames; ++i) // a frame that was not located keeps (I, 0) in every coordinate system
                    if (located_status[i]) {
                        for (int e = 0; e < 9; ++e) R[9 * (int64_t)i + e] = (e % 4 == 0) ? 1.0 : 0.0;
                        for (int e = 0; e < 3; ++e) T[3 * (int64_t)i + e] = 0.0;
                    }
        }
        return SRK_OK;
    } catch (const std::bad_alloc&) {
        h->last_error = "locate: out of host memory";
        return SRK_E_NOMEM;
    }
}

// ------------------------------------------------------------------ two-view relative pose
// the refinement of section 26, defined below: its kernels over pairs that are on the device, and the copies back
static int pair_device(srk_ba* h, double f0, int32_t n_pairs, int64_t O, const int64_t* d_row, const double* d_uva, const double* d_uvb, const double* d_q,
                       const double* d_ka, const double* d_kb, int shared_k, const double* d_R0, const double* d_T0, const uint32_t* d_related_status,
                       const uint8_t* d_inlier, const srk_pair_options& o, bool want_w);
static int pair_download(srk_ba* h, int32_t n_pairs, int64_t O, double* R, double* T, double* E, double* quality, double* info, double* basis,
                         uint32_t* status, double* w_out);
struct RelateRefine {
    const srk_pair_options* opts;
    double *R, *T, *E, *quality, *info, *basis, *w_out;
    uint32_t* status;
};
// The checked pairs of a call to the device, gather / solve / score / pick, the results back.  refine (srk_relate_frames_refined): the
// refinement follows on the same stream before anything is copied back, R, T and E are the refined ones (the three of this call
// are not used), and with inliers_only the inlier flags are formed on the device even when the caller does not ask for them.
static int relate_run(srk_ba* h, double f0, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                      const double* K_a, const double* K_b, int shared_k, const srk_relate_options& lo, double* R, double* T, double* E,
                      double* related, uint32_t* status, uint8_t* inlier_out, const RelateRefine* refine = nullptr)
{
    hipStream_t s = h->main_stream;
    const int64_t O = row_ptr[n_pairs], n = n_pairs;
    const int64_t waves = (lo.hypotheses + SRK_RELATE_LANES - 1) / SRK_RELATE_LANES;
    DevBuf* l = h->rl;
    int rc;
    struct { DevBuf* b; const void* src; size_t bytes; } up[] = {
        { &l[srk_ba::RL_ROW], row_ptr, (size_t)(8 * (n + 1)) }, { &l[srk_ba::RL_UVA], uv_a, (size_t)(16 * O) },
        { &l[srk_ba::RL_UVB], uv_b, (size_t)(16 * O) },         { &l[srk_ba::RL_Q], q, q ? (size_t)(8 * O) : 0 },
        { &l[srk_ba::RL_KA], K_a, (size_t)(72 * (shared_k ? 1 : n)) }, { &l[srk_ba::RL_KB], K_b, (size_t)(72 * (shared_k ? 1 : n)) },
    };
    for (auto& u : up) {
        if ((rc = dev_alloc(h, *u.b, u.bytes)) != SRK_OK) return rc;
        if (u.bytes) HIPCHK(h, hipMemcpyAsync(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice, s));
    }
    const bool keep_inl = refine && refine->opts->inliers_only && O > 0;
    const bool want_inl = (inlier_out && O > 0) || keep_inl;
    if ((rc = dev_alloc(h, l[srk_ba::RL_STRIP], (size_t)(8 * SRK_RELATE_STRIP * O))) != SRK_OK || (rc = dev_alloc(h, l[srk_ba::RL_COUNT], (size_t)(8 * n))) != SRK_OK ||
        (rc = dev_alloc(h, l[srk_ba::RL_HYP], (size_t)(8 * SRK_RELATE_HYP * n * lo.hypotheses))) != SRK_OK ||
        (rc = dev_alloc(h, l[srk_ba::RL_SLOTS], (size_t)(8 * SRK_RELATE_SLOT * n * waves))) != SRK_OK ||
        (rc = dev_alloc(h, l[srk_ba::RL_R], (size_t)(72 * n))) != SRK_OK || (rc = dev_alloc(h, l[srk_ba::RL_T], (size_t)(24 * n))) != SRK_OK ||
        (rc = dev_alloc(h, l[srk_ba::RL_E], (size_t)(72 * n))) != SRK_OK || (rc = dev_alloc(h, l[srk_ba::RL_RELATED], (size_t)(64 * n))) != SRK_OK ||
        (rc = dev_alloc(h, l[srk_ba::RL_STATUS], (size_t)(4 * n))) != SRK_OK || (rc = dev_alloc(h, l[srk_ba::RL_INL], want_inl ? (size_t)O : 0)) != SRK_OK)
        return rc;
    for (hipEvent_t& e : h->rl_ev)
        if (!e) HIPCHK(h, hipEventCreate(&e));
    const int64_t* d_row = P<int64_t>(l[srk_ba::RL_ROW]);
    const double* d_q = q ? P<double>(l[srk_ba::RL_Q]) : nullptr;
    const double* d_strip = P<double>(l[srk_ba::RL_STRIP]);
    const int64_t* d_count = P<int64_t>(l[srk_ba::RL_COUNT]);
    HIPCHK(h, hipEventRecord(h->rl_ev[0], s));
    srk_launch_relate_gather(s, n_pairs, d_row, P<double>(l[srk_ba::RL_UVA]), P<double>(l[srk_ba::RL_UVB]), d_q, P<double>(l[srk_ba::RL_STRIP]),
                             P<int64_t>(l[srk_ba::RL_COUNT]));
    srk_launch_relate_solve(s, n_pairs, lo.hypotheses, lo.seed, f0, d_row, d_strip, d_count, P<double>(l[srk_ba::RL_KA]), P<double>(l[srk_ba::RL_KB]),
                            shared_k, P<double>(l[srk_ba::RL_HYP]));
    HIPCHK(h, hipEventRecord(h->rl_ev[1], s));
    srk_launch_relate_score(s, n_pairs, lo.hypotheses, lo.inlier_pixels, f0, d_row, d_strip, d_count, P<double>(l[srk_ba::RL_HYP]),
                            P<double>(l[srk_ba::RL_SLOTS]));
    HIPCHK(h, hipEventRecord(h->rl_ev[2], s));
    srk_launch_relate_pick(s, n_pairs, lo.hypotheses, lo.inlier_pixels, f0, d_row, d_q, d_strip, d_count, P<double>(l[srk_ba::RL_KA]),
                           P<double>(l[srk_ba::RL_KB]), shared_k, P<double>(l[srk_ba::RL_HYP]), P<double>(l[srk_ba::RL_SLOTS]), P<double>(l[srk_ba::RL_R]),
                           P<double>(l[srk_ba::RL_T]), P<double>(l[srk_ba::RL_E]), P<double>(l[srk_ba::RL_RELATED]), P<uint32_t>(l[srk_ba::RL_STATUS]),
                           want_inl ? P<uint8_t>(l[srk_ba::RL_INL]) : nullptr);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->rl_ev[3], s));
    if (refine) { // the related poses never leave the device: they are the starts of the refinement
        if ((rc = pair_device(h, f0, n_pairs, O, d_row, P<double>(l[srk_ba::RL_UVA]), P<double>(l[srk_ba::RL_UVB]), d_q, P<double>(l[srk_ba::RL_KA]),
                              P<double>(l[srk_ba::RL_KB]), shared_k, P<double>(l[srk_ba::RL_R]), P<double>(l[srk_ba::RL_T]),
                              P<uint32_t>(l[srk_ba::RL_STATUS]), keep_inl ? P<uint8_t>(l[srk_ba::RL_INL]) : nullptr, *refine->opts,
                              refine->w_out != nullptr)) != SRK_OK)
            return rc;
    } else {
        HIPCHK(h, hipMemcpyAsync(R, l[srk_ba::RL_R].p, (size_t)(72 * n), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemcpyAsync(T, l[srk_ba::RL_T].p, (size_t)(24 * n), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemcpyAsync(E, l[srk_ba::RL_E].p, (size_t)(72 * n), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(h, hipMemcpyAsync(related, l[srk_ba::RL_RELATED].p, (size_t)(64 * n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(status, l[srk_ba::RL_STATUS].p, (size_t)(4 * n), hipMemcpyDeviceToHost, s));
    if (inlier_out && O > 0) HIPCHK(h, hipMemcpyAsync(inlier_out, l[srk_ba::RL_INL].p, (size_t)O, hipMemcpyDeviceToHost, s));
    if (refine) { // copies, the synchronisation and the refinement's own time
        if ((rc = pair_download(h, n_pairs, O, refine->R, refine->T, refine->E, refine->quality, refine->info, refine->basis, refine->status,
                                refine->w_out)) != SRK_OK)
            return rc;
    } else
        HIPCHK(h, hipStreamSynchronize(s));
    float ms = 0, score_ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->rl_ev[0], h->rl_ev[3]));
    HIPCHK(h, hipEventElapsedTime(&score_ms, h->rl_ev[1], h->rl_ev[2]));
    h->rl_ms = ms;
    h->rl_score_ms = score_ms;
    return SRK_OK;
}

extern "C" double srk_ba_relate_kernel_ms(const srk_ba* h) { return h ? h->rl_ms : 0.0; }
extern "C" double srk_ba_relate_score_ms(const srk_ba* h) { return h ? h->rl_score_ms : 0.0; }

extern "C" int srk_relate_frames(srk_ba* h, double f0, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                                 const double* K_a, const double* K_b, int shared_k, const srk_relate_options* opts, double* R, double* T, double* E,
                                 double* related, uint32_t* status, uint8_t* inlier_out)
{
    if (!h) return SRK_E_ARGS;
    try {
        std::string why = srk_relate_check(n_pairs, row_ptr, uv_a, uv_b, q, K_a, K_b, shared_k, opts);
        if (why.empty() && (!std::isfinite(f0) || srk::is_close(0.0, f0))) why = "relate: f0 must be finite and not ~0";
        if (why.empty() && n_pairs > 0 && (!R || !T || !E || !related || !status)) why = "relate: a NULL output array";
        if (!why.empty()) { h->last_error = why; return SRK_E_ARGS; }
        if (n_pairs == 0) return SRK_OK;
        HIPCHK(h, hipSetDevice(h->device));
        return relate_run(h, f0, n_pairs, row_ptr, uv_a, uv_b, q, K_a, K_b, shared_k ? 1 : 0, srk_relate_effective_options(opts), R, T, E, related, status,
                          inlier_out);
    } catch (const std::bad_alloc&) {
        h->last_error = "relate: out of host memory";
        return SRK_E_NOMEM;
    }
}

// ------------------------------------------------------------------ two-view pose refinement
// The refinement's kernels over pairs that are on the device already (every pointer a device pointer): the inverses of K, with
// d_inlier the product q * inlier, then one wave a pair.  Nothing is copied back and nothing is waited for.
static int pair_device(srk_ba* h, double f0, int32_t n_pairs, int64_t O, const int64_t* d_row, const double* d_uva, const double* d_uvb, const double* d_q,
                       const double* d_ka, const double* d_kb, int shared_k, const double* d_R0, const double* d_T0, const uint32_t* d_related_status,
                       const uint8_t* d_inlier, const srk_pair_options& o, bool want_w)
{
    hipStream_t s = h->main_stream;
    const int64_t n = n_pairs;
    DevBuf* g = h->pr;
    int rc;
    if ((rc = dev_alloc(h, g[srk_ba::PR_KINV], (size_t)(8 * SRK_PAIR_KINV * n))) != SRK_OK || (rc = dev_alloc(h, g[srk_ba::PR_QE], d_inlier ? (size_t)(8 * O) : 0)) != SRK_OK ||
        (rc = dev_alloc(h, g[srk_ba::PR_R], (size_t)(72 * n))) != SRK_OK || (rc = dev_alloc(h, g[srk_ba::PR_T], (size_t)(24 * n))) != SRK_OK ||
        (rc = dev_alloc(h, g[srk_ba::PR_E], (size_t)(72 * n))) != SRK_OK || (rc = dev_alloc(h, g[srk_ba::PR_QUAL], (size_t)(48 * n))) != SRK_OK ||
        (rc = dev_alloc(h, g[srk_ba::PR_INFO], (size_t)(200 * n))) != SRK_OK || (rc = dev_alloc(h, g[srk_ba::PR_BASIS], (size_t)(48 * n))) != SRK_OK ||
        (rc = dev_alloc(h, g[srk_ba::PR_STATUS], (size_t)(4 * n))) != SRK_OK || (rc = dev_alloc(h, g[srk_ba::PR_W], want_w && O > 0 ? (size_t)(8 * O) : 0)) != SRK_OK)
        return rc;
    for (hipEvent_t& e : h->pr_ev)
        if (!e) HIPCHK(h, hipEventCreate(&e));
    HIPCHK(h, hipEventRecord(h->pr_ev[0], s));
    srk_launch_pair_pack(s, n_pairs, d_ka, d_kb, shared_k, P<double>(g[srk_ba::PR_KINV]));
    if (d_inlier) {
        srk_launch_pair_mask(s, O, d_q, d_inlier, P<double>(g[srk_ba::PR_QE]));
        d_q = P<double>(g[srk_ba::PR_QE]);
    }
    srk_launch_pair_refine(s, n_pairs, d_row, d_uva, d_uvb, d_q, P<double>(g[srk_ba::PR_KINV]), d_R0, d_T0, d_related_status, f0, o.attempts, o.rel_change,
                           o.loss_kind, o.loss_delta_pixels, P<double>(g[srk_ba::PR_R]), P<double>(g[srk_ba::PR_T]), P<double>(g[srk_ba::PR_E]),
                           P<double>(g[srk_ba::PR_QUAL]), P<double>(g[srk_ba::PR_INFO]), P<double>(g[srk_ba::PR_BASIS]), P<uint32_t>(g[srk_ba::PR_STATUS]),
                           want_w && O > 0 ? P<double>(g[srk_ba::PR_W]) : nullptr);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->pr_ev[1], s));
    return SRK_OK;
}

// the results of pair_device back, the synchronisation and the kernels' time
static int pair_download(srk_ba* h, int32_t n_pairs, int64_t O, double* R, double* T, double* E, double* quality, double* info, double* basis,
                         uint32_t* status, double* w_out)
{
    hipStream_t s = h->main_stream;
    const int64_t n = n_pairs;
    DevBuf* g = h->pr;
    HIPCHK(h, hipMemcpyAsync(R, g[srk_ba::PR_R].p, (size_t)(72 * n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(T, g[srk_ba::PR_T].p, (size_t)(24 * n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(E, g[srk_ba::PR_E].p, (size_t)(72 * n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(quality, g[srk_ba::PR_QUAL].p, (size_t)(48 * n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(info, g[srk_ba::PR_INFO].p, (size_t)(200 * n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(basis, g[srk_ba::PR_BASIS].p, (size_t)(48 * n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(status, g[srk_ba::PR_STATUS].p, (size_t)(4 * n), hipMemcpyDeviceToHost, s));
    if (w_out && O > 0) HIPCHK(h, hipMemcpyAsync(w_out, g[srk_ba::PR_W].p, (size_t)(8 * O), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->pr_ev[0], h->pr_ev[1]));
    h->pr_ms = ms;
    return SRK_OK;
}

extern "C" double srk_ba_pair_kernel_ms(const srk_ba* h) { return h ? h->pr_ms : 0.0; }

extern "C" int srk_refine_pairs(srk_ba* h, double f0, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                                const double* K_a, const double* K_b, int shared_k, const double* R0, const double* T0, const srk_pair_options* opts,
                                double* R, double* T, double* E, double* quality, double* info, double* basis, uint32_t* status, double* w_out)
{
    if (!h) return SRK_E_ARGS;
    try {
        std::string why = srk_pair_check(n_pairs, row_ptr, uv_a, uv_b, q, K_a, K_b, shared_k, R0, T0, opts);
        if (why.empty() && (!std::isfinite(f0) || srk::is_close(0.0, f0))) why = "pair: f0 must be finite and not ~0";
        if (why.empty() && n_pairs > 0 && (!R || !T || !E || !quality || !info || !basis || !status)) why = "pair: a NULL output array";
        if (!why.empty()) { h->last_error = why; return SRK_E_ARGS; }
        if (n_pairs == 0) return SRK_OK;
        HIPCHK(h, hipSetDevice(h->device));
        hipStream_t s = h->main_stream;
        const int64_t O = row_ptr[n_pairs], n = n_pairs;
        const int sk = shared_k ? 1 : 0;
        DevBuf* g = h->pr;
        int rc;
        struct { DevBuf* b; const void* src; size_t bytes; } up[] = {
            { &g[srk_ba::PR_ROW], row_ptr, (size_t)(8 * (n + 1)) }, { &g[srk_ba::PR_UVA], uv_a, (size_t)(16 * O) },
            { &g[srk_ba::PR_UVB], uv_b, (size_t)(16 * O) },         { &g[srk_ba::PR_Q], q, q ? (size_t)(8 * O) : 0 },
            { &g[srk_ba::PR_KA], K_a, (size_t)(72 * (sk ? 1 : n)) }, { &g[srk_ba::PR_KB], K_b, (size_t)(72 * (sk ? 1 : n)) },
            { &g[srk_ba::PR_R0], R0, (size_t)(72 * n) },            { &g[srk_ba::PR_T0], T0, (size_t)(24 * n) },
        };
        for (auto& u : up) {
            if ((rc = dev_alloc(h, *u.b, u.bytes)) != SRK_OK) return rc;
            if (u.bytes) HIPCHK(h, hipMemcpyAsync(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice, s));
        }
        if ((rc = pair_device(h, f0, n_pairs, O, P<int64_t>(g[srk_ba::PR_ROW]), P<double>(g[srk_ba::PR_UVA]), P<double>(g[srk_ba::PR_UVB]),
                              q ? P<double>(g[srk_ba::PR_Q]) : nullptr, P<double>(g[srk_ba::PR_KA]), P<double>(g[srk_ba::PR_KB]), sk,
                              P<double>(g[srk_ba::PR_R0]), P<double>(g[srk_ba::PR_T0]), nullptr, nullptr, srk_pair_effective_options(opts),
                              w_out != nullptr)) != SRK_OK)
            return rc;
        return pair_download(h, n_pairs, O, R, T, E, quality, info, basis, status, w_out);
    } catch (const std::bad_alloc&) {
        h->last_error = "pair: out of host memory";
        return SRK_E_NOMEM;
    }
}

extern "C" int srk_relate_frames_refined(srk_ba* h, double f0, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b,
                                         const double* q, const double* K_a, const double* K_b, int shared_k, const srk_relate_options* opts,
                                         const srk_pair_options* refine, double* R, double* T, double* E, double* related, uint32_t* related_status,
                                         uint8_t* inlier_out, double* quality, double* info, double* basis, uint32_t* status, double* w_out)
{
    if (!h) return SRK_E_ARGS;
    try {
        std::string why = srk_relate_check(n_pairs, row_ptr, uv_a, uv_b, q, K_a, K_b, shared_k, opts);
        if (why.empty() && !refine) why = "pair: the refinement's options are NULL (srk_relate_frames is the call without)";
        if (why.empty()) why = srk_pair_check_options(refine, true);
        if (why.empty() && n_pairs > SRK_PAIR_MAX_PAIRS_HOST) why = "pair: too many pairs in one call";
        if (why.empty() && (!std::isfinite(f0) || srk::is_close(0.0, f0))) why = "relate: f0 must be finite and not ~0";
        if (why.empty() && n_pairs > 0 && (!R || !T || !E || !related || !related_status || !quality || !info || !basis || !status))
            why = "pair: a NULL output array";
        if (!why.empty()) { h->last_error = why; return SRK_E_ARGS; }
        if (n_pairs == 0) return SRK_OK;
        HIPCHK(h, hipSetDevice(h->device));
        const RelateRefine rf = { refine, R, T, E, quality, info, basis, w_out, status };
        return relate_run(h, f0, n_pairs, row_ptr, uv_a, uv_b, q, K_a, K_b, shared_k ? 1 : 0, srk_relate_effective_options(opts), nullptr, nullptr, nullptr,
                          related, related_status, inlier_out, &rf);
    } catch (const std::bad_alloc&) {
        h->last_error = "pair: out of host memory";
        return SRK_E_NOMEM;
    }
}

// ------------------------------------------------------------------ map alignment
// The checked sets of a call to the device, gather / hypotheses and scores / pick with its rounds, the results back.  The sources
// are a (host, [O][3]) or, with point != NULL, the landmarks dX (a device pointer) as point numbers them.
static int align_run(srk_ba* h, int32_t n_sets, const int64_t* row_ptr, const int32_t* point, const double* a, const double* dX, const double* b,
                     const double* q, const srk_align_options& lo, double* sc, double* R, double* t, double* aligned, uint32_t* status,
                     uint8_t* inlier_out)
{
    hipStream_t s = h->main_stream;
    const int64_t O = row_ptr[n_sets], n = n_sets;
    const int64_t waves = (lo.hypotheses + SRK_ALIGN_LANES - 1) / SRK_ALIGN_LANES;
    DevBuf* l = h->al;
    int rc;
    struct { DevBuf* b; const void* src; size_t bytes; } up[] = {
        { &l[srk_ba::AL_ROW], row_ptr, (size_t)(8 * (n + 1)) }, { &l[srk_ba::AL_POINT], point, point ? (size_t)(4 * O) : 0 },
        { &l[srk_ba::AL_A], a, point ? 0 : (size_t)(24 * O) },  { &l[srk_ba::AL_B], b, (size_t)(24 * O) },
        { &l[srk_ba::AL_Q], q, q ? (size_t)(8 * O) : 0 },
    };
    for (auto& u : up) {
        if ((rc = dev_alloc(h, *u.b, u.bytes)) != SRK_OK) return rc;
        if (u.bytes) HIPCHK(h, hipMemcpyAsync(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice, s));
    }
    const bool want_inl = inlier_out && O > 0;
    if ((rc = dev_alloc(h, l[srk_ba::AL_STRIP], (size_t)(8 * SRK_ALIGN_STRIP * O))) != SRK_OK || (rc = dev_alloc(h, l[srk_ba::AL_COUNT], (size_t)(8 * n))) != SRK_OK ||
        (rc = dev_alloc(h, l[srk_ba::AL_SLOTS], (size_t)(8 * SRK_ALIGN_SLOT * n * waves))) != SRK_OK || (rc = dev_alloc(h, l[srk_ba::AL_S], (size_t)(8 * n))) != SRK_OK ||
        (rc = dev_alloc(h, l[srk_ba::AL_R], (size_t)(72 * n))) != SRK_OK || (rc = dev_alloc(h, l[srk_ba::AL_T], (size_t)(24 * n))) != SRK_OK ||
        (rc = dev_alloc(h, l[srk_ba::AL_ALIGNED], (size_t)(64 * n))) != SRK_OK || (rc = dev_alloc(h, l[srk_ba::AL_STATUS], (size_t)(4 * n))) != SRK_OK ||
        (rc = dev_alloc(h, l[srk_ba::AL_INL], want_inl ? (size_t)O : 0)) != SRK_OK)
        return rc;
    for (hipEvent_t& e : h->al_ev)
        if (!e) HIPCHK(h, hipEventCreate(&e));
    const int64_t* d_row = P<int64_t>(l[srk_ba::AL_ROW]);
    const int32_t* d_point = point ? P<int32_t>(l[srk_ba::AL_POINT]) : nullptr;
    const double* d_a = point ? dX : P<double>(l[srk_ba::AL_A]);
    const double* d_b = P<double>(l[srk_ba::AL_B]);
    const double* d_q = q ? P<double>(l[srk_ba::AL_Q]) : nullptr;
    const double* d_strip = P<double>(l[srk_ba::AL_STRIP]);
    const int64_t* d_count = P<int64_t>(l[srk_ba::AL_COUNT]);
    HIPCHK(h, hipEventRecord(h->al_ev[0], s));
    srk_launch_align_gather(s, n_sets, d_row, d_point, d_a, d_b, d_q, P<double>(l[srk_ba::AL_STRIP]), P<int64_t>(l[srk_ba::AL_COUNT]));
    HIPCHK(h, hipEventRecord(h->al_ev[1], s));
    srk_launch_align_score(s, n_sets, lo.hypotheses, lo.seed, lo.inlier_distance, lo.with_scale, d_row, d_strip, d_count, P<double>(l[srk_ba::AL_SLOTS]));
    HIPCHK(h, hipEventRecord(h->al_ev[2], s));
    srk_launch_align_pick(s, n_sets, lo.hypotheses, lo.inlier_distance, lo.with_scale, lo.refine_rounds, d_row, d_point, d_a, d_b, d_q, d_strip, d_count,
                          P<double>(l[srk_ba::AL_SLOTS]), P<double>(l[srk_ba::AL_S]), P<double>(l[srk_ba::AL_R]), P<double>(l[srk_ba::AL_T]),
                          P<double>(l[srk_ba::AL_ALIGNED]), P<uint32_t>(l[srk_ba::AL_STATUS]), want_inl ? P<uint8_t>(l[srk_ba::AL_INL]) : nullptr);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->al_ev[3], s));
    HIPCHK(h, hipMemcpyAsync(sc, l[srk_ba::AL_S].p, (size_t)(8 * n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(R, l[srk_ba::AL_R].p, (size_t)(72 * n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(t, l[srk_ba::AL_T].p, (size_t)(24 * n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(aligned, l[srk_ba::AL_ALIGNED].p, (size_t)(64 * n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(status, l[srk_ba::AL_STATUS].p, (size_t)(4 * n), hipMemcpyDeviceToHost, s));
    if (want_inl) HIPCHK(h, hipMemcpyAsync(inlier_out, l[srk_ba::AL_INL].p, (size_t)O, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    float ms = 0, score_ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->al_ev[0], h->al_ev[3]));
    HIPCHK(h, hipEventElapsedTime(&score_ms, h->al_ev[1], h->al_ev[2]));
    h->al_ms = ms;
    h->al_score_ms = score_ms;
    return SRK_OK;
}

extern "C" double srk_ba_align_kernel_ms(const srk_ba* h) { return h ? h->al_ms : 0.0; }
extern "C" double srk_ba_align_score_ms(const srk_ba* h) { return h ? h->al_score_ms : 0.0; }

extern "C" int srk_align_points(srk_ba* h, int32_t n_sets, const int64_t* row_ptr, const double* a, const double* b, const double* q,
                                const srk_align_options* opts, double* s, double* R, double* t, double* aligned, uint32_t* status, uint8_t* inlier_out)
{
    if (!h) return SRK_E_ARGS;
    try {
        std::string why = srk_align_check(n_sets, row_ptr, nullptr, 0, a, b, q, opts);
        if (why.empty() && n_sets > 0 && (!s || !R || !t || !aligned || !status)) why = "align: a NULL output array";
        if (!why.empty()) { h->last_error = why; return SRK_E_ARGS; }
        if (n_sets == 0) return SRK_OK;
        HIPCHK(h, hipSetDevice(h->device));
        return align_run(h, n_sets, row_ptr, nullptr, a, nullptr, b, q, srk_align_effective_options(opts), s, R, t, aligned, status, inlier_out);
    } catch (const std::bad_alloc&) {
        h->last_error = "align: out of host memory";
        return SRK_E_NOMEM;
    }
}

extern "C" int srk_ba_align(srk_ba* h, int32_t n_sets, const int64_t* row_ptr, const int32_t* point, const double* target, const double* q,
                            const srk_align_options* opts, int revert_normalization, double* s, double* R, double* t, double* aligned,
                            uint32_t* status, uint8_t* inlier_out)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    try {
        std::string why;
        std::vector<int32_t> pt;
        if (h->world > 1 || h->allreduce || h->comm) why = "align: more than one rank is not supported";
        else if (n_sets >= 0 && row_ptr && row_ptr[n_sets] > 0 && !point) why = "align: a NULL correspondence array";
        else {
            std::vector<int64_t> pt_int((size_t)h->d.N); // the caller's landmark -> its place in the handle's landmark order
            for (int64_t i = 0; i < h->d.N; ++i) pt_int[(size_t)h->perm[(size_t)i]] = i;
            static const int32_t none = 0; // an empty call still takes the map's branch of the checks
            why = srk_align_check(n_sets, row_ptr, point ? point : &none, h->d.N, nullptr, target, q, opts, pt_int.data(), &pt);
        }
        if (why.empty() && n_sets > 0 && (!s || !R || !t || !aligned || !status)) why = "align: a NULL output array";
        if (!why.empty()) { h->last_error = why; return SRK_E_ARGS; }
        if (n_sets == 0) return SRK_OK;
        HIPCHK(h, hipSetDevice(h->device));
        for (auto& a : h->att) // nothing of an earlier call is still writing the scene
            if (a.allocated && a.stream) HIPCHK(h, hipStreamSynchronize(a.stream));
        pt.push_back(0); // never read: keeps data() valid without correspondences
        const int rc = align_run(h, n_sets, row_ptr, pt.data(), nullptr, P<double>(h->pts[h->cur]), target, q, srk_align_effective_options(opts), s, R, t,
                                 aligned, status, inlier_out);
        if (rc != SRK_OK) return rc;
        if (revert_normalization && h->normalized_on_upload)
            for (int32_t i = 0; i < n_sets; ++i) // a set that was not aligned keeps (1, I, 0) in every coordinate system
                if (!status[i]) srk_align_revert(h->nrm, 1, s + i, R + 9 * (int64_t)i, t + 3 * (int64_t)i);
        return SRK_OK;
    } catch (const std::bad_alloc&) {
        h->last_error = "align: out of host memory";
        return SRK_E_NOMEM;
    }
}

// ------------------------------------------------------------------ two-view homography
// The checked pairs of a call to the device, gather / hypotheses and scores / pick with its rounds and the decomposition, the
// results back.
static int homog_run(srk_ba* h, double f0, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                     const double* K_a, const double* K_b, int shared_k, const srk_homography_options& lo, double* G, double* H, int32_t* n_poses,
                     double* R, double* T, double* N, int32_t* front, double* homog, uint32_t* status, uint8_t* inlier_out)
{
    hipStream_t s = h->main_stream;
    const int64_t O = row_ptr[n_pairs], n = n_pairs;
    const int64_t waves = (lo.hypotheses + SRK_HOMOG_LANES - 1) / SRK_HOMOG_LANES;
    DevBuf* l = h->hg;
    int rc;
    struct { DevBuf* b; const void* src; size_t bytes; } up[] = {
        { &l[srk_ba::HG_ROW], row_ptr, (size_t)(8 * (n + 1)) }, { &l[srk_ba::HG_UVA], uv_a, (size_t)(16 * O) },
        { &l[srk_ba::HG_UVB], uv_b, (size_t)(16 * O) },         { &l[srk_ba::HG_Q], q, q ? (size_t)(8 * O) : 0 },
        { &l[srk_ba::HG_KA], K_a, (size_t)(72 * (shared_k ? 1 : n)) }, { &l[srk_ba::HG_KB], K_b, (size_t)(72 * (shared_k ? 1 : n)) },
    };
    for (auto& u : up) {
        if ((rc = dev_alloc(h, *u.b, u.bytes)) != SRK_OK) return rc;
        if (u.bytes) HIPCHK(h, hipMemcpyAsync(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice, s));
    }
    const bool want_inl = inlier_out && O > 0;
    struct { int buf; size_t bytes; void* dst; } outs[] = {
        { srk_ba::HG_G, (size_t)(72 * n), G },       { srk_ba::HG_H, (size_t)(72 * n), H },         { srk_ba::HG_POSES, (size_t)(4 * n), n_poses },
        { srk_ba::HG_R, (size_t)(144 * n), R },      { srk_ba::HG_T, (size_t)(48 * n), T },         { srk_ba::HG_N, (size_t)(48 * n), N },
        { srk_ba::HG_FRONT, (size_t)(8 * n), front }, { srk_ba::HG_HOMOG, (size_t)(64 * n), homog }, { srk_ba::HG_STATUS, (size_t)(4 * n), status },
        { srk_ba::HG_INL, want_inl ? (size_t)O : 0, inlier_out },
    };
    if ((rc = dev_alloc(h, l[srk_ba::HG_STRIP], (size_t)(8 * SRK_HOMOG_STRIP * O))) != SRK_OK || (rc = dev_alloc(h, l[srk_ba::HG_COUNT], (size_t)(8 * n))) != SRK_OK ||
        (rc = dev_alloc(h, l[srk_ba::HG_SLOTS], (size_t)(8 * SRK_HOMOG_SLOT * n * waves))) != SRK_OK)
        return rc;
    for (auto& o : outs)
        if ((rc = dev_alloc(h, l[o.buf], o.bytes)) != SRK_OK) return rc;
    for (hipEvent_t& e : h->hg_ev)
        if (!e) HIPCHK(h, hipEventCreate(&e));
    const int64_t* d_row = P<int64_t>(l[srk_ba::HG_ROW]);
    const double* d_uva = P<double>(l[srk_ba::HG_UVA]);
    const double* d_uvb = P<double>(l[srk_ba::HG_UVB]);
    const double* d_q = q ? P<double>(l[srk_ba::HG_Q]) : nullptr;
    const double* d_strip = P<double>(l[srk_ba::HG_STRIP]);
    const int64_t* d_count = P<int64_t>(l[srk_ba::HG_COUNT]);
    HIPCHK(h, hipEventRecord(h->hg_ev[0], s));
    srk_launch_homog_gather(s, n_pairs, d_row, d_uva, d_uvb, d_q, P<double>(l[srk_ba::HG_STRIP]), P<int64_t>(l[srk_ba::HG_COUNT]));
    HIPCHK(h, hipEventRecord(h->hg_ev[1], s));
    srk_launch_homog_score(s, n_pairs, lo.hypotheses, lo.seed, lo.inlier_pixels, f0, d_row, d_strip, d_count, P<double>(l[srk_ba::HG_SLOTS]));
    HIPCHK(h, hipEventRecord(h->hg_ev[2], s));
    srk_launch_homog_pick(s, n_pairs, lo.hypotheses, lo.inlier_pixels, f0, lo.refine_rounds, d_row, d_uva, d_uvb, d_q, d_strip, d_count,
                          P<double>(l[srk_ba::HG_KA]), P<double>(l[srk_ba::HG_KB]), shared_k, P<double>(l[srk_ba::HG_SLOTS]), P<double>(l[srk_ba::HG_G]),
                          P<double>(l[srk_ba::HG_H]), P<int32_t>(l[srk_ba::HG_POSES]), P<double>(l[srk_ba::HG_R]), P<double>(l[srk_ba::HG_T]),
                          P<double>(l[srk_ba::HG_N]), P<int32_t>(l[srk_ba::HG_FRONT]), P<double>(l[srk_ba::HG_HOMOG]), P<uint32_t>(l[srk_ba::HG_STATUS]),
                          want_inl ? P<uint8_t>(l[srk_ba::HG_INL]) : nullptr);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->hg_ev[3], s));
    for (auto& o : outs)
        if (o.bytes) HIPCHK(h, hipMemcpyAsync(o.dst, l[o.buf].p, o.bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    float ms = 0, score_ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->hg_ev[0], h->hg_ev[3]));
    HIPCHK(h, hipEventElapsedTime(&score_ms, h->hg_ev[1], h->hg_ev[2]));
    h->hg_ms = ms;
    h->hg_score_ms = score_ms;
    return SRK_OK;
}

extern "C" double srk_ba_homography_kernel_ms(const srk_ba* h) { return h ? h->hg_ms : 0.0; }
extern "C" double srk_ba_homography_score_ms(const srk_ba* h) { return h ? h->hg_score_ms : 0.0; }

extern "C" int srk_relate_homography(srk_ba* h, double f0, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                                     const double* K_a, const double* K_b, int shared_k, const srk_homography_options* opts, double* G, double* H,
                                     int32_t* n_poses, double* R, double* T, double* N, int32_t* front, double* homog, uint32_t* status,
                                     uint8_t* inlier_out)
{
    if (!h) return SRK_E_ARGS;
    try {
        std::string why = srk_homog_check(n_pairs, row_ptr, uv_a, uv_b, q, K_a, K_b, shared_k, opts);
        if (why.empty() && (!std::isfinite(f0) || srk::is_close(0.0, f0))) why = "homography: f0 must be finite and not ~0";
        if (why.empty() && n_pairs > 0 && (!G || !H || !n_poses || !R || !T || !N || !front || !homog || !status)) why = "homography: a NULL output array";
        if (!why.empty()) { h->last_error = why; return SRK_E_ARGS; }
        if (n_pairs == 0) return SRK_OK;
        HIPCHK(h, hipSetDevice(h->device));
        return homog_run(h, f0, n_pairs, row_ptr, uv_a, uv_b, q, K_a, K_b, shared_k ? 1 : 0, srk_homog_effective_options(opts), G, H, n_poses, R, T, N,
                         front, homog, status, inlier_out);
    } catch (const std::bad_alloc&) {
        h->last_error = "homography: out of host memory";
        return SRK_E_NOMEM;
    }
}

// ------------------------------------------------------------------ two-view fundamental matrix
// The checked pairs of a call to the device, gather / solve / score / pick with its attempts, the results back.
static int fund_run(srk_ba* h, double f0, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                    const srk_fundamental_options& lo, double* F, double* U, double* V, double* sigma, double* fund, double* info, uint32_t* status,
                    uint8_t* inlier_out)
{
    hipStream_t s = h->main_stream;
    const int64_t O = row_ptr[n_pairs], n = n_pairs;
    const int64_t waves = (lo.hypotheses + SRK_FUND_LANES - 1) / SRK_FUND_LANES;
    DevBuf* l = h->fd;
    int rc;
    struct { DevBuf* b; const void* src; size_t bytes; } up[] = {
        { &l[srk_ba::FD_ROW], row_ptr, (size_t)(8 * (n + 1)) }, { &l[srk_ba::FD_UVA], uv_a, (size_t)(16 * O) },
        { &l[srk_ba::FD_UVB], uv_b, (size_t)(16 * O) },         { &l[srk_ba::FD_Q], q, q ? (size_t)(8 * O) : 0 },
    };
    for (auto& u : up) {
        if ((rc = dev_alloc(h, *u.b, u.bytes)) != SRK_OK) return rc;
        if (u.bytes) HIPCHK(h, hipMemcpyAsync(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice, s));
    }
    const bool want_inl = inlier_out && O > 0;
    struct { int buf; size_t bytes; void* dst; } outs[] = {
        { srk_ba::FD_F, (size_t)(72 * n), F },        { srk_ba::FD_U, (size_t)(72 * n), U },        { srk_ba::FD_V, (size_t)(72 * n), V },
        { srk_ba::FD_SIGMA, (size_t)(8 * n), sigma }, { srk_ba::FD_FUND, (size_t)(96 * n), fund },  { srk_ba::FD_INFO, (size_t)(392 * n), info },
        { srk_ba::FD_STATUS, (size_t)(4 * n), status }, { srk_ba::FD_INL, want_inl ? (size_t)O : 0, inlier_out },
    };
    if ((rc = dev_alloc(h, l[srk_ba::FD_STRIP], (size_t)(8 * SRK_FUND_STRIP * O))) != SRK_OK || (rc = dev_alloc(h, l[srk_ba::FD_COUNT], (size_t)(8 * n))) != SRK_OK ||
        (rc = dev_alloc(h, l[srk_ba::FD_HYP], (size_t)(8 * SRK_FUND_HYP * n * lo.hypotheses))) != SRK_OK ||
        (rc = dev_alloc(h, l[srk_ba::FD_SLOTS], (size_t)(8 * SRK_FUND_SLOT * n * waves))) != SRK_OK)
        return rc;
    for (auto& o : outs)
        if ((rc = dev_alloc(h, l[o.buf], o.bytes)) != SRK_OK) return rc;
    for (hipEvent_t& e : h->fd_ev)
        if (!e) HIPCHK(h, hipEventCreate(&e));
    const int64_t* d_row = P<int64_t>(l[srk_ba::FD_ROW]);
    const double* d_uva = P<double>(l[srk_ba::FD_UVA]);
    const double* d_uvb = P<double>(l[srk_ba::FD_UVB]);
    const double* d_q = q ? P<double>(l[srk_ba::FD_Q]) : nullptr;
    const double* d_strip = P<double>(l[srk_ba::FD_STRIP]);
    const int64_t* d_count = P<int64_t>(l[srk_ba::FD_COUNT]);
    HIPCHK(h, hipEventRecord(h->fd_ev[0], s));
    srk_launch_fund_gather(s, n_pairs, d_row, d_uva, d_uvb, d_q, P<double>(l[srk_ba::FD_STRIP]), P<int64_t>(l[srk_ba::FD_COUNT]));
    HIPCHK(h, hipEventRecord(h->fd_ev[4], s));
    srk_launch_fund_solve(s, n_pairs, lo.hypotheses, lo.seed, f0, d_row, d_strip, d_count, P<double>(l[srk_ba::FD_HYP]));
    HIPCHK(h, hipEventRecord(h->fd_ev[1], s));
    srk_launch_fund_score(s, n_pairs, lo.hypotheses, lo.inlier_pixels, f0, d_row, d_strip, d_count, P<double>(l[srk_ba::FD_HYP]), P<double>(l[srk_ba::FD_SLOTS]));
    HIPCHK(h, hipEventRecord(h->fd_ev[2], s));
    srk_launch_fund_pick(s, n_pairs, lo.hypotheses, lo.inlier_pixels, f0, lo.refine_rounds, d_row, d_uva, d_uvb, d_q, d_strip, d_count,
                         P<double>(l[srk_ba::FD_HYP]), P<double>(l[srk_ba::FD_SLOTS]), P<double>(l[srk_ba::FD_F]), P<double>(l[srk_ba::FD_U]),
                         P<double>(l[srk_ba::FD_V]), P<double>(l[srk_ba::FD_SIGMA]), P<double>(l[srk_ba::FD_FUND]), P<double>(l[srk_ba::FD_INFO]),
                         P<uint32_t>(l[srk_ba::FD_STATUS]), want_inl ? P<uint8_t>(l[srk_ba::FD_INL]) : nullptr);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->fd_ev[3], s));
    for (auto& o : outs)
        if (o.bytes) HIPCHK(h, hipMemcpyAsync(o.dst, l[o.buf].p, o.bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    float ms = 0, score_ms = 0, solve_ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->fd_ev[0], h->fd_ev[3]));
    HIPCHK(h, hipEventElapsedTime(&score_ms, h->fd_ev[1], h->fd_ev[2]));
    HIPCHK(h, hipEventElapsedTime(&solve_ms, h->fd_ev[4], h->fd_ev[1]));
    h->fd_ms = ms;
    h->fd_score_ms = score_ms;
    h->fd_solve_ms = solve_ms;
    return SRK_OK;
}

extern "C" double srk_ba_fundamental_kernel_ms(const srk_ba* h) { return h ? h->fd_ms : 0.0; }
extern "C" double srk_ba_fundamental_score_ms(const srk_ba* h) { return h ? h->fd_score_ms : 0.0; }
extern "C" double srk_ba_fundamental_solve_ms(const srk_ba* h) { return h ? h->fd_solve_ms : 0.0; }

extern "C" int srk_relate_uncalibrated(srk_ba* h, double f0, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                                       const srk_fundamental_options* opts, double* F, double* U, double* V, double* sigma, double* fund, double* info,
                                       uint32_t* status, uint8_t* inlier_out)
{
    if (!h) return SRK_E_ARGS;
    try {
        std::string why = srk_fund_check(n_pairs, row_ptr, uv_a, uv_b, q, opts);
        if (why.empty() && (!std::isfinite(f0) || srk::is_close(0.0, f0))) why = "fundamental: f0 must be finite and not ~0";
        if (why.empty() && n_pairs > 0 && (!F || !U || !V || !sigma || !fund || !info || !status)) why = "fundamental: a NULL output array";
        if (!why.empty()) { h->last_error = why; return SRK_E_ARGS; }
        if (n_pairs == 0) return SRK_OK;
        HIPCHK(h, hipSetDevice(h->device));
        return fund_run(h, f0, n_pairs, row_ptr, uv_a, uv_b, q, srk_fund_effective_options(opts), F, U, V, sigma, fund, info, status, inlier_out);
    } catch (const std::bad_alloc&) {
        h->last_error = "fundamental: out of host memory";
        return SRK_E_NOMEM;
    }
}

// ------------------------------------------------------------------ the LM loop (bundle-adj-kanatani.cpp:720-893)

namespace {

// One srk_ba_optimize call: the reference's LM control flow, the speculative-pair schedule, the damping-parallel schedule of
// several ranks and the repeat after a hand-off timeout.  begin(), then iterate() for as long as it returns Again, then
// finish(); a negative return value is an error code and ends the call at once.
struct LmRun {
    enum { Done = 0, Again = 1 };
    enum class Decrease { Undecided, Accepted, Overflow, Converged };

    srk_ba* const h;
    srk_ba_report* const rep;
    const double* const allowed_err_change; // the two optional criteria
    const double* const max_hessian_factor;
    const int64_t max_iterations;
    const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
    double hessian_factor = (double)0.0001f; // :723 (float literal)
    double err_value = 0;
    bool result_true = false, spec_wanted = false, spec_drain = false;
    int64_t prev_attempts = 0; // attempts the previous iteration needed
    // state of one iteration (iterate() resets it)
    Decrease decrease = Decrease::Undecided;
    bool have_prev = false, jac_timed = false, dp_mode = false;
    double err_new_prev = 0, err_new = 0;
    int accepted_slot = 0, round = 0;
    unsigned spec_in_flight = 0; // slots whose speculative attempt has been enqueued and not judged
    std::chrono::steady_clock::time_point t_iter; // SRK_DEBUG trace only

    bool undecided() const { return decrease == Decrease::Undecided; }
    int fail_device(int rc)
    {
        rep->status = SRK_STATUS_DEVICE_ERROR;
        rep->optimized = 0;
        return rc;
    }
    double ev_ms(int a, int b) const
    {
        float ms = 0;
        if (h->profile_level < 1 || hipEventElapsedTime(&ms, h->ev[a], h->ev[b]) != hipSuccess) return 0.0;
        return (double)ms;
    }
    int mark(int i) // phase event i on the main stream; nothing at profile level 0
    {
        if (h->profile_level >= 1) HIPCHK(h, hipEventRecord(h->ev[i], h->main_stream));
        return SRK_OK;
    }

    int begin()
    {
        hipStream_t s = h->main_stream;
        const SrkDims& d = h->d;
        srk_ba::Attempt& a0 = h->att[0];
        h->iter_log.clear();
        rep->world_scale = h->nrm.world_scale;
        rearm_fusion(h);
        int rc = clear_poison(h);
        if (rc != SRK_OK) return rc;
        // clear the status words and point accumulators of every slot once; from here on the kernels keep them clear
        for (auto& a : h->att)
            if (a.allocated) {
                HIPCHK(h, hipMemsetAsync(a.info.p, 0, 4, s));
                HIPCHK(h, hipMemsetAsync(a.acc.p, 0, 8 * 3 * d.Ns + 64, s));
            }
        HIPCHK(h, hipStreamSynchronize(s)); // the second slot's stream starts after this
        // seen_points_count over all shards (:483, :726)
        // once per uploaded scene: it does not change between optimise calls
        if (h->seen_global < 0) {
            double seen_d = (double)d.O;
            if (h->allreduce || h->comm) {
                HIPCHK(h, hipMemcpyAsync(a0.err_dst, &seen_d, 8, hipMemcpyHostToDevice, s));
                rc = exchange(h, a0, a0.err_dst, 1);
                if (rc != SRK_OK) return fail_device(rc);
                HIPCHK(h, hipMemcpyAsync(&seen_d, a0.err_dst, 8, hipMemcpyDeviceToHost, s));
                HIPCHK(h, hipStreamSynchronize(s));
            }
            h->seen_global = (int64_t)seen_d;
        }
        rep->seen = h->seen_global;

        double err_initial = 0;
        if ((rc = mark(0)) != SRK_OK) return rc;
        rc = phase_error(h, a0, h->cur, nullptr);
        if (rc != SRK_OK) return fail_device(rc);
        if ((rc = mark(1)) != SRK_OK) return rc;
        HIPCHK(h, hipMemcpyAsync(&err_initial, a0.err_dst, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        rep->ms_error += ev_ms(0, 1);
        rep->err_initial = rep->err_final = err_value = err_initial;
        if (allowed_err_change && err_initial < *allowed_err_change) { // :749-753
            rep->status = SRK_STATUS_ABS_ERR_THRESHOLD;
            result_true = true;
            return Done;
        }
        return Again;
    }

    // one attempt, enqueued on slot sl's stream without waiting for it, in two parts so that a pair can put both
    // Schur sums (which fill the chip one after the other) in front of both solves
    int enqueue_schur(int sl, double c)
    {
        srk_ba::Attempt& a = h->att[sl];
        int r2 = SRK_OK, e;
        if (sl >= 1 && hipStreamWaitEvent(a.stream, h->ev_jac, 0) != hipSuccess) r2 = SRK_E_DEVICE;
        if (sl == 0 && (e = mark(2)) != SRK_OK) return e;
        if (r2 == SRK_OK) r2 = phase_schur(h, a, c);
        if (sl == 0 && (e = mark(3)) != SRK_OK) return e;
        return r2;
    }
    int enqueue_rest(int sl, double c)
    {
        srk_ba::Attempt& a = h->att[sl];
        int e, r2 = phase_solve(h, a, h->profile_level >= 2);
        if (sl == 0 && (e = mark(4)) != SRK_OK) return e;
        if (r2 == SRK_OK) r2 = phase_backsub_apply(h, a, c);
        if (sl == 0 && (e = mark(5)) != SRK_OK) return e;
        if (r2 == SRK_OK) r2 = phase_cam_apply(h, a);
        if (sl == 0 && (e = mark(6)) != SRK_OK) return e;
        if (r2 == SRK_OK) r2 = phase_error(h, a, a.trial, nullptr, true);
        if (sl == 0 && (e = mark(7)) != SRK_OK) return e;
        // one read-back per attempt into pinned host memory: {error, solver info, point-update info}
        if (r2 == SRK_OK && hipMemcpyAsync(a.host_back, a.err_dst, 24, hipMemcpyDeviceToHost, a.stream) != hipSuccess)
            r2 = SRK_E_DEVICE;
        if (r2 == SRK_OK && hipEventRecord(a.done, a.stream) != hipSuccess) r2 = SRK_E_DEVICE;
        return r2;
    }
    // repeats one attempt after a hand-off timeout
    int redo_unfused(int sl, double c)
    {
        fusion_off(h);
        if (srk_debug()) fprintf(stderr, "srk_ba[rank %d]: hand-off timeout in the fused solve (slot %d); repeating unfused\n", h->rank, sl);
        h->poisoned = true;
        int r2 = clear_poison(h); // waits for both slots' streams, re-zeroes systems, plans, status words, accumulators
        if (r2 == SRK_OK) r2 = enqueue_schur(sl, c);
        if (r2 == SRK_OK) r2 = enqueue_rest(sl, c);
        return r2;
    }

    // wait for slot sl's attempt and judge it exactly as the reference judges the attempt with factor `hessian_factor`
    int judge(int sl)
    {
        if (hipStreamSynchronize(h->att[sl].stream) != hipSuccess) return SRK_E_DEVICE;
        const double* hb = h->att[sl].host_back;
        // (several ranks: the status words are SUMMED over the ranks, so bit 8 cannot be told from two ranks' bit 4; any
        // non-zero status of a fused solve is then taken for a possible timeout -- every rank sees the same sum and
        // repeats, a genuine failure shows again without the fused kernels)
        // (damping-parallel schedule: only the rank that solved a factor contributes its status word, bit 8 is exact, and
        // the round loop has dealt with it before anything is judged)
        const bool multi_rank = (h->allreduce || h->comm) && !dp_mode;
        if (multi_rank ? ((int)hb[1] != 0 && h->att[sl].sync.fused) : (((int)hb[1] & 8) != 0 && !dp_mode)) {
            // an in-launch hand-off of the fused solve timed out (srk_chol.hip: k_step256; its spins are bounded): the
            // numbers of this attempt are void.  From now on the unfused launch sequence (the two agree to rounding);
            // this attempt is repeated with the factor it stands for, which is `hessian_factor` at this point.
            int r2 = redo_unfused(sl, hessian_factor);
            if (r2 != SRK_OK) return r2;
            if (hipStreamSynchronize(h->att[sl].stream) != hipSuccess) return SRK_E_DEVICE;
        }
        struct { double err; int info; } back{ hb[0], (int)hb[1] };
        const int info2 = (int)hb[2];
        rep->attempts += 1;
        rep->schur_launches += 2;
        h->last_slot = sl;
        if (srk_debug())
            fprintf(stderr, "srk_ba[rank %d] iteration %lld attempt %lld (slot %d, +%.3f ms): hessian_factor %.3g err %.17g -> "
                            "%.17g, solver info %d, point-update info %d\n", h->rank, (long long)rep->iterations + 1,
                    (long long)rep->attempts, sl,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_iter).count(),
                    hessian_factor, err_value, back.err, back.info, info2);
        // Solve failed (:807-808, :1912-1913, :1953-1954).  The multiplicative damping keeps the diagonally scaled
        // system's smallest eigenvalue >= c, so a Cholesky pivot can only fail where diag(G) holds an exact
        // zero or a non-finite value -- exactly where the reference's Householder QR divides by a zero diagonal of R
        // and returns non-finite numbers: both sides end with "hessian overflow".
        if (back.info != 0 || info2 != 0) { h->poisoned = true; decrease = Decrease::Overflow; return SRK_OK; }
        err_new = back.err;
        if (err_new - err_value < 0) { decrease = Decrease::Accepted; accepted_slot = sl; return SRK_OK; } // :816-819
        // restore = drop the trial buffers (:823-826)
        if (have_prev && allowed_err_change) { // :828-838
            double change = err_new - err_new_prev;
            if (std::fabs(change) < *allowed_err_change) { decrease = Decrease::Converged; return SRK_OK; }
        }
        hessian_factor *= 10; // :841
        if (max_hessian_factor && hessian_factor > *max_hessian_factor) { decrease = Decrease::Overflow; return SRK_OK; } // :843-847
        err_new_prev = err_new;
        have_prev = true;
        return SRK_OK;
    }

    // one round of the single-rank and the all-reduce schedule: the attempt with `hessian_factor` and, when a pair pays, its
    // successor beside it
    int pair_round()
    {
        // several ranks: every rank takes the same decisions, so the two slots' exchanges are issued in the same order
        // everywhere; the native path wants the second slot's own communicator (srk_ba_rccl_init_second), the callback
        // serialises the exchanges on the host
        const bool multi = h->allreduce || h->comm;
        const bool can_speculate = h->speculate && h->att[1].allocated && h->profile_level == 0 &&
                                   (!multi || (h->spec_multi && (h->allreduce || h->comm2)));
        // speculate once this optimise call has seen a rejection (or from its second iteration on): the first
        // iteration of a fresh scene is usually accepted at once -- and after a rejected pair the third attempt
        // usually is the last one: it runs alone unless the previous iteration needed four or more (then the damping
        // factor has a long way to climb and pairs pay again)
        const bool pair_pays = round == 0 ? (spec_wanted || rep->iterations >= 1) : (round >= 2 || prev_attempts >= 4);
        // (Round 3, measured and dropped: TRIPLES when the previous iteration needed three attempts -- late in a run on
        // the circle-grid scenes 16 of 20 iterations reject c / 10 and c and accept 10 c.  Three solves side by side are
        // slower than a pair plus a lone attempt, 299-302 against 331 it/s: one solve's fused outer steps hold ~200
        // workgroups of 66 KB LDS, two solves fill the chip's LDS, the third waits for slots.  Holding the solves back
        // until the last Schur sum is done: 325 against 331 it/s with pairs, 283-299 with triples.)
        const int want = (can_speculate && pair_pays) ? 2 : 1;
        int n_now = 1; // attempts enqueued this round: the factors hessian_factor * 10^k that the cap allows
        for (double cc = hessian_factor * 10; n_now < want && !(max_hessian_factor && cc > *max_hessian_factor); cc *= 10) ++n_now;
        const bool speculate_now = n_now >= 2;
        ++round;
        // one rank: all Schur sums first (a later one would otherwise wait behind ~0.6 ms of launch calls), then the
        // solves.  Several ranks: a Schur phase ends in a blocking exchange, so slot 0's solve is enqueued before it
        // and runs under slot 1's Schur sum and exchange.
        double cfk[SRK_SLOTS];
        for (int k = 0; k < SRK_SLOTS; ++k) cfk[k] = k == 0 ? hessian_factor : cfk[k - 1] * 10;
        int rc = enqueue_schur(0, cfk[0]);
        if (multi) {
            if (rc == SRK_OK) rc = enqueue_rest(0, cfk[0]);
            if (rc == SRK_OK && speculate_now) rc = enqueue_schur(1, cfk[1]);
        } else {
            for (int k = 1; k < n_now && rc == SRK_OK; ++k) rc = enqueue_schur(k, cfk[k]);
            if (rc == SRK_OK) rc = enqueue_rest(0, cfk[0]);
        }
        for (int k = 1; k < n_now && rc == SRK_OK; ++k) rc = enqueue_rest(k, cfk[k]);
        if (rc != SRK_OK) return fail_device(rc);
        for (int k = 1; k < n_now; ++k) spec_in_flight |= 1u << k;
        rc = judge(0);
        if (rc != SRK_OK) return fail_device(rc);
        if (!jac_timed) {
            rep->ms_jacobian += ev_ms(0, 1);
            rep->ms_jacobian_kernel += ev_ms(12, 13);
            jac_timed = true;
        }
        rep->ms_schur += ev_ms(2, 3);
        rep->ms_solve += ev_ms(3, 4);
        rep->ms_backsub += ev_ms(4, 5);
        rep->ms_apply += ev_ms(5, 6);
        rep->ms_error += ev_ms(6, 7);
        if (h->profile_level >= 2) {
            for (size_t kb = 0; kb < h->att[0].solve_prof.n; ++kb) {
                float ms = 0;
                if (hipEventElapsedTime(&ms, h->chol_ev[2 * kb], h->chol_ev[2 * kb + 1]) == hipSuccess)
                    rep->ms_solve_syrk += ms;
            }
            rep->solve_mfma_flops += h->att[0].solve_prof.flops;
        }
        if (undecided()) spec_wanted = true; // a rejection: from now on pairs pay
        for (int k = 1; k < n_now && undecided(); ++k) { // the successors were computed meanwhile, with exactly these factors
            rc = judge(k);
            if (rc != SRK_OK) return fail_device(rc);
            spec_in_flight &= ~(1u << k);
        }
        return SRK_OK;
    }

    // ---- several ranks: one round = the next G damping factors c, 10c, (100c), one attempt slot each.
    //   every rank: Schur sum of its landmarks for each factor (+ its share of the frame blocks), band packed;
    //   band k REDUCED to rank k % world (a reduce, not an all-reduce: half the traffic, and one ncclGroup for all k);
    //   rank k % world: unpack, factorise and solve factor k -- the G solves run at the same time on G GPUs;
    //   corrections of factor k BROADCAST from its rank (80 KB at 1000 frames);
    //   every rank: back-substitution, camera update and error of its shard for every factor;
    //   ONE all-reduce of the G x {error, solver status, point-update status}; every rank judges the attempts in the
    //   reference's order and takes the same decisions.  An iteration that needs <= G attempts costs about one solve.
    int dp_round(int G, const double* cf)
    {
        double* ptrs[SRK_SLOTS];
        int64_t counts[SRK_SLOTS];
        // first native round of this handle: every rooted collective is checked against a plain all-reduce of checksums
        const bool verify = h->comm != nullptr && !h->dp_verified;
        double expect[2 * SRK_SLOTS] = {}, rootv[2 * SRK_SLOTS] = {};
        int r2 = dp_build_and_reduce(G, cf, ptrs, counts, verify ? expect : nullptr);
        if (verify && (r2 = dp_verify_reduce(G, r2, ptrs, counts, expect)) == SRK_RETRY_ALLREDUCE) return r2;
        if (r2 == SRK_OK) r2 = dp_solve_and_broadcast(G, ptrs, counts, verify ? rootv : nullptr);
        if (verify && (r2 = dp_verify_broadcast(G, r2, ptrs, counts, rootv)) == SRK_RETRY_ALLREDUCE) return r2;
        if (r2 == SRK_OK) r2 = dp_score(G, cf);
        if (r2 == SRK_OK) r2 = dp_collect_status(G);
        return r2;
    }
    // expect (first native round only): what the sum over the ranks of band k must be
    int dp_build_and_reduce(int G, const double* cf, double** ptrs, int64_t* counts, double* expect)
    {
        int r2 = SRK_OK;
        for (int k = 0; k < G && r2 == SRK_OK; ++k) {
            srk_ba::Attempt& a = h->att[k];
            if (k > 0 && hipStreamWaitEvent(a.stream, h->ev_jac, 0) != hipSuccess) r2 = SRK_E_DEVICE;
            if (r2 == SRK_OK) r2 = phase_schur(h, a, cf[k], true);
            if (r2 == SRK_OK) r2 = schur_pack(h, a);
            ptrs[k] = P<double>(a.packed);
            counts[k] = h->band_packed + h->d.ld;
        }
        if (expect && r2 == SRK_OK) {
            for (int k = 0; k < G && r2 == SRK_OK; ++k) r2 = dp_checksum(h, h->att[k].stream, ptrs[k], counts[k], expect + 2 * k);
            if (r2 == SRK_OK) r2 = dp_allreduce_host(h, expect, 2 * G);
        }
        if (r2 == SRK_OK) r2 = coll_group(h, SRK_COLL_REDUCE, G, ptrs, counts);
        return r2;
    }
    // rootv (first native round only): the checksum of the corrections on the rank that solved them, known to everybody
    int dp_solve_and_broadcast(int G, double** ptrs, int64_t* counts, double* rootv)
    {
        int r2 = SRK_OK;
        for (int k = 0; k < G && r2 == SRK_OK; ++k) {
            srk_ba::Attempt& a = h->att[k];
            if (h->rank == k % h->world) {
                r2 = schur_unpack(h, a);
                if (r2 == SRK_OK) r2 = phase_solve(h, a, false);
            }
            ptrs[k] = P<double>(a.dc);
            counts[k] = h->d.ld;
        }
        if (rootv && r2 == SRK_OK) {
            for (int k = 0; k < G && r2 == SRK_OK; ++k)
                if (h->rank == k % h->world) r2 = dp_checksum(h, h->att[k].stream, ptrs[k], counts[k], rootv + 2 * k);
            if (r2 == SRK_OK) r2 = dp_allreduce_host(h, rootv, 2 * G);
        }
        if (r2 == SRK_OK) r2 = coll_group(h, SRK_COLL_BCAST, G, ptrs, counts);
        return r2;
    }
    int dp_score(int G, const double* cf)
    {
        int r2 = SRK_OK;
        for (int k = 0; k < G && r2 == SRK_OK; ++k) {
            srk_ba::Attempt& a = h->att[k];
            r2 = phase_backsub_apply(h, a, cf[k]);
            if (r2 == SRK_OK) r2 = phase_cam_apply(h, a);
            if (r2 == SRK_OK) r2 = phase_error(h, a, a.trial, nullptr, true, true);
        }
        return r2;
    }
    // the status words of all slots in one all-reduce, then one read-back
    int dp_collect_status(int G)
    {
        if (h->comm) {
            for (int k = 0; k < G; ++k) {
                if (hipEventRecord(h->att[k].ev_b, h->att[k].stream) != hipSuccess ||
                    hipStreamWaitEvent(h->comm_stream, h->att[k].ev_b, 0) != hipSuccess) return SRK_E_DEVICE;
            }
            ncclResult_t nr = rccl().AllReduce(h->status_all.p, h->status_all.p, (size_t)(8 * G), ncclDouble, ncclSum, h->comm, h->comm_stream);
            if (nr != ncclSuccess) { h->last_error = std::string("ncclAllReduce: ") + rccl().GetErrorString(nr); return SRK_E_DEVICE; }
            if (hipMemcpyAsync(h->dp_back, h->status_all.p, (size_t)(64 * G), hipMemcpyDeviceToHost, h->comm_stream) != hipSuccess ||
                hipStreamSynchronize(h->comm_stream) != hipSuccess) return SRK_E_DEVICE;
        } else {
            for (int k = 0; k < G; ++k)
                if (hipStreamSynchronize(h->att[k].stream) != hipSuccess) return SRK_E_DEVICE;
            if (h->allreduce(h->allreduce_ctx, P<double>(h->status_all), 8 * G) != 0) { h->last_error = "allreduce hook failed"; return SRK_E_DEVICE; }
            if (hipMemcpy(h->dp_back, h->status_all.p, (size_t)(64 * G), hipMemcpyDeviceToHost) != hipSuccess) return SRK_E_DEVICE;
        }
        for (int k = 0; k < G; ++k)
            for (int e = 0; e < 3; ++e) h->att[k].host_back[e] = h->dp_back[8 * k + e];
        return SRK_OK;
    }
    int dp_selfcheck_failed(const char* what)
    {
        h->dp_schedule = false;
        h->dp_selfcheck_failed = true;
        h->last_error = std::string("damping-parallel schedule: self-check of the first native round failed (") + what +
                        "); this handle runs the all-reduce schedule";
        if (srk_debug()) fprintf(stderr, "srk_ba[rank %d]: %s\n", h->rank, h->last_error.c_str());
        return SRK_RETRY_ALLREDUCE;
    }
    // The two verdicts of the first native round on what the round has returned so far: r2 (SRK_OK: the round goes on) or
    // SRK_RETRY_ALLREDUCE.
    // TODO: advisor finding (medium): a failure local to one rank returns SRK_RETRY_ALLREDUCE while its peers enter the collective
    int dp_verify_reduce(int G, int r2, double* const* ptrs, const int64_t* counts, const double* expect)
    {
        if (r2 == SRK_E_DEVICE) return dp_selfcheck_failed("an RCCL call of the reduce group returned an error");
        double bad = 0;
        for (int k = 0; k < G && r2 == SRK_OK; ++k) {
            if (h->rank != k % h->world) continue;
            double got[2];
            r2 = dp_checksum(h, h->att[k].stream, ptrs[k], counts[k], got); // (the slot's stream waits for the group)
            if (!(std::fabs(got[0] - expect[2 * k]) <= 1e-9 * expect[2 * k + 1] + 1e-300)) bad += 1;
        }
#ifdef SRK_DEV
        if (g_dp_corrupt == 1) bad += 1, g_dp_corrupt = 0;
#endif
        if (r2 == SRK_OK) r2 = dp_allreduce_host(h, &bad, 1);
        if (r2 == SRK_OK && bad > 0) return dp_selfcheck_failed("a reduced band does not sum to the all-reduced checksum");
        return r2;
    }
    int dp_verify_broadcast(int G, int r2, double* const* ptrs, const int64_t* counts, const double* rootv)
    {
        if (r2 == SRK_E_DEVICE) return dp_selfcheck_failed("an RCCL call of the broadcast group returned an error");
        double bad = 0;
        for (int k = 0; k < G && r2 == SRK_OK; ++k) {
            double got[2];
            r2 = dp_checksum(h, h->att[k].stream, ptrs[k], counts[k], got);
            // (a broadcast copies bits and the checksum has a fixed order: equal, not close; NaN corrections of a failed
            // solve compare unequal to themselves and are let through -- the status words deal with them)
            if (got[0] == got[0] && rootv[2 * k] == rootv[2 * k] && (got[0] != rootv[2 * k] || got[1] != rootv[2 * k + 1])) bad += 1;
        }
#ifdef SRK_DEV
        if (g_dp_corrupt == 2) bad += 1, g_dp_corrupt = 0;
#endif
        if (r2 == SRK_OK) r2 = dp_allreduce_host(h, &bad, 1);
        if (r2 == SRK_OK && bad > 0) return dp_selfcheck_failed("broadcast corrections differ from the solving rank's");
        if (r2 == SRK_OK) h->dp_verified = true;
        return r2;
    }
    // the damping-parallel rounds of one iteration: until an attempt decides it, or the schedule is given up
    int dp_rounds()
    {
        while (dp_mode && undecided()) {
            double cf[SRK_SLOTS];
            int G = 0;
            for (double cc = hessian_factor; G < SRK_SLOTS && h->att[G].allocated; cc *= 10) {
                if (G > 0 && max_hessian_factor && cc > *max_hessian_factor) break; // the reference stops before such an attempt (:843-847)
                cf[G++] = cc;
            }
            int rc = dp_round(G, cf);
            if (rc == SRK_RETRY_ALLREDUCE) { // the first native round failed its self-check (every rank saw the same verdict):
                // nothing of it was judged; the systems are rebuilt and this iteration's attempts run through the all-reduce schedule
                dp_mode = false;
                h->poisoned = true;
                rc = clear_poison(h);
                if (rc != SRK_OK) return fail_device(rc);
                break;
            }
            if (rc != SRK_OK) return fail_device(rc);
            bool timeout = false;
            for (int k = 0; k < G; ++k) timeout = timeout || (((int)h->att[k].host_back[1] & 8) != 0);
            if (timeout && h->chol_fused) { // a hand-off of the fused solve timed out on the rank that solved: the round again, unfused, everywhere
                fusion_off(h);
                h->poisoned = true;
                rc = clear_poison(h);
                if (rc != SRK_OK) return fail_device(rc);
                continue;
            }
            for (int k = 0; k < G && undecided(); ++k) {
                rc = judge(k);
                if (rc != SRK_OK) return fail_device(rc);
            }
        }
        return SRK_OK;
    }

    // one iteration: accepted (Again, unless a criterion ends the run) or the run's last
    int iterate()
    {
        hipStream_t s = h->main_stream;
        if (max_iterations > 0 && rep->iterations >= max_iterations) {
            rep->status = SRK_STATUS_MAX_ITERATIONS;
            result_true = false;
            return Done;
        }
        // ComputeCloseFormReprErrorDerivatives (:759)
        int rc;
        if ((rc = mark(0)) != SRK_OK) return rc;
        rc = phase_derivatives(h);
        if (rc != SRK_OK) return fail_device(rc);
        if ((rc = mark(1)) != SRK_OK) return rc;
        rep->jacobian_launches += 2;
        HIPCHK(h, hipEventRecord(h->ev_jac, s));
        t_iter = std::chrono::steady_clock::now();

        // try_decrease_targ_fun (:764-852): the backup is the untouched `cur` buffer set, every attempt slot has a trial
        // set of its own.  With two slots the NEXT damping factor (x10) is tried speculatively beside the current one on
        // a second stream: the solve is a latency chain that leaves most of the chip idle, so the pair costs little more
        // than one attempt, and a rejected first attempt finds its successor already done.  Attempts are still judged
        // strictly in the reference's order; a speculative result that is not needed is dropped unseen.
        decrease = Decrease::Undecided;
        have_prev = jac_timed = false;
        err_new_prev = 0, err_new = std::nan("");
        accepted_slot = round = 0;
        spec_in_flight = 0;
        // several ranks, damping-parallel schedule (instrumentation off): see dp_round
        dp_mode = (h->allreduce || h->comm) && (h->world >= 2 || h->dp_force) && h->dp_schedule &&
                  h->profile_level == 0 && h->att[1].allocated;
        const int64_t attempts_before = rep->attempts;
        if ((rc = dp_rounds()) != SRK_OK) return rc;
        while (undecided())
            if ((rc = pair_round()) != SRK_OK) return rc;
        prev_attempts = rep->attempts - attempts_before;
        if (spec_in_flight) {
            // speculative attempts nobody needs are still running: later work on the main stream (the next derivatives
            // overwrite what they read) must come after them; nothing on the host waits
            for (int k = 1; k < SRK_SLOTS; ++k)
                if (spec_in_flight & (1u << k)) HIPCHK(h, hipStreamWaitEvent(s, h->att[k].done, 0));
            spec_in_flight = 0;
            spec_drain = true;
        }
        if (decrease != Decrease::Accepted) { // :857-873
            rep->status = decrease == Decrease::Overflow ? SRK_STATUS_HESSIAN_OVERFLOW : SRK_STATUS_ERR_CONVERGED;
            result_true = false;
            return Done;
        }
        { // accept: the winning slot's trial scene becomes current, the old current set becomes that slot's trial set
            const int newcur = h->att[accepted_slot].trial;
            h->att[accepted_slot].trial = h->cur;
            h->cur = newcur;
        }
        rep->iterations += 1;
        if (h->iter_log.size() < (size_t)1 << 20)
            h->iter_log.push_back({ (int32_t)prev_attempts, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(),
                                    err_new, hessian_factor });
        double change = err_new - err_value;
        rep->err_final = err_new;
        if (allowed_err_change && std::fabs(change) < *allowed_err_change) { // :880-884
            rep->status = SRK_STATUS_SMALL_ERR_CHANGE;
            result_true = true;
            return Done;
        }
        err_value = err_new;
        hessian_factor /= 10; // :889
        return Again;
    }

    int finish()
    {
        if (spec_drain) {
            for (int k = 1; k < SRK_SLOTS; ++k) {
                if (!h->att[k].allocated) continue;
                HIPCHK(h, hipStreamSynchronize(h->att[k].stream)); // leave no speculative work behind
                if (h->att[k].host_back[1] != 0.0 || h->att[k].host_back[2] != 0.0) h->poisoned = true; // a dropped attempt that failed
            }
        }
        rep->hessian_factor = hessian_factor;
        rep->optimized = result_true ? 1 : 0;
        rep->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
        return result_true ? 0 : 1;
    }
};

} // namespace

extern "C" {

int srk_ba_optimize(srk_ba* h, const double* allowed_err_change, const double* max_hessian_factor,
                    int64_t max_iterations, srk_ba_report* rep)
{
    srk_ba_report local;
    if (!rep) rep = &local;
    std::memset(rep, 0, sizeof *rep);
    if (!h || !h->have_scene) return SRK_E_STATE;
    HIPCHK(h, hipSetDevice(h->device));
    LmRun run{ h, rep, allowed_err_change, max_hessian_factor, max_iterations };
    struct LeanGuard { // no per-attempt memsets while the loop runs (see phase_solve)
        srk_ba* h;
        explicit LeanGuard(srk_ba* hh) : h(hh) { h->lean_resets = true; }
        ~LeanGuard() { h->lean_resets = false; }
    } lean_guard(h);
    int rc = run.begin();
    while (rc == LmRun::Again) rc = run.iterate();
    return rc < 0 ? rc : run.finish();
}

int srk_ba_compute_inplace(srk_ba* h, double f0, int64_t N, double* pts, int32_t M, double* cam_R, double* cam_T,
                           const double* K, int shared_k, const int64_t* row_ptr, const int32_t* obs_frame,
                           const double* obs_uv, const double* allowed_err_change, const double* max_hessian_factor,
                           int64_t max_iterations, srk_ba_report* rep)
{
    srk_ba_report local;
    if (!rep) rep = &local;
    std::memset(rep, 0, sizeof *rep);
    if (!h) return SRK_E_ARGS;
    int rc = srk_ba_upload_scene(h, f0, N, pts, M, cam_R, cam_T, K, shared_k, row_ptr, obs_frame, obs_uv, 0);
    if (rc == 1) { // normalisation failed: reference returns false with an empty status string (:681-682)
        rep->status = SRK_STATUS_NONE;
        return 1;
    }
    if (rc != SRK_OK) return rc;
    int result = srk_ba_optimize(h, allowed_err_change, max_hessian_factor, max_iterations, rep);
    if (result < 0) return result;
    if (!h->cst.set.set) {
        rc = srk_ba_download_scene(h, pts, cam_R, cam_T, 1);
        if (rc != SRK_OK) return rc;
        return result;
    }
    // constant blocks are not written back: the caller's entries stay what they were, bit for bit
    std::vector<double> p2((size_t)(3 * N)), r2((size_t)(9 * (int64_t)M)), t2((size_t)(3 * (int64_t)M));
    rc = srk_ba_download_scene(h, p2.data(), r2.data(), t2.data(), 1);
    if (rc != SRK_OK) return rc;
    for (int64_t i = 0; i < N; ++i)
        if (h->cst.set.points.empty() || !h->cst.set.points[(size_t)i]) std::memcpy(pts + 3 * i, &p2[(size_t)(3 * i)], 24);
    for (int32_t j = 0; j < M; ++j)
        if (h->cst.set.frames.empty() || !h->cst.set.frames[(size_t)j]) {
            std::memcpy(cam_R + 9 * (int64_t)j, &r2[9 * (size_t)j], 72);
            std::memcpy(cam_T + 3 * (int64_t)j, &t2[3 * (size_t)j], 24);
        }
    return result;
}

// Standalone scoring: ReprojError callers that only score a scene (multi-view-factorization.cpp:373,409-413) do not
// need the LM state -- no gauge normalisation, landmark sort, grouping or solver plan; the uploaded BA scene (if any)
// stays untouched.  z_tol < 0 keeps every observation (BundleAdjustmentKanatani::ReprojError, :589-600).
static int score_scene(srk_ba* h, double f0, int64_t N, const double* pts, int32_t M, const double* cam_R,
                       const double* cam_T, const double* K, int shared_k, const int64_t* row_ptr,
                       const int32_t* obs_frame, const double* obs_uv, int32_t min_frames, double z_tol, double* err,
                       int64_t* count)
{
    int rc = validate_scene(h, f0, N, pts, M, cam_R, cam_T, K, row_ptr, obs_frame, obs_uv, min_frames);
    if (rc != SRK_OK) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->main_stream;
    const int64_t O = row_ptr[N];
    std::vector<int32_t> obs_pt((size_t)O);
    for (int64_t i = 0; i < N; ++i)
        for (int64_t o = row_ptr[i]; o < row_ptr[i + 1]; ++o) obs_pt[(size_t)o] = (int32_t)i;
    std::vector<double> Kexp(9 * (size_t)M);
    for (int32_t j = 0; j < M; ++j) std::memcpy(&Kexp[9 * (size_t)j], shared_k ? K : K + 9 * (int64_t)j, 72);
    SrkDims d{};
    d.O = O;
    d.fv = 10;
    const int32_t np = srk_error_partials(d);
    struct { DevBuf* b; const void* src; size_t bytes; } up[] = {
        { &h->sc_pts, pts, (size_t)(24 * N) },          { &h->sc_R, cam_R, (size_t)(72 * (int64_t)M) },
        { &h->sc_T, cam_T, (size_t)(24 * (int64_t)M) }, { &h->sc_K, Kexp.data(), (size_t)(72 * (int64_t)M) },
        { &h->sc_frame, obs_frame, (size_t)(4 * O) },   { &h->sc_pt, obs_pt.data(), (size_t)(4 * O) },
        { &h->sc_uv, obs_uv, (size_t)(16 * O) },
    };
    for (auto& u : up) {
        if ((rc = dev_alloc(h, *u.b, u.bytes)) != SRK_OK) return rc;
        if (u.bytes) HIPCHK(h, hipMemcpyAsync(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice, s));
    }
    if ((rc = dev_alloc(h, h->sc_cam, (size_t)(8 * SRK_CAM_PACK * (int64_t)M))) != SRK_OK) return rc;
    if ((rc = dev_alloc(h, h->sc_partial, (size_t)(16 * np))) != SRK_OK) return rc;
    if ((rc = dev_alloc(h, h->sc_out, 16)) != SRK_OK) return rc;
    srk_launch_cam_pack(s, M, P<double>(h->sc_R), P<double>(h->sc_T), P<double>(h->sc_K), f0, P<double>(h->sc_cam));
    srk_launch_error_score(s, O, P<double>(h->sc_pts), P<double>(h->sc_cam), P<int32_t>(h->sc_frame), P<int32_t>(h->sc_pt),
                           P<double>(h->sc_uv), z_tol, P<double>(h->sc_partial), np, P<double>(h->sc_out));
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(h->att[0].host_back, h->sc_out.p, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    *err = h->att[0].host_back[0];
    *count = (int64_t)h->att[0].host_back[1];
    return SRK_OK;
}

double srk_ba_reproj_error(srk_ba* h, double f0, int64_t N, const double* pts, int32_t M, const double* cam_R,
                           const double* cam_T, const double* K, int shared_k, const int64_t* row_ptr,
                           const int32_t* obs_frame, const double* obs_uv, int64_t* seen)
{
    if (!h) return std::nan("");
    double e = std::nan("");
    int64_t cnt = 0;
    if (score_scene(h, f0, N, pts, M, cam_R, cam_T, K, shared_k, row_ptr, obs_frame, obs_uv, 2, -1.0, &e, &cnt) != SRK_OK)
        return std::nan("");
    if (seen) *seen = cnt;
    return e;
}

int srk_ba_reproj_error_mvf(srk_ba* h, double f0, int64_t N, const double* pts, int32_t M, const double* cam_R,
                            const double* cam_T, const double* K, int shared_k, const int64_t* row_ptr,
                            const int32_t* obs_frame, const double* obs_uv, double z_tol, double* reproj_err,
                            int64_t* summands)
{
    if (!h || !reproj_err || z_tol < 0) return SRK_E_ARGS;
    double e = 0;
    int64_t cnt = 0;
    int rc = score_scene(h, f0, N, pts, M, cam_R, cam_T, K, shared_k, row_ptr, obs_frame, obs_uv, 1, z_tol, &e, &cnt);
    if (rc != SRK_OK) return rc;
    if (summands) *summands = cnt;
    if (cnt == 0) return 0; // no points, or every point at infinity: the reference returns false (:470-471)
    *reproj_err = e;
    return 1;
}

// ------------------------------------------------------------------ f32 boundary (suriko_scalar_type_string = f32)
// A reference built with Scalar = float (rt-config.h:41-48, suriko-engine/CMakeLists.txt:14-15,76-82) hands over float
// arrays.  They are widened here, the fp64 pipeline runs unchanged, the result is rounded back: the arithmetic is
// strictly more accurate than the reference's own f32 build (an f32 device pipeline is not implemented).
extern "C" int srk_ba_compute_inplace_f32(srk_ba* h, float f0, int64_t N, float* pts, int32_t M, float* cam_R, float* cam_T,
                                          const float* K, int shared_k, const int64_t* row_ptr, const int32_t* obs_frame,
                                          const float* obs_uv, const float* allowed_err_change,
                                          const float* max_hessian_factor, int64_t max_iterations, srk_ba_report* out)
{
    if (!h) return SRK_E_ARGS;
    if (N < 0 || M < 1 || !row_ptr || !cam_R || !cam_T || !K || (N > 0 && !pts)) {
        h->last_error = "null scene array";
        return SRK_E_ARGS;
    }
    const int64_t O = row_ptr[N];
    if (O > 0 && !obs_uv) { h->last_error = "null observation arrays"; return SRK_E_ARGS; }
    auto widen = [](const float* p, size_t n) { return std::vector<double>(p, p + n); };
    std::vector<double> dp = widen(pts, (size_t)(3 * N)), dR = widen(cam_R, 9 * (size_t)M), dT = widen(cam_T, 3 * (size_t)M),
                        dK = widen(K, shared_k ? 9 : 9 * (size_t)M), duv = widen(obs_uv, (size_t)(2 * O));
    double a = allowed_err_change ? (double)*allowed_err_change : 0, m = max_hessian_factor ? (double)*max_hessian_factor : 0;
    int rc = srk_ba_compute_inplace(h, (double)f0, N, dp.data(), M, dR.data(), dT.data(), dK.data(), shared_k, row_ptr,
                                    obs_frame, duv.data(), allowed_err_change ? &a : nullptr,
                                    max_hessian_factor ? &m : nullptr, max_iterations, out);
    if (rc < 0) return rc;
    for (size_t i = 0; i < dp.size(); ++i) pts[i] = (float)dp[i];
    for (size_t i = 0; i < dR.size(); ++i) cam_R[i] = (float)dR[i];
    for (size_t i = 0; i < dT.size(); ++i) cam_T[i] = (float)dT[i];
    return rc;
}

// ------------------------------------------------------------------ multi-view-factorization steps
namespace {
// cyclic Jacobi eigen-decomposition of a symmetric n x n matrix (row-major, destroyed): V's columns = eigenvectors
void jacobi_eig(int n, double* A, double* V, double* ev)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) V[i * n + j] = i == j;
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0, diag = 0;
        for (int i = 0; i < n; ++i) {
            diag += A[i * n + i] * A[i * n + i];
            for (int j = i + 1; j < n; ++j) off += A[i * n + j] * A[i * n + j];
        }
        if (off <= 1e-34 * diag || off == 0) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                double apq = A[p * n + q];
                if (apq == 0) continue;
                double theta = (A[q * n + q] - A[p * n + p]) / (2 * apq);
                double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(1 + theta * theta));
                double c = 1 / std::sqrt(1 + t * t), sn = c * t;
                for (int k = 0; k < n; ++k) { // columns p, q
                    double x = A[k * n + p], y = A[k * n + q];
                    A[k * n + p] = c * x - sn * y;
                    A[k * n + q] = sn * x + c * y;
                }
                for (int k = 0; k < n; ++k) { // rows p, q
                    double x = A[p * n + k], y = A[q * n + k];
                    A[p * n + k] = c * x - sn * y;
                    A[q * n + k] = sn * x + c * y;
                }
                for (int k = 0; k < n; ++k) {
                    double x = V[k * n + p], y = V[k * n + q];
                    V[k * n + p] = c * x - sn * y;
                    V[k * n + q] = sn * x + c * y;
                }
            }
    }
    for (int i = 0; i < n; ++i) ev[i] = A[i * n + i];
}

// ProjectOntoSO3 (multi-view-factorization.cpp:79-104; MASKS 8.41, 8.42): R = sign(det(U V^T)) U V^T from the SVD of
// the noisy R (via the eigen-decomposition of R^T R), T scaled by sign / cbrt(det S).  false when det S ~ 0.
bool project_onto_so3(const double Rn[9], const double Tn[3], double R[9], double T[3])
{
    double G[9], V[9], ev[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) G[3 * i + j] = Rn[i] * Rn[j] + Rn[3 + i] * Rn[3 + j] + Rn[6 + i] * Rn[6 + j];
    jacobi_eig(3, G, V, ev);
    double sv[3];
    for (int k = 0; k < 3; ++k) sv[k] = std::sqrt(std::max(ev[k], 0.0));
    double det_S = sv[0] * sv[1] * sv[2];
    if (srk::is_close(0.0, det_S)) return false; // :88-89
    double U[9]; // U = R V S^-1
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) U[3 * i + k] = (Rn[3 * i] * V[k] + Rn[3 * i + 1] * V[3 + k] + Rn[3 * i + 2] * V[6 + k]) / sv[k];
    double ng[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) ng[3 * i + j] = U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1] + U[3 * i + 2] * V[3 * j + 2];
    double det = ng[0] * (ng[4] * ng[8] - ng[5] * ng[7]) - ng[1] * (ng[3] * ng[8] - ng[5] * ng[6]) +
                 ng[2] * (ng[3] * ng[7] - ng[4] * ng[6]);
    int sign = det >= 0 ? 1 : -1; // approx-alg.h:41
    for (int i = 0; i < 9; ++i) R[i] = sign * ng[i];
    double sc = sign / std::cbrt(det_S);
    for (int i = 0; i < 3; ++i) T[i] = sc * Tn[i];
    return true;
}
} // namespace

extern "C" int srk_mvf_project_onto_so3(const double* R_noisy, const double* T_noisy, double* R_out, double* T_out)
{
    if (!R_noisy || !T_noisy || !R_out || !T_out) return SRK_E_ARGS;
    return project_onto_so3(R_noisy, T_noisy, R_out, T_out) ? 1 : 0;
}

extern "C" int srk_mvf_estimate_depths(srk_ba* h, int64_t n_tracks, const int64_t* row_ptr, const int32_t* frame,
                                       const double* x_meter, int32_t n_frames, const double* cam_R, const double* cam_T,
                                       double* depth_out)
{
    if (!h) return SRK_E_ARGS;
    if (n_tracks < 0 || n_frames < 1 || !row_ptr || !cam_R || !cam_T || (n_tracks > 0 && !depth_out) || row_ptr[0] != 0) {
        h->last_error = "srk_mvf_estimate_depths: bad arguments";
        return SRK_E_ARGS;
    }
    const int64_t O = row_ptr[n_tracks];
    if (O > 0 && (!frame || !x_meter)) { h->last_error = "srk_mvf_estimate_depths: null observation arrays"; return SRK_E_ARGS; }
    for (int64_t i = 0; i < n_tracks; ++i) {
        if (row_ptr[i + 1] < row_ptr[i]) { h->last_error = "row_ptr not monotone"; return SRK_E_ARGS; }
        for (int64_t o = row_ptr[i]; o < row_ptr[i + 1]; ++o)
            if (frame[o] < 0 || frame[o] >= n_frames) { h->last_error = "frame out of range"; return SRK_E_ARGS; }
    }
    if (n_tracks == 0) return SRK_OK;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->main_stream;
    int rc;
    struct { DevBuf* b; const void* src; size_t bytes; } up[] = {
        { &h->sc_pts, x_meter, (size_t)(24 * O) },       { &h->sc_R, cam_R, (size_t)(72 * (int64_t)n_frames) },
        { &h->sc_T, cam_T, (size_t)(24 * (int64_t)n_frames) }, { &h->sc_frame, frame, (size_t)(4 * O) },
        { &h->sc_uv, row_ptr, (size_t)(8 * (n_tracks + 1)) },
    };
    for (auto& u : up) {
        if ((rc = dev_alloc(h, *u.b, u.bytes)) != SRK_OK) return rc;
        if (u.bytes) HIPCHK(h, hipMemcpyAsync(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice, s));
    }
    if ((rc = dev_alloc(h, h->sc_partial, (size_t)(8 * n_tracks))) != SRK_OK) return rc;
    srk_launch_mvf_depth(s, n_tracks, P<int64_t>(h->sc_uv), P<int32_t>(h->sc_frame), P<double>(h->sc_pts), P<double>(h->sc_R),
                         P<double>(h->sc_T), P<double>(h->sc_partial));
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(depth_out, h->sc_partial.p, (size_t)(8 * n_tracks), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return SRK_OK;
}

extern "C" int srk_mvf_relative_motion(srk_ba* h, int64_t n_points, const double* x_anchor, const double* x_target,
                                       const double* depth_anchor, double* R_out, double* T_out)
{
    if (!h) return SRK_E_ARGS;
    // every point contributes two independent equations ([x2]x has rank 2) towards the 11 needed for a unique
    // null vector of the 12 unknowns: fewer than 6 points leave the answer arbitrary (the reference does not check)
    if (n_points < 6 || !x_anchor || !x_target || !depth_anchor || !R_out || !T_out) {
        h->last_error = "srk_mvf_relative_motion: need at least 6 common points and non-null arrays";
        return SRK_E_ARGS;
    }
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->main_stream;
    int rc;
    const int64_t nblk = (n_points + 255) / 256;
    struct { DevBuf* b; const void* src; size_t bytes; } up[] = {
        { &h->sc_pts, x_anchor, (size_t)(24 * n_points) }, { &h->sc_uv, x_target, (size_t)(24 * n_points) },
        { &h->sc_R, depth_anchor, (size_t)(8 * n_points) },
    };
    for (auto& u : up) {
        if ((rc = dev_alloc(h, *u.b, u.bytes)) != SRK_OK) return rc;
        HIPCHK(h, hipMemcpyAsync(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice, s));
    }
    if ((rc = dev_alloc(h, h->sc_partial, (size_t)(8 * 78 * nblk))) != SRK_OK) return rc;
    srk_launch_mvf_gram(s, n_points, P<double>(h->sc_pts), P<double>(h->sc_uv), P<double>(h->sc_R), P<double>(h->sc_partial));
    HIPCHK(h, hipGetLastError());
    std::vector<double> part((size_t)(78 * nblk));
    HIPCHK(h, hipMemcpyAsync(part.data(), h->sc_partial.p, part.size() * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    double G[144], V[144], ev[12];
    int e = 0;
    for (int a = 0; a < 12; ++a)
        for (int b = a; b < 12; ++b, ++e) {
            double sum = 0;
            for (int64_t k = 0; k < nblk; ++k) sum += part[(size_t)(78 * k + e)]; // fixed order
            G[a * 12 + b] = G[b * 12 + a] = sum;
        }
    jacobi_eig(12, G, V, ev);
    int jmin = 0;
    for (int j = 1; j < 12; ++j)
        if (ev[j] < ev[jmin]) jmin = j;
    double Rn[9], Tn[3];
    for (int col = 0; col < 3; ++col) // vec(R) is column-major in the reference (:174)
        for (int row = 0; row < 3; ++row) Rn[3 * row + col] = V[(3 * col + row) * 12 + jmin];
    for (int i = 0; i < 3; ++i) Tn[i] = V[(9 + i) * 12 + jmin];
    return project_onto_so3(Rn, Tn, R_out, T_out) ? 1 : 0;
}

// ------------------------------------------------------------------ downloads for the parity tests

// shared intrinsics: storage index of the caller's reduced variable u (pose 6 frame + v, then 4 g + k behind the 6M)
static int64_t shk_index(const srk_ba* h, int64_t u)
{
    const int64_t n6 = 6 * (int64_t)h->d.M;
    if (u >= n6) return h->shk_ncols + (u - n6);
    const int64_t f = u / 6;
    return 6 * (int64_t)(h->frame_int.empty() ? f : h->frame_int[(size_t)f]) + u % 6;
}
// row r (caller's layout) of the folded system, columns <= r; S: the slot's S_sh (lower triangle authoritative)
static int shk_row(srk_ba* h, const double* S, int64_t r, double* out)
{
    const int64_t n = 6 * (int64_t)h->d.M + 4 * (int64_t)h->shk_G, ldb = h->shk_ldb, ri = shk_index(h, r);
    std::vector<double> rowi((size_t)ldb, 0.0), coli((size_t)ldb, 0.0);
    HIPCHK(h, hipMemcpy(rowi.data(), S + ri * ldb, (size_t)(8 * (ri + 1)), hipMemcpyDeviceToHost));
    if (ri + 1 < ldb)
        HIPCHK(h, hipMemcpy2D(coli.data() + ri + 1, 8, S + (ri + 1) * ldb + ri, (size_t)(8 * ldb), 8, (size_t)(ldb - ri - 1), hipMemcpyDeviceToHost));
    for (int64_t c = 0; c <= r && c < n; ++c) {
        const int64_t ci = shk_index(h, c);
        out[c] = ci <= ri ? rowi[(size_t)ci] : coli[(size_t)ci];
    }
    return SRK_OK;
}
int64_t srk_ba_buffer_size(srk_ba* h, int which);
// SRK_BUF_GRAD / RCS / RCS_RHS / CORRECTIONS in the shared layout (the caller's frame and group numbering)
static int download_shared(srk_ba* h, int which, double* dst)
{
    const SrkDims& d = h->d;
    const int32_t M = d.M, G = h->shk_G;
    const int64_t n6 = 6 * (int64_t)M, n = n6 + 4 * (int64_t)G;
    int rc;
    if (which == SRK_BUF_GRAD) { // P^T of the 10-variable gradient (the landmark part as it is)
        std::vector<double> vg((size_t)(9 * d.Ns)), ug((size_t)(SRK_UG * (int64_t)M));
        HIPCHK(h, hipMemcpy(vg.data(), h->Vg.p, vg.size() * 8, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(ug.data(), h->Ug.p, ug.size() * 8, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < d.N; ++i)
            for (int e = 0; e < 3; ++e) dst[3 * h->perm[(size_t)i] + e] = vg[(size_t)((6 + e) * d.Ns + i)];
        double* out = dst + 3 * d.N;
        std::fill(out, out + n, 0.0);
        for (int32_t u = 0; u < M; ++u) { // the caller's frames in ascending order: a fixed summation order
            const int32_t fi = h->frame_int.empty() ? u : h->frame_int[(size_t)u];
            const double* gf = ug.data() + SRK_UG * (int64_t)fi + 55;
            for (int v = 0; v < 6; ++v) out[6 * (int64_t)u + v] = gf[4 + v];
            for (int k = 0; k < 4; ++k) out[n6 + 4 * (int64_t)h->shk_grp_h[(size_t)fi] + k] += gf[k];
        }
        return SRK_OK;
    }
    const srk_ba::Attempt& a = h->att[h->last_slot];
    if (which == SRK_BUF_RCS) {
        for (int64_t r = 0; r < n; ++r) {
            if ((rc = shk_row(h, P<double>(a.Ssh), r, dst + r * n)) != SRK_OK) return rc;
            for (int64_t c = 0; c < r; ++c) dst[c * n + r] = dst[r * n + c];
        }
        return SRK_OK;
    }
    std::vector<double> v((size_t)h->shk_ldb);
    const DevBuf& src = which == SRK_BUF_RCS_RHS ? a.rsh : a.dcsh;
    HIPCHK(h, hipMemcpy(v.data(), src.p, (size_t)(8 * h->shk_ldb), hipMemcpyDeviceToHost));
    double* out = dst;
    if (which == SRK_BUF_CORRECTIONS) {
        std::vector<double> tmp((size_t)(3 * d.N));
        HIPCHK(h, hipMemcpy(tmp.data(), a.dx.p, (size_t)(24 * d.N), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < d.N; ++i) std::memcpy(dst + 3 * h->perm[(size_t)i], &tmp[(size_t)(3 * i)], 24);
        out = dst + 3 * d.N;
    }
    for (int64_t u = 0; u < n; ++u) out[u] = v[(size_t)shk_index(h, u)];
    return SRK_OK;
}

int64_t srk_ba_buffer_size(srk_ba* h, int which)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    const SrkDims& d = h->d;
    if (h->shk_G > 0) { // shared intrinsics: the reduced layout is 6M pose variables + 4G group intrinsics
        const int64_t n = 6 * (int64_t)d.M + 4 * (int64_t)h->shk_G;
        if (which == SRK_BUF_GRAD || which == SRK_BUF_CORRECTIONS) return 3 * d.N + n;
        if (which == SRK_BUF_RCS) return n * n;
        if (which == SRK_BUF_RCS_RHS) return n;
    }
    switch (which) {
    case SRK_BUF_GRAD: return 3 * d.N + d.fv * (int64_t)d.M;
    case SRK_BUF_POINT_BLOCKS: return 9 * d.N;
    case SRK_BUF_FRAME_BLOCKS: return d.fv * d.fv * (int64_t)d.M;
    case SRK_BUF_POINT_FRAME: return 3 * d.fv * d.O;
    case SRK_BUF_RCS: return d.fv * d.fv * (int64_t)d.M * d.M;
    case SRK_BUF_RCS_RHS: return d.fv * (int64_t)d.M;
    case SRK_BUF_CORRECTIONS: return 3 * d.N + d.fv * (int64_t)d.M;
    case SRK_BUF_POINTS: return 3 * d.N;
    case SRK_BUF_CAM_R: return 9 * (int64_t)d.M;
    case SRK_BUF_CAM_T: return 3 * (int64_t)d.M;
    default: return SRK_E_ARGS;
    }
}

int srk_ba_download(srk_ba* h, int which, double* dst, int64_t count)
{
    if (!h || !h->have_scene || !dst) return SRK_E_STATE;
    if (count != srk_ba_buffer_size(h, which)) { h->last_error = "download: wrong count"; return SRK_E_ARGS; }
    HIPCHK(h, hipSetDevice(h->device));
    const SrkDims& d = h->d;
    hipStream_t s = h->main_stream;
    HIPCHK(h, hipStreamSynchronize(s));
    for (int sl = 1; sl < SRK_SLOTS; ++sl) HIPCHK(h, hipStreamSynchronize(h->att[sl].stream));
    // reduced camera system, rhs and corrections: those of the last attempt the LM loop judged (or of the staged calls)
    const srk_ba::Attempt& att = h->att[h->last_slot];
    auto d2h = [&](void* dstp, const void* src, size_t bytes) -> int {
        if (bytes == 0) return SRK_OK;
        HIPCHK(h, hipMemcpy(dstp, src, bytes, hipMemcpyDeviceToHost));
        return SRK_OK;
    };
    int rc = SRK_OK;
    if (h->shk_G > 0 && (which == SRK_BUF_GRAD || which == SRK_BUF_RCS || which == SRK_BUF_RCS_RHS || which == SRK_BUF_CORRECTIONS))
        return download_shared(h, which, dst);
    switch (which) {
    case SRK_BUF_GRAD:
    case SRK_BUF_POINT_BLOCKS: {
        std::vector<double> vg((size_t)(9 * d.Ns));
        if ((rc = d2h(vg.data(), h->Vg.p, vg.size() * 8)) != SRK_OK) return rc;
        if (which == SRK_BUF_POINT_BLOCKS) {
            static const int map[9] = { 0, 1, 2, 1, 3, 4, 2, 4, 5 };
            for (int64_t i = 0; i < d.N; ++i)
                for (int e = 0; e < 9; ++e) dst[9 * h->perm[(size_t)i] + e] = vg[(size_t)(map[e] * d.Ns + i)];
            return SRK_OK;
        }
        for (int64_t i = 0; i < d.N; ++i)
            for (int e = 0; e < 3; ++e) dst[3 * h->perm[(size_t)i] + e] = vg[(size_t)((6 + e) * d.Ns + i)];
        const int ugs = SRK_UGS(d.fv), ut = d.fv * (d.fv + 1) / 2; // Ug: block upper triangle, then the gradient
        std::vector<double> ug((size_t)(ugs * (int64_t)d.M));
        if ((rc = d2h(ug.data(), h->Ug.p, ug.size() * 8)) != SRK_OK) return rc;
        for (int32_t j = 0; j < d.M; ++j)
            for (int e = 0; e < d.fv; ++e) // (constant frames report 0: their sums in Ug stay unmasked)
                dst[3 * d.N + d.fv * (int64_t)j + e] = (!h->cst.frame_int.empty() && h->cst.frame_int[(size_t)j]) ? 0.0 : ug[(size_t)(ugs * (int64_t)j + ut + e)];
        frames_to_user(h, dst + 3 * d.N, d.fv);
        return SRK_OK;
    }
    case SRK_BUF_FRAME_BLOCKS: {
        const int fv = d.fv, ugs = SRK_UGS(fv);
        std::vector<double> ug((size_t)(ugs * (int64_t)d.M));
        if ((rc = d2h(ug.data(), h->Ug.p, ug.size() * 8)) != SRK_OK) return rc;
        for (int32_t j = 0; j < d.M; ++j)
            for (int v1 = 0; v1 < fv; ++v1)
                for (int v2 = 0; v2 < fv; ++v2) {
                    int a = v1 < v2 ? v1 : v2, b = v1 < v2 ? v2 : v1;
                    dst[fv * fv * (int64_t)j + fv * v1 + v2] = ug[(size_t)(ugs * (int64_t)j + a * fv - a * (a - 1) / 2 + (b - a))];
                }
        frames_to_user(h, dst, fv * fv);
        return SRK_OK;
    }
    case SRK_BUF_POINT_FRAME: {
        const int fv3 = 3 * d.fv, off = 10 - d.fv;
        std::vector<double> w((size_t)(fv3 * d.Os));
        {
            // the library keeps the rank-2 factors (srk_dev.hpp SRK_WF_*; as floats in the f32 storage mode): the products are formed here
            std::vector<double> f((size_t)(SRK_WF_PLANES * d.Os));
            if (d.w_f32) {
                std::vector<float> ff(f.size());
                if ((rc = d2h(ff.data(), h->W.p, ff.size() * 4)) != SRK_OK) return rc;
                for (size_t i = 0; i < ff.size(); ++i) f[i] = (double)ff[i];
            } else if ((rc = d2h(f.data(), h->W.p, f.size() * 8)) != SRK_OK) return rc;
            auto F = [&](int plane, int64_t o) { return plane >= 0 ? f[(size_t)(plane * d.Os + o)] : 0.0; };
            for (int64_t o = 0; o < d.O; ++o)
                for (int pv = 0; pv < 3; ++pv)
                    for (int fv = off; fv < 10; ++fv) {
                        const int pa = fv >= 4 ? SRK_WF_AF4 + fv - 4 : (fv == 0 ? SRK_WF_AF0 : (fv == 2 ? SRK_WF_G : -1));
                        const int pb = fv >= 4 ? SRK_WF_BF4 + fv - 4 : (fv == 1 ? SRK_WF_BF1 : (fv == 3 ? SRK_WF_G : -1));
                        w[(size_t)((d.fv * pv + fv - off) * d.Os + o)] = F(SRK_WF_AP + pv, o) * F(pa, o) + F(SRK_WF_BP + pv, o) * F(pb, o);
                    }
        }
        for (int64_t i = 0; i < d.N; ++i) {
            int64_t oi = h->row_ptr_int[(size_t)i], ou = h->row_ptr_user[(size_t)h->perm[(size_t)i]];
            int64_t cnt = h->row_ptr_int[(size_t)i + 1] - oi;
            for (int64_t a = 0; a < cnt; ++a) { // the caller's observation ou + a: internal place obs_rank inside its landmark
                const int64_t ai = h->obs_rank.empty() ? a : h->obs_rank[(size_t)(ou + a)];
                for (int k = 0; k < fv3; ++k) dst[fv3 * (ou + a) + k] = w[(size_t)(k * d.Os + oi + ai)];
            }
        }
        return SRK_OK;
    }
    case SRK_BUF_RCS: {
        const int64_t fv = d.fv, n = fv * (int64_t)d.M;
        std::vector<double> row((size_t)d.ld);
        auto uvar = [&](int64_t v) { return h->frame_user.empty() ? v : fv * (int64_t)h->frame_user[(size_t)(v / fv)] + v % fv; };
        for (int64_t r = 0; r < n; ++r) {
            if ((rc = d2h(row.data(), P<double>(att.S) + r * d.ld, (size_t)(8 * n))) != SRK_OK) return rc;
            const int64_t ur = uvar(r);
            for (int64_t c = 0; c <= r; ++c) {
                const int64_t uc = uvar(c);
                dst[ur * n + uc] = row[(size_t)c];
                dst[uc * n + ur] = row[(size_t)c]; // lower triangle is authoritative
            }
        }
        return SRK_OK;
    }
    case SRK_BUF_RCS_RHS:
        if ((rc = d2h(dst, att.rhs.p, (size_t)(8 * d.fv * (int64_t)d.M))) != SRK_OK) return rc;
        frames_to_user(h, dst, d.fv);
        return SRK_OK;
    case SRK_BUF_CORRECTIONS: {
        std::vector<double> tmp((size_t)(3 * d.N));
        if ((rc = d2h(tmp.data(), att.dx.p, (size_t)(24 * d.N))) != SRK_OK) return rc;
        for (int64_t i = 0; i < d.N; ++i) std::memcpy(dst + 3 * h->perm[(size_t)i], &tmp[(size_t)(3 * i)], 24);
        if ((rc = d2h(dst + 3 * d.N, att.dc.p, (size_t)(8 * d.fv * (int64_t)d.M))) != SRK_OK) return rc;
        frames_to_user(h, dst + 3 * d.N, d.fv);
        return SRK_OK;
    }
    case SRK_BUF_POINTS: {
        std::vector<double> tmp((size_t)(3 * d.N));
        if ((rc = d2h(tmp.data(), h->pts[h->cur].p, (size_t)(24 * d.N))) != SRK_OK) return rc;
        for (int64_t i = 0; i < d.N; ++i) std::memcpy(dst + 3 * h->perm[(size_t)i], &tmp[(size_t)(3 * i)], 24);
        return SRK_OK;
    }
    case SRK_BUF_CAM_R:
        if ((rc = d2h(dst, h->camR[h->cur].p, (size_t)(72 * (int64_t)d.M))) != SRK_OK) return rc;
        frames_to_user(h, dst, 9);
        return SRK_OK;
    case SRK_BUF_CAM_T:
        if ((rc = d2h(dst, h->camT[h->cur].p, (size_t)(24 * (int64_t)d.M))) != SRK_OK) return rc;
        frames_to_user(h, dst, 3);
        return SRK_OK;
    default: return SRK_E_ARGS;
    }
}

int srk_ba_download_rcs_rows(srk_ba* h, const int64_t* rows, int64_t n_rows, double* dst)
{
    if (!h || !h->have_scene || !rows || !dst || n_rows < 0) return SRK_E_STATE;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->main_stream));
    for (int sl = 1; sl < SRK_SLOTS; ++sl) HIPCHK(h, hipStreamSynchronize(h->att[sl].stream));
    const SrkDims& d = h->d;
    if (h->shk_G > 0) {
        const int64_t n = 6 * (int64_t)d.M + 4 * (int64_t)h->shk_G;
        for (int64_t k = 0; k < n_rows; ++k) {
            if (rows[k] < 0 || rows[k] >= n) { h->last_error = "download_rcs_rows: row out of range"; return SRK_E_ARGS; }
            std::memset(dst + k * n, 0, (size_t)(8 * n));
            const int rc = shk_row(h, P<double>(h->att[h->last_slot].Ssh), rows[k], dst + k * n);
            if (rc != SRK_OK) return rc;
        }
        return SRK_OK;
    }
    const int64_t fv = d.fv, n = fv * (int64_t)d.M;
    const double* S = P<double>(h->att[h->last_slot].S);
    std::vector<double> rowi, coli;
    for (int64_t k = 0; k < n_rows; ++k) {
        const int64_t r = rows[k];
        if (r < 0 || r >= n) { h->last_error = "download_rcs_rows: row out of range"; return SRK_E_ARGS; }
        std::memset(dst + k * n, 0, (size_t)(8 * n));
        if (h->frame_int.empty()) {
            HIPCHK(h, hipMemcpy(dst + k * n, S + r * d.ld, (size_t)(8 * (r + 1)), hipMemcpyDeviceToHost));
            continue;
        }
        // reordered frames: the caller's row r is internal row ri; its entries left of the diagonal in the CALLER's order
        // lie in internal row ri (internal columns <= ri) and in internal column ri (rows > ri)
        const int64_t ri = fv * (int64_t)h->frame_int[(size_t)(r / fv)] + r % fv;
        rowi.assign((size_t)n, 0.0);
        coli.assign((size_t)n, 0.0);
        HIPCHK(h, hipMemcpy(rowi.data(), S + ri * d.ld, (size_t)(8 * (ri + 1)), hipMemcpyDeviceToHost));
        if (ri + 1 < n)
            HIPCHK(h, hipMemcpy2D(coli.data() + ri + 1, 8, S + (ri + 1) * d.ld + ri, (size_t)(8 * d.ld), 8, (size_t)(n - ri - 1), hipMemcpyDeviceToHost));
        for (int64_t ci = 0; ci < n; ++ci) {
            const int64_t c = fv * (int64_t)h->frame_user[(size_t)(ci / fv)] + ci % fv;
            if (c <= r) dst[k * n + c] = ci <= ri ? rowi[(size_t)ci] : coli[(size_t)ci];
        }
    }
    return SRK_OK;
}

// ------------------------------------------------------------------ dense SPD solve on its own

int srk_ba_dense_spd_solve(srk_ba* h, int64_t n, const double* A, const double* b, double* x, double* ms_factor)
{
    if (!h || n <= 0 || !A || !b || !x) return SRK_E_ARGS;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->main_stream;
    int64_t ld = ((n + SRK_CHOL_NB - 1) / SRK_CHOL_NB) * SRK_CHOL_NB;
    DevBuf dA, dw, dy, dx, dinfo, ddinv;
    int rc;
    if ((rc = dev_alloc(h, ddinv, (size_t)(8 * 64 * ld))) != SRK_OK) return rc;
    if ((rc = dev_alloc(h, dA, (size_t)(8 * ld * ld))) != SRK_OK) return rc;
    if ((rc = dev_alloc(h, dw, (size_t)(8 * ld))) != SRK_OK) return rc;
    if ((rc = dev_alloc(h, dy, (size_t)(8 * ld))) != SRK_OK) return rc;
    if ((rc = dev_alloc(h, dx, (size_t)(8 * ld))) != SRK_OK) return rc;
    if ((rc = dev_alloc(h, dinfo, 64)) != SRK_OK) return rc;
    std::vector<double> Ap((size_t)(ld * ld), 0.0), bp((size_t)ld, 0.0);
    for (int64_t r = 0; r < ld; ++r) {
        if (r < n) std::memcpy(&Ap[(size_t)(r * ld)], A + r * n, (size_t)(8 * n));
        else Ap[(size_t)(r * ld + r)] = 1.0;
    }
    std::memcpy(bp.data(), b, (size_t)(8 * n));
    HIPCHK(h, hipMemcpyAsync(dA.p, Ap.data(), Ap.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(dw.p, bp.data(), bp.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemsetAsync(dinfo.p, 0, 4, s));
    HIPCHK(h, hipEventRecord(h->ev[14], s));
    DevBuf dflags;
    if ((rc = dev_alloc(h, dflags, 4 * SRK_SYNC_WORDS)) != SRK_OK) return rc;
    HIPCHK(h, hipMemsetAsync(dflags.p, 0, 4 * SRK_SYNC_WORDS, s));
    SrkCholSync sync;
    sync.flags = P<unsigned>(dflags);
    sync.fused = h->chol_fused;
    srk_chol_solve(s, ld, P<double>(dA), P<double>(dw), P<double>(dy), P<double>(dx), P<int>(dinfo), nullptr, nullptr,
                   P<double>(ddinv), nullptr, &sync, n);
    HIPCHK(h, hipEventRecord(h->ev[15], s));
    HIPCHK(h, hipGetLastError());
    int info = 0;
    std::vector<double> xs(bp.size());
    HIPCHK(h, hipMemcpyAsync(xs.data(), dx.p, xs.size() * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(&info, dinfo.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (info & 8) { // a hand-off timed out (a scheduling event): the inputs again from the host copies, unfused, once
        ++h->sync_timeouts;
        sync.fused = false;
        HIPCHK(h, hipMemcpyAsync(dA.p, Ap.data(), Ap.size() * 8, hipMemcpyHostToDevice, s));
        HIPCHK(h, hipMemcpyAsync(dw.p, bp.data(), bp.size() * 8, hipMemcpyHostToDevice, s));
        HIPCHK(h, hipMemsetAsync(dinfo.p, 0, 4, s));
        srk_chol_solve(s, ld, P<double>(dA), P<double>(dw), P<double>(dy), P<double>(dx), P<int>(dinfo), nullptr, nullptr,
                       P<double>(ddinv), nullptr, &sync, n);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(xs.data(), dx.p, xs.size() * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemcpyAsync(&info, dinfo.p, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
    }
    bp.swap(xs);
    if (ms_factor) {
        float ms = 0;
        hipEventElapsedTime(&ms, h->ev[14], h->ev[15]);
        *ms_factor = ms;
    }
    std::memcpy(x, bp.data(), (size_t)(8 * n));
    dev_free(dA); dev_free(dw); dev_free(dy); dev_free(dx); dev_free(dinfo); dev_free(ddinv); dev_free(dflags);
    return info ? 1 : 0;
}

// global covisibility for sharded runs: min_cv[j] = smallest frame index that shares a landmark with frame j,
// taken over ALL ranks' landmarks.  Call after srk_ba_upload_scene.  NULL = dense (full lower triangle).
int srk_ba_set_covisibility(srk_ba* h, const int32_t* min_cv)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    HIPCHK(h, hipSetDevice(h->device));
    // a covisibility in the caller's numbering says nothing about the internal one: with a SUPPLIED frame order
    // (srk_ba_set_frame_order) min_cv is taken in that numbering, which the caller knows; an automatic one is one rank's own
    if (min_cv && !h->frame_int.empty() && !h->frame_order_supplied) {
        h->last_error = "set_covisibility: the frames of this scene were renumbered (srk_ba_set_frame_reordering 0 keeps the caller's order)";
        return SRK_E_STATE;
    }
    if (min_cv) {
        for (int32_t j = 0; j < h->d.M; ++j) {
            if (min_cv[j] < 0 || min_cv[j] > j) { h->last_error = "min_cv[j] must be in [0, j]"; return SRK_E_ARGS; }
            h->min_cv[(size_t)j] = min_cv[j];
        }
        for (size_t i = 0; i < h->rp.int_a.size(); ++i) { // the pairs of the relative-pose factors are part of the skyline
            const int32_t hi = std::max(h->rp.int_a[i], h->rp.int_b[i]), lo = std::min(h->rp.int_a[i], h->rp.int_b[i]);
            h->min_cv[(size_t)hi] = std::min(h->min_cv[(size_t)hi], lo);
        }
        for (size_t i = 0; i < h->jp.pair_a.size(); ++i) // so are the coupled pairs of the joint pose priors (lo, hi)
            h->min_cv[(size_t)h->jp.pair_b[i]] = std::min(h->min_cv[(size_t)h->jp.pair_b[i]], h->jp.pair_a[i]);
    } else {
        std::fill(h->min_cv.begin(), h->min_cv.end(), 0);
    }
    return build_envelope(h);
}

// 0 = treat the reduced camera system as dense (full lower triangle), 1 = exploit its skyline (default)
int srk_ba_set_rcs_mode(srk_ba* h, int use_envelope)
{
    if (!h) return SRK_E_ARGS;
    h->use_envelope = use_envelope != 0;
    h->use_chunks = use_envelope != 1; // 0 dense, 1 skyline in one chain, 2 (default) skyline cut into chunks
    if (h->have_scene) return build_envelope(h);
    return SRK_OK;
}

int srk_ba_rcs_chunks(srk_ba* h) { return (h && h->have_scene) ? h->att[0].plan.P : 0; }

// fraction of the lower triangle inside the skyline (1.0 = dense)
double srk_ba_rcs_fill(srk_ba* h)
{
    if (!h || !h->have_scene) return -1.0;
    double full = 0.5 * (double)h->d.ld * (double)h->d.ld;
    return (double)h->env_packed / full;
}

// flops executed by the MFMA trailing updates of one solve with the current skyline (2 flops per FMA)
double srk_ba_solve_mfma_flops(srk_ba* h)
{
    if (!h || !h->have_scene) return -1.0;
    SrkSolveProf dry;
    dry.dry = true; // walks the launch sequence of the current mode without launching anything
    return launch_solve(h, h->att[0], &dry) == SRK_OK ? dry.flops : -1.0;
}

// 1 (default) = an outer step of the blocked Cholesky is ONE launch whose workgroups hand tiles to each other (k_step256),
// 0 = the k_panel / k_upd64 launch sequence.  Each is bit-reproducible; they agree with each other to rounding
// (include/srk_ba.h).  Takes effect at once.
int srk_ba_set_solver_fusion(srk_ba* h, int on)
{
    if (!h || (on != 0 && on != 1)) return SRK_E_ARGS;
    h->chol_fused = h->chol_fused_wanted = on != 0;
    h->fusion_rearms_left = SRK_FUSION_RETRIES; // an explicit request renews the budget
    for (auto& a : h->att) a.sync.fused = h->chol_fused;
    return SRK_OK;
}
int64_t srk_ba_solver_sync_timeouts(srk_ba* h) { return h ? h->sync_timeouts : -1; }
int64_t srk_ba_iteration_log(srk_ba* h, int64_t cap, int32_t* attempts, double* ms_since_start, double* err, double* hessian_factor)
{
    if (!h) return -1;
    const int64_t n = (int64_t)h->iter_log.size();
    for (int64_t k = 0; k < n && k < cap; ++k) {
        if (attempts) attempts[k] = h->iter_log[k].attempts;
        if (ms_since_start) ms_since_start[k] = h->iter_log[k].ms;
        if (err) err[k] = h->iter_log[k].err;
        if (hessian_factor) hessian_factor[k] = h->iter_log[k].factor;
    }
    return n;
}
int srk_ba_solver_fusion(srk_ba* h) { return h ? (h->chol_fused ? 1 : 0) : -1; }

int srk_ba_set_deterministic(srk_ba* h, int on)
{
    if (!h) return SRK_E_ARGS;
    if (refuse_modes(h, h->fixed_k, on != 0, h->store_f32, h->schur_fp32, h->world, !h->igroup_user.empty())) return SRK_E_ARGS;
    h->deterministic = on != 0;
    return SRK_OK;
}
int srk_ba_deterministic(srk_ba* h) { return (h && h->have_scene && h->det_active) ? 1 : 0; }
int srk_ba_set_multi_schedule(srk_ba* h, int mode)
{
    if (!h || mode < 0 || mode > 2) return SRK_E_ARGS;
    h->dp_schedule = mode != 0;
    h->dp_force = mode == 2;
    h->dp_selfcheck_failed = false;
    return SRK_OK;
}
int srk_ba_multi_schedule(srk_ba* h)
{
    if (!h) return -1;
    if (h->dp_selfcheck_failed) return 3;
    if (!h->dp_schedule) return 0;
    return h->dp_verified ? 2 : 1;
}
int srk_ba_set_speculation(srk_ba* h, int on)
{
    if (!h || (on != 0 && on != 1)) return SRK_E_ARGS;
    h->speculate = on != 0; // takes effect at the next upload (the second attempt slot is allocated there)
    return SRK_OK;
}

// internal frame order (srk_frame_reorder, srk_plan.cpp): -1 = automatic (renumber when the caller's order is far from banded), 0 = never,
// 1 = whenever reverse Cuthill-McKee gives another order than the caller's; takes effect at the next upload
int srk_ba_set_frame_reordering(srk_ba* h, int mode)
{
    if (!h || mode < -1 || mode > 1) return SRK_E_ARGS;
    h->frame_order_mode = mode;
    return SRK_OK;
}
// the numbering to use at the next upload instead of the automatic one (NULL: automatic again); with landmark shards every
// rank must be given the same one, found on the WHOLE scene (srk_frame_order)
int srk_ba_set_frame_order(srk_ba* h, const int32_t* to_internal, int32_t n_frames)
{
    if (!h || (to_internal && n_frames < 1)) return SRK_E_ARGS;
    if (!to_internal) { h->frame_order_given.clear(); return SRK_OK; }
    std::vector<char> hit((size_t)n_frames, 0);
    for (int32_t j = 0; j < n_frames; ++j) {
        if (to_internal[j] < 0 || to_internal[j] >= n_frames || hit[(size_t)to_internal[j]]) { h->last_error = "set_frame_order: not a permutation"; return SRK_E_ARGS; }
        hit[(size_t)to_internal[j]] = 1;
    }
    h->frame_order_given.assign(to_internal, to_internal + n_frames);
    return SRK_OK;
}
// 1 = the uploaded scene's frames are stored in another order (to_internal[caller's frame] filled when not NULL), 0 = the caller's order
int srk_ba_frame_order(srk_ba* h, int32_t* to_internal)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    for (int32_t j = 0; to_internal && j < h->d.M; ++j) to_internal[j] = h->frame_int.empty() ? j : h->frame_int[(size_t)j];
    return h->frame_int.empty() ? 0 : 1;
}
// the ordering alone (host only, no device needed): what srk_ba_upload_scene would decide for these tracks
int srk_frame_order(int mode, int64_t N, int32_t M, const int64_t* row_ptr, const int32_t* obs_frame, int32_t* to_internal)
{
    if (N < 0 || M < 1 || !row_ptr || (row_ptr[N] > 0 && !obs_frame) || !to_internal) return SRK_E_ARGS;
    std::vector<int32_t> to_int;
    const bool on = srk_frame_reorder(mode, N, M, row_ptr, obs_frame, to_int);
    for (int32_t j = 0; j < M; ++j) to_internal[j] = on ? to_int[(size_t)j] : j;
    return on ? 1 : 0;
}

// -1 = automatic (run-based kernel when the runs of identical frame lists are long enough), 0 = per-observation kernels
// only, 1 = run-based (uniform runs) whenever the scene allows it, 2 = run-based over frame unions (the ragged-track form)
// whenever the scene allows it; takes effect at the next upload.  For A/B runs and for the parity tests of both kernels on the same scene.
int srk_ba_set_jacobian_mode(srk_ba* h, int mode)
{
    if (!h || mode < -1 || mode > 2) return SRK_E_ARGS;
    h->jac_mode = mode;
    return SRK_OK;
}
int srk_ba_jacobian_kernel(srk_ba* h) { return (h && h->have_scene) ? (h->jac_runs ? (h->jac_runs_masked ? 3 : 2) : (h->jac_fused ? 1 : 0)) : -1; }

// 0 = everything stored in fp64 (default, the reference's Scalar = double); 1 = the point-frame blocks W -- 240 of the
// 260 bytes per observation the derivative kernel writes and the Schur and back-substitution kernels read -- are stored
// as float and widened on load; every sum, the reduced camera system and the solve stay fp64.  Next upload.
int srk_ba_set_storage_precision(srk_ba* h, int f32)
{
    if (!h || (f32 != 0 && f32 != 1)) return SRK_E_ARGS;
    if (refuse_modes(h, h->fixed_k, h->deterministic, f32 != 0, h->schur_fp32, h->world, !h->igroup_user.empty())) return SRK_E_ARGS;
    h->store_f32 = f32 != 0;
    return SRK_OK;
}

int srk_ba_set_schur_precision(srk_ba* h, int fp32)
{
    if (!h || (fp32 != 0 && fp32 != 1)) return SRK_E_ARGS;
    if (refuse_modes(h, h->fixed_k, h->deterministic, h->store_f32, fp32 != 0, h->world, !h->igroup_user.empty())) return SRK_E_ARGS;
    h->schur_fp32 = fp32 != 0;
    return SRK_OK;
}

// calibrated bundle adjustment: the intrinsics are constants, six variables per frame (bundle-adj-kanatani.h:113-118);
// next upload.  1 = on, 0 = the reference's ten variables (default)
int srk_ba_set_fixed_intrinsics(srk_ba* h, int on)
{
    if (!h || (on != 0 && on != 1)) return SRK_E_ARGS;
    if (refuse_modes(h, on != 0, h->deterministic, h->store_f32, h->schur_fp32, h->world, !h->igroup_user.empty())) return SRK_E_ARGS;
    h->fixed_k = on != 0;
    return SRK_OK;
}
int srk_ba_frame_vars(srk_ba* h)
{
    if (!h) return SRK_E_ARGS;
    if (h->have_scene) return h->shk_G > 0 ? 6 : h->d.fv;
    return (h->fixed_k || !h->igroup_user.empty()) ? 6 : 10;
}

// shared intrinsics: group[caller's frame] in [0, n_groups), every group used; NULL = off.  Next upload.
int srk_ba_set_intrinsic_groups(srk_ba* h, const int32_t* group, int32_t n_frames, int32_t n_groups)
{
    if (!h) return SRK_E_ARGS;
    if (!group) {
        h->igroup_user.clear();
        h->igroup_n = 0;
        return SRK_OK;
    }
    if (n_groups < 1 || n_groups > SRK_SHK_MAX_GROUPS) { h->last_error = "intrinsic groups: the number of groups must be 1..32"; return SRK_E_ARGS; }
    if (n_frames < 1) { h->last_error = "intrinsic groups: need at least one frame"; return SRK_E_ARGS; }
    std::vector<int32_t> used((size_t)n_groups, 0);
    for (int32_t j = 0; j < n_frames; ++j) {
        if (group[j] < 0 || group[j] >= n_groups) { h->last_error = "intrinsic groups: a group id is out of range"; return SRK_E_ARGS; }
        used[(size_t)group[j]] = 1;
    }
    for (int32_t g = 0; g < n_groups; ++g)
        if (!used[(size_t)g]) { h->last_error = "intrinsic groups: a group has no frame"; return SRK_E_ARGS; }
    if (refuse_modes(h, h->fixed_k, h->deterministic, h->store_f32, h->schur_fp32, h->world, true)) return SRK_E_ARGS;
    h->igroup_user.assign(group, group + n_frames);
    h->igroup_n = n_groups;
    return SRK_OK;
}
int srk_ba_intrinsic_groups(srk_ba* h)
{
    if (!h) return SRK_E_ARGS;
    return h->have_scene ? h->shk_G : h->igroup_n;
}
int srk_ba_download_intrinsics(srk_ba* h, double* K, int32_t n_groups)
{
    if (!h || !K) return SRK_E_ARGS;
    if (!h->have_scene || h->shk_G == 0) { h->last_error = "download_intrinsics: the uploaded scene has no intrinsic groups"; return SRK_E_ARGS; }
    if (n_groups != h->shk_G) { h->last_error = "download_intrinsics: wrong number of groups"; return SRK_E_ARGS; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->main_stream));
    for (int sl = 1; sl < SRK_SLOTS; ++sl) HIPCHK(h, hipStreamSynchronize(h->att[sl].stream));
    for (int32_t g = 0; g < n_groups; ++g) {
        const int32_t fi = h->shk_first[(size_t)g]; // internal frame
        double* k = K + 9 * (int64_t)g;
        HIPCHK(h, hipMemcpy(k, P<double>(h->Ks[h->cur]) + 9 * (int64_t)fi, 72, hipMemcpyDeviceToHost));
        const double k22 = h->shk_k22_user[(size_t)(h->frame_user.empty() ? fi : h->frame_user[(size_t)fi])];
        const double s = k22 / h->f0; // back to the caller's convention
        for (int e = 0; e < 8; ++e) k[e] *= s;
        k[8] = k22;
    }
    return SRK_OK;
}
// constant parameter blocks: flags in the caller's numbering, non-zero = constant; both NULL = none
// (default).  Next upload.
int srk_ba_set_constant_blocks(srk_ba* h, const uint8_t* frame_const, int32_t n_frames, const uint8_t* point_const, int64_t n_points,
                               int keep_gauge)
{
    if (!h) return SRK_E_ARGS;
    if (!frame_const && !point_const) {
        h->cst.set = SrkConstSetting{};
        return SRK_OK;
    }
    if (keep_gauge != 0 && keep_gauge != 1) { h->last_error = "constant blocks: keep_gauge must be 0 or 1"; return SRK_E_ARGS; }
    if (frame_const && n_frames < 1) { h->last_error = "constant blocks: need at least one frame"; return SRK_E_ARGS; }
    if (point_const && n_points < 0) { h->last_error = "constant blocks: negative number of landmarks"; return SRK_E_ARGS; }
    if (refuse_setting(h, "constant blocks")) return SRK_E_ARGS;
    bool all_frames = frame_const != nullptr, all_points = point_const != nullptr;
    for (int32_t j = 0; frame_const && j < n_frames; ++j) all_frames = all_frames && frame_const[j] != 0;
    for (int64_t i = 0; point_const && i < n_points; ++i) all_points = all_points && point_const[i] != 0;
    if (all_frames && all_points) { h->last_error = "constant blocks: every frame and every landmark is constant, nothing is left to solve"; return SRK_E_ARGS; }
    SrkConstSetting& s = h->cst.set;
    s.frames.clear();
    s.points.clear();
    if (frame_const) s.frames.assign(frame_const, frame_const + n_frames);
    if (point_const) s.points.assign(point_const, point_const + n_points);
    for (auto& f : s.frames) f = f ? 1 : 0;
    for (auto& f : s.points) f = f ? 1 : 0;
    s.keep_gauge = keep_gauge;
    s.set = true;
    return SRK_OK;
}
int srk_ba_constant_blocks(srk_ba* h, uint8_t* frame_const, uint8_t* point_const, int* keep_gauge)
{
    if (!h) return SRK_E_ARGS;
    if (keep_gauge) *keep_gauge = h->cst.set.keep_gauge;
    copy_out(frame_const, h->cst.set.frames);
    copy_out(point_const, h->cst.set.points);
    return h->cst.set.set ? 1 : 0;
}
int srk_ba_constant_counts(srk_ba* h, int32_t* n_frames, int64_t* n_points)
{
    if (!h) return SRK_E_ARGS;
    if (n_frames) *n_frames = (int32_t)h->cst.set.frames.size();
    if (n_points) *n_points = (int64_t)h->cst.set.points.size();
    return h->cst.set.set ? 1 : 0;
}
int srk_ba_constant_pass_ms(srk_ba* h, double* points_ms, double* frames_ms)
{
    double* const out[2] = { points_ms, frames_ms };
    return pass_ms(h, h ? h->cst.pass : nullptr, 2, out);
}
// position priors.  Next upload.
int srk_ba_set_position_priors(srk_ba* h, int64_t n_point_priors, const int64_t* point_index, const double* point_pos,
                               const double* point_info, int32_t n_frame_priors, const int32_t* frame_index,
                               const double* frame_centre, const double* frame_info, int keep_gauge)
{
    if (!h) return SRK_E_ARGS;
    if (n_point_priors == 0 && n_frame_priors == 0) {
        h->pri.set = SrkPriorSetting{};
        return SRK_OK;
    }
    if (keep_gauge != 0 && keep_gauge != 1) { h->last_error = "position priors: keep_gauge must be 0 or 1"; return SRK_E_ARGS; }
    if (n_point_priors < 0 || n_frame_priors < 0) { h->last_error = "position priors: negative count"; return SRK_E_ARGS; }
    if ((n_point_priors > 0 && (!point_index || !point_pos || !point_info)) || (n_frame_priors > 0 && (!frame_index || !frame_centre || !frame_info))) {
        h->last_error = "position priors: null array";
        return SRK_E_ARGS;
    }
    if (refuse_setting(h, "position priors")) return SRK_E_ARGS;
    for (int64_t i = 0; i < n_point_priors; ++i)
        if (point_index[i] < 0 || point_index[i] > 2147483000LL || (i > 0 && point_index[i - 1] >= point_index[i])) {
            h->last_error = "position priors: landmark indices must be non-negative and strictly ascending";
            return SRK_E_ARGS;
        }
    for (int32_t i = 0; i < n_frame_priors; ++i)
        if (frame_index[i] < 0 || (i > 0 && frame_index[i - 1] >= frame_index[i])) {
            h->last_error = "position priors: frame indices must be non-negative and strictly ascending";
            return SRK_E_ARGS;
        }
    const char* e = srk_check_prior_values(n_point_priors, point_pos, point_info);
    if (!e) e = srk_check_prior_values(n_frame_priors, frame_centre, frame_info);
    if (e) { h->last_error = e; return SRK_E_ARGS; }
    SrkPriorSetting& s = h->pri.set;
    s.pt_idx.assign(point_index, point_index + n_point_priors);
    s.pt_pos.assign(point_pos, point_pos + 3 * n_point_priors);
    s.pt_info.assign(point_info, point_info + 6 * n_point_priors);
    s.fr_idx.assign(frame_index, frame_index + n_frame_priors);
    s.fr_pos.assign(frame_centre, frame_centre + 3 * (int64_t)n_frame_priors);
    s.fr_info.assign(frame_info, frame_info + 6 * (int64_t)n_frame_priors);
    s.keep_gauge = keep_gauge;
    s.set = true;
    return SRK_OK;
}
int srk_ba_position_prior_counts(srk_ba* h, int64_t* n_point_priors, int32_t* n_frame_priors)
{
    if (!h) return SRK_E_ARGS;
    if (n_point_priors) *n_point_priors = (int64_t)h->pri.set.pt_idx.size();
    if (n_frame_priors) *n_frame_priors = (int32_t)h->pri.set.fr_idx.size();
    return h->pri.set.set ? 1 : 0;
}
int srk_ba_position_priors(srk_ba* h, int64_t* point_index, double* point_pos, double* point_info, int32_t* frame_index,
                           double* frame_centre, double* frame_info, int* keep_gauge)
{
    if (!h) return SRK_E_ARGS;
    const SrkPriorSetting& s = h->pri.set;
    copy_out(point_index, s.pt_idx); copy_out(point_pos, s.pt_pos); copy_out(point_info, s.pt_info);
    copy_out(frame_index, s.fr_idx); copy_out(frame_centre, s.fr_pos); copy_out(frame_info, s.fr_info);
    if (keep_gauge) *keep_gauge = s.keep_gauge;
    return s.set ? 1 : 0;
}
int srk_ba_prior_error(srk_ba* h, double* e_points, double* e_frames)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    if (e_points) *e_points = 0;
    if (e_frames) *e_frames = 0;
    SrkPrior pr;
    if (!position_priors(h, pr)) return SRK_OK;
    double out2[2] = { 0, 0 };
    const int rc = error_pass(h, srk_prior_partials(pr.n_pts, pr.n_frames), 2, out2, [&](hipStream_t s, double* partial, double* sums) {
        srk_launch_prior_error(s, P<double>(h->pts[h->cur]), P<double>(h->cam[h->cur]), pr, partial, sums);
    });
    if (rc != SRK_OK) return rc;
    if (e_points) *e_points = out2[0];
    if (e_frames) *e_frames = out2[1];
    return SRK_OK;
}
int srk_ba_prior_residuals(srk_ba* h, double* d_points, double* d_frames)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    // the offsets belong to the setting the resident scene was uploaded with: a setter call since then has not reached the
    // scene (srk_ba_prior_error still sums the uploaded lists), so the two must not be mixed
    if (!h->pri.app.is(h->pri.set)) {
        h->last_error = "prior_residuals: the position priors were changed after the upload; upload the scene again";
        return SRK_E_STATE;
    }
    if (h->pri.app.pt_idx.empty() && h->pri.app.fr_idx.empty()) return SRK_OK;
    WorldScene w(h);
    if (w.rc != SRK_OK) return w.rc;
    srk_prior_residuals(h->pri.app, w.pts.data(), w.R.data(), w.T.data(), d_points, d_frames);
    return SRK_OK;
}
int srk_ba_prior_pass_ms(srk_ba* h, double* derivative_ms, double* error_ms)
{
    double* const out[2] = { derivative_ms, error_ms };
    return pass_ms(h, h ? h->pri.pass : nullptr, 2, out);
}
// relative-pose factors.  Next upload.
int srk_ba_check_relative_pose_factors(int32_t n, const int32_t* frame_a, const int32_t* frame_b, const double* rel_R,
                                       const double* rel_t, const double* info, const char** why)
{
    const char* e = nullptr;
    if (n < 0) e = "relative-pose factors: negative count";
    else if (n > 0 && (!frame_a || !frame_b || !rel_R || !rel_t || !info)) e = "relative-pose factors: null array";
    else e = srk_check_relpose(n, frame_a, frame_b, rel_R, rel_t, info);
    if (why) *why = e;
    return e ? SRK_E_ARGS : SRK_OK;
}
int srk_ba_set_relative_pose_factors(srk_ba* h, int32_t n, const int32_t* frame_a, const int32_t* frame_b, const double* rel_R,
                                     const double* rel_t, const double* info)
{
    if (!h) return SRK_E_ARGS;
    if (n == 0) {
        h->rp.set = SrkRelPoseSetting{};
        return SRK_OK;
    }
    const char* e = nullptr;
    if (srk_ba_check_relative_pose_factors(n, frame_a, frame_b, rel_R, rel_t, info, &e) != SRK_OK) { h->last_error = e; return SRK_E_ARGS; }
    if (refuse_setting(h, "relative-pose factors")) return SRK_E_ARGS;
    SrkRelPoseSetting& s = h->rp.set;
    s.a.assign(frame_a, frame_a + n);
    s.b.assign(frame_b, frame_b + n);
    s.R.assign(rel_R, rel_R + 9 * (int64_t)n);
    s.t.assign(rel_t, rel_t + 3 * (int64_t)n);
    s.info.assign(info, info + 21 * (int64_t)n);
    s.set = true;
    return SRK_OK;
}
int srk_ba_relative_pose_factor_count(srk_ba* h, int32_t* n)
{
    if (!h) return SRK_E_ARGS;
    if (n) *n = (int32_t)h->rp.set.a.size();
    return h->rp.set.set ? 1 : 0;
}
int srk_ba_relative_pose_factors(srk_ba* h, int32_t* frame_a, int32_t* frame_b, double* rel_R, double* rel_t, double* info)
{
    if (!h) return SRK_E_ARGS;
    const SrkRelPoseSetting& s = h->rp.set;
    copy_out(frame_a, s.a); copy_out(frame_b, s.b); copy_out(rel_R, s.R); copy_out(rel_t, s.t); copy_out(info, s.info);
    return s.set ? 1 : 0;
}
int srk_ba_relative_pose_error(srk_ba* h, double* e_out)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    if (e_out) *e_out = 0;
    SrkRelPose rp;
    if (!relpose_factors(h, rp)) return SRK_OK;
    double out = 0;
    const int rc = error_pass(h, srk_relpose_partials(rp.n), 1, &out, [&](hipStream_t s, double* partial, double* sum) {
        srk_launch_relpose_error(s, P<double>(h->cam[h->cur]), rp, partial, sum);
    });
    if (rc != SRK_OK) return rc;
    if (e_out) *e_out = out;
    return SRK_OK;
}
int srk_ba_relative_pose_residuals(srk_ba* h, double* r_out)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    // the residuals belong to the setting the resident scene was uploaded with: a setter call since then has not reached it
    if (!h->rp.app.is(h->rp.set)) {
        h->last_error = "relative_pose_residuals: the factors were changed after the upload; upload the scene again";
        return SRK_E_STATE;
    }
    if (h->rp.app.a.empty() || !r_out) return SRK_OK;
    WorldScene w(h);
    if (w.rc != SRK_OK) return w.rc;
    srk_relpose_residuals(h->rp.app, w.R.data(), w.T.data(), r_out);
    return SRK_OK;
}
int srk_ba_relative_pose_pass_ms(srk_ba* h, double* derivative_ms, double* couple_ms, double* error_ms)
{
    double* const out[3] = { derivative_ms, couple_ms, error_ms };
    return pass_ms(h, h ? h->rp.pass : nullptr, 3, out);
}
// joint Gaussian pose priors over sets of frames.  Next upload.
int srk_ba_check_joint_pose_priors(int32_t n_sets, const int32_t* set_ptr, const int32_t* frame, const double* lin_R, const double* lin_C,
                                   const double* mean, const double* info, int keep_gauge, const char** why)
{
    const char* e = nullptr;
    if (n_sets < 0) e = "joint pose priors: negative count";
    else if (n_sets > 0 && (!set_ptr || !frame || !lin_R || !lin_C || !info)) e = "joint pose priors: null array";
    else if (n_sets > 0) e = srk_check_jprior(n_sets, set_ptr, frame, lin_R, lin_C, mean, info, keep_gauge);
    if (why) *why = e;
    return e ? SRK_E_ARGS : SRK_OK;
}
int srk_ba_set_joint_pose_priors(srk_ba* h, int32_t n_sets, const int32_t* set_ptr, const int32_t* frame, const double* lin_R,
                                 const double* lin_C, const double* mean, const double* info, int keep_gauge)
{
    if (!h) return SRK_E_ARGS;
    if (n_sets == 0) {
        h->jp.set = SrkJPriorSetting{};
        return SRK_OK;
    }
    const char* e = nullptr;
    if (srk_ba_check_joint_pose_priors(n_sets, set_ptr, frame, lin_R, lin_C, mean, info, keep_gauge, &e) != SRK_OK) { h->last_error = e; return SRK_E_ARGS; }
    if (refuse_setting(h, "joint pose priors")) return SRK_E_ARGS;
    const int64_t nq = set_ptr[n_sets];
    int64_t ni = 0;
    for (int32_t g = 0; g < n_sets; ++g) ni += 36 * (int64_t)(set_ptr[g + 1] - set_ptr[g]) * (set_ptr[g + 1] - set_ptr[g]);
    SrkJPriorSetting& s = h->jp.set;
    s.ptr.assign(set_ptr, set_ptr + n_sets + 1);
    s.frame.assign(frame, frame + nq);
    s.R.assign(lin_R, lin_R + 9 * nq);
    s.C.assign(lin_C, lin_C + 3 * nq);
    if (mean) s.mean.assign(mean, mean + 6 * nq);
    else s.mean.assign((size_t)(6 * nq), 0.0);
    s.info.assign(info, info + ni);
    for (int32_t g = 0; g < n_sets; ++g) // stored symmetrised
        srk_symmetrise(const_cast<double*>(s.info_of((size_t)g)), 6 * (int64_t)(set_ptr[g + 1] - set_ptr[g]));
    s.keep_gauge = keep_gauge;
    s.set = true;
    return SRK_OK;
}
int srk_ba_joint_pose_prior_counts(srk_ba* h, int32_t* n_sets, int32_t* n_frames, int64_t* n_info)
{
    if (!h) return SRK_E_ARGS;
    const SrkJPriorSetting& s = h->jp.set;
    if (n_sets) *n_sets = s.set ? (int32_t)s.ptr.size() - 1 : 0;
    if (n_frames) *n_frames = (int32_t)s.frame.size();
    if (n_info) *n_info = (int64_t)s.info.size();
    return s.set ? 1 : 0;
}
int srk_ba_joint_pose_priors(srk_ba* h, int32_t* set_ptr, int32_t* frame, double* lin_R, double* lin_C, double* mean, double* info,
                             int* keep_gauge)
{
    if (!h) return SRK_E_ARGS;
    const SrkJPriorSetting& s = h->jp.set;
    copy_out(set_ptr, s.ptr); copy_out(frame, s.frame); copy_out(lin_R, s.R); copy_out(lin_C, s.C); copy_out(mean, s.mean); copy_out(info, s.info);
    if (keep_gauge) *keep_gauge = s.keep_gauge;
    return s.set ? 1 : 0;
}
int srk_ba_joint_pose_prior_error(srk_ba* h, double* e_out)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    if (e_out) *e_out = 0;
    SrkJointPrior jp;
    if (!joint_priors(h, jp)) return SRK_OK;
    double out = 0;
    const int rc = error_pass(h, srk_jprior_partials(jp.n_sets), 1, &out, [&](hipStream_t s, double* partial, double* sum) {
        srk_launch_jprior_error(s, P<double>(h->cam[h->cur]), jp, partial, sum);
    });
    if (rc != SRK_OK) return rc;
    if (e_out) *e_out = out;
    return SRK_OK;
}
int srk_ba_joint_pose_prior_residuals(srk_ba* h, double* r_out)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    // the residuals belong to the setting the resident scene was uploaded with: a setter call since then has not reached it
    if (!h->jp.app.is(h->jp.set)) {
        h->last_error = "joint_pose_prior_residuals: the priors were changed after the upload; upload the scene again";
        return SRK_E_STATE;
    }
    if (h->jp.app.frame.empty() || !r_out) return SRK_OK;
    WorldScene w(h);
    if (w.rc != SRK_OK) return w.rc;
    srk_jprior_residuals(h->jp.app, w.R.data(), w.T.data(), r_out);
    return SRK_OK;
}
int srk_ba_joint_pose_prior_pass_ms(srk_ba* h, double* derivative_ms, double* couple_ms, double* error_ms)
{
    double* const out[3] = { derivative_ms, couple_ms, error_ms };
    return pass_ms(h, h ? h->jp.pass : nullptr, 3, out);
}
int64_t srk_ba_schur_fallback_landmarks(srk_ba* h)
{
    if (!h || !h->have_scene) return SRK_E_STATE;
    return h->d.fv == 6 ? h->n_cal_list : h->n_generic;
}

// robust loss: 0 none (plain least squares, the reference's objective), 1 Huber, 2 Cauchy, with the
// scale delta in pixels.  Takes effect at the next optimise / phase call; the scene, skyline and plan stay as they are.
int srk_ba_set_robust_loss(srk_ba* h, int kind, double delta_pixels)
{
    if (!h) return SRK_E_ARGS;
    if (kind < SRK_LOSS_NONE || kind > SRK_LOSS_CAUCHY) { h->last_error = "set_robust_loss: unknown loss kind"; return SRK_E_ARGS; }
    if (kind != SRK_LOSS_NONE && !(std::isfinite(delta_pixels) && delta_pixels > 0)) {
        h->last_error = "set_robust_loss: delta must be finite and positive";
        return SRK_E_ARGS;
    }
    h->loss_kind = kind;
    h->loss_delta_pix = kind == SRK_LOSS_NONE ? 0.0 : delta_pixels;
    return SRK_OK;
}
int srk_ba_robust_loss(srk_ba* h, int* kind, double* delta_pixels)
{
    if (!h) return SRK_E_ARGS;
    if (kind) *kind = h->loss_kind;
    if (delta_pixels) *delta_pixels = h->loss_delta_pix;
    return SRK_OK;
}
// the IRLS weights of the resident scene's observations in the caller's order (the CSR order of the upload); all 1
// without a loss.  Scene of this rank: count = its observations.
int srk_ba_observation_weights(srk_ba* h, double* w, int64_t count)
{
    if (!h || !h->have_scene || !w) return SRK_E_STATE;
    const SrkDims& d = h->d;
    if (count != d.O) { h->last_error = "observation_weights: count must be the number of observations"; return SRK_E_ARGS; }
    if (d.O == 0) return SRK_OK;
    SrkLoss Ls;
    const SrkLoss* L = robust_loss(h, Ls);
    if (!L || L->kind == SRK_LOSS_NONE) { // (information alone: the loss's factor is 1)
        std::fill(w, w + d.O, 1.0);
        return SRK_OK;
    }
    std::vector<double> wi((size_t)d.O);
    const int rc = error_pass(h, 0, (int64_t)d.O, wi.data(), [&](hipStream_t s, double*, double* out) {
        srk_launch_obs_weights(s, d, P<double>(h->pts[h->cur]), P<double>(h->cam[h->cur]), P<int32_t>(h->obs_frame),
                               P<int32_t>(h->obs_pt), P<double>(h->obs_uv), *L, out);
    });
    if (rc != SRK_OK) return rc;
    const std::vector<int64_t> at = srk_observation_places(*h, d.N, d.O); // internal order -> the caller's
    for (int64_t o = 0; o < d.O; ++o) w[o] = wi[(size_t)at[(size_t)o]];
    return SRK_OK;
}

// per-observation information: q[o] >= 0 multiplies observation o's squared residual, E = sum rho(q s).
// q in the caller's observation order (the CSR order of the upload), NULL = none.  The handle keeps a copy: it is applied by
// every later upload and survives srk_ba_reset_scene; with a scene resident it takes effect at the next optimise / phase
// call, without another upload.  A refused call (SRK_E_ARGS) leaves the previous setting in force.
int srk_ba_set_observation_information(srk_ba* h, const double* q, int64_t count)
{
    if (!h) return SRK_E_ARGS;
    if (!q) {
        h->obs_info.set.q.clear();
        h->obs_info.on = false;
        return SRK_OK;
    }
    try {
        if (count < 0) { h->last_error = "set_observation_information: negative count"; return SRK_E_ARGS; }
        if (h->have_scene) {
            if (check_information(h, "set_observation_information", q, count, h->d.N, h->row_ptr_user.data()) != SRK_OK) return SRK_E_ARGS;
        } else {
            for (int64_t o = 0; o < count; ++o)
                if (!(std::isfinite(q[o]) && q[o] >= 0)) {
                    h->last_error = "set_observation_information: observation information must be finite and not negative (observation " + std::to_string(o) + ")";
                    return SRK_E_ARGS;
                }
        }
        std::vector<double> keep(q, q + count);
        if (!h->have_scene) {
            h->obs_info.set.q.swap(keep);
            return SRK_OK;
        }
        for (auto& a : h->att) // nothing of an earlier call may still read the values on the device
            if (a.allocated && a.stream) HIPCHK(h, hipStreamSynchronize(a.stream));
        h->obs_info.set.q.swap(keep);
        const bool was_on = h->obs_info.on;
        const int rc = apply_information(h);
        if (rc != SRK_OK) { // (device failure: back to the previous values)
            h->obs_info.set.q.swap(keep);
            h->obs_info.on = false;
            if (was_on) apply_information(h);
        }
        return rc;
    } catch (const std::bad_alloc&) {
        h->last_error = "set_observation_information: out of host memory";
        return SRK_E_NOMEM;
    }
}
// the setting in the caller's order; all 1 when none is set
int srk_ba_observation_information(srk_ba* h, double* q, int64_t count)
{
    if (!h || !q) return SRK_E_ARGS;
    const int64_t want = !h->obs_info.set.q.empty() ? (int64_t)h->obs_info.set.q.size() : (h->have_scene ? h->d.O : count);
    if (count != want) { h->last_error = "observation_information: count must be the number of observations"; return SRK_E_ARGS; }
    if (h->obs_info.set.q.empty()) std::fill(q, q + count, 1.0);
    else std::copy(h->obs_info.set.q.begin(), h->obs_info.set.q.end(), q);
    return SRK_OK;
}
// the raw residuals f0 (ex, ey) in pixels of the resident scene's observations, [count][2] in the caller's order; neither
// information nor a loss touches them.  After srk_ba_optimize: the residuals of the result.
int srk_ba_observation_residuals(srk_ba* h, double* exy_pixels, int64_t count)
{
    if (!h || !h->have_scene || !exy_pixels) return SRK_E_STATE;
    const SrkDims& d = h->d;
    if (count != d.O) { h->last_error = "observation_residuals: count must be the number of observations"; return SRK_E_ARGS; }
    if (d.O == 0) return SRK_OK;
    std::vector<double> ei((size_t)(2 * d.O));
    const int rc = error_pass(h, 0, 2 * (int64_t)d.O, ei.data(), [&](hipStream_t s, double*, double* out) {
        srk_launch_obs_residuals(s, d, P<double>(h->pts[h->cur]), P<double>(h->cam[h->cur]), P<int32_t>(h->obs_frame),
                                 P<int32_t>(h->obs_pt), P<double>(h->obs_uv), out);
    });
    if (rc != SRK_OK) return rc;
    const std::vector<int64_t> at = srk_observation_places(*h, d.N, d.O); // internal order -> the caller's
    for (int64_t o = 0; o < d.O; ++o) std::memcpy(exy_pixels + 2 * o, &ei[(size_t)(2 * at[(size_t)o])], 16);
    return SRK_OK;
}

// knob for bench.py: event pairs around every MFMA trailing-update launch (report.ms_solve_syrk)
int srk_ba_set_profile(srk_ba* h, int level)
{
    if (!h || level < 0 || level > 2) return SRK_E_ARGS;
    h->profile_level = level;
    return SRK_OK;
}

} // extern "C"
