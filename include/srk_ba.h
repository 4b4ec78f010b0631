/*
 * srk_ba.h -- C ABI of the MI355X-native bundle-adjustment core (libsrk_ba.so).
 *
 * Drop-in boundary for whigg/surikatoko's BundleAdjustmentKanatani
 * (cpp_impl/suriko-engine/include/suriko/bundle-adj-kanatani.h:165-193).  The reference has no
 * FFI layer: its boundary is the C++ class API.  These entry points are what a thin adapter with
 * that class's signature binds (see include/suriko_amd/bundle-adj-kanatani.hpp and INTEGRATION.md):
 *
 *   reference (file:line)                                       C ABI
 *   ----------------------------------------------------------  ------------------------------------
 *   BundleAdjustmentKanatani::ComputeInplace  .h:179-184        srk_ba_compute_inplace
 *   BundleAdjustmentKanatani::ReprojError     .h:167-172        srk_ba_reproj_error
 *   ...::OptimizationStatusString             .h:193            srk_ba_status_string
 *   NormalizeSceneInplace / SceneNormalizer   .h:16-62          srk_ba_normalize_scene / srk_ba_revert_normalization
 *   CheckWorldIsNormalized                    .h:64-65          srk_ba_check_world_is_normalized
 *   BundleAdjustmentKanataniTermCriteria      .h:68-92          the two optional-double pointers
 *
 * Flat, caller-owned, row-major doubles; no exceptions cross the ABI; one srk_ba per thread/GPU.
 *   points      [N][3]   world coordinates, index = pnt_ind (order of reconstructed tracks, .cpp:1161-1169)
 *   cam_R,cam_T [M][9],[M][3]  world->camera ("inverse orientation", as on the reference API)
 *   K           [M][9] or [1][9] when shared_k != 0 (exactly one of shared_K / Ks in the reference, .cpp:421)
 *   obs_row_ptr [N+1] int64; obs_frame [O] int32 strictly ascending inside a point; obs_uv [O][2] pixels
 * Per-frame variable order [fx fy u0 v0 Tx Ty Tz Wx Wy Wz] (bundle-adj-kanatani.h:113-118).
 *
 * Return convention of the optimisation calls: 0 = optimised (reference `true`), 1 = not optimised
 * (reference `false`, see report.status), negative = SRK_E_* argument / device error.
 */
#ifndef SRK_BA_H
#define SRK_BA_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct srk_ba srk_ba; /* opaque: owns device buffers, stream, events */

enum srk_status {
    SRK_STATUS_NONE = 0,               /* "" : normalisation failed (.cpp:681-682) or not run */
    SRK_STATUS_ABS_ERR_THRESHOLD = 1,  /* "abs err threshold"           -> true  (.cpp:749-753) */
    SRK_STATUS_SMALL_ERR_CHANGE = 2,   /* "small relative err change"   -> true  (.cpp:880-884) */
    SRK_STATUS_HESSIAN_OVERFLOW = 3,   /* "hessian overflow"            -> false (.cpp:843-847,866) */
    SRK_STATUS_ERR_CONVERGED = 4,      /* "err converged to limit value"-> false (.cpp:828-838,868) */
    SRK_STATUS_MAX_ITERATIONS = 5,     /* harness addition (the reference has no cap, .cpp:756) */
    SRK_STATUS_DEVICE_ERROR = 6        /* "device error" */
};

enum srk_error {
    SRK_OK = 0,
    SRK_E_ARGS = -1,     /* bad argument (f0 ~ 0, M < 2, NULL arrays, unsorted frames, ...) */
    SRK_E_DEVICE = -2,   /* HIP error, see srk_ba_last_error */
    SRK_E_STATE = -3,    /* staged call without an uploaded scene */
    SRK_E_NOMEM = -4
};

typedef struct srk_ba_report {
    int32_t status;          /* enum srk_status */
    int32_t optimized;       /* reference bool */
    int64_t iterations;      /* accepted outer LM iterations (.cpp:756-891) */
    int64_t attempts;        /* solve+apply+error attempts (.cpp:775-850) */
    int64_t seen;            /* observation count over all ranks (.cpp:483) */
    double err_initial;      /* (pix/f0)^2 units */
    double err_final;
    double hessian_factor;   /* value at exit */
    double world_scale;      /* SceneNormalizer::WorldScale */
    /* device time per phase, milliseconds, summed over the call (hipEvent pairs) */
    double ms_jacobian;      /* residuals + all normal-equation blocks (.cpp:1140-1448) */
    double ms_schur;         /* reduced camera system build (.cpp:1780-1908) */
    double ms_solve;         /* dense factor + solve (.cpp:1911) */
    double ms_backsub;       /* point back-substitution (.cpp:1919-1960) */
    double ms_apply;         /* apply corrections (.cpp:1997-2063) */
    double ms_error;         /* reprojection error (.cpp:410-490) */
    double ms_total;         /* wall time of the optimise call */
    int64_t schur_launches, jacobian_launches; /* kernel launches of the two HBM-bound phases */
    double ms_jacobian_kernel; /* time of the point-major Jacobian kernel alone (roofline numerator) */
    double ms_solve_syrk;      /* time inside the MFMA trailing-update kernels of the solve (srk_ba_set_profile) */
    double solve_mfma_flops;   /* flops those launches executed, summed over the call (srk_ba_set_profile) */
} srk_ba_report;

typedef struct srk_ba_normalizer {
    double R0[9], T0[3];   /* cam0 before normalisation (SceneNormalizer::prenorm_cam0_from_world) */
    double world_scale;
} srk_ba_normalizer;

/* ---- lifetime ---- */
srk_ba* srk_ba_create(int device_id);            /* NULL on failure (no HIP device, bad id) */
void srk_ba_destroy(srk_ba*);
const char* srk_ba_last_error(const srk_ba*);    /* text of the last SRK_E_DEVICE / SRK_E_ARGS */
const char* srk_ba_status_string(int status);    /* the four reference strings (+ harness additions) */
int srk_ba_device_count(void);                   /* HIP devices visible; 0 when none */
/* run on a caller-provided hipStream_t (e.g. torch's current stream) instead of the handle's own */
int srk_ba_set_stream(srk_ba*, void* hip_stream);

/* ---- multi-GPU (landmark sharding) ----
 * Every rank owns a contiguous pnt_ind range and passes only that range to the scene calls; cameras
 * are replicated.  With world_size >= 2 an LM iteration runs in ROUNDS of the next two or three damping
 * factors: every rank builds each factor's reduced camera system on its landmarks (the
 * frame blocks are added before the exchange, so they need none of their own), the packed band of
 * factor k with its rhs behind it is reduced to rank k, rank k solves and broadcasts the frame
 * corrections, every rank back-substitutes and scores every factor on its shard, and one all-reduce
 * carries the {error, solver status, point-update status} words of all factors; plus one exchange at
 * the start of an optimise call (initial error, observation count).  (SRK_MULTI_SCHEDULE=allreduce in
 * the environment of srk_ba_create: the older schedule -- the band all-reduced, every rank solves.)
 * The callback `fn` sums `count` doubles in place across ranks; it is all the library needs (a reduce
 * is a sum the other ranks ignore, a broadcast a sum of a buffer they zeroed).
 * Buffers downloaded with srk_ba_download (GRAD, UG, ...) hold this rank's partial sums.
 * `dev_ptr` is device memory; the hook is called with everything queued for the buffer complete and
 * must return after the reduction is complete.  Returns 0 on success. */
typedef int (*srk_allreduce_fn)(void* ctx, double* dev_ptr, int64_t count);
int srk_ba_set_allreduce(srk_ba*, srk_allreduce_fn fn, void* ctx, int rank, int world_size);
/* The same exchanges natively: ncclReduce / ncclBroadcast groups and ncclAllReduce (sum, fp64) on a stream of the handle,
 * ordered against the attempts' streams by events, with no host synchronisation and no Python -- what a C++ caller on the
 * 8 GPUs of a node uses (one process or thread per GPU, one handle each).  librccl.so is opened on first use.
 *   srk_ba_rccl_get_unique_id: rank 0 fills 128 bytes (ncclUniqueId) and hands them to the other ranks by any means;
 *   srk_ba_rccl_init:          every rank creates the communicator on its handle's device (collective call);
 *   srk_ba_rccl_init_second:   (optional, collective, after srk_ba_rccl_init, with a second unique id) a communicator of
 *                              its own for the second attempt slot of the `allreduce` schedule (speculative attempt pairs
 *                              with several ranks, each slot's all-reduces on its own stream and communicator); the
 *                              default schedule needs one communicator only;
 *   srk_ba_rccl_set_comm:      use a communicator (ncclComm_t) the caller owns instead; NULL detaches.
 * Either replaces a callback set with srk_ba_set_allreduce.  Call before srk_ba_upload_scene. */
int srk_ba_rccl_get_unique_id(void* id128 /* out: 128 bytes */);
int srk_ba_rccl_init(srk_ba*, const void* id128, int rank, int world_size);
int srk_ba_rccl_init_second(srk_ba*, const void* id128);
int srk_ba_rccl_set_comm(srk_ba*, void* nccl_comm, int rank, int world_size);

/* ---- the reference API, one call ---- */
int srk_ba_compute_inplace(srk_ba*, double f0,
                           int64_t n_points, double* points_xyz,
                           int32_t n_frames, double* cam_R, double* cam_T,
                           const double* K, int shared_k,
                           const int64_t* obs_row_ptr, const int32_t* obs_frame, const double* obs_uv,
                           const double* allowed_err_change /* NULL = unset */,
                           const double* max_hessian_factor /* NULL = unset */,
                           int64_t max_iterations /* <= 0 = unlimited (reference behaviour) */,
                           srk_ba_report* out);

/* The same call for a reference built with Scalar = float (rt-config.h:41-48; CMake option suriko_scalar_type_string =
 * f32, suriko-engine/CMakeLists.txt:14-15,76-82): float arrays at the boundary, widened to the fp64 pipeline and
 * rounded back (strictly more accurate than the reference's f32 arithmetic; there is no f32 device pipeline). */
int srk_ba_compute_inplace_f32(srk_ba*, float f0,
                               int64_t n_points, float* points_xyz,
                               int32_t n_frames, float* cam_R, float* cam_T,
                               const float* K, int shared_k,
                               const int64_t* obs_row_ptr, const int32_t* obs_frame, const float* obs_uv,
                               const float* allowed_err_change, const float* max_hessian_factor,
                               int64_t max_iterations, srk_ba_report* out);

double srk_ba_reproj_error(srk_ba*, double f0,
                           int64_t n_points, const double* points_xyz,
                           int32_t n_frames, const double* cam_R, const double* cam_T,
                           const double* K, int shared_k,
                           const int64_t* obs_row_ptr, const int32_t* obs_frame, const double* obs_uv,
                           int64_t* seen /* may be NULL */); /* NaN on error */

/* MultiViewIterativeFactorizer::ReprojError (multi-view-factorization.cpp:415-475): the score the MVF driver takes
 * before deciding to run BA (:372-379).  Observations whose homogeneous image point has |z| <= z_tol (reference:
 * 1e-5, :455) are skipped.  Returns 1 = ok (*reproj_err and *summands set), 0 = nothing was summed (the reference
 * returns false), negative = argument / device error.  Both scorers leave an uploaded BA scene untouched and do no
 * gauge normalisation, sorting or solver planning. */
int srk_ba_reproj_error_mvf(srk_ba*, double f0,
                            int64_t n_points, const double* points_xyz,
                            int32_t n_frames, const double* cam_R, const double* cam_T,
                            const double* K, int shared_k,
                            const int64_t* obs_row_ptr, const int32_t* obs_frame, const double* obs_uv,
                            double z_tol, double* reproj_err, int64_t* summands /* may be NULL */);

/* ---- multi-view-factorization steps (the caller on the other side of the BA path) ----
 * Estimate3DPointDepthFromFrames (multi-view-factorization.cpp:223-253, MASKS 8.44), batched over tracks: track i has
 * observations [row_ptr[i], row_ptr[i+1]) = (frame, metric homogeneous image point); its FIRST observation is the
 * base frame (:195-215) and depth_out[i] is the depth in that frame (NaN for tracks with fewer than 2 observations).
 * cam_R / cam_T: world -> camera of every frame. */
int srk_mvf_estimate_depths(srk_ba*, int64_t n_tracks, const int64_t* row_ptr, const int32_t* frame,
                            const double* x_meter /* [O][3] */, int32_t n_frames, const double* cam_R, const double* cam_T,
                            double* depth_out /* [n_tracks] */);
/* FindRelativeMotionMultiPoints (:107-189) + ProjectOntoSO3 (:79-104): camera motion anchor -> target from the common
 * points' homogeneous image coordinates in both frames and their depths in the anchor frame.  The Gram matrix of the
 * 3P x 12 system is reduced on the device; its smallest eigenvector replaces the reference's JacobiSVD (same vector up
 * to sign, and the projection is sign-invariant).  At least 6 points (each gives two independent equations of the 11
 * needed).  Returns 1 ok, 0 = projection failed (det S ~ 0), negative = error.
 * Accuracy: forming A^T A squares the condition number of A, so with NOISY tracks the null vector carries about half
 * the digits a one-sided SVD of A would (relative error ~ eps * cond(A)^2 instead of eps * cond(A)); with exact
 * geometry (the reference demo's matcher projects ground truth) both are exact to rounding -- the demo's poses agree
 * with the ground truth to 1e-11..1e-5 over its first 27 frames.  No reference fixture exists for this function
 * (parity unpinned); the oracle restates it with a one-sided Jacobi SVD and the tests use noise-free geometry. */
int srk_mvf_relative_motion(srk_ba*, int64_t n_points, const double* x_anchor /* [P][3] */, const double* x_target /* [P][3] */,
                            const double* depth_anchor /* [P] */, double* R_out /* [9] row-major */, double* T_out /* [3] */);
/* ProjectOntoSO3 alone (host code, no GPU needed): 1 ok, 0 = det S ~ 0 */
int srk_mvf_project_onto_so3(const double* R_noisy, const double* T_noisy, double* R_out, double* T_out);

/* host-side gauge normalisation (bundle-adj-kanatani.cpp:203-270); no GPU needed */
int srk_ba_normalize_scene(int64_t n_points, double* points_xyz, int32_t n_frames, double* cam_R, double* cam_T,
                           double t1y, int32_t unity_comp_ind, srk_ba_normalizer* out); /* 1 = ok, 0 = failed */
void srk_ba_revert_normalization(int64_t n_points, double* points_xyz, int32_t n_frames, double* cam_R,
                                 double* cam_T, const srk_ba_normalizer* nrm);
int srk_ba_check_world_is_normalized(int32_t n_frames, const double* cam_R, const double* cam_T, double t1y,
                                     int32_t unity_comp_ind);

/* ---- staged API: scene resident in HBM (bench, parity tests, repeated solves) ----
 * upload = gauge-normalise on the host (unless already_normalized) + copy to the device;
 * optimize = the device-resident LM loop (.cpp:720-893); download = copy back + revert normalisation. */
int srk_ba_upload_scene(srk_ba*, double f0,
                        int64_t n_points, const double* points_xyz,
                        int32_t n_frames, const double* cam_R, const double* cam_T,
                        const double* K, int shared_k,
                        const int64_t* obs_row_ptr, const int32_t* obs_frame, const double* obs_uv,
                        int already_normalized);
int srk_ba_optimize(srk_ba*, const double* allowed_err_change, const double* max_hessian_factor,
                    int64_t max_iterations, srk_ba_report* out);
int srk_ba_download_scene(srk_ba*, double* points_xyz, double* cam_R, double* cam_T, int revert_normalization);
/* restore the scene that was uploaded (device-side copy), so that a bench can repeat identical steps */
int srk_ba_reset_scene(srk_ba*);

/* single phases on the resident scene (parity tests and per-kernel timing) */
int srk_ba_phase_error(srk_ba*, double* err, int64_t* seen); /* err = E = sum rho(s) when a robust loss is set */
int srk_ba_phase_derivatives(srk_ba*);
int srk_ba_phase_schur(srk_ba*, double hessian_factor);
int srk_ba_phase_solve(srk_ba*);                            /* 0 ok, 1 non-finite / not positive definite */
int srk_ba_phase_backsub(srk_ba*, double hessian_factor);   /* also forms the trial scene (apply) */
int srk_ba_phase_accept(srk_ba*);                           /* trial scene becomes current */

/* copies of device buffers for the parity tests, expanded to the oracle's layouts */
enum srk_buffer {
    SRK_BUF_GRAD = 0,        /* [3N + FV M] gradE; FV = srk_ba_frame_vars: 10, or 6 */
    SRK_BUF_POINT_BLOCKS,    /* [N][3][3] */
    SRK_BUF_FRAME_BLOCKS,    /* [M][FV][FV] */
    SRK_BUF_POINT_FRAME,     /* [O][3][FV] */
    SRK_BUF_RCS,             /* [FV M][FV M] padded reduced camera system (fixed variables: identity rows) */
    SRK_BUF_RCS_RHS,         /* [FV M] */
    SRK_BUF_CORRECTIONS,     /* [3N + FV M] corrections with zero gaps */
    SRK_BUF_POINTS,          /* [N][3] current (normalised) points */
    SRK_BUF_CAM_R,           /* [M][9] */
    SRK_BUF_CAM_T            /* [M][3] */
};
int64_t srk_ba_buffer_size(srk_ba*, int which);                 /* doubles; negative on error */
int srk_ba_download(srk_ba*, int which, double* dst, int64_t count);
/* selected rows of the padded reduced camera system (SRK_BUF_RCS is 12.8 GB at 4000 frames): dst[n_rows][FV M], row
 * rows[k] of the system with its columns <= the row filled (the lower triangle is authoritative), zeros right of it */
int srk_ba_download_rcs_rows(srk_ba*, const int64_t* rows, int64_t n_rows, double* dst);

/* The reduced camera system is non-zero only where two frames share a landmark; the solver skips everything
 * outside that skyline (exact: Cholesky fill stays inside it).  With landmark shards every rank must be given the
 * GLOBAL covisibility after upload: min_cv[j] = smallest frame index sharing a landmark with frame j. */
int srk_ba_set_covisibility(srk_ba*, const int32_t* min_cv /* [M], NULL = dense */);
int srk_ba_set_rcs_mode(srk_ba*, int mode /* 0 = dense lower triangle, 1 = skyline as one chain,
                                              2 = skyline cut into independent chunks + separator system (default) */);
int srk_ba_rcs_chunks(srk_ba*); /* number of chunks of the current plan (0 = one chain) */
double srk_ba_rcs_fill(srk_ba*); /* skyline size / lower-triangle size */
double srk_ba_solve_mfma_flops(srk_ba*); /* flops of the MFMA trailing updates of one solve (current mode / plan) */

/* Solver launch structure (harness knob; the reference has one dense solve, bundle-adj-kanatani.cpp:1911): 1 (default) =
 * each 256-column outer step of the blocked Cholesky is ONE launch whose workgroups hand factored tiles to one another
 * (bounded spins; a timed-out hand-off makes the LM loop repeat that attempt with the unfused sequence and stay there),
 * 0 = one launch per 64-column panel and per rank-64 update.  Each is bit-reproducible from run to run; they agree with each
 * other to rounding (since round 4 the fused step eliminates the diagonal block's own rows in the factorisation's unscaled
 * form).  Takes effect at once.
 * srk_ba_solver_sync_timeouts: how many solves had to be repeated (0 in every run so far).  A timeout is a scheduling event
 * (another process on the GPU, a debugger), so the unfused sequence is kept only for the rest of that call: the next upload /
 * optimise call uses the fused step again -- until the handle has seen three timeouts since the last
 * srk_ba_set_solver_fusion(h, 1); then the unfused sequence stays.  srk_ba_solver_fusion: 1 = fused right now, 0 = unfused. */
int srk_ba_set_solver_fusion(srk_ba*, int on);
int64_t srk_ba_solver_sync_timeouts(srk_ba*);
int srk_ba_solver_fusion(srk_ba*);

/* The accepted outer iterations of the last srk_ba_optimize / srk_ba_compute_inplace call (the reference logs them with
 * VLOG, bundle-adj-kanatani.cpp:756-891): for iteration k the attempts it needed (solve + apply + error each), the host
 * time in ms since the call began at which it was accepted, the error it reached and the damping factor that was
 * accepted.  Returns the number of iterations (arrays, each may be NULL, receive at most cap entries). */
int64_t srk_ba_iteration_log(srk_ba*, int64_t cap, int32_t* attempts, double* ms_since_start, double* err,
                             double* hessian_factor);

/* Speculative attempts (default on; takes effect at the next upload): with the instrumentation off
 * (srk_ba_set_profile 0, the default) the LM loop runs the next damping factor on a second stream beside the current
 * one and judges the attempts in the reference's order, so results are those of the sequential loop; costs a second
 * reduced camera system in memory.  With several ranks every rank takes the same decisions, so the exchanges of the
 * two attempts are issued in the same order everywhere.  0 = strictly one attempt at a time -- with several ranks too: one
 * attempt slot, i.e. the all-reduce schedule without pairs (the damping-parallel schedule runs two or three factors a round). */
int srk_ba_set_speculation(srk_ba*, int on);

/* Deterministic mode (default off; takes effect at the next upload).  The reference is sequential: it adds every landmark's
 * contribution in point order (bundle-adj-kanatani.cpp:1862-1898) and two runs give the same bits.  By default the derivative
 * and the Schur kernels here combine partial sums with fp64 atomics, whose arrival order differs from run to run: results
 * agree to rounding, and where two attempts' errors tie at that level the accept / reject sequence can fork.  With the mode
 * on, a derivative task's frame sums and a run's Schur sum go to staging buffers and an ordered second pass adds them (per
 * frame in task order, per block in run order): the same scene gives the same bits every time, at the cost of that pass
 * (+ ~0.16 GB of staging per attempt slot at 1000 frames).  Covered: scenes whose tracks span at most 20 frames (the
 * run-based derivative kernel and the MFMA Schur kernel; every BASELINE configuration), one rank, fp64 run sums.
 * srk_ba_deterministic: 1 when the uploaded scene runs that way, 0 when the mode is off or the scene is not covered (the
 * default kernels then run). */
int srk_ba_set_deterministic(srk_ba*, int on);
int srk_ba_deterministic(srk_ba*);

/* Exchange schedule of the LM loop with several ranks (landmark shards; takes effect at the next upload):
 *   1 (default) damping-parallel: a round builds the next min(3, world) damping factors c, 10c, 100c on every shard, band k is
 *     REDUCED to rank k, rank k solves factor k and broadcasts its corrections, every rank scores all of them and one
 *     all-reduce carries the status words -- an iteration that needs <= 3 attempts costs about one solve;
 *   0 all-reduce: the band of each attempt is all-reduced and every rank solves the same system redundantly (round 2);
 *   2 the damping-parallel schedule at world size 1 as well (rehearsal of its collectives on one GPU).
 * The native (RCCL) form of schedule 1 issues groups of ncclReduce / ncclBroadcast rooted at different ranks on one
 * communicator.  Its FIRST round on a handle checks itself: checksums of every band and of every corrections vector travel
 * beside the rooted collectives through plain all-reduces; on a mismatch or an RCCL error the handle switches to schedule 0
 * for good, the round is repeated that way and srk_ba_last_error says why.
 * srk_ba_multi_schedule: 0 all-reduce (asked for), 1 damping-parallel (no native round has run yet), 2 damping-parallel
 * with its self-check passed, 3 all-reduce after a failed self-check. */
int srk_ba_set_multi_schedule(srk_ba*, int mode);
int srk_ba_multi_schedule(srk_ba*);

/* Internal frame order.  The reference's dense solve (bundle-adj-kanatani.cpp:1911) does not care how the frames are
 * numbered; the skyline solver, its nested dissection and the derivative kernels' frame windows here want covisible frames
 * to have nearby indices.  When the caller's numbering is far from banded (an unordered image set, a sequence that closes
 * a loop) the frames are renumbered internally by reverse Cuthill-McKee on the covisibility graph; the gauge stays on the
 * CALLER's frames 0 and 1, every download and the scene itself come back in the caller's order, results are those of the
 * caller's order up to summation order.  One rank only (landmark shards keep the caller's order).
 * mode -1 = automatic (default), 0 = never, 1 = whenever the ordering differs; takes effect at the next upload.
 * srk_ba_frame_order: 1 = renumbered (to_internal[caller's frame] = internal index, may be NULL), 0 = caller's order.
 * srk_frame_order: the decision and the numbering alone, on the host (no device needed). */
int srk_ba_set_frame_reordering(srk_ba*, int mode);
/* The numbering to use at the next upload instead of the automatic one (to_internal = NULL: automatic again).  This is how
 * landmark shards get a renumbering: the caller finds it on the WHOLE scene (srk_frame_order) and gives every rank the same
 * one; srk_ba_set_covisibility then takes min_cv in THAT numbering (covisibility of the renumbered scene). */
int srk_ba_set_frame_order(srk_ba*, const int32_t* to_internal /* [n_frames] or NULL */, int32_t n_frames);
int srk_ba_frame_order(srk_ba*, int32_t* to_internal /* [M] or NULL */);
int srk_frame_order(int mode, int64_t n_points, int32_t n_frames, const int64_t* obs_row_ptr, const int32_t* obs_frame,
                    int32_t* to_internal /* [M] */);

/* Derivative kernel selection (harness knob, the reference has one code path: bundle-adj-kanatani.cpp:1140-1448).
 * mode -1 = automatic: the run-based kernel (a lane keeps one frame's sums in registers over a run of landmarks with
 * identical frame lists) when the runs are long enough, else the per-observation kernels; 0 = per-observation kernels
 * only; 1 = run-based whenever the scene allows it (tracks of <= 64 frames, narrow frame windows); 2 = run-based over the
 * UNION of the frame lists of a run of landmarks (ragged feature tracks: a lane per (landmark, frame slot) cell, masks) whenever
 * the scene allows it (every track of <= 24 frames) -- automatic mode takes it when the uniform runs are too short to pay.
 * Takes effect at the next upload.  srk_ba_jacobian_kernel: 3 = run-based over frame unions, 2 = run-based, 1 = fused
 * per-observation, 0 = two-kernel path, -1 = no scene. */
int srk_ba_set_jacobian_mode(srk_ba*, int mode);
int srk_ba_jacobian_kernel(srk_ba*);

/* f32 storage mode (the reference's suriko_scalar_type_string = f32 switch, suriko-engine/
 * CMakeLists.txt:14-15,76-82, rt-config.h:41-48, applied where the bytes are): f32 = 1 stores the point-frame blocks W
 * (3 x 10 per observation: 240 of the 260 algorithmic bytes per observation of the derivative pass, and what the Schur
 * and back-substitution passes read; the library keeps each block as its 21 rank-2 factors) as float, 84 bytes an
 * observation; they are widened on load, every sum, the reduced camera system and the solve stay fp64.  Takes effect at the next upload.  Tolerances against the fp64 path and against the oracle with W
 * rounded the same way: tests/test_gpu_parity.py::test_f32_storage_*.  Default 0. */
int srk_ba_set_storage_precision(srk_ba*, int f32);

/* Opt-in mixed precision for the reduced camera system (the reference's suriko_scalar_type_string = f32 switch,
 * suriko-engine/CMakeLists.txt:14-15, applied where it pays on this hardware): fp32 = 1 rounds W and E^-1 W to fp32
 * when they are staged and accumulates each run of <= 128 landmarks with packed fp32 FMAs; the runs' sums, the frame
 * blocks, the factorisation and everything else stay fp64.  Default 0 = the reference's fp64 arithmetic (the only
 * mode the parity tests and the benchmark's headline use). */
int srk_ba_set_schur_precision(srk_ba*, int fp32);

/* Calibrated bundle adjustment (an extension; the reference declares the intrinsic variable count as "0 if K is shared for
 * all frames; 3 ...; 4", bundle-adj-kanatani.h:113-118, but only wires up 10, and ApplyCorrections adds the intrinsic
 * corrections to a copy of K that is thrown away, bundle-adj-kanatani.cpp:2025-2033): on = 1 makes the intrinsics constants.
 * Each frame then has the 6 pose variables [Tx Ty Tz Wx Wy Wz] (variables 4..9 of the default layout, same gauge), the
 * reduced camera system is 6M wide, and every step is the Gauss-Newton / LM step of the problem actually solved -- the
 * 10-variable damped system restricted to the pose and point variables.  K is never changed.  Takes effect at the next
 * upload (srk_ba_compute_inplace included); the staged API and the downloads then use the compact layout: SRK_BUF_GRAD and
 * SRK_BUF_CORRECTIONS [3N + 6M], SRK_BUF_FRAME_BLOCKS [M][6][6], SRK_BUF_POINT_FRAME [O][3][6], SRK_BUF_RCS [6M][6M],
 * SRK_BUF_RCS_RHS [6M], srk_ba_download_rcs_rows rows of 6M.  Refused with SRK_E_ARGS (and a srk_ba_last_error text) by
 * whichever call comes second: deterministic mode, f32 storage, fp32 Schur accumulation, more than one rank.  Default 0. */
int srk_ba_set_fixed_intrinsics(srk_ba*, int on);
/* variables per frame: 6 with fixed intrinsics, else 10 (of the uploaded scene; before an upload, of the next one) */
int srk_ba_frame_vars(srk_ba*);
/* landmarks of the uploaded scene whose Schur terms take the per-landmark kernel (fp64 atomics) instead of the run-based
 * kernels: with fixed intrinsics every landmark outside the runs of <= 20 frames k_schur_mm takes (wider runs, long tracks);
 * otherwise the tracks too long for the long-track kernel.  0 on the circle-grid bench scenes; negative without a scene. */
int64_t srk_ba_schur_fallback_landmarks(srk_ba*);

/* ---- shared intrinsics (EXTENSION) ----
 * Every frame belongs to one of n_groups camera groups (1..32); each group has one set of intrinsics [fx fy u0 v0], solved
 * together with the poses and points and written back (bundle-adj-kanatani.cpp:2025-2033 applies the same additions to a
 * copy of K).  group[caller's frame] = its group; NULL = off (default).  Takes effect at the next upload
 * (srk_ba_compute_inplace included).  SRK_E_ARGS (and a srk_ba_last_error text) for n_groups outside 1..32, a group id out
 * of range or a group without frames; at upload, for another number of frames or frames of one group whose K differ in
 * any bit (shared_k = 1 always passes).  Refused with SRK_E_ARGS by whichever call comes second: fixed intrinsics, f32
 * storage, fp32 Schur accumulation, more than one rank.  Deterministic mode, speculation, robust losses, frame reordering
 * and every Jacobian mode work unchanged; rcs mode 2 runs as one chain with the border (srk_ba_rcs_chunks: 0).
 * The reduced system is then P^T S P over n = 6M + 4G variables: pose variables 6 frame + [Tx Ty Tz Wx Wy Wz], then
 * 6M + 4 g + [fx fy u0 v0], in the caller's frame and group numbering.  srk_ba_frame_vars returns 6; SRK_BUF_RCS [n][n],
 * SRK_BUF_RCS_RHS [n], SRK_BUF_CORRECTIONS [3N + n], SRK_BUF_GRAD [3N + n] (P^T of the 10-variable gradient) and
 * srk_ba_download_rcs_rows (rows of n) use this layout; SRK_BUF_FRAME_BLOCKS and SRK_BUF_POINT_FRAME stay the 10-variable
 * per-frame blocks.  srk_ba_reset_scene restores the uploaded K.
 * The closed-form frame derivatives are those of the error only when K(2,2) = f0 (the project's scenes divide K by f0), so
 * with groups every frame's K is held as K * f0 / K(2,2) (the same projections; K(2,2) must be finite and non-zero, else
 * SRK_E_ARGS): the [fx fy u0 v0] entries of SRK_BUF_RCS / _RHS / _CORRECTIONS / _GRAD refer to that K, and
 * srk_ba_download_intrinsics returns the caller's convention (its K(2,2) restored). */
int srk_ba_set_intrinsic_groups(srk_ba*, const int32_t* group /* [n_frames] or NULL */, int32_t n_frames, int32_t n_groups);
/* the number of intrinsic groups of the uploaded scene (before an upload: of the next one); 0 = off */
int srk_ba_intrinsic_groups(srk_ba*);
/* the current intrinsics of every group, K[n_groups][9] row-major 3 x 3 (after srk_ba_optimize: the result).  SRK_E_ARGS
 * when the uploaded scene has no groups or n_groups differs. */
int srk_ba_download_intrinsics(srk_ba*, double* K, int32_t n_groups);

/* ---- robust bundle adjustment (EXTENSION) ----
 * Observation o has the residual (ex, ey) = (p/r - u/f0, q/r - v/f0) and s = ex^2 + ey^2 in the (pix/f0)^2 units of
 * srk_ba_report::err_initial.  With a loss set, LM minimises E = sum_o rho(s_o) instead of sum_o s_o:
 *   kind 1, Huber:   rho(s) = s for s <= d^2, 2 d sqrt(s) - d^2 above;   weight w = rho'(s) = min(1, d / sqrt(s))
 *   kind 2, Cauchy:  rho(s) = d^2 log(1 + s / d^2);                      weight w = 1 / (1 + s / d^2)
 * with d = delta_pixels / f0.  Every derivative pass (the speculative one included) weights each observation's Gauss-Newton
 * blocks and gradient terms by its w at the current scene (first-order IRLS, no second-order correction); the weighted
 * gradient is the exact gradient of E.  E is what the accept / reject test, the relative-change termination,
 * err_initial / err_final, srk_ba_iteration_log and srk_ba_phase_error report.  srk_ba_reproj_error and
 * srk_ba_reproj_error_mvf never apply a loss.  Works with every mode the library accepts (fixed intrinsics,
 * deterministic, f32 storage, fp32 Schur, every Jacobian mode, frame reordering, several ranks).
 * Takes effect at the next optimise / phase call (srk_ba_compute_inplace and srk_ba_compute_inplace_f32 included); no
 * re-upload is needed.  kind 0 = none: the reference's plain least squares (default).  SRK_E_ARGS (and a
 * srk_ba_last_error text) for an unknown kind or, with kind != 0, a delta that is not finite and positive. */
int srk_ba_set_robust_loss(srk_ba*, int kind /* 0 none, 1 Huber, 2 Cauchy */, double delta_pixels);
/* the loss set on the handle: kind and delta in pixels (0 with kind 0); either pointer may be NULL */
int srk_ba_robust_loss(srk_ba*, int* kind, double* delta_pixels);
/* the IRLS weights w of the resident scene's observations (current scene: after srk_ba_optimize, the result), in the
 * caller's observation order (the CSR order of the upload; internal landmark and frame orders undone); count = the number
 * of observations (of this rank's shard with several ranks).  All 1 without a loss.  Observations with w < 1 lie beyond
 * the threshold: the outliers of a robust solve. */
int srk_ba_observation_weights(srk_ba*, double* w, int64_t count);

/* ---- per-observation information (EXTENSION) ----
 * Observation o gets a scalar information q_o >= 0, a dimensionless multiplier of its squared residual (typically
 * (sigma_ref / sigma_o)^2).  LM then minimises E = sum_o rho(q_o s_o): rho the identity without a loss (E = sum q_o s_o),
 * Huber or Cauchy as above otherwise, the threshold delta keeping its meaning (pixels at unit information).  The weight
 * of an observation in the Gauss-Newton blocks and the gradient is q rho'(q s); the gradient is the exact gradient of E.
 * E is what the accept / reject test, the termination test, err_initial / err_final, srk_ba_iteration_log and
 * srk_ba_phase_error report.  srk_ba_reproj_error and srk_ba_reproj_error_mvf stay unweighted, and
 * srk_ba_observation_weights keeps returning the loss's factor rho'(q s) alone (all 1 without a loss).  q_o = 0 switches
 * the observation off: exact zeros everywhere, stored factors (SRK_BUF_POINT_FRAME) included.  q = 1 everywhere is bit for
 * bit the run without information.
 *
 * q is in the caller's observation order (the CSR order of the upload, the order of srk_ba_observation_weights); with
 * several ranks it covers the rank's shard.  NULL clears the setting (the default).  The handle keeps a copy: it is
 * applied by every later upload (srk_ba_compute_inplace and srk_ba_compute_inplace_f32 included) and is not touched by
 * srk_ba_reset_scene.  With a scene resident it takes effect at the next optimise / phase call WITHOUT another upload:
 * the scene, its internal orders, the skyline and the solver plan stay as they are.
 * SRK_E_ARGS (text in srk_ba_last_error), the previous setting staying in force: a value that is negative or not finite;
 * a count that is not the resident scene's number of observations (at an upload: a stored count that is not the new
 * scene's); a landmark left with fewer than two observations of positive information (its 3 x 3 block would be
 * singular).  A frame left without a positive observation is the caller's business: like any degenerate scene the solve
 * reports failure. */
int srk_ba_set_observation_information(srk_ba*, const double* q /* [count] or NULL */, int64_t count);
/* the setting in the caller's order, or all 1 when none is set; count = the number of values set (of observations) */
int srk_ba_observation_information(srk_ba*, double* q, int64_t count);
/* the raw, unwhitened residuals f0 (ex, ey) of the resident scene in pixels (current scene: after srk_ba_optimize, the
 * result), [count][2] in the caller's observation order; count = the number of observations (of this rank's shard).
 * Works with or without information or a loss, and neither changes it. */
int srk_ba_observation_residuals(srk_ba*, double* exy_pixels /* [count][2] */, int64_t count);

/* ---- constant parameter blocks (EXTENSION) ----
 * Frames and landmarks that keep their values: old keyframes of a sliding window, a fixed map, ground-control points,
 * motion-only (every landmark constant) and structure-only (every frame constant) refinement.  Flags are non-zero for
 * constant, in the caller's frame and landmark numbering; either array may be NULL (none of that kind), both NULL clears
 * the setting (the default).  The handle keeps a copy: it is applied by every later upload (srk_ba_compute_inplace and
 * srk_ba_compute_inplace_f32 included; the gauge choice below is part of the uploaded scene) and is not touched by
 * srk_ba_reset_scene.  An upload whose scene has other counts than the stored setting fails with SRK_E_ARGS.
 *
 * A constant frame: every one of its frame variables (10, or 6 with fixed intrinsics) has correction exactly 0; its rows and
 * columns of the reduced camera system are identity and its rhs 0.  A constant landmark: its 3 x 3 block is the identity, its
 * gradient 0 and the point-frame blocks of its observations exact zeros, so it adds nothing to the reduced system and its
 * correction is exactly 0; its observations still enter the frame blocks, the frame gradients and the error.
 * Nothing is compacted: a constant frame keeps its rows of the system and a constant landmark still passes through the
 * Schur sum (as zeros).  Two small masking passes after the derivative pass and after the assembly impose the blocks; none
 * is launched without constant blocks, and every other kernel runs unchanged.
 *
 * keep_gauge = 1: the reference's seven gauge variables (the pose of frame 0, one translation component of frame 1) stay
 * constant in addition -- for a constant set that does not determine the similarity, or one that holds the caller's frames 0
 * and 1 anyway.  keep_gauge = 0: only the listed blocks are constant; the caller asserts that they fix the seven gauge
 * freedoms (two constant frames with distinct centres, a frame and a landmark off its centre, three non-collinear
 * landmarks); if they do not, the system is singular and the solve reports failure like any degenerate scene.  The gauge
 * NORMALISATION of the world still uses the caller's frames 0 and 1: it is only a change of coordinates.
 * Every frame constant and every landmark constant are both valid; everything constant is SRK_E_ARGS.
 * Refused with SRK_E_ARGS (and a srk_ba_last_error text) by whichever call comes second: intrinsic groups, more than one
 * rank.  Fixed intrinsics, deterministic mode, f32 storage, fp32 Schur sums, every Jacobian and rcs mode, solver fusion,
 * speculation, frame reordering, robust losses and information work unchanged.
 *
 * Results: in the resident (normalised) scene the constant blocks keep the uploaded bits through every attempt and accept
 * (SRK_BUF_POINTS, SRK_BUF_CAM_R, SRK_BUF_CAM_T).  srk_ba_compute_inplace does not write constant blocks back: the caller's
 * entries stay bit-identical.  srk_ba_download_scene writes their reverted values (the input up to the normalise / revert
 * round trip).  Downloads: SRK_BUF_RCS, SRK_BUF_RCS_RHS and srk_ba_download_rcs_rows show the identity rows and zero rhs,
 * SRK_BUF_POINT_BLOCKS the identity and SRK_BUF_POINT_FRAME zeros for constant landmarks, SRK_BUF_CORRECTIONS and
 * SRK_BUF_GRAD zeros at constant entries; SRK_BUF_FRAME_BLOCKS stays the unmasked per-frame blocks. */
int srk_ba_set_constant_blocks(srk_ba*, const uint8_t* frame_const /* [n_frames] or NULL */, int32_t n_frames,
                               const uint8_t* point_const /* [n_points] or NULL */, int64_t n_points, int keep_gauge);
/* the setting: flags (0 / 1) into the arrays given (an array is left untouched when that kind was set as NULL) and
 * keep_gauge; any pointer may be NULL.  Returns 1 if a setting is stored, 0 if not. */
int srk_ba_constant_blocks(srk_ba*, uint8_t* frame_const, uint8_t* point_const, int* keep_gauge);
/* the lengths of the stored flag arrays (0 = that kind was set as NULL); returns 1 if a setting is stored, 0 if not */
int srk_ba_constant_counts(srk_ba*, int32_t* n_frames, int64_t* n_points);
/* device time in ms of the last launch of the two masking passes (the landmark pass of the last derivative pass, the frame
 * pass of the last assembly), taken with srk_ba_set_profile >= 1; 0 for a pass that was not launched or not timed */
int srk_ba_constant_pass_ms(srk_ba*, double* points_ms, double* frames_ms);

/* ---- Gaussian position priors on landmarks and camera centres (EXTENSION) ----
 * "This landmark was surveyed to 2 cm", "this camera's GPS fix is good to 1 m": the finite variances that constant blocks (the
 * limit of zero variance) cannot state, and a solve that lands in the caller's absolute coordinates.  With priors LM minimises
 *
 *     E = sum_o rho(q_o s_o) + sum_{i in P} (X_i - Xbar_i)^T L_i (X_i - Xbar_i) + sum_{j in F} (C_j - Cbar_j)^T L_j (C_j - Cbar_j)
 *
 * X_i landmark i, C_j = -R_j^T T_j the centre of frame j; Xbar, Cbar and the information matrices L in the caller's world
 * coordinates (the coordinates of the arrays passed to the upload).  L: symmetric positive semi-definite 3 x 3, given as
 * [xx xy xz yy yz zz], in units of E -- (pix / f0)^2 -- per squared world unit: a prior of covariance Sigma beside
 * observations of pixel noise sigma_px is L = (sigma_px / f0)^2 Sigma^-1.  No robust loss acts on a prior.  This E is what the
 * accept / reject test, both termination tests, report.err_initial / err_final, srk_ba_iteration_log and srk_ba_phase_error
 * use; srk_ba_reproj_error* stay the reprojection sums.  A landmark prior adds 2 L to the landmark's 3 x 3 block and
 * 2 L (X - Xbar) to its gradient; a frame prior adds 2 L to the [Tx Ty Tz] part of the frame block and 2 L (C - Cbar) to those
 * gradient entries (the translation variables move the centre directly and the rotation variables leave it alone), before the
 * damping.  Neither adds a coupling: the skyline, the Schur kernels and the solver plans are those of the scene without priors.
 *
 * Both counts 0 clears the setting (the default).  The handle keeps a copy: it is applied by every later upload
 * (srk_ba_compute_inplace and srk_ba_compute_inplace_f32 included) and is not touched by srk_ba_reset_scene.  It takes effect
 * at the next upload, which maps it to the normalised scene X_n = s (R0 X + T0): Xbar_n = s (R0 Xbar + T0),
 * L_n = R0 L R0^T / s^2 (the prior energy is invariant; srk_ba_normalize_position_priors).  An index beyond the uploaded scene's
 * counts fails that upload with SRK_E_ARGS.
 *
 * keep_gauge = 1: the reference's seven gauge variables stay constant and the priors pull within that gauge.  keep_gauge = 0:
 * nothing is held; the caller asserts that the priors fix the similarity (three non-collinear positions with positive definite
 * L do); otherwise the system is singular and the solve reports failure like any degenerate scene.  The gauge is released
 * when either this setting or srk_ba_set_constant_blocks says keep_gauge = 0.  The gauge NORMALISATION still uses the caller's
 * frames 0 and 1.  A prior on a constant block adds a constant to E and nothing else.
 *
 * SRK_E_ARGS (text in srk_ba_last_error), the previous setting staying in force: indices not strictly ascending or negative,
 * a value that is not finite, an L that is not positive semi-definite (all zeros is a valid, switched-off prior), keep_gauge
 * outside {0, 1}, a NULL array of a kind whose count is positive.  Refused with SRK_E_ARGS by whichever call comes second:
 * intrinsic groups, more than one rank.  Fixed intrinsics, deterministic mode, f32 storage, fp32 Schur sums, every Jacobian
 * and rcs mode, solver fusion, speculation, frame reordering, robust losses, information and constant blocks work unchanged.
 * Two small passes impose the priors (one behind the derivative kernels, one beside the error kernel); neither is launched
 * without priors. */
int srk_ba_set_position_priors(srk_ba*, int64_t n_point_priors, const int64_t* point_index /* strictly ascending */,
                               const double* point_pos /* [n][3] */, const double* point_info /* [n][6]: xx xy xz yy yz zz */,
                               int32_t n_frame_priors, const int32_t* frame_index /* strictly ascending, caller's numbering */,
                               const double* frame_centre /* [n][3] */, const double* frame_info /* [n][6] */, int keep_gauge);
/* the counts of the stored setting; returns 1 if a setting is stored, 0 if not */
int srk_ba_position_prior_counts(srk_ba*, int64_t* n_point_priors, int32_t* n_frame_priors);
/* the stored setting in the caller's coordinates, into arrays of the sizes srk_ba_position_prior_counts gives; any pointer may
 * be NULL.  Returns 1 if a setting is stored, 0 if not.  Both calls report what the setter stored, i.e. what the NEXT upload
 * applies; the resident scene runs with the setting that was stored when it was uploaded. */
int srk_ba_position_priors(srk_ba*, int64_t* point_index, double* point_pos, double* point_info, int32_t* frame_index,
                           double* frame_centre, double* frame_info, int* keep_gauge);
/* the two prior sums of the resident scene's current state (0 without priors); srk_ba_phase_error minus these is the
 * observation part */
int srk_ba_prior_error(srk_ba*, double* e_points, double* e_frames);
/* X - Xbar [n_point_priors][3] and C - Cbar [n_frame_priors][3] of the resident scene's current state in the caller's world
 * coordinates (normalisation reverted), in the order of the setting: for chi-square checks of control points.  The offsets are
 * those of the setting the resident scene was uploaded with; if the stored setting has been changed since (indices or
 * positions), the call fails with SRK_E_STATE until the scene is uploaded again, so that counts and values cannot be mixed.
 * srk_ba_prior_error always sums the lists of the resident scene. */
int srk_ba_prior_residuals(srk_ba*, double* d_points, double* d_frames);
/* host only, no device needed: positions [n][3] and information matrices [n][6] through a normaliser, as the upload maps them
 * (pos_n = s (R0 pos + T0), L_n = R0 L R0^T / s^2).  Either pair of arrays may be NULL.  Returns SRK_OK or SRK_E_ARGS. */
int srk_ba_normalize_position_priors(const srk_ba_normalizer* nrm, int64_t n, const double* pos, const double* info,
                                     double* pos_out, double* info_out);
/* device time in ms of the last launch of the two prior passes (behind the derivative kernels, beside the error kernel), taken
 * with srk_ba_set_profile >= 1; 0 for a pass that was not launched or not timed.  One event pair serves all attempt slots: with
 * speculation on, the error-side figure is that of whichever attempt recorded last (tools/prior_rate.py switches it off). */
int srk_ba_prior_pass_ms(srk_ba*, double* derivative_ms, double* error_ms);

/* ---- relative-pose factors between frames (EXTENSION) ----
 * A calibrated stereo rig, odometry between consecutive keyframes, a loop closure between frames that share no landmark: terms
 * that tie two frames together.  With R_j, T_j the world -> camera pose of frame j and C_j = -R_j^T T_j its centre, factor k
 * between frames a != b carries a measured relative rotation Z_k of R_a R_b^T (3 x 3, row-major), a measured relative
 * translation z_k of R_a (C_b - C_a) (the centre of b in a's frame, world units) and a symmetric positive semi-definite 6 x 6
 * information matrix L_k, given as the 21 entries of its upper triangle row by row in the order [t; r]:
 *
 *     e_t = R_a (C_b - C_a) - z_k,   e_r = Log(Z_k^T R_a R_b^T) (rotation vector, angle < pi),
 *     E = (everything E is without factors) + sum_k [e_t; e_r]^T L_k [e_t; e_r]
 *
 * L is in units of E, (pix / f0)^2, per squared world unit (tt), per world unit and radian (tr), per squared radian (rr): a
 * factor of covariance Sigma beside observations of pixel noise sigma_px is L = (sigma_px / f0)^2 Sigma^-1.  No robust loss
 * and no observation information acts on a factor.  This E is what the accept / reject test, both termination tests,
 * report.err_initial / err_final, srk_ba_iteration_log and srk_ba_phase_error use; srk_ba_reproj_error* stay the reprojection
 * sums.  A factor adds 2 J_a^T L J_a and 2 J_b^T L J_b to the pose part of the two frame blocks (before the damping),
 * 2 J_a^T L e and 2 J_b^T L e to the two frame gradients, and 2 J_a^T L J_b as the pose x pose block (a, b) of the reduced camera
 * system, undamped.  The Jacobians are exact (the inverse right Jacobian of SO(3) at e_r included), so the gradient is the
 * gradient of E.  The pairs enter the covisibility: the frame renumbering, the skyline and the solver plans know them.
 *
 * n = 0 clears the setting (the default).  The handle keeps a copy: it is applied by every later upload
 * (srk_ba_compute_inplace and srk_ba_compute_inplace_f32 included) and is not touched by srk_ba_reset_scene.  It takes effect
 * at the next upload, which maps it to the normalised scene X_n = s (R0 X + T0): Z and L_rr stay, z_n = s z, L_tt / s^2,
 * L_tr / s (srk_ba_normalize_relative_pose_factors).  An index beyond the uploaded scene's frames fails that upload with
 * SRK_E_ARGS.  A factor whose L is all zeros is switched off: the upload leaves it out, plan included.
 *
 * There is no keep_gauge argument: relative poses leave the rigid motion of the world free and fix its scale only through
 * their translation parts.  The gauge is what srk_ba_set_constant_blocks and srk_ba_set_position_priors say, by default the
 * reference's seven variables -- the scale is then held at the initial scene's and metric factors pull within it.  For metric
 * scale: srk_ba_set_constant_blocks with frame 0 constant and keep_gauge = 0.  A factor to a constant frame acts as an
 * absolute pull on the other frame.
 *
 * SRK_E_ARGS (text in srk_ba_last_error), the previous setting staying in force: a == b, a negative index, an unordered pair
 * given twice (in either direction), pairs not sorted by (min, max), a value that is not finite, a Z that is not a rotation to
 * 1e-9 (orthogonality and determinant), an L that is not positive semi-definite, a NULL array.  Refused with SRK_E_ARGS by
 * whichever call comes second: intrinsic groups, more than one rank.  Everything else works unchanged.  Three small passes
 * impose the factors (behind the derivative kernels, behind the assembly of the reduced camera system, beside the error
 * kernel); none is launched without factors. */
int srk_ba_set_relative_pose_factors(srk_ba*, int32_t n, const int32_t* frame_a, const int32_t* frame_b /* caller's numbering */,
                                     const double* rel_R /* [n][9] */, const double* rel_t /* [n][3] */,
                                     const double* info /* [n][21] */);
/* host only, no device and no handle needed: the checks of the setter on their own.  SRK_OK, or SRK_E_ARGS with *why (may be
 * NULL) pointing at a static text. */
int srk_ba_check_relative_pose_factors(int32_t n, const int32_t* frame_a, const int32_t* frame_b, const double* rel_R,
                                       const double* rel_t, const double* info, const char** why);
/* the count of the stored setting; returns 1 if a setting is stored, 0 if not */
int srk_ba_relative_pose_factor_count(srk_ba*, int32_t* n);
/* the stored setting (what the NEXT upload applies) into arrays of the sizes the count gives; any pointer may be NULL.
 * Returns 1 if a setting is stored, 0 if not. */
int srk_ba_relative_pose_factors(srk_ba*, int32_t* frame_a, int32_t* frame_b, double* rel_R, double* rel_t, double* info);
/* the factor sum of the resident scene's current state (0 without factors) */
int srk_ba_relative_pose_error(srk_ba*, double* e);
/* [e_t; e_r] [n][6] of the resident scene's current state in the caller's world units and radians, in the order of the
 * setting.  They belong to the setting the resident scene was uploaded with; if the stored setting has been changed since,
 * the call fails with SRK_E_STATE until the scene is uploaded again. */
int srk_ba_relative_pose_residuals(srk_ba*, double* r);
/* host only, no device needed: measured translations [n][3] and information matrices [n][21] through a normaliser, as the
 * upload maps them.  Either pair of arrays may be NULL.  Returns SRK_OK or SRK_E_ARGS. */
int srk_ba_normalize_relative_pose_factors(const srk_ba_normalizer* nrm, int32_t n, const double* rel_t, const double* info,
                                           double* rel_t_out, double* info_out);
/* device time in ms of the last launch of the three passes, taken with srk_ba_set_profile >= 1; 0 for a pass that was not
 * launched or not timed.  One event pair a pass serves all attempt slots (tools/relpose_rate.py switches speculation off). */
int srk_ba_relative_pose_pass_ms(srk_ba*, double* derivative_ms, double* couple_ms, double* error_ms);

/* ---- joint Gaussian pose priors over sets of frames (EXTENSION) ----
 * The prior a marginalised window leaves behind: a dense Gaussian over the poses of the k frames that shared landmarks with
 * what was dropped, the inverse of a joint covariance block (srk_ba_cross_covariances).  With k = 1 it is the full pose prior:
 * position and attitude of one frame with a 6 x 6 information matrix.  Set g holds k_g frames, 1 <= k_g <= 16: the slots
 * set_ptr[g] .. set_ptr[g + 1] of frame[], caller's numbering, strictly ascending inside a set.  Slot i has a linearisation
 * pose: the world -> camera rotation Rbar_i (lin_R, 3 x 3 row-major) and the centre Cbar_i (lin_C), in the caller's world
 * coordinates.  The set has a mean m_g of 6 k_g values (mean; NULL = zeros for every set) and a symmetric positive semi-definite
 * information matrix L_g, dense row-major (6 k_g)^2, the sets' matrices one behind the other in info[]; variable order slot by
 * slot, [t; r] inside a slot.  With R_i, C_i = -R_i^T T_i the current pose:
 *
 *     r_i = [ C_i - Cbar_i ; Log(R_i^T Rbar_i) ]    (rotation vector of the direct rotation relative to the linearisation, angle < pi)
 *     E = (everything E is without these priors) + sum_g (r_g - m_g)^T L_g (r_g - m_g)
 *
 * This is the pose perturbation of the covariance calls ([centre; rotation vector applied to the direct rotation from the
 * left], srk_ba_revert_covariances), so the inverse of a joint covariance is usable as it comes.  L is in units of E,
 * (pix / f0)^2, per squared world unit (tt), per world unit and radian (tr), per squared radian (rr): a Gaussian of covariance
 * Sigma beside observations of pixel noise sigma_px is L = (sigma_px / f0)^2 Sigma^-1.  No robust loss and no observation
 * information acts on it.  This E is what the accept / reject test, both termination tests, report.err_initial / err_final,
 * srk_ba_iteration_log and srk_ba_phase_error use; srk_ba_reproj_error* stay the reprojection sums.  With J_i = diag(I,
 * Jl^-1(r_r,i)) (the inverse left Jacobian of SO(3), exact, so the gradient is the gradient of E) a set adds 2 J_i^T L_ii J_i to
 * the pose part of frame i's block (before the damping), 2 J_i^T (L (r - m))_i to its gradient and 2 J_i^T L_ij J_j as the
 * pose x pose block (i, j) of the reduced camera system, undamped.  The intrinsic variables get nothing.
 *
 * A pair of slots whose 6 x 6 block L_ij is all zeros is no coupling; the other pairs enter the covisibility like the pairs of
 * relative-pose factors: the frame renumbering, the skyline and the solver plans know them.  A set whose L is all zeros is
 * switched off: the upload leaves it out, plan included.  Two sets may share at most one frame.  A pair may carry a
 * relative-pose factor as well.
 *
 * keep_gauge as for position priors: 1 keeps the reference's seven gauge variables; 0 releases them -- the caller then asserts
 * that the priors fix the seven freedoms (one full-rank pose prior fixes six, a second frame with a distinct centre the scale).
 * The gauge is released when any of srk_ba_set_constant_blocks, srk_ba_set_position_priors and this call says 0.
 *
 * n_sets = 0 clears the setting (the default).  The handle keeps a copy (L symmetrised): it is applied by every later upload
 * (srk_ba_compute_inplace and srk_ba_compute_inplace_f32 included) and is not touched by srk_ba_reset_scene.  The upload maps it
 * to the normalised scene (srk_ba_normalize_joint_pose_priors).  An index beyond the uploaded scene's frames fails that upload
 * with SRK_E_ARGS.
 *
 * SRK_E_ARGS (text in srk_ba_last_error), the previous setting staying in force: a set size outside 1..16, frames not strictly
 * ascending or negative, two sets sharing more than one frame, a value that is not finite, a lin_R that is not a rotation to
 * 1e-9, an L not symmetric to 1e-12 of its largest entry, an L that is not positive semi-definite, a NULL array (mean
 * excepted), keep_gauge outside {0, 1}.  Refused with SRK_E_ARGS by whichever call comes second: intrinsic groups, more than one
 * rank.  Everything else works unchanged.  Three small passes impose the priors (behind the derivative kernels, behind the
 * assembly of the reduced camera system, beside the error kernel); none is launched without switched-on sets. */
int srk_ba_set_joint_pose_priors(srk_ba*, int32_t n_sets, const int32_t* set_ptr /* [n_sets + 1] */, const int32_t* frame,
                                 const double* lin_R /* [][9] */, const double* lin_C /* [][3] */, const double* mean /* [][6] or NULL */,
                                 const double* info, int keep_gauge);
/* host only, no device and no handle needed: the checks of the setter on their own.  SRK_OK, or SRK_E_ARGS with *why (may be
 * NULL) pointing at a static text. */
int srk_ba_check_joint_pose_priors(int32_t n_sets, const int32_t* set_ptr, const int32_t* frame, const double* lin_R,
                                   const double* lin_C, const double* mean, const double* info, int keep_gauge, const char** why);
/* the sizes of the stored setting: sets, slots (the length of frame[]) and doubles of info[]; returns 1 if a setting is stored,
 * 0 if not */
int srk_ba_joint_pose_prior_counts(srk_ba*, int32_t* n_sets, int32_t* n_frames, int64_t* n_info);
/* the stored setting (what the NEXT upload applies) into arrays of the sizes the counts give; any pointer may be NULL.
 * Returns 1 if a setting is stored, 0 if not. */
int srk_ba_joint_pose_priors(srk_ba*, int32_t* set_ptr, int32_t* frame, double* lin_R, double* lin_C, double* mean, double* info,
                             int* keep_gauge);
/* the priors' sum of the resident scene's current state (0 without switched-on sets) */
int srk_ba_joint_pose_prior_error(srk_ba*, double* e);
/* r - m [slots][6] of the resident scene's current state in the caller's world units and radians, in the order of the setting.
 * They belong to the setting the resident scene was uploaded with; if the stored setting has been changed since, the call fails
 * with SRK_E_STATE until the scene is uploaded again. */
int srk_ba_joint_pose_prior_residuals(srk_ba*, double* r);
/* host only, no device needed: linearisation poses, means and information matrices through a normaliser, as the upload maps
 * them.  With X_n = s (R0 X + T0): Cbar_n = s (R0 Cbar + T0), Rbar_n = Rbar R0^T, m_n = D m and L_n = D^-T L D^-1 with
 * D = diag(s R0, R0) per slot; the energy is invariant.  Each in / out pair of arrays may be NULL.  SRK_OK or SRK_E_ARGS. */
int srk_ba_normalize_joint_pose_priors(const srk_ba_normalizer* nrm, int32_t n_sets, const int32_t* set_ptr, const double* lin_R,
                                       const double* lin_C, const double* mean, const double* info, double* lin_R_out,
                                       double* lin_C_out, double* mean_out, double* info_out);
/* device time in ms of the last launch of the three passes, taken with srk_ba_set_profile >= 1; 0 for a pass that was not
 * launched or not timed.  One event pair a pass serves all attempt slots (tools/jointprior_rate.py switches speculation off). */
int srk_ba_joint_pose_prior_pass_ms(srk_ba*, double* derivative_ms, double* couple_ms, double* error_ms);

/* ---- marginalisation priors in information form (EXTENSION) ----
 * The operation a sliding window needs: drop a few frames D of the resident scene and the landmarks P that go with them, and get
 * the Gaussian that exactly the factors touching them leave on the poses of the frames that stay -- in information form,
 * linearised at the current poses, ready for srk_ba_set_joint_pose_priors on the reduced scene.  A joint pose prior set that
 * contains a dropped frame is absorbed, mean included, so a window can slide again and again.
 *
 * drop [n_drop]: frames, the caller's numbering, strictly ascending, n_drop <= 8.  points [n_points]: landmarks, the caller's
 * numbering, strictly ascending.  One of the lists may be empty.  The involved factors F are: every observation with information
 * q > 0 of a landmark of P; the position priors of the landmarks of P and of the centres of the frames of D; every switched-on
 * relative-pose factor with an end in D; every switched-on joint set that contains a frame of D (the whole set).  A landmark of
 * P with fewer than two weighted observations is left out with its prior (one view constrains no pose).  The kept frames K are
 * the frames outside D that F touches, ascending, at most 32; a result over at most 16 can be set as one joint set as it comes.
 *
 * With x the pose perturbations of sections 16 to 18 ([centre; rotation vector applied to the direct rotation from the left]; at
 * the linearisation the solver's [Tx Ty Tz Wx Wy Wz] step) of D, then K, the Gauss-Newton model of the sum of F at the current
 * scene is E_F(x) ~ E_0 + 2 b^T x + x^T A x: robust and information weights frozen at the current residuals, the relative-pose and
 * joint-set terms with their exact Jacobians, the intrinsics constants (ten-variable layout too), the gauge ignored.  The
 * landmarks of P are eliminated first, then D:
 *     Lam = A_KK - A_KD A_DD^-1 A_DK,   eta = b_K - A_KD A_DD^-1 b_D,   Lam m = -eta
 * so that (r - m)^T Lam (r - m) is E_F on K up to a constant.  A and b are HALF of what the reduced camera system and its
 * right-hand side carry in the library's factor-2 convention.  Lam is singular along whatever F does not determine; m is the
 * basic solution of a diagonally pivoted elimination (components of null pivots are zero).
 *
 * Refused with SRK_E_ARGS (text in srk_ba_last_error), nothing written: a weighted observation in a frame of D whose landmark is
 * not in P (the result would be a prior on a landmark: put it into P, or switch the observation off with
 * srk_ba_set_observation_information); constant blocks; intrinsic groups; more than one rank; an index beyond the scene; a list
 * not strictly ascending; both lists empty; more than 8 dropped or more than 32 kept frames (the text names the count); kept_cap
 * smaller than the number of kept frames.  None of the calls changes the resident scene, its systems or any setting, and no other
 * call launches their kernels. */
typedef struct srk_ba_marg_counts {
    int32_t n_drop, n_kept;
    int64_t n_landmarks;          /* landmarks of P that enter */
    int64_t n_landmarks_skipped;  /* landmarks of P with fewer than two weighted observations */
    int64_t n_observations;       /* observations (weighted or not) of the entering landmarks */
    int32_t n_factors, n_sets, n_frame_priors; /* involved relative-pose factors, joint sets, priors on centres of D */
} srk_ba_marg_counts;
typedef struct srk_ba_marg_report {
    int64_t landmarks_used;       /* landmarks of P that entered the sum */
    int64_t landmarks_skipped;    /* fewer than two weighted observations, or an undamped 3 x 3 block that fails the pivot test */
    int32_t factors, sets, frame_priors; /* absorbed relative-pose factors, joint sets, priors on centres of D */
    double defect;                /* |Lam m + eta|_inf / |eta|_inf in the normalised variables (0 when eta is zero) */
    double ms_rows, ms_gram;      /* device ms of the two kernels with their small second passes, from event pairs */
    double ms_host;               /* host ms of the factor terms, the elimination and the map into the caller's coordinates */
} srk_ba_marg_report;
/* The plan of a call on the resident scene, for sizing: no kernel is launched.  kept (may be NULL: counts only) receives the kept
 * frames when kept_cap holds them.  SRK_OK, SRK_E_STATE without a scene, SRK_E_ARGS for every refusal above. */
int srk_ba_marginalization_plan(srk_ba*, int32_t n_drop, const int32_t* drop, int64_t n_points, const int64_t* points, int32_t kept_cap,
                                int32_t* kept, srk_ba_marg_counts* counts);
/* The staged form, in the variables of the resident (normalised) scene, n = n_drop + n_kept slots, D first: A0 [(6 n)^2], b0 [6 n]
 * what the two kernels give (observations and landmark priors, P eliminated), A1, b1 the same plus the host's terms (priors on
 * centres of D, relative-pose factors, joint sets), before the elimination of D.  Any output may be NULL.  Returns as the plan. */
int srk_ba_phase_marginalization(srk_ba*, int32_t n_drop, const int32_t* drop, int64_t n_points, const int64_t* points, int32_t kept_cap,
                                 int32_t* kept, int32_t* n_kept, double* A0, double* b0, double* A1, double* b1, srk_ba_marg_report* report);
/* The whole operation.  Outputs over the k kept frames, in the coordinates of the uploaded arrays and the units
 * srk_ba_set_joint_pose_priors takes (through srk_ba_revert_marginalization_prior when the upload normalised the scene): lin_R
 * [k][9], lin_C [k][3] the current poses, info [(6 k)^2] Lam (symmetric), eta [6 k], mean [6 k].  Any output may be NULL.  Returns
 * SRK_OK; 1 when A_DD is not positive definite (a lone kept frame cannot fix a dropped frame's scale, for instance), nothing
 * written; else as the plan. */
int srk_ba_marginalization_prior(srk_ba*, int32_t n_drop, const int32_t* drop, int64_t n_points, const int64_t* points, int32_t kept_cap,
                                 int32_t* kept, int32_t* n_kept, double* lin_R, double* lin_C, double* info, double* eta, double* mean,
                                 srk_ba_marg_report* report);
/* host only, no device and no handle needed: the dense elimination on caller-given A [(6 (d + k))^2] (symmetric) and b, D first.
 * A_DD is eliminated with diagonal pivoting and the threshold of the positive-semi-definite check of the setters (a pivot
 * <= 1e-12 of its largest entry is not positive: returns 1, nothing written); mean is the basic solution of the same elimination
 * of Lam.  Any output may be NULL.  SRK_OK, 1, or SRK_E_ARGS. */
int srk_ba_marginalize_dense(const double* A, const double* b, int32_t d, int32_t k, double* info, double* eta, double* mean, double* defect);
/* host only: the inverse of the map of srk_ba_normalize_joint_pose_priors on one result over k frames, in place; any array may be
 * NULL.  lin_R = lin_R_n R0, lin_C = R0^T (lin_C_n / s - T0), Lam = D^T Lam_n D, eta = D^T eta_n, m = D^-1 m_n with
 * D = diag(s R0, R0) per frame; the energy is invariant.  SRK_OK or SRK_E_ARGS. */
int srk_ba_revert_marginalization_prior(const srk_ba_normalizer* nrm, int32_t k, double* lin_R, double* lin_C, double* info, double* eta,
                                        double* mean);

/* ---- batched landmark triangulation and refinement on the device (EXTENSION) ----
 * The front half of a sliding window: a new keyframe brings new tracks, and a landmark has to exist before srk_ba_upload_scene
 * can take it.  Track i owns the observations row_ptr[i] .. row_ptr[i + 1] (any length, 0 included): frame[o] in [0, n_frames),
 * uv[o] in pixels, q[o] >= 0 its information (q NULL = all 1; q = 0 switches an observation off, and the track then has the
 * bits of the track without it).
 *
 * Linear stage: the system of Triangulate3DPointByLeastSquares (cpp_impl/suriko-engine/src/obs-geom.cpp:679-727), two rows
 * x p2 - f0 p0 and y p2 - f0 p1 per observation with P = K [R | T] built on the device, scaled by sqrt(q), solved by a streaming
 * Givens QR factorisation (never the normal equations: relative error ~ eps cond(A), not eps cond(A)^2).  Refinement (options
 * given, refine_attempts > 0): Levenberg-Marquardt on E(X) = sum q |uv - pi(X)|^2 in pixels from the linear result: damping factor
 * 1e-4, x 10 on a rejected attempt, / 10 on an accepted one, each attempt solves (H + c diag H) d = -g with H = sum q J^T J, an
 * attempt is accepted iff E decreases, the loop stops when an accepted attempt changes E by less than refine_rel_change E or
 * after refine_attempts attempts (at most 64).  The result never has a larger E than the linear one.
 *
 * Outputs per track: X [3]; quality [4] = { sqrt(E / n) in pixels at X, the largest angle in degrees between the viewing ray of
 * a weighted observation and that of the first weighted one, the 1-norm condition number of the 3 x 3 triangular factor, the
 * number n of weighted observations }; status, a mask of SRK_TRI_*.  The library applies no threshold of its own: condition and
 * parallax are reported, the caller decides (min_parallax_deg = 0: no gate).  With SRK_TRI_FEW_VIEWS X, quality[0] and
 * quality[2] are NaN.  No atomics and a fixed merge order: a track's bits depend on its own observations alone.
 *
 * srk_triangulate_tracks takes the poses from the caller (cam_R [n_frames][9], cam_T [n_frames][3] inverse poses, K
 * [n_frames][9] or [9] with shared_k) and, like srk_mvf_estimate_depths, leaves an uploaded scene untouched; no normalisation, no
 * planning.  srk_ba_triangulate reads the CURRENT poses and K of the resident scene on the device (after srk_ba_optimize: the
 * refined ones), maps the caller's frame numbers through the handle's frame order, triangulates in the normalised coordinates
 * and, with revert_normalization = 1, returns X in the coordinates of the uploaded arrays; nothing is downloaded but the results
 * and the resident scene is not modified.  It is refused with more than one rank and with intrinsic groups.
 *
 * Every index is checked on the host before anything is launched: SRK_E_ARGS (text in srk_ba_last_error) for a row_ptr that does
 * not start at 0 or decreases, a frame outside [0, n_frames), a q that is negative or not finite, a uv that is not finite, a NULL
 * array with a positive count, refine_attempts outside 0..64, a refine_rel_change or min_parallax_deg that is negative or not
 * finite.  SRK_E_STATE: srk_ba_triangulate without a scene. */
enum {
    SRK_TRI_FEW_VIEWS = 1,      /* fewer than two observations with q > 0: X is NaN */
    SRK_TRI_DEGENERATE = 2,     /* a zero or non-finite diagonal of the factor, or a non-finite X (srk_triangulate_least_squares returns 0) */
    SRK_TRI_BEHIND = 4,         /* depth <= 0 in some weighted frame */
    SRK_TRI_LOW_PARALLAX = 8,   /* quality[1] < min_parallax_deg */
    SRK_TRI_NOT_CONVERGED = 16  /* the refinement used all its attempts */
};
typedef struct srk_tri_options {
    int32_t refine_attempts;    /* 0 = linear only; at most 64 */
    double refine_rel_change;   /* stop when an accepted attempt changes E by less than this times E */
    double min_parallax_deg;    /* 0 = no gate */
} srk_tri_options;
void srk_tri_default_options(srk_tri_options*); /* { 10, 1e-9, 0 } */
int srk_triangulate_tracks(srk_ba*, double f0, int64_t n_tracks, const int64_t* row_ptr, const int32_t* frame, const double* uv /* [O][2] */,
                           const double* q /* [O], NULL = all 1 */, int32_t n_frames, const double* cam_R, const double* cam_T,
                           const double* K, int shared_k, const srk_tri_options* /* NULL = linear only */, double* X /* [n][3] */,
                           double* quality /* [n][4] */, uint32_t* status /* [n] */);
int srk_ba_triangulate(srk_ba*, int64_t n_tracks, const int64_t* row_ptr, const int32_t* frame /* caller's numbering */, const double* uv,
                       const double* q, const srk_tri_options*, int revert_normalization, double* X, double* quality, uint32_t* status);
/* device ms of the two kernels (the frames' packs, the tracks) of the last of the two calls on this handle, from an event pair */
double srk_ba_triangulate_kernel_ms(const srk_ba*);
/* host only, no device and no handle needed: the checks of the two calls on their own.  SRK_OK, or SRK_E_ARGS with *why (may be
 * NULL) pointing at a static text. */
int srk_tri_check_tracks(int64_t n_tracks, const int64_t* row_ptr, const int32_t* frame, const double* uv, const double* q, int32_t n_frames,
                         const srk_tri_options* opts, const char** why);
/* host only: points of the normalised scene to the caller's coordinates, in place: X = R0^T (X_n / s - T0) */
int srk_tri_revert_points(const srk_ba_normalizer* nrm, int64_t n, double* X);

/* ---- batched camera resection with robust pose refinement on the device (EXTENSION) ----
 * The other half of a sliding window's front: a new keyframe needs a pose before its tracks can be triangulated and before
 * srk_ba_upload_scene can take it, and that pose comes from 2D-3D correspondences with landmarks the map already has -- wrong
 * matches among them.  Relocalising frames against a finished map and checking loop-closure candidates have the same shape.
 * Frame i owns the observations row_ptr[i] .. row_ptr[i + 1] (any length, 0 included): point[o] in [0, n_points) indexes the
 * landmarks X [n_points][3], uv[o] in pixels, q[o] >= 0 its information (q NULL = all 1, bit for bit; q = 0 switches an
 * observation off, and the frame then has the bits of the frame without it).  The caller gives a predicted inverse pose
 * (R0, T0) per frame (the previous keyframe, odometry, srk_mvf_relative_motion): there is no start without a pose.
 *
 * With x_cam = R X + T, C = -R^T T and e_o = pi(K (R X_o + T)) - uv_o in pixels, s_o = |e_o|^2, the call minimises
 * E = sum_o rho(q_o s_o) per frame: rho none (0), Huber (1) or Cauchy (2) with delta in pixels, the formulas of
 * srk_ba_set_robust_loss.  The six variables are the pose perturbation of the covariance and joint-prior calls, [t; w] with
 * C <- C + t and R^T <- Exp(w) R^T; the Jacobian d x_cam / d [t; w] = R [ -I | [X - C]x ] is exact, and with w_o = rho'(q_o s_o)
 * H = sum q_o w_o J_o^T J_o, g = sum q_o w_o J_o^T e_o.  Levenberg-Marquardt with the project's damping rule: factor 1e-4, x 10 on
 * a rejected attempt, / 10 on an accepted one; an attempt solves (H + c diag H) d = -g by a written-out 6 x 6 Cholesky
 * factorisation and walks the moved pose once; it is accepted iff E decreases (a failed factorisation or a non-finite E is a
 * rejected attempt); the loop stops when an accepted attempt changes E by less than rel_change E, or after `attempts` attempts
 * (at most 64; 0 = evaluate only).  The result never has a larger E than the start.
 *
 * Outputs per frame: R [9], T [3] the inverse pose (the rotation is a product of rotations, never a sum); quality [6] =
 * { sqrt(E / n) in pixels, the number n of observations with q > 0, sum w_o / n (the effective inlier share; 1 without a loss),
 * cond_1 of the Jacobi-scaled H_s = D^-1/2 H D^-1/2, the smallest depth of a weighted observation, the attempts used };
 * info [36] = H / f0^2 at the result, undamped, row-major; status, a mask of SRK_RESECT_*; and optionally w_out [O], the robust
 * weight rho'(q s) of every observation at the result (0 where q = 0; NULL = not wanted), from which the caller reads the wrong
 * matches.  The library applies no threshold of its own.
 *
 * info is in the units of srk_ba_set_joint_pose_priors: with pixel noise sigma_px the covariance of the six variables is
 * Sigma = sigma_px^2 H^-1; the library's energies are in units of (pixels / f0)^2, in which the observations' noise is
 * (sigma_px / f0)^2, so the information that reproduces this frame's observations as a prior term (r - m)^T L (r - m) is
 * L = (sigma_px / f0)^2 Sigma^-1 = H / f0^2.  With the result as linearisation pose and a zero mean it is a one-frame set as it
 * comes.
 *
 * srk_resect_frames takes landmarks and poses from the caller and leaves an uploaded scene untouched.  srk_ba_resect reads the
 * CURRENT landmarks of the resident scene on the device (after srk_ba_optimize: the refined ones), maps the caller's landmark
 * numbers through the handle's landmark order, maps the start poses into the normalised coordinates (R_n = R R0^T,
 * T_n = s (T - R_n T0)), refines there and, with revert_normalization = 1, returns poses and info in the coordinates of the
 * uploaded arrays (info by the inverse of what srk_ba_revert_covariances does to a pose covariance; quality[3] is then taken
 * again from that info and quality[4] divided by the scale, so that both are those of the returned coordinates).  Nothing is
 * downloaded but the results and no buffer of the scene is written.  It is refused with more than one rank.
 *
 * Every index is checked on the host before anything is launched: SRK_E_ARGS (text in srk_ba_last_error) for a row_ptr that does
 * not start at 0 or decreases, a point outside [0, n_points), a q that is negative or not finite, a uv, X, K, R0 or T0 entry that
 * is not finite, an R0 that is not a rotation to 1e-9 (the joint-prior setter's rule), attempts outside 0..64, a negative or
 * non-finite rel_change, a loss kind outside 0..2, a loss with delta <= 0, a NULL array with a positive count.  SRK_E_STATE:
 * srk_ba_resect without a scene. */
enum {
    SRK_RESECT_FEW_POINTS = 1,    /* fewer than three observations with q > 0: the pose is the start, quality[3] is NaN */
    SRK_RESECT_DEGENERATE = 2,    /* the scaled H at the result is not positive definite, or something is not finite */
    SRK_RESECT_BEHIND = 4,        /* a weighted observation at depth <= 0 at the result */
    SRK_RESECT_NOT_CONVERGED = 8  /* the loop used all its attempts */
};
typedef struct srk_resect_options {
    int32_t attempts;           /* 0 = evaluate only; at most 64 */
    double rel_change;          /* stop when an accepted attempt changes E by less than this times E */
    int32_t loss_kind;          /* 0 none, 1 Huber, 2 Cauchy */
    double loss_delta_pixels;   /* > 0 with a loss */
} srk_resect_options;
void srk_resect_default_options(srk_resect_options*); /* { 10, 1e-9, 0, 0 } */
int srk_resect_frames(srk_ba*, double f0, int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv /* [O][2] */,
                      const double* q /* [O], NULL = all 1 */, int64_t n_points, const double* X /* [n_points][3] */,
                      const double* K /* [n_frames][9], or [9] with shared_k */, int shared_k, const double* R0 /* [n][9] */,
                      const double* T0 /* [n][3] */, const srk_resect_options* /* NULL = the defaults */, double* R /* [n][9] */,
                      double* T /* [n][3] */, double* quality /* [n][6] */, double* info /* [n][36] */, uint32_t* status /* [n] */,
                      double* w_out /* [O] or NULL */);
int srk_ba_resect(srk_ba*, int32_t n_frames, const int64_t* row_ptr, const int32_t* point /* caller's landmark numbering */,
                  const double* uv, const double* q, const double* K, int shared_k, const double* R0, const double* T0,
                  const srk_resect_options*, int revert_normalization, double* R, double* T, double* quality, double* info,
                  uint32_t* status, double* w_out);
/* device ms of the two kernels (the start poses' packs, the frames) of the last of the two calls on this handle, from an event pair */
double srk_ba_resect_kernel_ms(const srk_ba*);
/* host only, no device and no handle needed: the checks of srk_resect_frames on their own.  SRK_OK, or SRK_E_ARGS with *why (may
 * be NULL) pointing at a static text. */
int srk_resect_check_frames(int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv, const double* q, int64_t n_points,
                            const double* X, const double* K, int shared_k, const double* R0, const double* T0, const srk_resect_options* opts,
                            const char** why);
/* host only: results of the normalised scene to the caller's coordinates, in place: R = R_n R0, T = T_n / s + R_n T0,
 * info = D^T info_n D with D = diag(s R0, R0); R and T together or both NULL, info may be NULL */
int srk_resect_revert(const srk_ba_normalizer* nrm, int32_t n, double* R, double* T, double* info);

/* ---- resection without a start pose: P3P hypotheses scored on the device (EXTENSION) ----
 * srk_resect_frames needs a predicted pose, and that is missing exactly where resection matters most: relocalisation after
 * tracking is lost, loop-closure candidates, the first frame against a finished map, unordered image sets.  "locate" finds the
 * pose of each frame from its 2D-3D correspondences alone, wrong matches among them, by hypothesise-and-verify (the reference's
 * GetMaxSubsetInConsensus / RansacIterationsCount, py_proto/suriko/mvg.py), and can hand it to the refinement of section 22
 * without leaving the device.
 *
 * Observations as in srk_resect_frames: CSR by frame, q >= 0 (NULL = all 1, bit for bit; q = 0 = the frame without that
 * observation, bit for bit).  Everything works on the frame's n weighted observations, numbered by rank 0 .. n - 1 in ascending o.
 *
 * Sampler (counter-based, no state): mix(seed, h, k) = the splitmix64 finaliser (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 * z *= 0x94D049BB133111EB; z ^= z >> 31) of seed + 0x9E3779B97F4A7C15 (4 h + k + 1) mod 2^64.  Draw k = 0..3 of hypothesis h is
 * r = umulhi64(mix, n - k), then for the earlier picks s in ascending order: if (r >= s) ++r.  Four distinct ranks; the key holds
 * neither the frame's place in the batch nor the batch size.
 *
 * Hypothesis: bearings b ~ K^-1 (u, v, f0), normalised (K a general 3 x 3, inverted by its adjugate).  P3P on picks 0-2 gives up
 * to four poses (R, T), x_cam = R X + T; those with a depth <= 0 at any of the four sample points are dropped and the one with the
 * smallest squared pixel error at pick 3 is the hypothesis' pose (a tie: the earlier root).  R is a product of two orthonormal
 * frames, so it passes the rotation check of srk_resect_frames.
 *
 * Score (MSAC): score(h) = sum over the ranks in ascending order of min(q s, tau^2), s the squared pixel error; an observation at
 * depth <= 0 counts tau^2; a hypothesis without a pose scores +inf.  The smallest score wins, an equal score goes to the smaller h.
 *
 * Outputs per frame: R [9], T [3]; located [6] = { sqrt(score / n) in pixels, n, the inlier count at the located pose, the winning
 * h, the number of hypotheses that produced a pose, the reprojection error in pixels of the winning sample's fourth point };
 * located_status, a mask of SRK_LOCATE_*: then the pose is (I, 0), located[0], [3], [5] are NaN and located[2] is 0.  inlier_out [O]
 * (may be NULL): 1 iff q_o > 0, the depth is positive and q_o s_o < tau^2 at the located pose, before any refinement.
 *
 * With refine != NULL the located poses stay on the device and are the R0, T0 of the kernels of srk_resect_frames: R, T, quality,
 * info, status and w_out are then bit for bit what srk_resect_frames returns from the located poses (a frame that was not located
 * is refined from (I, 0) like any other; its located_status says not to trust the result), and located, located_status and
 * inlier_out are the same with and without.  Without refine, R and T are the located poses and the last four may be NULL.
 *
 * srk_ba_locate reads the CURRENT landmarks of the resident scene on the device through the handle's landmark order, locates in
 * the normalised coordinates and, with revert_normalization = 1, maps poses and info back with the maps of srk_ba_resect.  It
 * writes no scene buffer and is refused with more than one rank.
 *
 * Host checks before any launch (SRK_E_ARGS with a text): everything srk_resect_check_frames checks except the start poses,
 * hypotheses outside 1..4096, inlier_pixels not finite or <= 0, a K that is singular, NULL outputs, and more than 2^22 waves of
 * hypotheses (frames x ceil(hypotheses / 64)) in one call: split the batch, a frame's bits do not depend on it. */
enum {
    SRK_LOCATE_FEW_POINTS = 1, /* fewer than four observations with q > 0 */
    SRK_LOCATE_NO_MODEL = 2    /* no sample gave a pose with positive depths */
};
typedef struct srk_locate_options {
    int32_t hypotheses;   /* samples per frame, 1 .. 4096 */
    double inlier_pixels; /* tau > 0: the truncation of the score and the inlier test */
    uint64_t seed;
} srk_locate_options;
void srk_locate_default_options(srk_locate_options*); /* { 256, 4.0, 1 } */
int srk_locate_frames(srk_ba*, double f0, int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv /* [O][2] */,
                      const double* q /* [O], NULL = all 1 */, int64_t n_points, const double* X /* [n_points][3] */,
                      const double* K /* [n_frames][9], or [9] with shared_k */, int shared_k, const srk_locate_options* /* NULL = the defaults */,
                      const srk_resect_options* refine /* NULL = no refinement */, double* R /* [n][9] */, double* T /* [n][3] */,
                      double* located /* [n][6] */, uint32_t* located_status /* [n] */, uint8_t* inlier_out /* [O] or NULL */,
                      double* quality, double* info, uint32_t* status, double* w_out /* the four of srk_resect_frames, used with refine */);
int srk_ba_locate(srk_ba*, int32_t n_frames, const int64_t* row_ptr, const int32_t* point /* caller's landmark numbering */,
                  const double* uv, const double* q, const double* K, int shared_k, const srk_locate_options*,
                  const srk_resect_options* refine, int revert_normalization, double* R, double* T, double* located,
                  uint32_t* located_status, uint8_t* inlier_out, double* quality, double* info, uint32_t* status, double* w_out);
/* device ms of the last of the two calls on this handle (gather, hypotheses and scores, pick, and the refinement when asked for),
 * from an event pair; and of the hypothesis-and-score kernel alone, from a second pair */
double srk_ba_locate_kernel_ms(const srk_ba*);
double srk_ba_locate_score_ms(const srk_ba*);
/* host only, no device and no handle needed: the checks of srk_locate_frames on their own.  SRK_OK, or SRK_E_ARGS with *why (may
 * be NULL) pointing at a static text. */
int srk_locate_check_frames(int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv, const double* q, int64_t n_points,
                            const double* X, const double* K, int shared_k, const srk_locate_options* opts, const srk_resect_options* refine,
                            const char** why);
/* the reference's RansacIterationsCount: ceil(log(1 - p) / log(1 - (1 - e)^s)) samples of size s reach, with probability p, one
 * without a wrong match at outlier ratio e.  e = 0 gives 1; e outside [0, 1), p outside (0, 1) or s < 1 gives SRK_E_ARGS. */
int64_t srk_ransac_hypotheses(int sample_size, double outlier_ratio, double success_probability);

/* ---- two-view relative pose: five-point hypotheses scored on the device (EXTENSION) ----
 * Triangulation, resection and locate all need a map or a pose to start from; "relate" produces the first one.  From the 2D-2D
 * matches of two images, wrong matches among them, it finds the rotation and the direction of the translation between the two
 * cameras by hypothesise-and-verify (the reference's FindRelativeMotion, py_proto/suriko/mvg.py: the five-point method, the
 * Sampson distance, the decomposition of the essential matrix and its GetMaxSubsetInConsensus loop).  The five-point method is not
 * degenerate on planar scenes, where the eight-point method is.
 *
 * Conventions: frame a is (I, 0), frame b is (R, T) with x_b ~ R x_a + T and |T| = 1 (the R X + T of srk_resect_frames).  E = [T]x R
 * exactly as returned, and x^_b^T E x^_a = 0 for the rays x^ = K^-1 (u, v, f0).  K and f0 as in srk_locate_frames.  Pairs in CSR
 * form with any number of matches; q >= 0 the optional information of a match (NULL = all 1, bit for bit; q = 0 = the pair without
 * that match, bit for bit).  Everything works on the pair's n weighted matches, numbered by rank 0 .. n - 1 in ascending o.
 *
 * Sampler (counter-based, no state, a stream of its own): mix(seed, h, k) = the splitmix64 finaliser of
 * seed + 0xD1B54A32D192ED03 (8 h + k + 1) mod 2^64.  Draw k = 0..5 of hypothesis h is r = umulhi64(mix, n - k), then for the
 * earlier picks s in ascending order: if (r >= s) ++r.  Six distinct ranks that depend on seed, h and k alone.
 *
 * Hypothesis: picks 0-4 give up to ten essential matrices (Nister's route: the null space of the 5 x 9 epipolar matrix, the ten
 * cubic constraints det E = 0 and 2 E E^T E - tr(E E^T) E = 0 eliminated to a 3 x 3 matrix B(z), the real roots of det B, a
 * polynomial of degree 10, by the derivative chain, each solution polished by Gauss-Newton steps on the constraints); pick 5
 * chooses the one with the smallest Sampson error, an equal error goes to the smaller root.
 *
 * Score (MSAC): score(h) = sum over the ranks in ascending order of min(q s, tau^2), s the squared Sampson distance in pixels of
 * F = K_b^-T E K_a^-1; a hypothesis without a model scores +inf.  The smallest score wins, an equal score goes to the smaller h.
 *
 * Pose: for the winner only (the four poses of an E have one score).  T is the unit vector along the largest cross product of two
 * columns of E, R1 = Cof(E) - [T]x E, R2 = Cof(E) + [T]x E; the four poses in the order (R1, T), (R1, -T), (R2, T), (R2, -T).  The
 * one with the most inliers at a positive distance along both rays is returned; a tie goes to the earlier in that order.
 *
 * Outputs per pair: R [9], T [3] (unit), E [9]; related [8] = { sqrt(score / n) in pixels, n, the inlier count, the winning h, the
 * number of hypotheses that gave a model, the sixth-match Sampson error in pixels, the number of inliers in front of both cameras
 * under the returned pose, the mean angle in radians between the two rays of those inliers (the parallax, summed per lane in
 * ascending rank and merged in a fixed tree) }.  The library has no threshold of its own: pure rotation and low parallax are read
 * from related[6] and related[7].  status, a mask of SRK_RELATE_*: then the pose is (I, 0), E is zero, related[0], [3], [5], [7] are
 * NaN and related[2], [6] are 0.  inlier_out [O] (may be NULL): 1 iff q_o > 0 and q_o s_o < tau^2 at the winner.
 *
 * Host checks before any launch (SRK_E_ARGS with a text): a descending or negative row_ptr, uv or K that is not finite, q negative
 * or not finite, a singular K, hypotheses outside 1..4096, inlier_pixels not finite or <= 0, NULL outputs, and more than 2^22
 * waves (pairs x ceil(hypotheses / 64)) in one call: split the batch, a pair's bits do not depend on it.  Nothing is allocated or
 * launched unless srk_relate_frames is called.  Absent: an adaptive early stop, several ranks.  The refinement of the winner over all
 * its matches is srk_relate_frames_refined, below. */
enum {
    SRK_RELATE_FEW_POINTS = 1, /* fewer than six matches with q > 0 */
    SRK_RELATE_NO_MODEL = 2    /* no sample gave an essential matrix */
};
typedef struct srk_relate_options {
    int32_t hypotheses;   /* samples per pair, 1 .. 4096 */
    double inlier_pixels; /* tau > 0: the truncation of the score and the inlier test */
    uint64_t seed;
} srk_relate_options;
void srk_relate_default_options(srk_relate_options*); /* { 256, 2.0, 1 } */
int srk_relate_frames(srk_ba*, double f0, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a /* [O][2] */, const double* uv_b /* [O][2] */,
                      const double* q /* [O], NULL = all 1 */, const double* K_a, const double* K_b /* [n_pairs][9], or [9] with shared_k */,
                      int shared_k, const srk_relate_options* /* NULL = the defaults */, double* R /* [n][9] */, double* T /* [n][3], unit */,
                      double* E /* [n][9] */, double* related /* [n][8] */, uint32_t* status /* [n] */, uint8_t* inlier_out /* [O] or NULL */);
/* device ms of the last srk_relate_frames on this handle (gather, solve, score, pick) from an event pair, and of the score kernel
 * alone from a second pair: the difference is, but for the gather and the pick, the five-point solve */
double srk_ba_relate_kernel_ms(const srk_ba*);
double srk_ba_relate_score_ms(const srk_ba*);
/* host only, no device and no handle needed: the checks of srk_relate_frames on their own.  SRK_OK, or SRK_E_ARGS with *why (may
 * be NULL) pointing at a static text. */
int srk_relate_check_pairs(int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q, const double* K_a,
                           const double* K_b, int shared_k, const srk_relate_options* opts, const char** why);
/* host only: one pair of n_obs matches in the kernels' own order of operations (the same statements, compiled for the host).
 * Returns the status bits, or SRK_E_ARGS (negative) when the checks refuse the pair. */
int srk_relate_host_pair(int64_t n_obs, const double* uv_a, const double* uv_b, const double* q, const double* K_a, const double* K_b, double f0,
                         const srk_relate_options* opts, double* R, double* T, double* E, double* related, uint8_t* inlier_out);

/* ---- two-view pose refinement: robust Sampson LM per pair on the device (EXTENSION) ----
 * srk_relate_frames returns the essential matrix of five matches, chosen by a sixth.  "refine pairs" is the step after it (the
 * reference's RefineFundMat, py_proto/suriko/mvg.py, minimises the Sampson distance from a start): per pair a Levenberg-Marquardt
 * loop on the robust Sampson error of all its matches over the five degrees of freedom of (R, unit T), one wave a pair, from a
 * start pose or chained behind relate without leaving the device, with the information of the result in the form
 * srk_ba_set_relative_pose_factors takes (srk_pair_factor).
 *
 * Conventions: relate's.  Frame a is (I, 0), frame b is (R, T) with x_b ~ R x_a + T and |T| = 1; E = [T]x R, F = K_b^-T E K_a^-1
 * (K a general 3 x 3, inverted by its adjugate), p = (u, v, f0).  The signed Sampson residual of a match is
 *     r = p_b^T F p_a / sqrt((F p_a)_0^2 + (F p_a)_1^2 + (F^T p_b)_0^2 + (F^T p_b)_1^2)   in pixels,   s = r^2,
 * the s of relate's score.  Pairs in CSR form; q >= 0 the optional information of a match (NULL = all 1, bit for bit; q = 0 = the
 * pair without that match, bit for bit).  Everything works on the pair's n weighted matches, numbered by rank in ascending o.
 *
 * Objective: E_pair = sum_o rho(q_o s_o), rho none, Huber or Cauchy with delta in pixels (the formulas of srk_ba_set_robust_loss).
 *
 * Variables d = [w (3); beta (2)]: R <- R Exp(w)^T, a product of rotations (as in srk_resect_frames), and T on the unit sphere,
 * T <- (T + b1 beta_1 + b2 beta_2) / |T + b1 beta_1 + b2 beta_2|.  The tangent basis is fixed by rule and recomputed from the
 * current T at every linearisation: k the index of the smallest |T_k| (a tie: the smaller k), b1 = (e_k x T) / |e_k x T|,
 * b2 = T x b1.
 *
 * Jacobian, exact: dE/dw_i = -[T]x R [e_i]x, dE/dbeta_j = [b_j]x R, dF_k = K_b^-T (dE/dd_k) K_a^-1, and dr by the quotient rule,
 * the derivative of the denominator included.  With w_o = rho'(q_o s_o): H = sum q_o w_o J_o^T J_o (5 x 5), g = sum q_o w_o J_o r_o.
 *
 * Loop: the rule of srk_resect_frames.  The damping factor c starts at 1e-4; an attempt solves (H + c diag H) d = -g by a
 * written-out 5 x 5 Cholesky factorisation, walks the moved pose once and is accepted iff E_pair decreases (c /= 10; otherwise, and
 * after a failed factorisation or a value that is not finite, c *= 10).  The loop stops when an accepted attempt changes E_pair by
 * less than rel_change E_pair, or after `attempts` attempts (0 .. 64; 0 = evaluate only: R0 and T0 come back bit for bit).  The
 * result never has a larger E_pair than the start.
 *
 * Outputs per pair: R [9], T [3] (unit), E [9] = [T]x R exactly as returned; quality [6] = { sqrt(E_pair / n) in pixels, n,
 * sum w_o / n, cond_1 of the Jacobi-scaled H (NaN when it is not positive definite), the number of weighted matches at a positive
 * distance along both rays at the result (the depth rule of relate's vote), the attempts used }; info [25] = H / f0^2 at the
 * result, undamped, row-major, in the order [w; beta]; basis [6] = b1, b2 at the result; status, a mask of SRK_PAIR_*; w_out [O]
 * (may be NULL): the robust weight of every match at the result, 0 where q = 0.  With FEW_POINTS the pose is the start, quality is
 * { NaN, n, NaN, NaN, NaN, 0 } and info is zero.  The library applies no threshold of its own: pure rotation (T not observable)
 * shows as a large quality[3].
 *
 * srk_relate_frames_refined runs relate's kernels unchanged; the related poses stay on the device and are the R0, T0 of the
 * refinement.  related, related_status and inlier_out are bit for bit those of srk_relate_frames; R, T, E, quality, info, basis,
 * status and w_out are bit for bit those of srk_refine_pairs from the related poses.  With inliers_only = 1 the refinement uses
 * q_o * inlier_o, the winner's inlier flags, formed on the device and frozen for the loop: the outputs are those of
 * srk_refine_pairs called with that product.  A pair that was not related is refined from (I, (1, 0, 0)) like any other; its
 * related_status says not to trust the result.
 *
 * Host checks before any allocation or launch (SRK_E_ARGS with a text): a row_ptr that does not start at 0 or decreases; a uv, K,
 * R0 or T0 entry that is not finite; a negative or not finite q; a singular K; an R0 that is not a rotation to 1e-9 (the rule of
 * srk_ba_set_joint_pose_priors); a T0 whose length is not 1 to 1e-9; attempts outside 0..64; a negative or not finite rel_change;
 * a loss kind outside 0..2; a loss with delta <= 0; inliers_only not 0 or 1 (and not 0 in srk_refine_pairs, where it has no
 * meaning); a NULL array with a positive count; NULL outputs (w_out may be NULL). */
enum {
    SRK_PAIR_FEW_POINTS = 1,   /* fewer than five matches with q > 0: the pose is the start */
    SRK_PAIR_DEGENERATE = 2,   /* the scaled H at the result is not positive definite, or something is not finite */
    SRK_PAIR_NOT_CONVERGED = 8 /* every attempt was used */
};
typedef struct srk_pair_options {
    int32_t attempts;         /* 0 .. 64; 0 = evaluate only */
    double rel_change;        /* stop when an accepted attempt changes E_pair by less than rel_change E_pair */
    int32_t loss_kind;        /* 0 none, 1 Huber, 2 Cauchy */
    double loss_delta_pixels; /* > 0 with a loss */
    int32_t inliers_only;     /* srk_relate_frames_refined: refine on the winner's inliers only; 0 elsewhere */
} srk_pair_options;
void srk_pair_default_options(srk_pair_options*); /* { 10, 1e-9, 0, 0, 0 } */
int srk_refine_pairs(srk_ba*, double f0, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a /* [O][2] */, const double* uv_b /* [O][2] */,
                     const double* q /* [O], NULL = all 1 */, const double* K_a, const double* K_b /* [n_pairs][9], or [9] with shared_k */,
                     int shared_k, const double* R0 /* [n][9] */, const double* T0 /* [n][3], unit */,
                     const srk_pair_options* /* NULL = the defaults */, double* R /* [n][9] */, double* T /* [n][3], unit */, double* E /* [n][9] */,
                     double* quality /* [n][6] */, double* info /* [n][25] */, double* basis /* [n][6] */, uint32_t* status /* [n] */,
                     double* w_out /* [O] or NULL */);
int srk_relate_frames_refined(srk_ba*, double f0, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                              const double* K_a, const double* K_b, int shared_k, const srk_relate_options* /* NULL = the defaults */,
                              const srk_pair_options* refine /* not NULL */, double* R, double* T, double* E, double* related /* [n][8] */,
                              uint32_t* related_status /* [n] */, uint8_t* inlier_out /* [O] or NULL */, double* quality, double* info,
                              double* basis, uint32_t* status, double* w_out /* [O] or NULL */);
/* device ms of the refinement's kernels (the inverses of K, the product with the inlier flags, the pairs) in the last of the two
 * calls on this handle, from an event pair; the chained call leaves relate's own time in srk_ba_relate_kernel_ms */
double srk_ba_pair_kernel_ms(const srk_ba*);
/* host only, no device and no handle needed: the checks of srk_refine_pairs on their own.  SRK_OK, or SRK_E_ARGS with *why (may be
 * NULL) pointing at a static text. */
int srk_pair_check_pairs(int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q, const double* K_a,
                         const double* K_b, int shared_k, const double* R0, const double* T0, const srk_pair_options* opts, const char** why);
/* host only: one pair of n_obs matches in the kernel's own order of operations (the same statements, compiled for the host; the
 * same deal of the weighted matches to 64 lanes, the same merge tree).  grad [5] (may be NULL): g at the result.  log (may be
 * NULL) receives (accepted, E_cur, E_cand) per attempt, [attempts][3], E_cand NaN when the factorisation failed, and *log_count
 * their number.  Returns the status bits, or SRK_E_ARGS (negative) when the checks refuse the pair. */
int srk_pair_host_pair(int64_t n_obs, const double* uv_a, const double* uv_b, const double* q, const double* K_a, const double* K_b, double f0,
                       const double* R0, const double* T0, const srk_pair_options* opts, double* R, double* T, double* E, double* quality,
                       double* info, double* basis, double* w_out, double* grad, double* log, int32_t* log_count);
/* host only: from a refined pair to the factor srk_ba_set_relative_pose_factors takes for the frames (a, b), at a baseline length
 * lambda > 0 that the caller knows (two views do not): rel_R = Z = R^T, rel_t = z = -lambda R^T T, and info21 the upper triangle
 * (row by row, order [t; r]) of L = M^T info M with the 5 x 6 matrix M = [[0, R^T], [-(1 / lambda) B^T R, B^T [T]x]], B = [b1 b2]:
 * to first order the factor's residual [e_t; e_r] moves the refinement's variables by w = R^T e_r and
 * beta = -(1 / lambda) B^T R e_t + B^T [T]x e_r.  L is positive semi-definite of rank at most 5; its null direction [z; 0] is the
 * scale.  SRK_E_ARGS for a NULL pointer, a value that is not finite or lambda <= 0. */
int srk_pair_factor(const double* R, const double* T, const double* info /* [25] */, const double* basis /* [6] */, double baseline,
                    double* rel_R /* [9] */, double* rel_t /* [3] */, double* info21 /* [21] */);

/* ---- map alignment: similarity hypotheses scored on the device (EXTENSION) ----
 * relate is 2D-2D and locate 2D-3D; "align" is the 3D-3D member: the similarity b ~ s R a + t (s > 0, R a proper rotation) between
 * two sets of corresponding points, wrong correspondences among them.  It brings one map into the coordinates of another: a
 * bootstrapped or relocalised sub-map into the main map, the two ends of a monocular loop (where the scale has drifted), a
 * free-gauge solve near surveyed coordinates before srk_ba_set_position_priors(..., keep_gauge = 0).  The reference has no such
 * function.
 *
 * Sets in CSR form (row_ptr [n_sets + 1], a [O][3], b [O][3]) with any number of correspondences; q >= 0 the optional information
 * of a correspondence (NULL = all 1, bit for bit; q = 0 = the set without that correspondence, bit for bit).  Everything works on
 * the set's n weighted correspondences, numbered by rank 0 .. n - 1 in ascending o.
 *
 * Sampler (counter-based, no state, a stream of its own): mix(seed, h, k) = the splitmix64 finaliser of
 * seed + 0xA0761D6478BD642F (4 h + k + 1) mod 2^64.  Draw k = 0..2 of hypothesis h is r = umulhi64(mix, n - k), then for the
 * earlier picks s in ascending order: if (r >= s) ++r.  Three distinct ranks that depend on seed, h and k alone.
 *
 * Hypothesis (Horn's three-point construction): on each side d1 = p1 - p0, d2 = p2 - p0, c = d1 x d2; no model when
 * |c|^2 <= 1e-12 |d1|^2 |d2|^2 on either side or anything is not finite.  Otherwise the orthonormal frames A = [d1^, c^ x d1^, c^]
 * and B likewise, R = B A^T, s = sqrt(sum |b_k - bm|^2 / sum |a_k - am|^2) over the three (1 with with_scale = 0), t = bm - s R am.
 *
 * Score (MSAC): score(h) = sum over the ranks in ascending order of min(q |b - (s R a + t)|^2, tau^2), tau = inlier_distance in
 * the units of b; a hypothesis without a model scores +inf.  The smallest score wins, an equal score goes to the smaller h.
 *
 * Local optimisation: up to refine_rounds rounds from the winner.  The inliers (q r^2 < tau^2) of the current model, at least
 * three; their weighted centroids, then M = sum q (b - bm)(a - am)^T and sum q |a - am|^2 (each lane of the wave sums the ranks
 * l, l + 64, .. in ascending order, the lanes merge in a fixed tree); R maximises tr(R^T M), the eigenvector of the largest
 * eigenvalue of Horn's symmetric 4 x 4 matrix by cyclic Jacobi (a proper rotation on mirrored and on coplanar sets);
 * s = tr(R^T M) / sum q |a - am|^2 (1 with with_scale = 0), t = bm - s R am; accepted only when its score over all n is strictly
 * smaller, else the rounds stop: the result is never worse than the winning hypothesis.
 *
 * Outputs per set: s, R [9], t [3]; aligned [8] = { sqrt(score / n) in the units of b, n, the inlier count, the winning h, the
 * number of hypotheses with a model, the rounds accepted, (lambda1 - lambda2) / |lambda1| of the last accepted closed form (NaN
 * when none was accepted; 0 = the inliers are collinear; the library sets no threshold on it), the RMS distance of the inliers };
 * status, a mask of SRK_ALIGN_*: then the model is (1, I, 0), aligned[0], [3], [6], [7] are NaN and aligned[2], [5] are 0.
 * inlier_out [O] (may be NULL): 1 iff q_o > 0 and q_o r_o^2 < tau^2 at the returned model.
 *
 * srk_ba_align: a is the CURRENT landmark point[o] (caller's numbering) of the resident scene, read on the device through the
 * handle's landmark order; target = b.  The kernels work in the normalised coordinates X_n = s_n (R0 X + T0); with
 * revert_normalization = 1 the result (sigma, Q, tau) comes back as (sigma s_n, Q R0, sigma s_n Q T0 + tau), which maps the
 * uploaded arrays' coordinates to b.  It writes no scene buffer and is refused with more than one rank.
 *
 * Host checks before any allocation or launch (SRK_E_ARGS with a text): a descending or negative row_ptr, a, b or q that is not
 * finite, a negative q, hypotheses outside 1..4096, inlier_distance not finite or <= 0 (it has no default: the 0 of
 * srk_align_default_options is refused), refine_rounds outside 0..16, with_scale not 0 or 1, NULL outputs, a point beyond the
 * map, and more than 2^22 waves (sets x ceil(hypotheses / 64)) in one call: split the batch, a set's bits do not depend on it.
 * Absent: an information matrix of the similarity, Sim(3) factors in the solver, transforming the resident scene in place, an
 * adaptive early stop, several ranks. */
enum {
    SRK_ALIGN_FEW_POINTS = 1, /* fewer than three correspondences with q > 0 */
    SRK_ALIGN_NO_MODEL = 2    /* no sample gave a similarity (every triple collinear) */
};
typedef struct srk_align_options {
    int32_t hypotheses;     /* samples per set, 1 .. 4096; srk_ransac_hypotheses(3, ...) gives the count for an outlier ratio */
    double inlier_distance; /* tau > 0 in the units of b: the truncation of the score and the inlier test */
    uint64_t seed;
    int32_t with_scale;     /* 1: a similarity; 0: a rigid motion, s = 1 */
    int32_t refine_rounds;  /* rounds of local optimisation, 0 .. 16 */
} srk_align_options;
void srk_align_default_options(srk_align_options*); /* { 256, 0 (must be set), 1, 1, 2 } */
int srk_align_points(srk_ba*, int32_t n_sets, const int64_t* row_ptr, const double* a /* [O][3] */, const double* b /* [O][3] */,
                     const double* q /* [O], NULL = all 1 */, const srk_align_options*, double* s /* [n] */, double* R /* [n][9] */,
                     double* t /* [n][3] */, double* aligned /* [n][8] */, uint32_t* status /* [n] */, uint8_t* inlier_out /* [O] or NULL */);
int srk_ba_align(srk_ba*, int32_t n_sets, const int64_t* row_ptr, const int32_t* point /* caller's landmark numbering */,
                 const double* target /* [O][3] */, const double* q, const srk_align_options*, int revert_normalization, double* s, double* R,
                 double* t, double* aligned, uint32_t* status, uint8_t* inlier_out);
/* device ms of the last of the two calls on this handle (gather, hypotheses and scores, pick with its rounds) from an event pair;
 * and of the hypothesis-and-score kernel alone, from a second pair */
double srk_ba_align_kernel_ms(const srk_ba*);
double srk_ba_align_score_ms(const srk_ba*);
/* host only, no device and no handle needed: the checks of srk_align_points (point NULL) or srk_ba_align (point and n_points, a
 * may be NULL) on their own.  SRK_OK, or SRK_E_ARGS with *why (may be NULL) pointing at a static text. */
int srk_align_check_sets(int32_t n_sets, const int64_t* row_ptr, const int32_t* point, int64_t n_points, const double* a, const double* b,
                         const double* q, const srk_align_options* opts, const double* s, const double* R, const double* t, const double* aligned,
                         const uint32_t* status, const char** why);
/* host only: one set of n_obs correspondences in the kernels' own order of operations (the same statements, compiled for the
 * host).  Returns the status bits, or SRK_E_ARGS (negative) when the checks refuse the set. */
int srk_align_host_set(int64_t n_obs, const double* a, const double* b, const double* q, const srk_align_options* opts, double* s, double* R, double* t,
                       double* aligned, uint8_t* inlier_out);
/* host only, in place: a scene under the similarity X' = s R X + t.  Points X [n_points][3]; poses (x_cam = R_c X + T_c):
 * R_c' = R_c R^T, T_c' = s T_c - R_c' t -- the camera frame is scaled by s, so every projection is unchanged.  Either group may be
 * NULL (cam_R and cam_T together). */
int srk_similarity_apply(double s, const double* R, const double* t, int64_t n_points, double* X, int64_t n_frames, double* cam_R, double* cam_T);

/* ---- two-view homography: four-point hypotheses scored on the device (EXTENSION) ----
 * The member of the family for planar scenes and for pure rotation, the two cases in which srk_relate_frames cannot answer: the
 * homography p_b ~ G p_a between the 2D-2D matches of a pair of images, wrong matches among them.  Inputs as srk_relate_frames:
 * pairs in CSR form, K_a, K_b [n_pairs][9] (or [9] with shared_k), f0; homogeneous pixels are p = (u, v, f0); everything works on
 * the pair's n weighted matches (q > 0) numbered by rank in ascending o.  G is the pixel homography, returned with Frobenius norm 1
 * and signed so that (G p_a)_3 > 0 for its inliers; H = K_b^-1 G K_a relates the rays x = K^-1 p.
 *
 * Gather, then hypothesis and score, then pick with local optimisation, as srk_align_points.  The sampler is the project's
 * counter-based one on a stream of its own (four distinct ranks per hypothesis).  A hypothesis is closed form through the
 * projective basis: on each side [p0 p1 p2] lambda = p3 by the adjugate, A = [lambda_k p_k], G = B adj(A); no model when three of
 * the four points are collinear (a determinant below 1e-9 of the product of its columns' norms), the four (G p_ak)_3 differ in
 * sign, |det G| <= 1e-12 at norm 1, or anything is not finite.  The score is MSAC, sum min(q s, tau^2), with s the symmetric transfer
 * error in pixels squared, |pi(G p_a) - uv_b|^2 + |pi(G^-1 p_b) - uv_a|^2, pi(y) = f0 y_xy / y_3; a match behind either image counts
 * tau^2 and is no inlier; the smallest score wins, an equal score goes to the smaller h.  Then up to refine_rounds Gauss-Newton steps
 * on the symmetric transfer error of the current model's inliers, q-weighted, G <- G (I + sum d_k B_k) over a fixed basis of the eight
 * traceless matrices, each accepted only when the score over all n gets strictly smaller: never worse than the winner.
 *
 * inlier_pixels (tau), default 6.0: with noise sigma per coordinate in both images each one-way distance carries both images'
 * noise, so s is about 2 sigma^2 chi^2_4, and P(chi^2_4 > t) = e^(-t/2) (1 + t/2): at sigma = 1, tau = 6 gives t = 18 and cuts
 * e^-9 (1 + 9) = 0.12 % of the true matches.
 *
 * The returned model is decomposed (Ma, Soatto, Kosecka, Sastry, algorithm 5.2): H over its middle singular value, signed so that
 * sum q x_b^T H x_a > 0 over the inliers, then the two poses of the plane, H = R + (T/d) N^T, each R passed through the nearest
 * rotation, N flipped so that at least half of the inliers have N^T x_a > 0.  Both are returned, the one with more inliers in front
 * first (a tie: u_1); the library does not choose between the twins.  When w1 - w3 <= 1e-10 of the normalised H^T H (a rotation, or
 * the plane at infinity) one candidate is returned: the rotation nearest to H, T/d = 0, N = 0.
 *
 * Outputs per pair: G [9]; H [9] normalised and signed; n_poses (0, 1 or 2); R [2][9], T [2][3] (= t/d), N [2][3], front [2] (the
 * inliers with N^T x_a > 0), unused entries zero; homog [8] = { sqrt(score / n) in pixels, n, the inlier count, the winning h, the
 * number of hypotheses with a model, the rounds accepted, w1 - w3, the RMS symmetric error of the inliers (0 when a model without an
 * inlier wins, as a huge q or a tiny tau allows) }; status, a mask of
 * SRK_HOMOGRAPHY_*: then G = H = I, n_poses = 0, homog[0], [3], [6], [7] are NaN and homog[2], [5] are 0.  inlier_out [O] (may be
 * NULL): 1 iff q > 0 and q s < tau^2 at the returned model.  The library sets no threshold between this model and the essential
 * matrix of srk_relate_frames: both deliver inlier counts and RMS figures to be compared by the caller.
 *
 * Host checks before any allocation or launch (SRK_E_ARGS with a text), as srk_relate_frames: a descending or negative row_ptr, uv
 * or K not finite, q negative or not finite, a singular K, hypotheses outside 1..4096, inlier_pixels not finite or <= 0,
 * refine_rounds outside 0..16, NULL outputs, and more than 2^22 waves (pairs x ceil(hypotheses / 64)) in one call.
 * Absent: a robust loss in the rounds, an information matrix, a library choice between the twins or between E and H, an adaptive
 * early stop, several ranks. */
enum {
    SRK_HOMOGRAPHY_FEW_POINTS = 1, /* fewer than four matches with q > 0 */
    SRK_HOMOGRAPHY_NO_MODEL = 2    /* no sample gave a homography */
};
typedef struct srk_homography_options {
    int32_t hypotheses;    /* samples per pair, 1 .. 4096; srk_ransac_hypotheses with a sample of 4 gives the count for an outlier ratio */
    double inlier_pixels;  /* tau > 0 in pixels: the truncation of the score and the inlier test */
    uint64_t seed;
    int32_t refine_rounds; /* rounds of local optimisation, 0 .. 16 */
} srk_homography_options;
void srk_homography_default_options(srk_homography_options*); /* { 256, 6.0, 1, 4 } */
int srk_relate_homography(srk_ba*, double f0, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a /* [O][2] */, const double* uv_b /* [O][2] */,
                          const double* q /* [O], NULL = all 1 */, const double* K_a, const double* K_b, int shared_k, const srk_homography_options*,
                          double* G /* [n][9] */, double* H /* [n][9] */, int32_t* n_poses /* [n] */, double* R /* [n][2][9] */,
                          double* T /* [n][2][3] */, double* N /* [n][2][3] */, int32_t* front /* [n][2] */, double* homog /* [n][8] */,
                          uint32_t* status /* [n] */, uint8_t* inlier_out /* [O] or NULL */);
/* device ms of the last call on this handle (gather, hypotheses and scores, pick with its rounds and the decomposition) from an
 * event pair; and of the hypothesis-and-score kernel alone, from a second pair */
double srk_ba_homography_kernel_ms(const srk_ba*);
double srk_ba_homography_score_ms(const srk_ba*);
/* host only, no device and no handle needed: the checks of srk_relate_homography on their own (f0 and the outputs excepted).
 * SRK_OK, or SRK_E_ARGS with *why (may be NULL) pointing at a static text. */
int srk_homography_check_pairs(int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q, const double* K_a,
                               const double* K_b, int shared_k, const srk_homography_options* opts, const char** why);
/* host only: one pair of n_obs matches in the kernels' own order of operations (the same statements, compiled for the host).
 * Returns the status bits, or SRK_E_ARGS (negative) when the checks refuse the pair. */
int srk_homography_host_pair(int64_t n_obs, const double* uv_a, const double* uv_b, const double* q, const double* K_a, const double* K_b, double f0,
                             const srk_homography_options* opts, double* G, double* H, int32_t* n_poses, double* R, double* T, double* N,
                             int32_t* front, double* homog, uint8_t* inlier_out);
/* host only: the decomposition on its own.  H_in [9] at any scale and sign, the rays x_a, x_b [n][3] of its inliers (q [n] or NULL
 * = all 1).  H_out [9], R [2][9], T [2][3], N [2][3], front [2], *gap = w1 - w3.  Returns n_poses (1 or 2), or SRK_E_ARGS (a NULL
 * argument, an H that is not finite or has no middle singular value) with nothing written. */
int srk_homography_decompose(const double* H_in, int64_t n, const double* x_a, const double* x_b, const double* q, double* H_out, double* R, double* T,
                             double* N, int32_t* front, double* gap);

/* ---- two-view fundamental matrix: seven-point hypotheses scored on the device (EXTENSION) ----
 * The member of the family that needs no intrinsics: the fundamental matrix p_b^T F p_a = 0 between the 2D-2D matches of a pair of
 * images, wrong matches among them -- geometric verification of matches when K is a guess (an EXIF focal length, an unordered image
 * set).  Inputs as srk_relate_frames without K_a, K_b, shared_k: pairs in CSR form, f0; homogeneous pixels are p = (u, v, f0) and
 * the solver works on p / f0; everything works on the pair's n weighted matches (q > 0) numbered by rank in ascending o.  The F
 * returned has Frobenius norm 1, rank exactly 2 by construction, F = U diag(1, sigma, 0) V^T / sqrt(1 + sigma^2) with proper
 * rotations U, V and 0 <= sigma <= 1, and is signed so that its entry of largest magnitude is positive (a tie: the first row by
 * row).  The epipoles are the third columns: F v_3 = 0, F^T u_3 = 0, homogeneous in (u, v, f0).
 *
 * Gather, solve, score, then pick with local optimisation.  The sampler is the project's counter-based one on a stream of its own
 * (eight distinct ranks per hypothesis).  Picks 0-6 give the 7 x 9 matrix of rows p_b (x) p_a; its null space F1, F2 by Gauss-Jordan
 * elimination with complete pivoting (a last pivot at most 1e-12 of the first: the rows are dependent, no model -- seven points of
 * a plane, a pure rotation: srk_relate_homography's cases); the cubic det(F1 + z F2), its real roots by the derivative chain; pick 7
 * chooses the root with the smallest Sampson error (an equal error: the smaller root).  The score is relate's: MSAC,
 * sum min(q s, tau^2), s the squared Sampson distance in pixels; the smallest score wins, an equal score goes to the smaller h.
 * The winner is brought into the representation above (the smallest singular value dropped), and that model is the current one.
 * Then up to refine_rounds Levenberg-Marquardt attempts on the Sampson error of the current model's inliers, q-weighted, over
 * d = [a; b; delta]: U <- U Exp(a), V <- V Exp(b), sigma <- sigma + delta, exact Jacobian, (H + c diag H) d = -g with c from 1e-4,
 * the candidate re-scored over all n matches and accepted iff its score is strictly smaller (c /= 10, else c *= 10).  The loop ends
 * after refine_rounds attempts, with fewer than eight inliers, with sums that are not finite, or after the first attempt whose
 * candidate score differs from the current one by at most 1e-9 of it.
 *
 * Outputs per pair: F [9]; U [9], V [9], sigma; fund [12] = { sqrt(score / n) in pixels, n, the inlier count, the winning h, the
 * hypotheses with a model, the eighth-match Sampson error in pixels, attempts accepted, attempts used, the inliers' RMS Sampson
 * distance, sigma, cond_1 of the Jacobi-scaled H at the result (NaN when it is not positive definite; sigma = 1, an essential
 * matrix, makes the rotations of U and V about their third axes one direction, and cond_1 reports it: the library sets no
 * threshold), the number of real roots of the winning sample }; info [49] = the undamped H = sum q J^T J over the inliers at the
 * result with r in pixels, row-major in the order [a; b; delta]: with pixel noise sigma_px the covariance of d is about
 * sigma_px^2 H^-1; status, a mask of SRK_FUNDAMENTAL_*: then F = 0, U = V = I, sigma = 0, info = 0, fund[0], [3], [5], [8], [10]
 * are NaN and the counts are 0.  inlier_out [O] (may be NULL): 1 iff q > 0 and q s < tau^2 at the returned model.
 *
 * Host checks before any allocation or launch (SRK_E_ARGS with a text), relate's minus K: a descending or negative row_ptr, uv not
 * finite, q negative or not finite, hypotheses outside 1..4096, inlier_pixels not finite or <= 0, refine_rounds outside 0..16, NULL
 * outputs, and more than 2^22 waves (pairs x ceil(hypotheses / 64)) in one call.
 * Absent: a robust loss in the attempts, a stand-alone refinement from a given start, focal lengths from F, a library choice
 * between F, E and H, an adaptive early stop, several ranks. */
enum {
    SRK_FUNDAMENTAL_FEW_POINTS = 1, /* fewer than eight matches with q > 0 */
    SRK_FUNDAMENTAL_NO_MODEL = 2    /* no sample gave a fundamental matrix */
};
typedef struct srk_fundamental_options {
    int32_t hypotheses;    /* samples per pair, 1 .. 4096; srk_ransac_hypotheses with a sample of 7 gives the count for an outlier ratio */
    double inlier_pixels;  /* tau > 0 in pixels: the truncation of the score and the inlier test */
    uint64_t seed;
    int32_t refine_rounds; /* Levenberg-Marquardt attempts, 0 .. 16 */
} srk_fundamental_options;
void srk_fundamental_default_options(srk_fundamental_options*); /* { 256, 2.0, 1, 8 } */
int srk_relate_uncalibrated(srk_ba*, double f0, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a /* [O][2] */, const double* uv_b /* [O][2] */,
                            const double* q /* [O], NULL = all 1 */, const srk_fundamental_options*, double* F /* [n][9] */, double* U /* [n][9] */,
                            double* V /* [n][9] */, double* sigma /* [n] */, double* fund /* [n][12] */, double* info /* [n][49] */,
                            uint32_t* status /* [n] */, uint8_t* inlier_out /* [O] or NULL */);
/* device ms of the last call on this handle (gather, solve, score, pick with its attempts) from an event pair; of the score
 * kernel alone, from a second pair; and of the solve kernel alone, from a third */
double srk_ba_fundamental_kernel_ms(const srk_ba*);
double srk_ba_fundamental_score_ms(const srk_ba*);
double srk_ba_fundamental_solve_ms(const srk_ba*);
/* host only, no device and no handle needed: the checks of srk_relate_uncalibrated on their own (f0 and the outputs excepted).
 * SRK_OK, or SRK_E_ARGS with *why (may be NULL) pointing at a static text. */
int srk_fundamental_check_pairs(int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                                const srk_fundamental_options* opts, const char** why);
/* host only: one pair of n_obs matches in the kernels' own order of operations (the same statements, compiled for the host).
 * Returns the status bits, or SRK_E_ARGS (negative) when the checks refuse the pair. */
int srk_fundamental_host_pair(int64_t n_obs, const double* uv_a, const double* uv_b, const double* q, double f0, const srk_fundamental_options* opts,
                              double* F, double* U, double* V, double* sigma, double* fund, double* info, uint8_t* inlier_out);

/* ---- marginal covariances of frames and landmarks (EXTENSION) ----
 * "How well is frame 37 determined?", "how good is this landmark?": the diagonal blocks of the covariance of the estimate, for
 * gating a loop closure, choosing keyframes to marginalise, weighting the map in a later stage or a chi-square test of a prior
 * residual.  E is the objective LM minimises, every loss, information weight, prior and factor included; the library's blocks are
 * the Gauss-Newton Hessian H of E in the factor-2 convention (a prior adds 2 L), so with pixel noise sigma_px the covariance of
 * the estimate is 2 (sigma_px / f0)^2 H^-1.  With H = [[V, W], [W^T, U]] in point-major order and S = L L^T its Schur complement
 * onto the frame variables, the block of frame j is Y^T Y with Y = L^-1 E_j (E_j the unit columns of the frame's variables) and
 * the block of landmark i is V_i^-1 + Z^T Z with Z = L^-1 B_i, B_i holding W_o^T V_i^-1 in the rows of the frame of each of its
 * observations o: one forward substitution with many right-hand sides on the factor of S and a small Gram product per block.
 * Variables that do not move -- the seven gauge variables, constant frames, constant landmarks -- have covariance exactly 0:
 * their rows and columns of a frame block are exact zeros and a constant landmark returns a zero block.  Every block is exactly
 * symmetric.  The blocks between two different frames or landmarks are the next section's (srk_ba_cross_covariances).
 *
 * srk_ba_phase_covariance: the staged entry point, after srk_ba_phase_derivatives and srk_ba_phase_schur(c).  Returns the raw
 * blocks of the inverse of the system in slot 0, in the resident (normalised) scene's variables: frame_blocks [n][FV][FV]
 * (FV = srk_ba_frame_vars, per-frame variable order as everywhere), point_blocks [n][3][3].  c = 0 is H^-1; with c > 0, V and the
 * diagonal of S carry (1 + c) and the result is the inverse of that damped matrix (well conditioned; what the tests pin the
 * arithmetic with).  Frame and landmark indices are in the caller's numbering, in any order, repeats allowed.  Whatever the rcs
 * mode or chunk plan, the call factorises slot 0's system in place with the single-chain solver's unfused launch sequence (no
 * hand-offs, so nothing can time out) and LEAVES THE SYSTEM CONSUMED, as srk_ba_phase_solve does in mode 1: SRK_BUF_RCS holds
 * the factor afterwards, SRK_BUF_RCS_RHS and SRK_BUF_CORRECTIONS zeros; call srk_ba_phase_schur again before another solve.
 * Returns 0 ok, 1 = the system is not positive definite, a landmark block is not invertible or a result is not finite (the
 * output arrays are untouched), negative on error.
 *
 * srk_ba_covariances: the convenience call on the resident scene's current state (after srk_ba_optimize: the result): the
 * derivative pass, the undamped system, the blocks above, scaled by 2 (sigma_pixels / f0)^2.  caller_coordinates = 1 maps them
 * to the coordinates of the uploaded arrays (srk_ba_revert_covariances), 0 leaves them in the normalised scene's.  The scene is
 * not changed.  In the default ten-variable mode the result is the covariance of the ten-variable problem; where per-frame
 * intrinsics are close to unobservable (planar scenes) the undamped system is numerically singular and the call returns 1: use
 * srk_ba_set_fixed_intrinsics for covariances of a calibrated rig.
 *
 * SRK_E_STATE without a scene.  SRK_E_ARGS (text in srk_ba_last_error): an index out of range, a negative count, a NULL array
 * with a positive count, sigma_pixels not finite and positive; intrinsic groups or more than one rank (as priors refuse them).
 * Fixed intrinsics, robust losses, information, constant blocks, priors, factors, frame reordering, deterministic mode and both
 * storage precisions work unchanged.  The three kernels use no atomics and a fixed summation order: the same system gives the
 * same bits.  Nothing is launched or allocated unless one of these calls is made. */
int srk_ba_phase_covariance(srk_ba*, int32_t n_frames_sel, const int32_t* frames /* caller's numbering */,
                            double* frame_blocks /* [n][FV][FV] */, int64_t n_points_sel, const int64_t* points,
                            double* point_blocks /* [n][3][3] */);
int srk_ba_covariances(srk_ba*, double sigma_pixels, int32_t n_frames_sel, const int32_t* frames, double* frame_cov /* [n][FV][FV] */,
                       int64_t n_points_sel, const int64_t* points, double* point_cov /* [n][3][3] */, int caller_coordinates);
/* host only, no device and no handle needed: blocks in the normalised scene's variables to the caller's coordinates, in place.
 * X_n = s (R0 X + T0), so a landmark maps as R0^T Sigma R0 / s^2.  The pose variables of a frame are [centre; rotation vector
 * applied to the direct rotation from the left] and map as D Sigma D^T with D = diag(R0^T / s, R0^T); with
 * frame_vars = 10 the four intrinsic variables in front are not transformed (D has the identity there).  frame_vars: 6 or 10.
 * Either count may be 0.  Returns SRK_OK or SRK_E_ARGS. */
int srk_ba_revert_covariances(const srk_ba_normalizer* nrm, int frame_vars, int32_t n_frames, double* frame_cov /* [n][fv][fv] */,
                              int64_t n_points, double* point_cov /* [n][3][3] */);
/* harness knob: the right-hand sides of the forward substitution are processed in batches of columns so that their buffer
 * (handle-owned, grown lazily, freed by srk_ba_destroy) stays under 256 MB; max_columns > 0 caps a batch at that many columns
 * instead (at least one block; tests force several batches at small sizes), 0 = the default. */
int srk_ba_set_covariance_batch(srk_ba*, int64_t max_columns);

/* ---- cross-covariances between blocks and relative-pose covariances (EXTENSION) ----
 * The marginal blocks above do not answer "how well is the pose of frame b known relative to frame a?": that is
 * J [[S_aa, S_ab], [S_ba, S_bb]] J^T and needs the block between the two frames, which far from the gauge frames is of the size
 * of the marginals themselves.  With the notation above (Y_j = L^-1 E_j of a frame, Z_i = L^-1 B_i of a landmark):
 *   frame a, frame b:        (H^-1)_ab =  Y_a^T Y_b   (FV x FV, rows a, columns b)
 *   landmark i, frame j:     (H^-1)_ij = -Z_i^T Y_j   (3 x FV)
 *   landmark i, landmark k:  (H^-1)_ik =  Z_i^T Z_k   (3 x 3; for i = k the marginal block, V_i^-1 added)
 * from the same factor and the same forward substitution, followed by one small product per requested pair (k_cov_cross).
 * Pairs are given in the caller's numbering, in any order; repeats are allowed, a == b is allowed and gives the marginal block
 * with the bits of srk_ba_phase_covariance; block (b, a) is the transpose of block (a, b) to the bit; a pair's result does not
 * depend on the batch cap (srk_ba_set_covariance_batch, here at least 20 columns) or on the other pairs of the call.  Rows and
 * columns of variables that do not move are exact zeros and any pair with a constant landmark returns a zero block.
 *
 * srk_ba_phase_cross_covariance: the staged form, with the contract of srk_ba_phase_covariance (after srk_ba_phase_derivatives
 * and srk_ba_phase_schur(c); consumes slot 0's system; blocks of the inverse of the damped matrix in the resident scene's
 * variables; 1 = not positive definite or a result not finite, outputs untouched).
 * srk_ba_cross_covariances: the convenience call: derivative pass, undamped system, blocks scaled by 2 (sigma_pixels / f0)^2 and,
 * with caller_coordinates = 1, mapped as srk_ba_revert_cross_covariances maps them -- except a block with itself, which is mapped
 * as srk_ba_revert_covariances maps it (exactly symmetric, with the bits of srk_ba_covariances), and a block (a, b) with a > b,
 * which is mapped as the transpose of (b, a): the two stay transposes of one another to the bit in the caller's coordinates.
 * srk_ba_revert_cross_covariances (host only): a block between p and q maps as D_p Sigma D_q^T, D of a frame
 * diag(I (the four intrinsics, frame_vars = 10 only), R0^T / s, R0^T), D of a landmark R0^T / s; in place.
 * srk_ba_relative_pose_covariances: for every pair a != b the 6 x 6 covariance, order [t; r], of the relative pose
 * z = R_a (C_b - C_a), Z = R_a R_b^T in the perturbation [e_t; e_r] of srk_ba_set_relative_pose_factors at zero residual:
 * J_a S_aa J_a^T + J_a S_ab J_b^T + J_b S_ba J_a^T + J_b S_bb J_b^T over the pose variables of the two frames (with ten variables
 * a frame the intrinsics are marginalised), J_a = [[-R_a, R_a [d]x], [0, -R_b]], J_b = [[R_a, 0], [0, R_b]], d = C_b - C_a at the
 * resident scene's current poses.  One factorisation serves all n pairs.  The result is in the caller's world units and
 * radians (z and Z do not change under a rigid motion of the world and z scales with it: tt / s^2, tr / s, rr) and exactly
 * symmetric.  A pair with a == b is refused.
 *
 * Refusals and return values are those of srk_ba_covariances.  Nothing is launched or allocated unless one of these calls is made. */
int srk_ba_phase_cross_covariance(srk_ba*, int64_t n_ff, const int32_t* ff_a, const int32_t* ff_b,
                                  double* ff_blocks /* [n][FV][FV]: rows a, columns b */, int64_t n_pf, const int64_t* pf_point,
                                  const int32_t* pf_frame, double* pf_blocks /* [n][3][FV] */, int64_t n_pp, const int64_t* pp_a,
                                  const int64_t* pp_b, double* pp_blocks /* [n][3][3] */);
int srk_ba_cross_covariances(srk_ba*, double sigma_pixels, int64_t n_ff, const int32_t* ff_a, const int32_t* ff_b, double* ff_cov,
                             int64_t n_pf, const int64_t* pf_point, const int32_t* pf_frame, double* pf_cov, int64_t n_pp,
                             const int64_t* pp_a, const int64_t* pp_b, double* pp_cov, int caller_coordinates);
int srk_ba_revert_cross_covariances(const srk_ba_normalizer* nrm, int frame_vars, int64_t n_ff, double* ff_blocks, int64_t n_pf,
                                    double* pf_blocks, int64_t n_pp, double* pp_blocks);
int srk_ba_relative_pose_covariances(srk_ba*, double sigma_pixels, int32_t n, const int32_t* frame_a, const int32_t* frame_b,
                                     double* cov /* [n][6][6], [t; r], caller's world units and radians */);

/* device-time instrumentation of srk_ba_optimize / srk_ba_compute_inplace: 0 = none (default; report.ms_* stay 0
 * except ms_total), 1 = one HIP event pair per phase (fills report.ms_*), 2 = additionally event pairs around
 * every MFMA trailing-update launch (fills report.ms_solve_syrk / solve_mfma_flops).  Every event costs a few
 * microseconds on the stream, and levels >= 1 serialise the attempts (no speculation).  Default 0. */
int srk_ba_set_profile(srk_ba*, int level);

/* dense SPD solve A x = b on the device (the reduced-camera-system solver on its own; A row-major
 * n x n, lower triangle read).  returns 0 ok, 1 not positive definite, negative on error. */
int srk_ba_dense_spd_solve(srk_ba*, int64_t n, const double* A, const double* b, double* x, double* ms_factor);

/* ---- synthetic scenes (host; restates demos/demo-bundle-adj-circle-grid.cpp:86-257 and
 * src/virt-world/scene-generator.cpp:9-55, with the visibility window of SURVEY 8d) ---- */
typedef struct srk_scene_spec {
    int32_t n_frames;        /* M */
    int32_t grid_nx, grid_ny;/* N = nx * ny */
    int32_t vis_window;      /* L consecutive frames per point; <= 0 or >= M: every frame (the demo) */
    double half_extent_x, half_extent_y; /* points on [-hx,hx] x [-hy,hy] */
    double f0;               /* 600 */
    double noise_x3d_hi;     /* 0.005 */
    double noise_r_hi;       /* 0.005 */
    double noise_uv_pix;     /* 0 (the demo projects exactly) */
    uint32_t seed;           /* 1234 */
} srk_scene_spec;
int64_t srk_scene_num_observations(const srk_scene_spec*);
/* fills caller arrays: points [N][3] (noisy), points_gt [N][3] (may be NULL), cam_R/T [M][..] (noisy),
 * cam_R_gt/cam_T_gt (may be NULL), K [M][9], row_ptr [N+1], obs_frame [O], obs_uv [O][2] */
int srk_scene_generate(const srk_scene_spec*, double* points, double* points_gt, double* cam_R, double* cam_T,
                       double* cam_R_gt, double* cam_T_gt, double* K, int64_t* row_ptr, int32_t* obs_frame,
                       double* obs_uv);
void srk_circle_camera_shots(const double center[3], double radius, double ascent_z, int32_t n,
                             const double* angles, double* cam_R, double* cam_T);

/* ---- callers of the BA path: the dinosaur loader and its pre-processing (host only) ----
 * srk_read_matrix_file          ReadMatrixFromFile        cpp_impl/suriko-engine/src/mat-serialization.cpp:12-87
 * srk_decompose_proj_mat        DecomposeProjMat          cpp_impl/suriko-engine/src/obs-geom.cpp:606-677
 * srk_triangulate_least_squares Triangulate3DPointByLeastSquares              obs-geom.cpp:679-727
 * srk_dino_load                 DinoDemo's scene build    cpp_impl/demos/demo-bundle-adj-dinosaur.cpp:24-54,85-230
 * all return 1 on success, 0 on failure (err receives the reference's message where it has one). */
int srk_read_matrix_file(const char* path, char delimiter, double* data /* NULL = count only */, int64_t capacity,
                         int64_t* rows, int64_t* cols, char* err, int errlen);
int srk_decompose_proj_mat(const double* P /* [3][4] */, double* scale_factor, double* K /* [9] */,
                           double* R_direct /* [9] */, double* T_direct /* [3] */);
int srk_triangulate_least_squares(int32_t n, const double* uv /* [n][2] */, const double* P /* [n][12] */, double f0,
                                  double* X /* [3] */);
int srk_dino_load(const char* dir, double f0, int64_t* n_points, int32_t* n_frames, int64_t* n_obs,
                  double* points /* NULL = sizes only */, double* cam_R, double* cam_T, double* K, int64_t* row_ptr,
                  int32_t* obs_frame, double* obs_uv, char* err, int errlen);

#ifdef __cplusplus
}
#endif
#endif
