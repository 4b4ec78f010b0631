// srk_dev.hpp -- internal declarations shared by the HIP translation units of libsrk_ba.so.
// Device data layout (all fp64 unless noted; see DESIGN.md "Data layout in HBM"):
//   pts      [N][3]            landmark coordinates (normalised world), two buffers: current / trial
//   cam      [M][SRK_CAM_PACK] per-frame pack recomputed from (R,T,K) once per pose change:
//              0-8 R  9-11 T  12-20 K  21-29 K*R  30-32 Td (direct translation)
//              33-35 rot1  36-38 rot2  39-41 rot3  (bundle-adj-kanatani.cpp:1511-1513)
//              42 1/fx  43 u0/(f0 fx)  44 1/fy  45 v0/(f0 fy)  46 1/f0  47 f0
//   obs      point-major CSR: row_ptr[N+1] i64, obs_frame[O] i32, obs_pt[O] i32, obs_uv[O][2]
//            frame-major copy:  col_ptr[M+1] i64, fobs_pt[O] i32, fobs_uv[O][2]
//   W        fp64 storage (default): [21][Os] the rank-2 FACTORS of the point-frame blocks (SRK_WF_* below), structure-of-
//            arrays, plane k of observation o at W[k*Os + o] (Os = O rounded up to 64): every store/load is lane-contiguous;
//            f32 storage mode: the same 21 planes as floats ([21][Os], plane k of observation o at W[k*Os + o]); widened on load
//   Vg       [9][Ns]   per point: V00 V01 V02 V11 V12 V22 g0 g1 g2 (SoA, Ns = N rounded up to 64)
//   Ug       [M][65]   per frame: 55 upper-triangle entries of the 10x10 block (row-major order) + 10 gradient
//            (fixed intrinsics, fv = 6: [M][27], 21 entries of the 6x6 pose block + 6 gradient; W then carries 18 planes:
//            AF0, G and BF1 are not written)
//   S        [ld][ld]  padded reduced camera system, row-major, LOWER triangle authoritative;
//            variable index = fv*frame + var (fv = 10, or 6 = [Tx Ty Tz Wx Wy Wz] with fixed intrinsics: SrkDims::fv);
//            the 7 gauge-fixed variables and the padding rows
//            carry an identity diagonal and zero rhs, so their correction is exactly 0; so do the variables of constant
//            frames (srk_ba_set_constant_blocks), through k_const_frames behind k_assemble
//   rhs,dc   [ld]
#pragma once
#include <hip/hip_runtime.h>
#include "srk_limits.hpp" // the SRK_*_HOST limits (shared with the host-only planner, srk_plan.hpp)
#include <stdint.h>
#include <vector>

#define SRK_CAM_PACK 48
#define SRK_UG 65
// frame sums a frame keeps in Ug for FV frame variables: the upper triangle of the FV x FV block (row-major) + FV gradient
// entries -- 65 for the reference's ten, 21 + 6 = 27 with fixed intrinsics (SrkDims::fv = 6)
#define SRK_UGS(FV) ((FV) * ((FV) + 1) / 2 + (FV))
// fp64 storage of the point-frame blocks: the rank-2 factors of W[pv][fv] = Ap[pv] Af[fv] + Bp[pv] Bf[fv] as SoA planes
// (srk_ba_kernels.hip: "storage of the point-frame blocks"); Af[1] = Af[3] = Bf[0] = Bf[2] = 0, Af[2] = Bf[3] = G
#define SRK_WF_AP 0   // planes 0..2   Ap[0..2]
#define SRK_WF_BP 3   // planes 3..5   Bp[0..2]
#define SRK_WF_AF0 6  // Af[0]
#define SRK_WF_G 7    // Af[2] = Bf[3]
#define SRK_WF_AF4 8  // planes 8..13  Af[4..9]
#define SRK_WF_BF1 14 // Bf[1]
#define SRK_WF_BF4 15 // planes 15..20 Bf[4..9]
#define SRK_WF_PLANES 21

struct SrkDims {
    int64_t N, O, Os, Ns;
    int32_t M;
    int32_t fv;          // variables per frame in the reduced camera system: 10, or 6 with fixed intrinsics (variable = fv*frame + var);
                         // in the padding behind M, so the struct keeps its size and layout
    int64_t ld;          // padded RCS dimension (multiple of SRK_CHOL_NB)
    int32_t comp;        // unity_t1_comp_ind (gauge), 1 by default
    int32_t w_f32;       // 1: the point-frame blocks W are stored as float (W then points at floats), arithmetic stays fp64
    int32_t g0, g1;      // internal indices of the caller's frames 0 and 1 (the gauge-fixed ones): 0, 1 unless the frames were reordered
};

#define SRK_CHOL_NB 256 // outer panel of the blocked Cholesky; ld is a multiple of it

// ---- deterministic mode (srk_ba_set_deterministic): the sums that take fp64 atomics by default go through staging buffers and
// an ordered second pass instead.  Derivative kernel: a task's 65 frame sums per frame slot, then per frame the tasks' sums in
// task order.  Schur kernel: a run's sum as the 10 x 10 blocks (slot a >= slot b) of its lower block triangle and its
// right-hand-side terms, then per block / per frame the runs' contributions in run order.
#define SRK_DET_LD 200       // local variables of a run: SRK_WS_NF_HOST frames x 10
#define SRK_DET_STRIDE 21000 // doubles of a run's staged sum: 20 * 21 / 2 blocks of 100
struct SrkDetJac {
    double* stage;            // [task][64][SRK_UG]
    const int32_t* ptr;       // [M + 1]
    const int32_t* ent;       // task * 64 + frame slot, by frame, tasks ascending
};
struct SrkDetSchur {
    double* stage;            // [run][SRK_DET_STRIDE]
    double* stage_rhs;        // [run][SRK_DET_LD]
    const int32_t *pair_ptr, *pair_fa, *pair_fb, *pair_ent; // blocks (fa >= fb) that receive something; ent: run | slot a << 20 | slot b << 25
    int32_t n_pairs;
    const int32_t *f_ptr, *f_ent; // per frame: run | slot << 20
};

// ---- robust loss (srk_ba_set_robust_loss): observation o with squared residual s = ex^2 + ey^2 ((pix/f0)^2) enters the
// objective as rho(s) and the normal equations with the IRLS weight w = rho'(s).  Kinds: SRK_LOSS_HUBER rho = s for s <= d^2,
// 2 d sqrt(s) - d^2 above; SRK_LOSS_CAUCHY rho = d^2 log(1 + s / d^2).  d = delta_pixels / f0.  The launchers below take a
// loss pointer: NULL (or kind 0 without information) launches the plain least-squares kernels, anything else their robust
// instantiations.
#define SRK_LOSS_NONE 0
#define SRK_LOSS_HUBER 1
#define SRK_LOSS_CAUCHY 2
struct SrkLoss {
    int32_t kind; // SRK_LOSS_*
    double d, d2; // threshold in normalised units (pix / f0) and its square
    // per-observation information q_o >= 0 (srk_ba_set_observation_information), device pointers, NULL =
    // none (q = 1): the observation enters the objective as rho(q s) and the normal equations with q rho'(q s).  q in the
    // internal (point-major) observation order, qf the same values in the frame-major order of fobs_* (k_jac_frames alone
    // reads it).  Kind SRK_LOSS_NONE with q given is valid: rho is the identity then.
    const double* q;
    const double* qf;
};

// ---- BA kernels (srk_ba_kernels.hip) ----
void srk_launch_cam_pack(hipStream_t s, int32_t M, const double* R, const double* T, const double* K, double f0,
                         double* pack);
void srk_launch_jac_points(hipStream_t s, const SrkDims& d, const double* pts, const double* cam,
                           const int32_t* obs_frame, const int32_t* obs_pt, const double* obs_uv, double* W,
                           double* Vg, const SrkLoss* loss = nullptr);
// fused single pass (point blocks + frame blocks); usable when every workgroup's frame range fits SRK_JF_SLOTS_HOST
void srk_launch_jac_fused(hipStream_t s, const SrkDims& d, const double* pts, const double* cam,
                          const int32_t* obs_frame, const int32_t* obs_pt, const double* obs_uv, double* W,
                          double* Vg, double* Ug, const int32_t* wg_jmin, const SrkLoss* loss = nullptr);
// run-based single pass: one wave per task = consecutive landmarks with identical frame lists (nf <= 64 frames), about
// SRK_JR_TASK_PTS_MIN_HOST .. MAX_HOST of them; four consecutive tasks (one workgroup) must touch fewer than
// SRK_JF_SLOTS_HOST consecutive frames
void srk_launch_jac_runs(hipStream_t s, const SrkDims& d, const double* pts, const double* cam, const int64_t* row_ptr,
                         const int32_t* obs_frame, const double* obs_uv, double* W, double* Vg, double* Ug,
                         const int32_t* task_first, const int32_t* task_count, int32_t n_tasks, const int32_t* wg_jmin,
                         const int32_t* task_group /* NULL: uniform runs; else the Schur run (grp_*) each task is a piece of */,
                         const int32_t* grp_nf, const int32_t* grp_frames, const uint32_t* pt_mask,
                         const SrkDetJac* det = nullptr /* deterministic mode */,
                         int frames_stride = 24 /* row length of grp_frames: SRK_GRP_MAXNF_HOST (the Schur runs) or 32 (the derivative kernel's own) */,
                         const SrkLoss* loss = nullptr);
void srk_launch_jac_frames(hipStream_t s, const SrkDims& d, int64_t max_frame_obs, const double* pts,
                           const double* cam, const int64_t* col_ptr, const int32_t* fobs_pt, const double* fobs_uv,
                           double* Ug, const SrkLoss* loss = nullptr);
void srk_launch_schur(hipStream_t s, const SrkDims& d, double c, const int64_t* row_ptr, const int32_t* obs_frame,
                      const double* W, const double* Vg, double* S, double* rhs, const int32_t* pt_list,
                      int64_t n_list);
void srk_launch_schur_grouped(hipStream_t s, const SrkDims& d, double c, const int64_t* row_ptr, const int32_t* obs_pt,
                              const uint8_t* obs_slot /* [O] slot of the observation's frame in its run's frame set */,
                              const uint32_t* pt_mask /* [N] slots a landmark sees */, const double* W, const double* Vg,
                              double* S, double* rhs, const int32_t* grp_first, const int32_t* grp_count,
                              const int32_t* grp_nf /* size of the run's frame set; negative = ragged run */,
                              const int32_t* grp_frames /* [n_groups][SRK_GRP_MAXNF_HOST] */, int64_t n_groups,
                              int64_t n_wide /* runs with more than SRK_GRP_NF1_HOST frames */,
                              int64_t n_mid /* runs with SRK_WS_NF_HOST < frames <= SRK_GRP_NF1_HOST */,
                              int fp32_accumulate /* 0 = fp64 (reference arithmetic), 1 = packed fp32 run sums */,
                              int32_t* irr /* [0] count + list of landmarks k_schur_mm hands back to the inverse path */,
                              int64_t n_mm_uniform, int64_t n_mm_ragged /* runs of <= SRK_WS_NF_HOST frames by kind */,
                              const SrkDetSchur* det = nullptr /* deterministic mode (every run must be one of those) */);
// tracks longer than SRK_GRP_MAXNF_HOST frames: runs of <= SRK_LONG_PTS_HOST landmarks over a frame set of
// <= SRK_LONG_MAXNF_HOST frames, one workgroup per pair of 8-frame blocks (k_schur_long); longer tracks stay with k_schur.
void srk_launch_schur_long(hipStream_t s, const SrkDims& d, double c, const double* W, const double* Vg, double* S, double* rhs,
                           const int32_t* item /* [n_items][4]: run, row block, column block (<= row block), 0 */,
                           int64_t n_items, const int32_t* run_np, const int32_t* run_nf,
                           const int32_t* run_pts /* [run][SRK_LONG_PTS_HOST] landmarks (internal order) */,
                           const int32_t* run_frames /* [run][SRK_LONG_MAXNF_HOST] the run's frame set, ascending */,
                           const int64_t* run_obs_off, const int32_t* run_obs /* [off + landmark * fb ceil(nf / fb) + slot]: observation or -1 */,
                           int fb = SRK_LONG_FB_HOST /* frames per block: 8 or 16 */);
void srk_launch_assemble(hipStream_t s, const SrkDims& d, double c, const double* Ug, double* S, double* rhs,
                         double ident /* diagonal of fixed / padding variables */, const int64_t* row_ptr,
                         const int32_t* obs_frame, const double* W, const double* Vg,
                         const int32_t* irr /* landmarks handed back by k_schur_mm: served by the tail workgroups */);
// constant parameter blocks (srk_ba_set_constant_blocks): masking passes behind the unchanged kernels,
// launched only when the list is not empty.
// after the derivative pass: identity block, zero gradient and zero point factors (planes 0..5 of W) for the listed landmarks
void srk_launch_const_points(hipStream_t s, const SrkDims& d, const int32_t* list /* landmarks, internal order */, int64_t n_list,
                             const int64_t* row_ptr, double* W, double* Vg);
// after srk_launch_assemble: identity rows / columns and zero rhs for the variables of the listed frames, inside the skyline
void srk_launch_const_frames(hipStream_t s, const SrkDims& d, const int32_t* frames /* internal frames, ascending */, int32_t n_frames,
                             const int64_t* env_col, double* S, double* rhs);
// after srk_launch_cam_apply: the trial pose and camera pack of the listed frames are those of the current scene, bit for bit
void srk_launch_const_cam_keep(hipStream_t s, const int32_t* frames, int32_t n_frames, const double* R, const double* T,
                               const double* pack, double* Rn, double* Tn, double* packn);
// position priors (srk_ba_set_position_priors): the lists of the resident scene.  Values as SoA planes
// val[k n + i], k = 0..2 the prior position (normalised world), 3..8 the information matrix xx xy xz yy yz zz.  Every index
// appears once, so each entry the passes touch has one owner.
struct SrkPrior {
    const int32_t* pt_list;  // landmarks with a prior, internal order, ascending
    const double* pt_val;    // [9][n_pts]
    int64_t n_pts;
    const int32_t* fr_list;  // internal frames with a prior, ascending
    const double* fr_val;    // [9][n_frames]
    int32_t n_frames;
};
// partial sums the prior energy pass writes: one per 256 landmark priors, then one per 256 frame priors
inline int32_t srk_prior_partials(int64_t n_pts, int64_t n_frames) { return (int32_t)((n_pts + 255) / 256 + (n_frames + 255) / 256); }
// behind the derivative kernels, before srk_launch_const_points: 2 L into the landmark blocks and the [Tx Ty Tz] part of the
// frame blocks, 2 L (X - Xbar) / 2 L (C - Cbar) into the gradients.  Launched only with priors.
void srk_launch_prior_add(hipStream_t s, const SrkDims& d, const double* pts, const double* cam, const SrkPrior& p, double* Vg,
                          double* Ug);
// the two prior sums of a scene on their own (srk_ba_prior_error): partial [srk_prior_partials], out2 = {landmarks, frames}
void srk_launch_prior_error(hipStream_t s, const double* pts, const double* cam, const SrkPrior& p, double* partial, double* out2);
// relative-pose factors (srk_ba_set_relative_pose_factors): the lists of the resident scene.  Values as
// SoA planes val[k n + i]: k = 0..8 the measured rotation Z (row-major), 9..11 the measured translation z (normalised world),
// 12..32 the upper triangle of the information matrix row by row.  Every unordered pair appears once, so each entry the
// passes touch has one owner.
#define SRK_RP_PLANES 33
struct SrkRelPose {
    const int32_t* fa;       // [n] internal frame a of each factor
    const int32_t* fb;       // [n] internal frame b
    const double* val;       // [SRK_RP_PLANES][n]
    int32_t n;
    const int32_t* fr_list;  // [n_frames] internal frames with incident factors, ascending
    const int32_t* fr_ptr;   // [n_frames + 1] CSR into fr_ent
    const int32_t* fr_ent;   // 2 * factor + side (0: the frame is a, 1: it is b), in factor order
    int32_t n_frames;
    const int64_t* tgt;      // [n] offset in S of entry (0, 0) of the factor's block: row = first pose variable of the frame
                             // with the larger internal index, column = that of the other
    double* cpl;             // [n][36] the blocks 2 J^T L J in that orientation, written by the derivative-side pass
};
// partial sums the factor energy pass writes: one per 256 factors
inline int32_t srk_relpose_partials(int64_t n) { return (int32_t)((n + 255) / 256); }
// behind srk_launch_prior_add, before srk_launch_const_points: the factors' terms into the frame blocks and gradients of Ug,
// and the coupling blocks into rp.cpl.  Launched only with factors.
void srk_launch_relpose_add(hipStream_t s, const SrkDims& d, const double* cam, const SrkRelPose& rp, double* Ug);
// behind srk_launch_assemble, before srk_launch_const_frames: rp.cpl into the lower triangle of S, fixed variables skipped
void srk_launch_relpose_couple(hipStream_t s, const SrkDims& d, const SrkRelPose& rp, double* S);
// the factor sum of a scene on its own (srk_ba_relative_pose_error): partial [srk_relpose_partials], out = the sum
void srk_launch_relpose_error(hipStream_t s, const double* cam, const SrkRelPose& rp, double* partial, double* out);
// joint Gaussian pose priors over sets of frames (srk_ba_set_joint_pose_priors): the lists of the resident
// scene.  Set g owns the slots set_ptr[g] .. set_ptr[g + 1] (at most SRK_JP_MAX_FRAMES_HOST); slot q is the internal frame
// frame[q] with the linearisation pose lin[12 q] (Rbar row-major, then Cbar, normalised world) and the mean mean[6 q]; the
// set's information matrix is the dense symmetric row-major (6 k)^2 block at info[info_ptr[g]].  Its coupled pairs (slots
// i > j whose block L_ij is not all zeros) are pair_ptr[g] .. pair_ptr[g + 1].  Two sets share at most one frame, so every
// entry of S the passes touch has one owner.
struct SrkJointPrior {
    int32_t n_sets;
    const int32_t* set_ptr;   // [n_sets + 1]
    const int32_t* frame;     // [n_slots] internal frame of each slot
    const double* lin;        // [n_slots][12]
    const double* mean;       // [n_slots][6]
    const int64_t* info_ptr;  // [n_sets]
    const double* info;
    const int32_t* pair_ptr;  // [n_sets + 1]
    const int32_t* pair_slot; // [n_pairs] (slot i of the set << 8) | slot j, i > j
    const int64_t* tgt;       // [n_pairs] offset in S of entry (0, 0) of the pair's block: row = first pose variable of the frame
                              // with the larger internal index, column = that of the other
    int32_t n_pairs;
    double* blk;              // [n_slots][42] 2 J_i^T L_ii J_i (6 x 6 row-major) and 2 J_i^T (L (r - m))_i, written by k_jprior_form
    double* cpl;              // [n_pairs][36] 2 J_i^T L_ij J_j, rows belonging to the frame with the larger internal index
    const int32_t* fr_list;   // [n_frames] internal frames with incident sets, ascending
    const int32_t* fr_ptr;    // [n_frames + 1] CSR into fr_ent
    const int32_t* fr_ent;    // slots of the frame, in set order
    int32_t n_frames;
};
// partial sums the joint-prior energy pass writes: one per set
inline int32_t srk_jprior_partials(int64_t n_sets) { return (int32_t)n_sets; }
// behind srk_launch_relpose_add, before srk_launch_const_points: blk and cpl from the current poses, then blk into Ug
void srk_launch_jprior_add(hipStream_t s, const SrkDims& d, const double* cam, const SrkJointPrior& jp, double* Ug);
// behind srk_launch_relpose_couple, before srk_launch_const_frames: jp.cpl into the lower triangle of S, fixed variables skipped
void srk_launch_jprior_couple(hipStream_t s, const SrkDims& d, const SrkJointPrior& jp, double* S);
// the prior sum of a scene on its own (srk_ba_joint_pose_prior_error): partial [srk_jprior_partials], out = the sum
void srk_launch_jprior_error(hipStream_t s, const double* cam, const SrkJointPrior& jp, double* partial, double* out);
void srk_launch_backsub(hipStream_t s, const SrkDims& d, double c, const int32_t* obs_frame, const int32_t* obs_pt,
                        const double* W, const double* Vg, const double* dc, double* acc, const double* pts,
                        double* pts_trial, double* dx);
void srk_launch_cam_apply(hipStream_t s, int32_t M, const double* R, const double* T, const double* dc, double* Rn,
                          double* Tn, const double* K, double f0, double* pack /* camera packs of the new poses, or NULL */,
                          int fv /* dc holds fv corrections per frame: 10, or 6 (pose only) */);
void srk_launch_error(hipStream_t s, const SrkDims& d, const double* pts, const double* cam,
                      const int32_t* obs_frame, const int32_t* obs_pt, const double* obs_uv, double* partial,
                      int32_t n_partial, double* err_out,
                      const int32_t* wg_jmin /* fused-Jacobian frame windows, or NULL: gather the cameras */,
                      int* info = nullptr, int* info2 = nullptr /* given: packed into err_out[1..2] and cleared */,
                      const SrkLoss* loss = nullptr /* given (kind != 0 or information): the sum of rho(q s) instead of s */,
                      const SrkPrior* prior = nullptr /* given: the prior sums of this scene as srk_prior_partials more partials
                                                         behind the observation partials, summed with them */,
                      const hipEvent_t* prior_ev = nullptr /* given: two events recorded around the prior pass */,
                      const SrkRelPose* relpose = nullptr /* given: the factor sum as srk_relpose_partials more partials behind
                                                             the priors' */,
                      const hipEvent_t* relpose_ev = nullptr /* given: two events recorded around that pass */,
                      const SrkJointPrior* jprior = nullptr /* given: the joint pose priors' sum as srk_jprior_partials more
                                                               partials behind the factors' */,
                      const hipEvent_t* jprior_ev = nullptr /* given: two events recorded around that pass */);
// the IRLS weights w = rho'(s) of the resident scene, one per observation in the internal order (srk_ba_observation_weights)
void srk_launch_obs_weights(hipStream_t s, const SrkDims& d, const double* pts, const double* cam, const int32_t* obs_frame,
                            const int32_t* obs_pt, const double* obs_uv, const SrkLoss& loss, double* w);
// the raw residuals f0 (ex, ey) in pixels, [O][2] in the internal order (srk_ba_observation_residuals)
void srk_launch_obs_residuals(hipStream_t s, const SrkDims& d, const double* pts, const double* cam, const int32_t* obs_frame,
                              const int32_t* obs_pt, const double* obs_uv, double* e);
int32_t srk_error_partials(const SrkDims& d);
int64_t srk_error_partials_staged(const SrkDims& d); // partial sums written when wg_jmin is given
void srk_launch_error_score(hipStream_t s, int64_t O, const double* pts, const double* cam, const int32_t* obs_frame,
                            const int32_t* obs_pt, const double* obs_uv, double z_tol /* < 0: keep every observation */,
                            double* partial /* 2 n_partial */, int32_t n_partial, double* out2 /* {error, count} */);
void srk_launch_expand_ug(hipStream_t s, int32_t M, const double* Ug, double* U_full, double* g_full);
void srk_launch_symmetrize(hipStream_t s, int64_t n, int64_t ld, double* S);

void srk_launch_env_zero(hipStream_t s, int64_t ld, const int64_t* env_col, double* S, double* rhs /* zeroed too, or null */,
                         int32_t* irr = nullptr /* hand-back counter of k_schur_mm, cleared too */);
void srk_launch_env_pack(hipStream_t s, int64_t ld, const int64_t* env_col, const int64_t* env_off, double* S,
                         double* packed, int dir);
void srk_launch_band_pack(hipStream_t s, int64_t ld, const int64_t* band_col, const int64_t* band_off, double* S,
                          double* packed, int dir /* 0 pack, 1 unpack */);

void srk_launch_checksum(hipStream_t s, const double* p, int64_t n, double* part /* 512 doubles of scratch */, double* out2 /* {sum, sum |.|} */);

// ---- multi-view-factorization steps (srk_ba_kernels.hip) ----
void srk_launch_mvf_depth(hipStream_t s, int64_t n_tracks, const int64_t* row_ptr, const int32_t* frame, const double* x_meter,
                          const double* cam_R, const double* cam_T, double* depth);
void srk_launch_mvf_gram(hipStream_t s, int64_t n_points, const double* x_anchor, const double* x_target, const double* depth,
                         double* partial /* [ceil(P / 256)][78] upper triangle of A^T A, row by row */);

// optional profile of one solve: event pairs around every MFMA trailing-update launch (n pairs recorded, at most
// cap / 2) and the flops those launches execute; dry = count only, launch nothing
struct SrkSolveProf {
    hipEvent_t* ev = nullptr;
    size_t cap = 0, n = 0;
    double flops = 0;
    bool dry = false;
};

// state of the fused outer-step kernel's in-launch hand-offs (k_step256): flag words (device, zeroed once, 16 per batch
// item) that hold the epoch of the launch that set them, and the host's launch counter.  One per stream.
#define SRK_SYNC_WORDS (16 * 32) // 16 words x SRK_MAX_CHUNKS items
struct SrkCholSync {
    unsigned* flags = nullptr;
    unsigned epoch = 0;
    bool fused = true; // false: the unfused k_panel / k_upd64 sequence
};

// ---- dense SPD solver (srk_chol.hip) ----
// In-place blocked Cholesky of the lower triangle of A (row-major, ld x ld, ld % SRK_CHOL_NB == 0) with the forward
// substitution folded in, then the backward substitution.  w: rhs (destroyed), y: scratch, x: solution.
// info (device int) is set non-zero when a pivot is not positive/finite or the solution is not finite.
// row_end / col_begin: optional host arrays describing the skyline of A (see srk_chol.hip); NULL = dense.
void srk_chol_solve(hipStream_t s, int64_t ld, double* A, double* w, double* y, double* x, int* d_info,
                    const int64_t* row_end, const int64_t* col_begin, double* dinv /* (ld / 64) * 4096 doubles */,
                    struct SrkSolveProf* prof /* may be NULL */, struct SrkCholSync* sync /* NULL: unfused kernels */,
                    int64_t n_real = 0 /* > 0: rows / columns from there on are padding (identity diagonal, zero rhs) */);

// ---- chunked (bordered block-diagonal) solve of a banded reduced camera system (srk_chol.hip) ----
#include <vector>
#define SRK_MAX_CHUNKS 32
#define SRK_MAX_SEPW 1024 // widest separator (= covisibility bandwidth in variables) the chunked solve takes on
struct SrkChunkPlan {
    int P = 0;                       // number of chunks; < 2 = not used
    int64_t sepw = 256;              // separator width (variables), >= bandwidth
    int64_t a[SRK_MAX_CHUNKS]{};     // first global variable of chunk c
    int64_t n[SRK_MAX_CHUNKS]{};     // interior size of chunk c (multiple of 256)
    int64_t ldc[SRK_MAX_CHUNKS]{};   // n + 2 sepw
    double* Ac[SRK_MAX_CHUNKS]{};    // chunk matrices (ldc x ldc)
    double* wc[SRK_MAX_CHUNKS]{};
    double* yc[SRK_MAX_CHUNKS]{};
    double* xc[SRK_MAX_CHUNKS]{};
    double* dinvc[SRK_MAX_CHUNKS]{};
    std::vector<int64_t> row_end[SRK_MAX_CHUNKS], col_begin[SRK_MAX_CHUNKS]; // local skylines
    int64_t lds = 0;                 // separator system size = sepw (P - 1)
    double *Cs = nullptr, *ws = nullptr, *ys = nullptr, *xs = nullptr, *dinvs = nullptr;
    std::vector<int64_t> s_row_end, s_col_begin;
    int64_t* d_sep_start = nullptr;  // device: first global variable of separator c
    int64_t* d_sep_env = nullptr;    // device: skyline (first column per 128-row tile) of the separator system
    SrkChunkPlan* child = nullptr;   // plan of the separator system itself (nested dissection); NULL = direct solve
};
void srk_chol_solve_chunked(hipStream_t s, const SrkChunkPlan& pl, int64_t ld, const double* S, const double* rhs,
                            double* x, const int64_t* d_env_col, int* d_info, struct SrkSolveProf* prof /* may be NULL */,
                            struct SrkCholSync* sync /* NULL: unfused kernels */);

// ---- shared intrinsics (srk_ba_set_intrinsic_groups) ----
// S_sh = P^T S10 P, stored ldb x ldb (row-major, lower part authoritative): pose variable 6 f + v ([Tx Ty Tz Wx Wy Wz]) in
// [0, ncols) (ncols = 6M rounded up to SRK_CHOL_NB; padding rows identity), then the border: row ncols + 4 g + k
// (k: fx fy u0 v0) for the G groups, rows up to ncols + SRK_SHK_BORDER identity, and SRK_SHK_BORDER more identity rows that
// pad the border system to one outer panel (ldb = ncols + 2 SRK_SHK_BORDER).
#define SRK_SHK_BORDER 128
#define SRK_SHK_MAX_GROUPS 32
struct SrkShk {
    int32_t M, G;
    int64_t ld10, ncols, ldb;
    const int32_t* grp;             // [M] group of each internal frame
    const int32_t* cpl_lo;          // [M] frames f with a (possibly) non-zero block (f, f') of S10: cpl_lo[f'] <= f <= cpl_hi[f']
    const int32_t* cpl_hi;
    const int32_t* mem_ptr;         // [G + 1] / [M]: the members of each group, ascending internal index
    const int32_t* mem;
    const int64_t* env_sh;          // [ncols / 128] first column of the compact pose skyline per 128-row tile
    double* T;                      // scratch [4G][4M]: border rows of P^T S10 at the intrinsic columns, per frame
};
// S_sh, rhs_sh from the damped 10-variable system S10, rhs10 (fixed summation order, no atomics)
void srk_launch_rcs_fold(hipStream_t s, const SrkShk& k, const double* S10, const double* rhs10, double* Ssh, double* rsh);
// dc10 = P dc_sh, and the trial intrinsics of every frame: Ktr = Kcur + the group's corrections (bundle-adj-kanatani.cpp:2025-2033)
void srk_launch_rcs_expand(hipStream_t s, const SrkShk& k, const double* dcsh, double* dc10, const double* Kcur, double* Ktr);
// the bordered system: the pose columns [0, ncols) on their skyline (row_end / col_begin NULL = dense) with the
// SRK_SHK_BORDER border rows riding along, then the border's own system, then the backward substitution.  w: rhs (destroyed),
// y: scratch [ldb], x: solution [ldb], dinv: (ldb / 64) * 4096 doubles
void srk_chol_solve_bordered(hipStream_t s, int64_t ncols, int64_t ldb, double* A, double* w, double* y, double* x,
                             double* dinv, int* d_info, const int64_t* row_end, const int64_t* col_begin, int64_t n_real,
                             int64_t n_border_real, struct SrkSolveProf* prof, struct SrkCholSync* sync);
