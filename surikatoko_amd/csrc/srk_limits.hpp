// srk_limits.hpp -- the kernels' limits as the host sees them: plain constants, no HIP.  Included by srk_dev.hpp (the HIP
// translation units) and by srk_plan.hpp (the host-only scene planner); srk_ba_kernels.hip asserts them against its own.
#pragma once

// fused single-pass derivative kernel: usable when every workgroup's frame range fits SRK_JF_SLOTS_HOST
#define SRK_JF_OBS_HOST 1024
#define SRK_JF_SLOTS_HOST 48
#define SRK_JF_PMAX_HOST 448
// run-based derivative kernel: one wave per task = consecutive landmarks with identical frame lists (nf <= 64 frames), about
// SRK_JR_TASK_PTS_MIN_HOST .. MAX_HOST of them; four consecutive tasks (one workgroup) must touch fewer than
// SRK_JF_SLOTS_HOST consecutive frames
#define SRK_JR_TASK_PTS_MIN_HOST 12
#define SRK_JR_TASK_PTS_MAX_HOST 96 // = SRK_JR_XMAX of the kernel
#define SRK_JD_MAXNF_HOST 32        // frames of a run of the derivative kernel's own: one mask word
#define SRK_GRP_MAXNF_HOST 24   // must match SRK_GRP_MAXNF in srk_ba_kernels.hip
#define SRK_GRP_MAXPTS_HOST 128 // landmarks per workgroup run
#define SRK_GRP_NF1_HOST 21     // must match SRK_GRP_NF1
#define SRK_WS_NF_HOST 20       // must match SRK_WS_NF (runs the MFMA kernel k_schur_mm takes)
// tracks longer than SRK_GRP_MAXNF_HOST frames: runs of <= SRK_LONG_PTS_HOST landmarks over a frame set of
// <= SRK_LONG_MAXNF_HOST frames, one workgroup per pair of 8-frame blocks (k_schur_long); longer tracks stay with k_schur.
// (Round 3: 4096 -- the limit is only the row length of the run_frames table; it was 256, and a track over more frames fell
// back to the per-landmark global-atomics kernel, a 30x cliff on all-visible scenes of more than 256 frames.)
#define SRK_LONG_PTS_HOST 128
#define SRK_LONG_MAXNF_HOST 4096
#define SRK_LONG_FB_HOST 8
// joint Gaussian pose priors (srk_ba_set_joint_pose_priors): frames of one set; its information matrix has 6 x that many rows
#define SRK_JP_MAX_FRAMES_HOST 16
// marginalisation priors (srk_ba_marginalization_prior): frames dropped by one call, frames its result may
// tie (the dense strip of k_marg_rows has 6 x (their sum) + 1 columns, padded to a multiple of 16: at most SRK_MARG_LDZ_HOST)
#define SRK_MARG_MAX_DROP_HOST 8
#define SRK_MARG_MAX_KEPT_HOST 32
#define SRK_MARG_LDZ_HOST 256
#define SRK_MARG_ROWS 4 // rows of the strip per landmark: three of L^-1 W and one of zeros (a step of the f64 MFMA takes four rows)
// batched triangulation (srk_triangulate_tracks): the track and observation counts are 64-bit and a track
// may have any length; the grid holds 32 tracks a workgroup, so a call takes at most 2^31 - 1 workgroups' worth of tracks
#define SRK_TRI_MAX_REFINE_ATTEMPTS_HOST 64
#define SRK_TRI_TRACKS_PER_WG_HOST 32
#define SRK_TRI_MAX_TRACKS_HOST (2147483647LL * SRK_TRI_TRACKS_PER_WG_HOST)
// batched camera resection (srk_resect_frames): one wave per frame and four frames a workgroup; a frame may
// have any number of observations (64-bit counts), landmarks are indexed by int32
#define SRK_RESECT_MAX_ATTEMPTS_HOST 64
#define SRK_RESECT_FRAMES_PER_WG_HOST 4
#define SRK_RESECT_MAX_FRAMES_HOST (1 << 22)
// resection without a start pose (srk_locate_frames): a wave scores 64 hypotheses of one frame; a call holds
// one slot of 160 bytes per wave, so frames x ceil(hypotheses / 64) is capped (640 MiB of slots at the cap)
#define SRK_LOCATE_MAX_HYPOTHESES_HOST 4096
#define SRK_LOCATE_LANES_HOST 64
#define SRK_LOCATE_MAX_WAVES_HOST (1 << 22)
// two-view relative pose (srk_relate_frames): a wave scores 64 hypotheses of one pair; a call holds one record
// of 160 bytes per hypothesis and one slot per wave, so pairs x ceil(hypotheses / 64) is capped like locate's
#define SRK_RELATE_MAX_HYPOTHESES_HOST 4096
#define SRK_RELATE_LANES_HOST 64
#define SRK_RELATE_MAX_WAVES_HOST (1 << 22)
// map alignment (srk_align_points): a wave scores 64 hypotheses of one set; a call holds one slot of 160 bytes
// per wave, so sets x ceil(hypotheses / 64) is capped like locate's
#define SRK_ALIGN_MAX_HYPOTHESES_HOST 4096
#define SRK_ALIGN_LANES_HOST 64
#define SRK_ALIGN_MAX_WAVES_HOST (1 << 22)
#define SRK_ALIGN_MAX_ROUNDS_HOST 16
// two-view homography (srk_relate_homography): a wave scores 64 hypotheses of one pair; a call holds one slot
// of 128 bytes per wave, so pairs x ceil(hypotheses / 64) is capped like align's
#define SRK_HOMOG_MAX_HYPOTHESES_HOST 4096
#define SRK_HOMOG_LANES_HOST 64
#define SRK_HOMOG_MAX_WAVES_HOST (1 << 22)
#define SRK_HOMOG_MAX_ROUNDS_HOST 16
// two-view fundamental matrix (srk_relate_uncalibrated): a wave scores 64 hypotheses of one pair; a call holds
// one record of 96 bytes per hypothesis and one slot per wave, so pairs x ceil(hypotheses / 64) is capped like relate's
#define SRK_FUND_MAX_HYPOTHESES_HOST 4096
#define SRK_FUND_LANES_HOST 64
#define SRK_FUND_MAX_WAVES_HOST (1 << 22)
#define SRK_FUND_MAX_ROUNDS_HOST 16
