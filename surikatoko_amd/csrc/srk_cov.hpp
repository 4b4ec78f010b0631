// srk_cov.hpp -- marginal covariances of frames and landmarks (srk_ba_phase_covariance) and the blocks
// between two of them (srk_ba_phase_cross_covariance; section 17): the kernels of srk_cov.hip.  They work on the factor the single-chain solver (srk_chol_solve) leaves behind: the strictly
// lower 64 x 64 tiles of L in the slot's S and the inverses of the diagonal tiles in dinv.
#pragma once
#include "srk_dev.hpp"

#define SRK_COV_CB 64 // right-hand-side columns one workgroup of k_cov_fwd owns

// one selected block: fv columns of a frame, or 3 columns of a landmark.  first_row: no row of its columns above it is
// non-zero (the frame's first variable; the first variable of the first frame that sees the landmark)
struct SrkCovGroup {
    int64_t idx;       // internal frame, or internal landmark
    int32_t col0;      // its first column of Y in this batch
    int32_t ncols;     // fv, or 3
    int32_t first_row;
    int32_t is_point;
};

// Y [ld][ncp] (row-major, zero on entry): the unit columns of the frames' free variables; for a landmark the rows
// W_o^T V^-1 of the frames of its observations (V at damping c), rows of fixed variables left zero.
// free_var [ld]: 1 = the variable moves (not gauge-fixed, not of a constant frame, not padding).  info |= 1 where a landmark
// block is not invertible.
void srk_launch_cov_rhs(hipStream_t s, const SrkDims& d, double c, const SrkCovGroup* grp, int32_t n_grp, const int64_t* row_ptr,
                        const int32_t* obs_frame, const double* W, const double* Vg, const uint8_t* free_var, double* Y, int64_t ncp,
                        int* info);
// Y <- L^-1 Y.  blk_first [ncp / SRK_COV_CB]: first 64-row tile with a non-zero in the block's columns.  col_begin (device,
// [ld / 64]): first column with a non-zero in each tile row.  n_tiles: tile rows that hold variables (the padding below is skipped).
void srk_launch_cov_fwd(hipStream_t s, int64_t ld, const double* L, const double* dinv, const int64_t* col_begin, int32_t n_tiles,
                        const int32_t* blk_first, double* Y, int64_t ncp);
// out [n_grp][100]: the ncols x ncols product Y_g^T Y_g over the rows [first_row, n_rows), row-major with stride ncols; for a
// landmark V^-1 is added
void srk_launch_cov_gram(hipStream_t s, const SrkDims& d, double c, const SrkCovGroup* grp, int32_t n_grp, const double* Vg,
                         const double* Y, int64_t ncp, int64_t n_rows, double* out);

// one requested pair of blocks of a batch (k_cov_cross): indices into the batch's group table
struct SrkCovPair {
    int32_t p, q;
};
// out [n_ff + n_pf + n_pp][100]: the product Y_p^T Y_q over the rows [max(first_row_p, first_row_q), n_rows), row-major
// n_p x n_q.  pairs holds the frame x frame pairs first, then the landmark x frame pairs (p the landmark; the block is
// negated), then the landmark x landmark pairs (V^-1 is added where p == q).  One launch per kind that has pairs.
void srk_launch_cov_cross(hipStream_t s, const SrkDims& d, double c, const SrkCovGroup* grp, const SrkCovPair* pairs, int32_t n_ff, int32_t n_pf,
                          int32_t n_pp, const double* Vg, const double* Y, int64_t ncp, int64_t n_rows, double* out);
