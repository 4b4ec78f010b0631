// srk_marg_dev.hpp -- the kernels of the marginalisation priors (srk_marg.hip).  The tables are those of a
// SrkMargPlan (srk_marg.hpp), copied to the device by srk_ba_host.hip.
#pragma once
#include "srk_dev.hpp"

#define SRK_MARG_STAGE 28 // doubles of an observation's staging row: 21 entries of the upper triangle of its 6 x 6 pose block (row by
                          // row), 6 gradient entries, one of padding

struct SrkMargTables {
    int32_t n_lm;               // selected landmarks
    int32_t n_slots;            // d + k
    int32_t ldz;                // columns of the strip: 6 n_slots + 1 rounded up to 16 (<= SRK_MARG_LDZ_HOST)
    const int32_t* lm;          // [n_lm] internal landmark
    const int64_t* lm_stage;    // [n_lm] first staging row of the landmark's observations
    const int32_t* lm_prior;    // [n_lm] place of the landmark's position prior in prior_val, -1 = none
    const int32_t* frame_slot;  // [M] slot of an internal frame, -1 = none
    const double* prior_val;    // [9][n_priors] (SrkPrior::pt_val)
    int64_t n_priors;
    const int32_t* slot_ptr;    // [n_slots + 1]
    const int64_t* slot_ent;    // staging rows of each slot's observations, landmarks ascending
};

// Z [4 n_lm][ldz] and stage [n_stage][SRK_MARG_STAGE] zero on entry.  One wave per selected landmark: rows 4 l .. 4 l + 2 of Z
// receive L^-1 W_o at the columns of the slot of each weighted observation's frame and L^-1 g_l in column 6 n_slots (V_l = L L^T
// with the landmark's position prior added, undamped), row 4 l + 3 stays zero; the staging row of every weighted observation
// receives the frame's own w J^T J and w J^T e.  skipped [n_lm]: 1 where V_l fails the determinant or a pivot test -- the
// landmark then writes nothing at all.  Blocks and gradients carry the factor 2 of the derivative kernels.
void srk_launch_marg_rows(hipStream_t s, const SrkDims& d, const double* pts, const double* cam, const int64_t* row_ptr,
                          const int32_t* obs_frame, const double* obs_uv, const SrkLoss* loss, const SrkMargTables& t, double* Z,
                          double* stage, int32_t* skipped);
// Us [n_slots][27]: per slot the sum of its observations' staging rows in the order of slot_ent
void srk_launch_marg_frame_sums(hipStream_t s, const SrkMargTables& t, const double* stage, double* Us);
// the partial Gram products of the row chunks: part [n_chunks][ldz][ldz], lower block triangle of 16 x 16 tiles
void srk_launch_marg_gram(hipStream_t s, const double* Z, int64_t n_rows, int32_t ldz, int32_t n_chunks, int64_t rows_per_chunk, double* part);
// A [(6 n_slots)^2] = (U_F - G) / 2 (both triangles) and b [6 n_slots] = (u_F - Z^T z) / 2, the chunks summed in their order
void srk_launch_marg_reduce(hipStream_t s, const double* part, int32_t n_chunks, int32_t ldz, int32_t n_slots, const double* Us, double* A,
                            double* b);
