// srk_fund.hpp -- the two-view fundamental matrix (srk_relate_uncalibrated), the host half: the option
// defaults, the argument checks and a walk of one pair on the host in the kernels' own order of operations.  Host only: no HIP, so
// all of it can be checked on a machine without a GPU (tests/cpp/test_fund_host.cpp).  srk_ba_host.hip allocates and copies; the
// kernels are in srk_fund.hip.
#pragma once
#include "../../include/srk_ba.h"
#include "srk_limits.hpp"

#include <stdint.h>
#include <string>
#include <vector>

// the options a call runs with: opts NULL = the defaults
srk_fundamental_options srk_fund_effective_options(const srk_fundamental_options* opts);

// The checks of a call, or the text of its refusal (empty = fine).  Every index the kernels will follow is looked at here.
std::string srk_fund_check(int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                           const srk_fundamental_options* opts);

// the outputs of one pair
struct SrkFundResult {
    double F[9], U[9], V[9], sigma, fund[12], info[49];
};

// One pair on the host, statement for statement what the kernels do (the ranks of the weighted matches, every hypothesis' sample,
// model and score in ascending rank order, the pick, the representation, the attempts with the lanes' strided sums merged in the
// wave's tree; only the contraction of multiply-adds and the last bits of sqrt may differ).  scores (may be NULL) receives every
// hypothesis' score, roots (may be NULL) every hypothesis' number of real roots (-1 without a model).  Returns the status bits.
uint32_t srk_fund_host_walk(int64_t n_obs, const double* uv_a, const double* uv_b, const double* q, double f0, const srk_fundamental_options& opts,
                            SrkFundResult& out, uint8_t* inlier_out, std::vector<double>* scores = nullptr, std::vector<int32_t>* roots = nullptr);
