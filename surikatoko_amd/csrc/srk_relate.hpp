// srk_relate.hpp -- two-view relative pose (srk_relate_frames), the host half: the option defaults, the
// argument checks and a walk of one pair on the host in the kernels' own order of operations.  Host only: no HIP, so all of it can
// be checked on a machine without a GPU (tests/cpp/test_relate_host.cpp).  srk_ba_host.hip allocates and copies; the kernels are
// in srk_relate.hip.
#pragma once
#include "../../include/srk_ba.h"
#include "srk_limits.hpp"

#include <stdint.h>
#include <string>
#include <vector>

// the options a call runs with: opts NULL = the defaults
srk_relate_options srk_relate_effective_options(const srk_relate_options* opts);

// The checks of a call, or the text of its refusal (empty = fine).  Every index the kernels will follow is looked at here.
std::string srk_relate_check(int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q, const double* K_a,
                             const double* K_b, int shared_k, const srk_relate_options* opts);

// One hypothesis on the host, statement for statement what the 16 lanes of k_relate_solve do together: the null space of the first
// five matches, the ten constraint rows, the elimination with the pivot's owner recorded in place of an exchange, det B(z), its real
// roots by the derivative chain (interval k is lane k's), and the choice among the roots' essential matrices by the sixth match.
// Kai, Kbi: the inverses of the intrinsics; uva, uvb [6][2].  rec [SRK_RELATE_HYP].  Returns the number of real roots; all_E
// (may be NULL) receives their essential matrices [10][9] in ascending order of the root.
int srk_relate_host_hypothesis(const double* Kai, const double* Kbi, const double* uva, const double* uvb, double f0, double* rec, double* all_E);

// One pair on the host, statement for statement what the kernels do (the ranks of the weighted matches, every hypothesis, its
// score summed in ascending rank order, the pick with the vote's counts and the parallax merged in the wave's tree; only the
// contraction of multiply-adds and the last bits of sqrt and atan2 may differ).  uv_a, uv_b, q, inlier_out: the pair's own matches.
// scores (may be NULL) receives every hypothesis' score.  Returns the status bits.
uint32_t srk_relate_host_pair_cpp(int64_t n_obs, const double* uv_a, const double* uv_b, const double* q, const double* K_a, const double* K_b,
                                  double f0, const srk_relate_options& opts, double R[9], double T[3], double E[9], double related[8],
                                  uint8_t* inlier_out, std::vector<double>* scores = nullptr);

// The decomposition alone, for the tests: the four poses of E in the order of srk_relate_math.hpp.  R [4][9], T [4][3].
void srk_relate_poses_of(const double* E, double* R, double* T);
