// srk_pair.hip -- two-view pose refinement (srk_refine_pairs, srk_relate_frames_refined), the device half.
//
// A pair is an independent problem of five variables and hundreds to thousands of matches: one wave of 64 lanes per pair, four
// pairs per workgroup, in the pattern of k_resect_frames.  Each lane adds the Gauss-Newton terms of its matches into 22 sums (E,
// the upper triangle of H, g, the weight sum); the lanes merge them with cross-lane moves in a fixed tree (down by 32, 16, 8, 4,
// 2, 1), lane 0 solves the damped 5 x 5 system and the step is broadcast.  No LDS, no workgroup barrier, no atomics: a pair's bits
// depend on its own matches, its start pose and the options alone.
//
// F and the five dF_k are uniform over a pair at one pose: every lane forms them once per linearisation (twelve 3 x 3 products),
// not per match.  The weighted matches (q > 0) of a pair are dealt to the lanes by their rank among the weighted ones, so a match
// with q = 0 leaves the very computation of the pair without it.
#include "srk_pair_dev.hpp"
#include "srk_pair_math.hpp"

#define PR_BLOCK 256
#define PR_L SRK_PAIR_LANES
static_assert(PR_L == 64, "a pair's ballot is the wave's");

__global__ __launch_bounds__(256) void k_pair_pack(int32_t n_pairs, const double* __restrict__ K_a, const double* __restrict__ K_b, int shared_k,
                                                   double* __restrict__ kinv)
{
    const int32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_pairs) return;
    const double* ka = shared_k ? K_a : K_a + 9 * (int64_t)j;
    const double* kb = shared_k ? K_b : K_b + 9 * (int64_t)j;
    double a[9], b[9], ai[9], bi[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) a[e] = ka[e], b[e] = kb[e];
    srk_relate_inverse3(a, ai);
    srk_relate_inverse3(b, bi);
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        kinv[(int64_t)SRK_PAIR_KINV * j + e] = ai[e];
        kinv[(int64_t)SRK_PAIR_KINV * j + 9 + e] = bi[e];
    }
}

void srk_launch_pair_pack(hipStream_t s, int32_t n_pairs, const double* K_a, const double* K_b, int shared_k, double* kinv)
{
    if (n_pairs <= 0) return;
    hipLaunchKernelGGL(k_pair_pack, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, s, n_pairs, K_a, K_b, shared_k, kinv);
}

__global__ __launch_bounds__(256) void k_pair_mask(int64_t n_obs, const double* __restrict__ q, const uint8_t* __restrict__ inlier,
                                                   double* __restrict__ qe)
{
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_obs) return;
    qe[o] = (q ? q[o] : 1.0) * (double)inlier[o];
}

void srk_launch_pair_mask(hipStream_t s, int64_t n_obs, const double* q, const uint8_t* inlier, double* qe)
{
    if (n_obs <= 0) return;
    hipLaunchKernelGGL(k_pair_mask, dim3((unsigned)((n_obs + 255) / 256)), dim3(256), 0, s, n_obs, q, inlier, qe);
}

// Lane `lane` visits its share of the weighted matches of [o0, o1), in ascending order: the match of rank r among the weighted
// ones belongs to lane r % 64 (the walk of srk_resect.hip).  The matches are looked at 64 at a time; the wave's ballot says which of
// them are weighted, and a lane finds the position of "its" set bit by halving.  body(o) holds no cross-lane move (the lanes diverge
// around it).  Returns the number of weighted matches, the same in every lane.
template <class Body>
__device__ __forceinline__ int64_t pr_walk(int64_t o0, int64_t o1, const double* __restrict__ q, int lane, Body&& body)
{
    int64_t base = 0;
    for (int64_t c0 = o0; c0 < o1; c0 += PR_L) {
        const int64_t o = c0 + lane;
        const bool w = o < o1 && (q == nullptr || q[o] > 0.0);
        const unsigned long long m = __ballot(w);
        const int cnt = __popcll(m);
        int k = (lane - (int)(base & (PR_L - 1))) & (PR_L - 1); // my place among this chunk's weighted matches
        if (k < cnt) {
            int pos = 0;
#pragma unroll
            for (int sh = PR_L / 2; sh >= 1; sh >>= 1) {
                const int c = __popcll((m >> pos) & ((1ull << sh) - 1ull));
                if (k >= c) {
                    k -= c;
                    pos += sh;
                }
            }
            body(c0 + pos);
        }
        base += cnt;
    }
    return base;
}

__device__ __forceinline__ void pr_sums_down(SrkPairSums& a)
{
#pragma unroll
    for (int d = PR_L / 2; d >= 1; d >>= 1) {
        SrkPairSums b;
        b.E = __shfl_down(a.E, d, PR_L);
#pragma unroll
        for (int e = 0; e < SRK_PAIR_NH; ++e) b.h[e] = __shfl_down(a.h[e], d, PR_L);
#pragma unroll
        for (int e = 0; e < SRK_PAIR_NV; ++e) b.g[e] = __shfl_down(a.g[e], d, PR_L);
        b.wsum = __shfl_down(a.wsum, d, PR_L);
        srk_pair_sums_add(a, b); // lane 0 ends with the whole tree; what the other lanes hold is not used
    }
}

// the sums of the pair at the pose p into lane 0; returns the number of weighted matches
__device__ __forceinline__ int64_t pr_eval(int64_t o0, int64_t o1, const double* __restrict__ uv_a, const double* __restrict__ uv_b,
                                           const double* __restrict__ q, const double* kinv, const SrkPairPose& p, double f0, int kind,
                                           double delta, int lane, SrkPairSums& sums)
{
    SrkPairLin lin;
    srk_pair_linearise(kinv, p, lin);
    srk_pair_sums_zero(sums);
    const int64_t n = pr_walk(o0, o1, q, lane, [&](int64_t o) {
        const double2 a = reinterpret_cast<const double2*>(uv_a)[o];
        const double2 b = reinterpret_cast<const double2*>(uv_b)[o];
        srk_pair_obs(sums, lin, a.x, a.y, b.x, b.y, f0, q ? q[o] : 1.0, kind, delta);
    });
    pr_sums_down(sums);
    return n;
}

__global__ __launch_bounds__(PR_BLOCK) void k_pair_refine(int32_t n_pairs, const int64_t* __restrict__ row_ptr, const double* __restrict__ uv_a,
                                                          const double* __restrict__ uv_b, const double* __restrict__ q,
                                                          const double* __restrict__ kinv_all, const double* __restrict__ R0,
                                                          const double* __restrict__ T0, const uint32_t* __restrict__ related_status, double f0,
                                                          int32_t attempts, double rel_change, int32_t kind, double delta,
                                                          double* __restrict__ Rout, double* __restrict__ Tout, double* __restrict__ Eout,
                                                          double* __restrict__ quality, double* __restrict__ info, double* __restrict__ basis,
                                                          uint32_t* __restrict__ status, double* __restrict__ w_out)
{
    const int lane = threadIdx.x & (PR_L - 1);
    const int64_t i = (int64_t)blockIdx.x * (PR_BLOCK / PR_L) + (threadIdx.x / PR_L);
    if (i >= n_pairs) return; // a whole wave: the lanes of a pair leave together
    const int64_t o0 = row_ptr[i], o1 = row_ptr[i + 1];
    double kinv[SRK_PAIR_KINV];
#pragma unroll
    for (int e = 0; e < SRK_PAIR_KINV; ++e) kinv[e] = kinv_all[(int64_t)SRK_PAIR_KINV * i + e];

    SrkPairPose cur;
    srk_pair_start_pose(R0 + 9 * i, T0 + 3 * i, related_status ? related_status[i] != 0u : 0, cur);
    SrkPairSums cs;
    const int64_t n = pr_eval(o0, o1, uv_a, uv_b, q, kinv, cur, f0, kind, delta, lane, cs);

    // Levenberg-Marquardt on the Sampson error: lane 0 holds the sums and solves, every lane carries the pose
    int hit_cap = 0, used = 0;
    if (n >= SRK_PAIR_NV && attempts > 0) {
        double c = SRK_RESECT_C0;
        hit_cap = 1;
        for (int32_t a = 0; a < attempts; ++a) {
            double d[SRK_PAIR_NV];
            int stepped = srk_pair_lm_step(cs, c, d);
#pragma unroll
            for (int e = 0; e < SRK_PAIR_NV; ++e) d[e] = __shfl(d[e], 0, PR_L);
            stepped = __shfl(stepped, 0, PR_L);
            SrkPairPose cand = cur;
            SrkPairSums ns;
            srk_pair_sums_zero(ns);
            if (stepped) {
                srk_pair_move(cur, d, cand);
                pr_eval(o0, o1, uv_a, uv_b, q, kinv, cand, f0, kind, delta, lane, ns);
            }
            const double cur_E = __shfl(cs.E, 0, PR_L), cand_E = __shfl(ns.E, 0, PR_L);
            const int verdict = srk_resect_judge(cur_E, cand_E, stepped, c, rel_change);
            ++used;
            if (verdict & 1) {
                cur = cand;
                cs = ns;
            }
            if (verdict & 2) {
                hit_cap = 0;
                break;
            }
        }
    }

    // the matches in front of both cameras at the result: a count per lane, merged in the same tree
    int front = 0;
    if (n >= SRK_PAIR_NV) {
        pr_walk(o0, o1, q, lane, [&](int64_t o) {
            const double2 a = reinterpret_cast<const double2*>(uv_a)[o];
            const double2 b = reinterpret_cast<const double2*>(uv_b)[o];
            front += srk_pair_front(kinv, cur, a.x, a.y, b.x, b.y, f0);
        });
#pragma unroll
        for (int d = PR_L / 2; d >= 1; d >>= 1) front += __shfl_down(front, d, PR_L);
    }

    if (lane == 0) {
        double el[9], ql[6], inf[25], bs[6];
        const uint32_t st = n >= SRK_PAIR_NV ? srk_pair_finish(cs, cur, n, front, f0, hit_cap, used, el, ql, inf, bs) : srk_pair_few(cur, n, el, ql, inf, bs);
#pragma unroll
        for (int e = 0; e < 9; ++e) Rout[9 * i + e] = cur.R[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) Tout[3 * i + e] = cur.T[e];
#pragma unroll
        for (int e = 0; e < 9; ++e) Eout[9 * i + e] = el[e];
#pragma unroll
        for (int e = 0; e < 6; ++e) quality[6 * i + e] = ql[e];
#pragma unroll
        for (int e = 0; e < 25; ++e) info[25 * i + e] = inf[e];
#pragma unroll
        for (int e = 0; e < 6; ++e) basis[6 * i + e] = bs[e];
        status[i] = st;
    }
    if (w_out) { // the robust weights at the result, 0 where q = 0
        double E[9], F[9];
        srk_relate_essential(cur.R, cur.T, E);
        srk_relate_fundamental(kinv, kinv + 9, E, F);
        for (int64_t o = o0 + lane; o < o1; o += PR_L) {
            const double qo = q ? q[o] : 1.0;
            double w = 0.0;
            if (qo > 0.0) {
                const double2 a = reinterpret_cast<const double2*>(uv_a)[o];
                const double2 b = reinterpret_cast<const double2*>(uv_b)[o];
                w = srk_pair_weight(F, a.x, a.y, b.x, b.y, f0, qo, kind, delta);
            }
            w_out[o] = w;
        }
    }
}

void srk_launch_pair_refine(hipStream_t s, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                            const double* kinv, const double* R0, const double* T0, const uint32_t* related_status, double f0, int32_t attempts,
                            double rel_change, int32_t loss_kind, double loss_delta, double* R, double* T, double* E, double* quality, double* info,
                            double* basis, uint32_t* status, double* w_out)
{
    if (n_pairs <= 0) return;
    const int32_t per = PR_BLOCK / PR_L;
    hipLaunchKernelGGL(k_pair_refine, dim3((unsigned)((n_pairs + per - 1) / per)), dim3(PR_BLOCK), 0, s, n_pairs, row_ptr, uv_a, uv_b, q, kinv, R0, T0,
                       related_status, f0, attempts, rel_change, loss_kind, loss_delta, R, T, E, quality, info, basis, status, w_out);
}
