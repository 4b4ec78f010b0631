// srk_resect.hip -- batched camera resection with robust pose refinement (srk_resect_frames, srk_ba_resect),
// the device half.
//
// A frame is an independent problem of six variables and hundreds to thousands of observations, and frames are few: one wave of
// 64 lanes per frame, four frames per workgroup.  Each lane adds the Gauss-Newton terms of its observations into 30 registers'
// worth of sums (E, the upper triangle of H, g, the weight sum, the smallest depth); the lanes merge them with cross-lane moves
// in a fixed tree (down by 32, 16, 8, 4, 2, 1), lane 0 solves the damped 6 x 6 system and the step is broadcast.  No LDS, no
// workgroup barrier, no atomics: a frame's bits depend on its own observations alone.
//
// The weighted observations (q > 0) of a frame are dealt to the lanes by their rank among the weighted ones, so an observation
// with q = 0 leaves the very computation of the frame without it.
#include "srk_resect_dev.hpp"
#include "srk_resect_math.hpp"

#define RS_BLOCK 256
#define RS_L SRK_RESECT_LANES
static_assert(RS_L == 64, "a frame's ballot is the wave's");

__global__ __launch_bounds__(256) void k_resect_pack(int32_t n_frames, const double* __restrict__ R0, const double* __restrict__ T0,
                                                     const double* __restrict__ K, int shared_k, double* __restrict__ pack)
{
    const int32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_frames) return;
    SrkResectPose s;
    srk_resect_start_pose(R0 + 9 * (int64_t)j, T0 + 3 * (int64_t)j, s);
    double p[SRK_RESECT_PACK];
    srk_resect_pack_pose(s, shared_k ? K : K + 9 * (int64_t)j, p);
#pragma unroll
    for (int e = 0; e < SRK_RESECT_PACK; ++e) pack[(int64_t)SRK_RESECT_PACK * j + e] = p[e];
}

void srk_launch_resect_pack(hipStream_t s, int32_t n_frames, const double* R0, const double* T0, const double* K, int shared_k, double* pack)
{
    if (n_frames <= 0) return;
    hipLaunchKernelGGL(k_resect_pack, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, s, n_frames, R0, T0, K, shared_k, pack);
}

// Lane `lane` visits its share of the weighted observations of [o0, o1), in ascending order: the observation of rank r among the
// weighted ones belongs to lane r % 64.  The observations are looked at 64 at a time; the wave's ballot says which of them are
// weighted, and a lane finds the position of "its" set bit by halving (six population counts).  body(o) holds no cross-lane
// move (the lanes diverge around it).  Returns the number of weighted observations, the same in every lane.
template <class Body>
__device__ __forceinline__ int64_t rs_walk(int64_t o0, int64_t o1, const double* __restrict__ q, int lane, Body&& body)
{
    int64_t base = 0;
    for (int64_t c0 = o0; c0 < o1; c0 += RS_L) {
        const int64_t o = c0 + lane;
        const bool w = o < o1 && (q == nullptr || q[o] > 0.0);
        const unsigned long long m = __ballot(w);
        const int cnt = __popcll(m);
        int k = (lane - (int)(base & (RS_L - 1))) & (RS_L - 1); // my place among this chunk's weighted observations
        if (k < cnt) {
            int pos = 0;
#pragma unroll
            for (int sh = RS_L / 2; sh >= 1; sh >>= 1) {
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

__device__ __forceinline__ void rs_sums_down(SrkResectSums& a)
{
#pragma unroll
    for (int d = RS_L / 2; d >= 1; d >>= 1) {
        SrkResectSums b;
        b.E = __shfl_down(a.E, d, RS_L);
#pragma unroll
        for (int e = 0; e < SRK_RESECT_NH; ++e) b.h[e] = __shfl_down(a.h[e], d, RS_L);
#pragma unroll
        for (int e = 0; e < 6; ++e) b.g[e] = __shfl_down(a.g[e], d, RS_L);
        b.wsum = __shfl_down(a.wsum, d, RS_L);
        b.min_depth = __shfl_down(a.min_depth, d, RS_L);
        srk_resect_sums_add(a, b); // lane 0 ends with the whole tree; what the other lanes hold is not used
    }
}

// the sums of the frame under the pack p into lane 0; returns the number of weighted observations
__device__ __forceinline__ int64_t rs_eval(int64_t o0, int64_t o1, const int32_t* __restrict__ point, const double* __restrict__ uv,
                                           const double* __restrict__ q, const double* __restrict__ X, const double* p, double f0, int kind,
                                           double delta, int lane, SrkResectSums& sums)
{
    srk_resect_sums_zero(sums);
    const int64_t n = rs_walk(o0, o1, q, lane, [&](int64_t o) {
        const double* x = X + 3 * (int64_t)point[o];
        const double xl[3] = { x[0], x[1], x[2] };
        const double2 m = reinterpret_cast<const double2*>(uv)[o];
        srk_resect_obs(sums, p, xl, m.x, m.y, f0, q ? q[o] : 1.0, kind, delta);
    });
    rs_sums_down(sums);
    return n;
}

__global__ __launch_bounds__(RS_BLOCK) void k_resect_frames(int32_t n_frames, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ point,
                                                            const double* __restrict__ uv, const double* __restrict__ q,
                                                            const double* __restrict__ X, const double* __restrict__ K, int shared_k,
                                                            const double* __restrict__ R0, const double* __restrict__ T0,
                                                            const double* __restrict__ pack, double f0, int32_t attempts, double rel_change,
                                                            int32_t kind, double delta, double* __restrict__ Rout, double* __restrict__ Tout,
                                                            double* __restrict__ quality, double* __restrict__ info, uint32_t* __restrict__ status,
                                                            double* __restrict__ w_out)
{
    const int lane = threadIdx.x & (RS_L - 1);
    const int64_t i = (int64_t)blockIdx.x * (RS_BLOCK / RS_L) + (threadIdx.x / RS_L);
    if (i >= n_frames) return; // a whole wave: the lanes of a frame leave together
    const int64_t o0 = row_ptr[i], o1 = row_ptr[i + 1];
    const double* Kf = shared_k ? K : K + 9 * i;

    SrkResectPose cur;
    srk_resect_start_pose(R0 + 9 * i, T0 + 3 * i, cur);
    SrkResectSums cs;
    int64_t n;
    {
        double p[SRK_RESECT_PACK];
#pragma unroll
        for (int e = 0; e < SRK_RESECT_PACK; ++e) p[e] = pack[(int64_t)SRK_RESECT_PACK * i + e];
        n = rs_eval(o0, o1, point, uv, q, X, p, f0, kind, delta, lane, cs);
    }

    // Levenberg-Marquardt on the reprojection error: lane 0 holds the sums and solves, every lane carries the pose
    int hit_cap = 0, used = 0;
    if (n >= 3 && attempts > 0) {
        double c = SRK_RESECT_C0;
        hit_cap = 1;
        for (int32_t a = 0; a < attempts; ++a) {
            double d[6];
            int stepped = srk_resect_lm_step(cs, c, d);
#pragma unroll
            for (int e = 0; e < 6; ++e) d[e] = __shfl(d[e], 0, RS_L);
            stepped = __shfl(stepped, 0, RS_L);
            SrkResectPose cand = cur;
            SrkResectSums ns;
            srk_resect_sums_zero(ns);
            if (stepped) {
                double kf[9], p[SRK_RESECT_PACK];
#pragma unroll
                for (int e = 0; e < 9; ++e) kf[e] = Kf[e];
                srk_resect_move(cur, d, cand);
                srk_resect_pack_pose(cand, kf, p);
                rs_eval(o0, o1, point, uv, q, X, p, f0, kind, delta, lane, ns);
            }
            const double cur_E = __shfl(cs.E, 0, RS_L), cand_E = __shfl(ns.E, 0, RS_L);
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

    if (lane == 0) {
        double ql[6], inf[36];
        const uint32_t st = n >= 3 ? srk_resect_finish(cs, n, f0, hit_cap, used, ql, inf) : srk_resect_few(n, ql, inf);
#pragma unroll
        for (int e = 0; e < 9; ++e) Rout[9 * i + e] = cur.R[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) Tout[3 * i + e] = cur.T[e];
#pragma unroll
        for (int e = 0; e < 6; ++e) quality[6 * i + e] = ql[e];
#pragma unroll
        for (int e = 0; e < 36; ++e) info[36 * i + e] = inf[e];
        status[i] = st;
    }
    if (w_out) { // the robust weights at the result, 0 where q = 0
        double kf[9], p[SRK_RESECT_PACK];
#pragma unroll
        for (int e = 0; e < 9; ++e) kf[e] = Kf[e];
        srk_resect_pack_pose(cur, kf, p);
        for (int64_t o = o0 + lane; o < o1; o += RS_L) {
            const double qo = q ? q[o] : 1.0;
            double w = 0.0;
            if (qo > 0.0) {
                const double* x = X + 3 * (int64_t)point[o];
                const double xl[3] = { x[0], x[1], x[2] };
                const double2 m = reinterpret_cast<const double2*>(uv)[o];
                w = srk_resect_weight(p, xl, m.x, m.y, f0, qo, kind, delta);
            }
            w_out[o] = w;
        }
    }
}

void srk_launch_resect_frames(hipStream_t s, int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv, const double* q,
                              const double* X, const double* K, int shared_k, const double* R0, const double* T0, const double* pack, double f0,
                              int32_t attempts, double rel_change, int32_t loss_kind, double loss_delta, double* R, double* T, double* quality,
                              double* info, uint32_t* status, double* w_out)
{
    if (n_frames <= 0) return;
    const int32_t per = RS_BLOCK / RS_L;
    hipLaunchKernelGGL(k_resect_frames, dim3((unsigned)((n_frames + per - 1) / per)), dim3(RS_BLOCK), 0, s, n_frames, row_ptr, point, uv, q, X, K,
                       shared_k, R0, T0, pack, f0, attempts, rel_change, loss_kind, loss_delta, R, T, quality, info, status, w_out);
}
