// srk_tri.hip -- batched landmark triangulation and refinement (srk_triangulate_tracks, srk_ba_triangulate),
// the device half.
//
// The linear stage is the reference's system Triangulate3DPointByLeastSquares (obs-geom.cpp:679-727): two rows per observation,
// x p2 - f0 p0 and y p2 - f0 p1 with P = K [R | T].  It is solved by an orthogonal factorisation that streams over the rows: a
// lane keeps the 3 x 3 triangular factor and Q^T b in nine registers and folds every new row in with three Givens rotations;
// the SRK_TRI_GROUP lanes of a track then merge their factors pairwise (TSQR) with cross-lane moves, in a fixed tree.  A^T A is
// never formed.  No atomics, no LDS, no workgroup barrier: a track's bits depend on its own observations alone.
//
// The weighted observations (q > 0) of a track are dealt to its lanes by their rank among the weighted ones, so an observation
// with q = 0 leaves the very computation of the track without it.
#include "srk_tri_dev.hpp"
#include "srk_tri_math.hpp"

#define TRI_BLOCK 256
#define TRI_G SRK_TRI_GROUP
static_assert(TRI_G == 8, "a group's ballot is one byte of the wave's");

__global__ __launch_bounds__(256) void k_tri_pack(int32_t n_frames, const double* __restrict__ R, const double* __restrict__ T,
                                                  const double* __restrict__ K, int shared_k, double* __restrict__ pack)
{
    const int32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_frames) return;
    double p[SRK_TRI_PACK];
    srk_tri_pack_frame(R + 9 * (int64_t)j, T + 3 * (int64_t)j, shared_k ? K : K + 9 * (int64_t)j, p);
#pragma unroll
    for (int e = 0; e < SRK_TRI_PACK; ++e) pack[(int64_t)SRK_TRI_PACK * j + e] = p[e];
}

void srk_launch_tri_pack(hipStream_t s, int32_t n_frames, const double* cam_R, const double* cam_T, const double* K, int shared_k, double* pack)
{
    if (n_frames <= 0) return;
    hipLaunchKernelGGL(k_tri_pack, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, s, n_frames, cam_R, cam_T, K, shared_k, pack);
}

// Lane `s` of a group visits its share of the weighted observations of [o0, o1), in ascending order: the observation of rank r
// among the weighted ones belongs to lane r % 8.  The observations are looked at eight at a time; the group's byte of the wave's
// ballot says which of the eight are weighted.  body(o) holds no cross-lane move (the lanes of a group diverge around it).
// Returns the number of weighted observations, the same in every lane of the group.
template <class Body>
__device__ __forceinline__ int64_t tri_walk(int64_t o0, int64_t o1, const double* __restrict__ q, int s, int shift, Body&& body)
{
    int64_t base = 0;
    for (int64_t c0 = o0; c0 < o1; c0 += TRI_G) {
        const int64_t o = c0 + s;
        const bool w = o < o1 && (q == nullptr || q[o] > 0.0);
        const unsigned m8 = (unsigned)(__ballot(w) >> shift) & 0xffu;
        const int cnt = __popc(m8);
        const int k = (s - (int)(base & 7)) & 7; // my place among this chunk's weighted observations
        if (k < cnt) {
            unsigned t = m8;
            for (int i = 0; i < k; ++i) t &= t - 1;
            body(c0 + (__ffs(t) - 1));
        }
        base += cnt;
    }
    return base;
}

__device__ __forceinline__ void tri_merge_down(SrkTriFactor& f)
{
#pragma unroll
    for (int d = 1; d < TRI_G; d <<= 1) {
        SrkTriFactor g;
        g.r00 = __shfl_down(f.r00, d, TRI_G);
        g.r01 = __shfl_down(f.r01, d, TRI_G);
        g.r02 = __shfl_down(f.r02, d, TRI_G);
        g.r11 = __shfl_down(f.r11, d, TRI_G);
        g.r12 = __shfl_down(f.r12, d, TRI_G);
        g.r22 = __shfl_down(f.r22, d, TRI_G);
        g.z0 = __shfl_down(f.z0, d, TRI_G);
        g.z1 = __shfl_down(f.z1, d, TRI_G);
        g.z2 = __shfl_down(f.z2, d, TRI_G);
        srk_tri_merge(f, g); // lane 0 ends with ((0 1)(2 3))((4 5)(6 7)); what the other lanes hold is not used
    }
}

template <bool ANGLE>
__device__ __forceinline__ void tri_sums_down(SrkTriSums& a)
{
#pragma unroll
    for (int d = 1; d < TRI_G; d <<= 1) {
        SrkTriSums b;
        b.E = __shfl_down(a.E, d, TRI_G);
        b.h00 = __shfl_down(a.h00, d, TRI_G);
        b.h01 = __shfl_down(a.h01, d, TRI_G);
        b.h02 = __shfl_down(a.h02, d, TRI_G);
        b.h11 = __shfl_down(a.h11, d, TRI_G);
        b.h12 = __shfl_down(a.h12, d, TRI_G);
        b.h22 = __shfl_down(a.h22, d, TRI_G);
        b.g0 = __shfl_down(a.g0, d, TRI_G);
        b.g1 = __shfl_down(a.g1, d, TRI_G);
        b.g2 = __shfl_down(a.g2, d, TRI_G);
        b.min_depth = __shfl_down(a.min_depth, d, TRI_G);
        b.max_angle = ANGLE ? __shfl_down(a.max_angle, d, TRI_G) : 0.0;
        srk_tri_sums_add(a, b);
    }
}

__device__ __forceinline__ void tri_bcast3(double v[3])
{
    v[0] = __shfl(v[0], 0, TRI_G);
    v[1] = __shfl(v[1], 0, TRI_G);
    v[2] = __shfl(v[2], 0, TRI_G);
}

// the sums of the track at X into lane 0 of the group
template <bool ANGLE>
__device__ __forceinline__ void tri_eval(int64_t o0, int64_t o1, const int32_t* __restrict__ frame, const double* __restrict__ uv,
                                         const double* __restrict__ q, const double* __restrict__ pack, double f0, int s, int shift,
                                         const double X[3], const double ray0[3], SrkTriSums& sums)
{
    srk_tri_sums_zero(sums);
    tri_walk(o0, o1, q, s, shift, [&](int64_t o) {
        const double* p = pack + (int64_t)SRK_TRI_PACK * frame[o];
        const double2 m = reinterpret_cast<const double2*>(uv)[o];
        srk_tri_eval_obs(sums, p, m.x, m.y, f0, q ? q[o] : 1.0, X);
        if constexpr (ANGLE) {
            double ray[3];
            srk_tri_ray(p, m.x, m.y, f0, ray);
            sums.max_angle = fmax(sums.max_angle, srk_tri_angle(ray0, ray));
        }
    });
    tri_sums_down<ANGLE>(sums);
}

__global__ __launch_bounds__(TRI_BLOCK) void k_tri_tracks(int64_t n_tracks, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ frame,
                                                          const double* __restrict__ uv, const double* __restrict__ q,
                                                          const double* __restrict__ pack, double f0, int32_t refine_attempts,
                                                          double refine_rel_change, double min_parallax_deg, double* __restrict__ Xout,
                                                          double* __restrict__ quality, uint32_t* __restrict__ status)
{
    const int s = threadIdx.x & (TRI_G - 1), shift = threadIdx.x & 63 & ~(TRI_G - 1);
    const int64_t t = (int64_t)blockIdx.x * (TRI_BLOCK / TRI_G) + (threadIdx.x / TRI_G);
    if (t >= n_tracks) return; // a whole group: the lanes of a track leave together
    const int64_t o0 = row_ptr[t], o1 = row_ptr[t + 1];

    // the linear stage
    SrkTriFactor f;
    srk_tri_factor_zero(f);
    double ray0[3] = { 0, 0, 0 };
    bool first = true;
    const int64_t nw = tri_walk(o0, o1, q, s, shift, [&](int64_t o) {
        const double* p = pack + (int64_t)SRK_TRI_PACK * frame[o];
        const double2 m = reinterpret_cast<const double2*>(uv)[o];
        srk_tri_fold_obs(f, p, m.x, m.y, f0, q ? sqrt(q[o]) : 1.0);
        if (first) { // lane 0's first observation is the first weighted one
            srk_tri_ray(p, m.x, m.y, f0, ray0);
            first = false;
        }
    });
    if (nw < 2) {
        if (s == 0) {
            const double nan = __builtin_nan("");
            Xout[3 * t] = Xout[3 * t + 1] = Xout[3 * t + 2] = nan;
            quality[4 * t] = nan;
            quality[4 * t + 1] = 0.0;
            quality[4 * t + 2] = nan;
            quality[4 * t + 3] = (double)nw;
            status[t] = 1u; // SRK_TRI_FEW_VIEWS
        }
        return;
    }
    tri_merge_down(f);
    double X[3];
    int solved = srk_tri_solve(f, X);
    tri_bcast3(X);
    tri_bcast3(ray0);
    solved = __shfl(solved, 0, TRI_G);

    SrkTriSums cur;
    tri_eval<true>(o0, o1, frame, uv, q, pack, f0, s, shift, X, ray0, cur);

    // the refinement: Levenberg-Marquardt on the reprojection error, lane 0 decides
    int hit_cap = 0;
    if (refine_attempts > 0 && solved) {
        double c = 1e-4;
        hit_cap = 1;
        for (int32_t a = 0; a < refine_attempts; ++a) {
            double d[3] = { 0, 0, 0 }, Xn[3];
            int stepped = srk_tri_lm_step(cur, c, d);
            Xn[0] = X[0] + d[0];
            Xn[1] = X[1] + d[1];
            Xn[2] = X[2] + d[2];
            tri_bcast3(Xn);
            stepped = __shfl(stepped, 0, TRI_G);
            SrkTriSums cand;
            srk_tri_sums_zero(cand);
            if (stepped) tri_eval<false>(o0, o1, frame, uv, q, pack, f0, s, shift, Xn, ray0, cand);
            int stop = srk_tri_lm_judge(cur, cand, stepped, X, Xn, c, refine_rel_change);
            stop = __shfl(stop, 0, TRI_G);
            if (stop) {
                hit_cap = 0;
                break;
            }
        }
    }
    if (s == 0) {
        double ql[4];
        const uint32_t st = srk_tri_finish(f, cur, solved, nw, min_parallax_deg, hit_cap, ql);
        Xout[3 * t] = X[0];
        Xout[3 * t + 1] = X[1];
        Xout[3 * t + 2] = X[2];
        quality[4 * t] = ql[0];
        quality[4 * t + 1] = ql[1];
        quality[4 * t + 2] = ql[2];
        quality[4 * t + 3] = ql[3];
        status[t] = st;
    }
}

void srk_launch_tri_tracks(hipStream_t s, int64_t n_tracks, const int64_t* row_ptr, const int32_t* frame, const double* uv, const double* q,
                           const double* pack, double f0, int32_t refine_attempts, double refine_rel_change, double min_parallax_deg,
                           double* X, double* quality, uint32_t* status)
{
    if (n_tracks <= 0) return;
    const int64_t per = TRI_BLOCK / TRI_G;
    hipLaunchKernelGGL(k_tri_tracks, dim3((unsigned)((n_tracks + per - 1) / per)), dim3(TRI_BLOCK), 0, s, n_tracks, row_ptr, frame, uv, q, pack, f0,
                       refine_attempts, refine_rel_change, min_parallax_deg, X, quality, status);
}
