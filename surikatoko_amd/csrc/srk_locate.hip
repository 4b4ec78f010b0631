// srk_locate.hip -- resection without a start pose (srk_locate_frames, srk_ba_locate), the device half.
//
// Hypothesise and verify: every hypothesis of a frame reads the same observations, so a wave is 64 hypotheses of one frame, one
// per lane, and the loop over the frame's observations has a wave-uniform index: an observation is fetched once per wave (a
// scalar load) and every lane projects it under its own pose.  Three kernels:
//   k_locate_gather  one wave per frame: the weighted observations (q > 0) compacted by the wave's ballot into a contiguous strip
//                    at row_ptr[i] + rank, landmark included, so that the sampler reads rank r directly and the scoring loop
//                    reads contiguous, aligned 64-byte records;
//   k_locate_score   one lane per (frame, hypothesis): the sample, P3P, the choice by the fourth point (srk_locate_math.hpp), then
//                    the MSAC score over the strip in ascending rank, one accumulator; the wave's best (score, h) by a fixed
//                    shuffle tree into the wave's slot, pose included.  The hypothesis lives in registers only: there is no
//                    hypothesis workspace, and the grid is frames x ceil(H / 64) waves, so one frame with many hypotheses
//                    spreads over several CUs;
//   k_locate_pick    one wave per frame: the slots in ascending wave order (an equal score stays with the smaller h), the outputs,
//                    and with inlier_out one pass over the frame's observations at the located pose.
// No LDS, no atomics, no workgroup barrier: a frame's bits depend on its own observations, the seed and the hypothesis count alone.
#include "srk_locate_dev.hpp"
#include "srk_locate_math.hpp"

#define LC_BLOCK 256
#define LC_L SRK_LOCATE_LANES
static_assert(LC_L == 64, "a hypothesis wave is the hardware's");

__global__ __launch_bounds__(LC_BLOCK) void k_locate_gather(int32_t n_frames, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ point,
                                                            const double* __restrict__ uv, const double* __restrict__ q,
                                                            const double* __restrict__ X, double* __restrict__ strip, int64_t* __restrict__ count)
{
    const int lane = threadIdx.x & (LC_L - 1);
    const int64_t i = (int64_t)blockIdx.x * (LC_BLOCK / LC_L) + (threadIdx.x / LC_L);
    if (i >= n_frames) return; // a whole wave: the lanes of a frame leave together
    const int64_t o0 = row_ptr[i], o1 = row_ptr[i + 1];
    int64_t base = 0;
    for (int64_t c0 = o0; c0 < o1; c0 += LC_L) {
        const int64_t o = c0 + lane;
        const bool w = o < o1 && (q == nullptr || q[o] > 0.0);
        const unsigned long long m = __ballot(w);
        if (w) { // the rank rule of the resection's walk: the weighted observations in ascending o
            const int64_t rank = base + __popcll(m & ((1ull << lane) - 1ull));
            const double* x = X + 3 * (int64_t)point[o];
            const double2 px = reinterpret_cast<const double2*>(uv)[o];
            double2* e = reinterpret_cast<double2*>(strip + SRK_LOCATE_STRIP * (o0 + rank)); // rank <= o - o0: inside the frame's rows
            e[0] = make_double2(x[0], x[1]);
            e[1] = make_double2(x[2], px.x);
            e[2] = make_double2(px.y, q ? q[o] : 1.0);
            e[3] = make_double2(0.0, 0.0);
        }
        base += __popcll(m);
    }
    if (lane == 0) count[i] = base;
}

__global__ __launch_bounds__(LC_BLOCK) void k_locate_score(int64_t n_waves, int32_t waves, int32_t hypotheses, uint64_t seed, double tau2, double f0,
                                                           const int64_t* __restrict__ row_ptr, const double* __restrict__ strip,
                                                           const int64_t* __restrict__ count, const double* __restrict__ K, int shared_k,
                                                           double* __restrict__ slots)
{
    const int lane = threadIdx.x & (LC_L - 1);
    // the wave's number through the scalar unit, so that everything derived from it (the frame, its rows) is known to be uniform
    const int64_t w = (int64_t)blockIdx.x * (LC_BLOCK / LC_L) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / LC_L));
    if (w >= n_waves) return;
    const int64_t i = w / waves;
    const int32_t h = (int32_t)(w % waves) * LC_L + lane;
    const int64_t n = count[i], o0 = row_ptr[i];
    double* __restrict__ slot = slots + SRK_LOCATE_SLOT * w;

    SrkLocateHyp hyp;
    hyp.valid = 0;
    if (n >= 4) {
        const double* Kf = shared_k ? K : K + 9 * i;
        double kf[9], ki[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) kf[e] = Kf[e];
        srk_locate_inverse3(kf, ki);
        // a lane past the last hypothesis works on a sample of its own and is dropped below: no divergence inside P3P
        int64_t r0, r1, r2, r3;
        srk_locate_sample(seed, (uint32_t)h, n, r0, r1, r2, r3);
        double X4[12], uv4[8];
        const double* e0 = strip + SRK_LOCATE_STRIP * (o0 + r0);
        const double* e1 = strip + SRK_LOCATE_STRIP * (o0 + r1);
        const double* e2 = strip + SRK_LOCATE_STRIP * (o0 + r2);
        const double* e3 = strip + SRK_LOCATE_STRIP * (o0 + r3);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            X4[a] = e0[a];
            X4[3 + a] = e1[a];
            X4[6 + a] = e2[a];
            X4[9 + a] = e3[a];
        }
        uv4[0] = e0[3], uv4[1] = e0[4], uv4[2] = e1[3], uv4[3] = e1[4], uv4[4] = e2[3], uv4[5] = e2[4], uv4[6] = e3[3], uv4[7] = e3[4];
        srk_locate_hypothesis(kf, ki, X4, uv4, f0, hyp);
        hyp.valid = hyp.valid && h < hypotheses;
    }

    double score = 0.0;
    int32_t inl = 0;
    if (__ballot(hyp.valid) != 0ull) { // uniform
        for (int64_t r = 0; r < n; ++r) { // ascending rank, one accumulator; the record's address is the same in every lane
            const double* e = strip + SRK_LOCATE_STRIP * (o0 + r);
            const double x[3] = { e[0], e[1], e[2] };
            int in;
            const double t = srk_locate_term(hyp.p, hyp.d, x, e[3], e[4], e[5], f0, tau2, in);
            score += t;
            inl += in;
        }
    }
    double bs = hyp.valid ? score : INFINITY;
    int32_t bh = h;
#pragma unroll
    for (int d = LC_L / 2; d >= 1; d >>= 1) { // the wave's best: the smallest score, an equal score to the smaller h
        const double os = __shfl_down(bs, d, LC_L);
        const int32_t oh = __shfl_down(bh, d, LC_L);
        if (os < bs || (os == bs && oh < bh)) {
            bs = os;
            bh = oh;
        }
    }
    bs = __shfl(bs, 0, LC_L);
    bh = __shfl(bh, 0, LC_L);
    const int poses = __popcll(__ballot(hyp.valid));
    if (bs < INFINITY) {
        if (h == bh) {
            slot[0] = score;
            slot[1] = (double)h;
            slot[2] = (double)inl;
            slot[3] = (double)poses;
            slot[4] = hyp.e4;
            slot[5] = 0.0;
#pragma unroll
            for (int e = 0; e < 9; ++e) slot[6 + e] = hyp.R[e];
#pragma unroll
            for (int e = 0; e < 3; ++e) slot[15 + e] = hyp.T[e];
            slot[18] = slot[19] = 0.0;
        }
    } else if (lane == 0) {
        slot[0] = INFINITY;
#pragma unroll
        for (int e = 1; e < SRK_LOCATE_SLOT; ++e) slot[e] = 0.0;
    }
}

__global__ __launch_bounds__(LC_BLOCK) void k_locate_pick(int32_t n_frames, int32_t waves, double tau2, double f0, const int64_t* __restrict__ row_ptr,
                                                          const int32_t* __restrict__ point, const double* __restrict__ uv,
                                                          const double* __restrict__ q, const double* __restrict__ X, const double* __restrict__ K,
                                                          int shared_k, const int64_t* __restrict__ count, const double* __restrict__ slots,
                                                          double* __restrict__ Rout, double* __restrict__ Tout, double* __restrict__ located,
                                                          uint32_t* __restrict__ status, uint8_t* __restrict__ inlier_out)
{
    const int lane = threadIdx.x & (LC_L - 1);
    const int64_t i = (int64_t)blockIdx.x * (LC_BLOCK / LC_L) + (threadIdx.x / LC_L);
    if (i >= n_frames) return;
    const int64_t o0 = row_ptr[i], o1 = row_ptr[i + 1], n = count[i];
    const double* fs = slots + SRK_LOCATE_SLOT * (i * waves);
    double best = INFINITY, poses = 0.0;
    int32_t bw = -1;
    for (int32_t w = 0; w < waves; ++w) { // ascending wave order = ascending h: an equal score stays with the smaller h
        const double s = fs[SRK_LOCATE_SLOT * w];
        poses += fs[SRK_LOCATE_SLOT * w + 3];
        if (s < best) {
            best = s;
            bw = w;
        }
    }
    double R[9] = { 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0 }, T[3] = { 0.0, 0.0, 0.0 };
    double l0 = NAN, l2 = 0.0, l3 = NAN, l5 = NAN;
    if (bw >= 0) {
        const double* s = fs + SRK_LOCATE_SLOT * bw;
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = s[6 + e];
#pragma unroll
        for (int e = 0; e < 3; ++e) T[e] = s[15 + e];
        l0 = sqrt(best / (double)n);
        l2 = s[2];
        l3 = s[1];
        l5 = sqrt(s[4]);
    }
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) Rout[9 * i + e] = R[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) Tout[3 * i + e] = T[e];
        double* l = located + 6 * i;
        l[0] = l0;
        l[1] = (double)n;
        l[2] = l2;
        l[3] = l3;
        l[4] = poses;
        l[5] = l5;
        status[i] = n < 4 ? 1u : (bw < 0 ? 2u : 0u); // SRK_LOCATE_FEW_POINTS, SRK_LOCATE_NO_MODEL
    }
    if (inlier_out) {
        const double* Kf = shared_k ? K : K + 9 * i;
        double kf[9], p[12], d[4];
#pragma unroll
        for (int e = 0; e < 9; ++e) kf[e] = Kf[e];
        srk_locate_pack(kf, R, T, p, d);
        for (int64_t o = o0 + lane; o < o1; o += LC_L) {
            const double qo = q ? q[o] : 1.0;
            int in = 0;
            if (bw >= 0 && qo > 0.0) {
                const double* x = X + 3 * (int64_t)point[o];
                const double xl[3] = { x[0], x[1], x[2] };
                const double2 m = reinterpret_cast<const double2*>(uv)[o];
                srk_locate_term(p, d, xl, m.x, m.y, qo, f0, tau2, in);
            }
            inlier_out[o] = (uint8_t)in;
        }
    }
}

void srk_launch_locate_gather(hipStream_t s, int32_t n_frames, const int64_t* row_ptr, const int32_t* point, const double* uv, const double* q,
                              const double* X, double* strip, int64_t* count)
{
    if (n_frames <= 0) return;
    const int32_t per = LC_BLOCK / LC_L;
    hipLaunchKernelGGL(k_locate_gather, dim3((unsigned)((n_frames + per - 1) / per)), dim3(LC_BLOCK), 0, s, n_frames, row_ptr, point, uv, q, X, strip,
                       count);
}

void srk_launch_locate_score(hipStream_t s, int32_t n_frames, int32_t hypotheses, uint64_t seed, double tau, double f0, const int64_t* row_ptr,
                             const double* strip, const int64_t* count, const double* K, int shared_k, double* slots)
{
    if (n_frames <= 0) return;
    const int32_t per = LC_BLOCK / LC_L, waves = (hypotheses + LC_L - 1) / LC_L;
    const int64_t n_waves = (int64_t)n_frames * waves;
    hipLaunchKernelGGL(k_locate_score, dim3((unsigned)((n_waves + per - 1) / per)), dim3(LC_BLOCK), 0, s, n_waves, waves, hypotheses, seed, tau * tau, f0,
                       row_ptr, strip, count, K, shared_k, slots);
}

void srk_launch_locate_pick(hipStream_t s, int32_t n_frames, int32_t hypotheses, double tau, double f0, const int64_t* row_ptr, const int32_t* point,
                            const double* uv, const double* q, const double* X, const double* K, int shared_k, const int64_t* count,
                            const double* slots, double* R, double* T, double* located, uint32_t* status, uint8_t* inlier_out)
{
    if (n_frames <= 0) return;
    const int32_t per = LC_BLOCK / LC_L, waves = (hypotheses + LC_L - 1) / LC_L;
    hipLaunchKernelGGL(k_locate_pick, dim3((unsigned)((n_frames + per - 1) / per)), dim3(LC_BLOCK), 0, s, n_frames, waves, tau * tau, f0, row_ptr, point, uv,
                       q, X, K, shared_k, count, slots, R, T, located, status, inlier_out);
}
