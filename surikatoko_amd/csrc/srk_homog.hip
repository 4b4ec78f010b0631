// srk_homog.hip -- the two-view homography (srk_relate_homography), the device half.
//
// Hypothesise and verify with a four-point sample, in the shape of srk_align.hip: every hypothesis of a pair reads the same
// matches, so a wave is 64 hypotheses of one pair, one per lane, and the loop over the pair's matches has a wave-uniform index: a
// record is fetched once per wave (a scalar load) and every lane transfers it under its own homography.
//   k_homog_gather  one wave per pair: the weighted matches (q > 0) compacted by the wave's ballot into a contiguous strip of
//                   64-byte records {uv_a, uv_b, q, 0, 0, 0} at row_ptr[i] + rank;
//   k_homog_score   one lane per (pair, hypothesis): the sample, the model through the projective basis (srk_homog_math.hpp),
//                   then the MSAC score over the strip in ascending rank, one accumulator; the wave's best (score, h) by a fixed
//                   shuffle tree into the wave's slot, model included.  The grid is pairs x ceil(H / 64) waves;
//   k_homog_pick    one wave per pair: the slots in ascending wave order, then up to refine_rounds Gauss-Newton rounds with the
//                   whole wave (the inliers' 36 + 8 sums lane-strided and merged in a fixed tree, the 8 x 8 Cholesky step computed
//                   redundantly by every lane, a re-score in the score kernel's order, accepted only when strictly smaller), the
//                   decomposition of the returned model, the outputs, and with inlier_out one pass at the final model.
// No LDS, no atomics, no workgroup barrier: a pair's bits depend on its own matches, the seed and the options alone.
#include "srk_homog_dev.hpp"
#include "srk_homog_math.hpp"

#define HG_BLOCK 256
#define HG_L SRK_HOMOG_LANES
static_assert(HG_L == 64, "a hypothesis wave is the hardware's");

__global__ __launch_bounds__(HG_BLOCK) void k_homog_gather(int32_t n_pairs, const int64_t* __restrict__ row_ptr, const double* __restrict__ uv_a,
                                                           const double* __restrict__ uv_b, const double* __restrict__ q, double* __restrict__ strip,
                                                           int64_t* __restrict__ count)
{
    const int lane = threadIdx.x & (HG_L - 1);
    const int64_t i = (int64_t)blockIdx.x * (HG_BLOCK / HG_L) + (threadIdx.x / HG_L);
    if (i >= n_pairs) return; // a whole wave: the lanes of a pair leave together
    const int64_t o0 = row_ptr[i], o1 = row_ptr[i + 1];
    int64_t base = 0;
    for (int64_t c0 = o0; c0 < o1; c0 += HG_L) {
        const int64_t o = c0 + lane;
        const bool w = o < o1 && (q == nullptr || q[o] > 0.0);
        const unsigned long long m = __ballot(w);
        if (w) { // the rank rule: the weighted matches in ascending o
            const int64_t rank = base + __popcll(m & ((1ull << lane) - 1ull));
            double2* e = reinterpret_cast<double2*>(strip + SRK_HOMOG_STRIP * (o0 + rank)); // rank <= o - o0: inside the pair's rows
            e[0] = make_double2(uv_a[2 * o], uv_a[2 * o + 1]);
            e[1] = make_double2(uv_b[2 * o], uv_b[2 * o + 1]);
            e[2] = make_double2(q ? q[o] : 1.0, 0.0);
            e[3] = make_double2(0.0, 0.0);
        }
        base += __popcll(m);
    }
    if (lane == 0) count[i] = base;
}

__global__ __launch_bounds__(HG_BLOCK) void k_homog_score(int64_t n_waves, int32_t waves, int32_t hypotheses, uint64_t seed, double tau2, double f0,
                                                          const int64_t* __restrict__ row_ptr, const double* __restrict__ strip,
                                                          const int64_t* __restrict__ count, double* __restrict__ slots)
{
    const int lane = threadIdx.x & (HG_L - 1);
    // the wave's number through the scalar unit, so that everything derived from it (the pair, its rows) is known to be uniform
    const int64_t w = (int64_t)blockIdx.x * (HG_BLOCK / HG_L) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / HG_L));
    if (w >= n_waves) return;
    const int64_t i = w / waves;
    const int32_t h = (int32_t)(w % waves) * HG_L + lane;
    const int64_t n = count[i], o0 = row_ptr[i];
    double* __restrict__ slot = slots + SRK_HOMOG_SLOT * w;

    SrkHomogModel m;
    int valid = 0;
    if (n >= 4) {
        // a lane past the last hypothesis works on a sample of its own and is dropped below
        int64_t r0, r1, r2, r3;
        srk_homog_sample(seed, (uint32_t)h, n, r0, r1, r2, r3); // every rank is below n: inside the pair's strip
        const double* e0 = strip + SRK_HOMOG_STRIP * (o0 + r0);
        const double* e1 = strip + SRK_HOMOG_STRIP * (o0 + r1);
        const double* e2 = strip + SRK_HOMOG_STRIP * (o0 + r2);
        const double* e3 = strip + SRK_HOMOG_STRIP * (o0 + r3);
        double pa[12], pb[12];
        pa[0] = e0[0], pa[1] = e0[1], pa[3] = e1[0], pa[4] = e1[1], pa[6] = e2[0], pa[7] = e2[1], pa[9] = e3[0], pa[10] = e3[1];
        pb[0] = e0[2], pb[1] = e0[3], pb[3] = e1[2], pb[4] = e1[3], pb[6] = e2[2], pb[7] = e2[3], pb[9] = e3[2], pb[10] = e3[3];
        pa[2] = pa[5] = pa[8] = pa[11] = pb[2] = pb[5] = pb[8] = pb[11] = f0;
        valid = srk_homog_hypothesis(pa, pb, m) && h < hypotheses;
    } else
        srk_homog_identity(m);

    double score = 0.0, ss = 0.0;
    int32_t inl = 0;
    if (__ballot(valid) != 0ull) { // uniform
        for (int64_t r = 0; r < n; ++r) { // ascending rank, one accumulator; the record's address is the same in every lane
            const double* e = strip + SRK_HOMOG_STRIP * (o0 + r);
            const double rec[5] = { e[0], e[1], e[2], e[3], e[4] };
            int in;
            double s2;
            score += srk_homog_term(m, rec, f0, tau2, in, s2);
            inl += in;
            ss += in ? s2 : 0.0;
        }
    }
    double bs = valid ? score : INFINITY;
    int32_t bh = h;
#pragma unroll
    for (int d = HG_L / 2; d >= 1; d >>= 1) { // the wave's best: the smallest score, an equal score to the smaller h
        const double os = __shfl_down(bs, d, HG_L);
        const int32_t oh = __shfl_down(bh, d, HG_L);
        if (os < bs || (os == bs && oh < bh)) {
            bs = os;
            bh = oh;
        }
    }
    bs = __shfl(bs, 0, HG_L);
    bh = __shfl(bh, 0, HG_L);
    const int models = __popcll(__ballot(valid));
    if (bs < INFINITY) {
        if (h == bh) {
            slot[0] = score;
            slot[1] = (double)h;
            slot[2] = (double)inl;
            slot[3] = (double)models;
            slot[4] = ss;
#pragma unroll
            for (int e = 0; e < 9; ++e) slot[5 + e] = m.G[e];
            slot[14] = slot[15] = 0.0;
        }
    } else if (lane == 0) {
        slot[0] = INFINITY;
#pragma unroll
        for (int e = 1; e < SRK_HOMOG_SLOT; ++e) slot[e] = 0.0;
    }
}

// the lanes' sums merged in the wave's fixed tree, the total to every lane
template <int W> __device__ __forceinline__ void hg_merge(double* acc)
{
#pragma unroll
    for (int d = HG_L / 2; d >= 1; d >>= 1) {
#pragma unroll
        for (int e = 0; e < W; ++e) acc[e] += __shfl_down(acc[e], d, HG_L);
    }
#pragma unroll
    for (int e = 0; e < W; ++e) acc[e] = __shfl(acc[e], 0, HG_L);
}

__device__ __forceinline__ void hg_record(const double* e, double* rec)
{
    rec[0] = e[0], rec[1] = e[1], rec[2] = e[2], rec[3] = e[3], rec[4] = e[4];
}

__global__ __launch_bounds__(HG_BLOCK) void k_homog_pick(int32_t n_pairs, int32_t waves, double tau2, double f0, int32_t refine_rounds,
                                                         const int64_t* __restrict__ row_ptr, const double* __restrict__ uv_a,
                                                         const double* __restrict__ uv_b, const double* __restrict__ q, const double* __restrict__ strip,
                                                         const int64_t* __restrict__ count, const double* __restrict__ K_a, const double* __restrict__ K_b,
                                                         int shared_k, const double* __restrict__ slots, double* __restrict__ Gout, double* __restrict__ Hout,
                                                         int32_t* __restrict__ n_poses, double* __restrict__ Rout, double* __restrict__ Tout,
                                                         double* __restrict__ Nout, int32_t* __restrict__ front, double* __restrict__ homog,
                                                         uint32_t* __restrict__ status, uint8_t* __restrict__ inlier_out)
{
    const int lane = threadIdx.x & (HG_L - 1);
    const int64_t i = (int64_t)blockIdx.x * (HG_BLOCK / HG_L) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / HG_L));
    if (i >= n_pairs) return;
    const int64_t o0 = row_ptr[i], o1 = row_ptr[i + 1], n = count[i];
    const double* fs = slots + SRK_HOMOG_SLOT * (i * waves);
    const double* rows = strip + SRK_HOMOG_STRIP * o0;
    double best = INFINITY, models = 0.0;
    int32_t bw = -1;
    for (int32_t w = 0; w < waves; ++w) { // ascending wave order = ascending h: an equal score stays with the smaller h
        const double s = fs[SRK_HOMOG_SLOT * w];
        models += fs[SRK_HOMOG_SLOT * w + 3];
        if (s < best) {
            best = s;
            bw = w;
        }
    }
    SrkHomogModel cur;
    srk_homog_identity(cur);
    // "not a number" for the figures of a pair without a model, formed at run time: written as a constant it can end up as a 64-bit
    // scalar literal, which the gfx950 assembler encodes as zero
    const double none = sqrt(-1.0 - (double)n);
    double inl = 0.0, ss = 0.0, hwin = 0.0, gap = 0.0;
    int32_t rounds = 0, poses = 0, fr[2] = { 0, 0 };
    double H[9], R[18], T[6], N[6];
#pragma unroll
    for (int e = 0; e < 9; ++e) H[e] = cur.G[e];
#pragma unroll
    for (int e = 0; e < 18; ++e) R[e] = 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) T[e] = N[e] = 0.0;
    if (bw >= 0) {
        const double* s = fs + SRK_HOMOG_SLOT * bw;
        hwin = s[1];
        inl = s[2];
        ss = s[4];
#pragma unroll
        for (int e = 0; e < 9; ++e) cur.G[e] = s[5 + e];
        srk_homog_complete(cur);
        for (int32_t round = 0; round < refine_rounds; ++round) { // every condition below is the same in every lane
            double acc[SRK_HOMOG_ACC];
#pragma unroll
            for (int e = 0; e < SRK_HOMOG_ACC; ++e) acc[e] = 0.0;
            int32_t cnt = 0;
            for (int64_t k = lane; k < n; k += HG_L) { // lane l takes ranks l, l + 64, ..
                double rec[5];
                hg_record(rows + SRK_HOMOG_STRIP * k, rec);
                int in;
                double s2;
                srk_homog_term(cur, rec, f0, tau2, in, s2);
                if (in) {
                    srk_homog_accumulate(acc, cur, rec, f0);
                    ++cnt;
                }
            }
#pragma unroll
            for (int d = HG_L / 2; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, HG_L);
            if (cnt < 4) break;
            hg_merge<SRK_HOMOG_ACC>(acc);
            SrkHomogModel cand;
            if (!srk_homog_step(acc, cur, cand)) break;
            double sc = 0.0, css = 0.0;
            int32_t cinl = 0;
            for (int64_t r = 0; r < n; ++r) { // the score kernel's order: ascending rank, one accumulator, in every lane alike
                double rec[5];
                hg_record(rows + SRK_HOMOG_STRIP * r, rec);
                int in;
                double s2;
                sc += srk_homog_term(cand, rec, f0, tau2, in, s2);
                cinl += in;
                css += in ? s2 : 0.0;
            }
            if (!(sc < best)) break; // only a strictly smaller score is accepted
            best = sc;
            inl = (double)cinl;
            ss = css;
            cur = cand;
            ++rounds;
        }
        // the decomposition of the returned model: the sign sum, the planes, the inliers ahead of each normal
        const double* ka = K_a + (shared_k ? 0 : 9 * i);
        const double* kb = K_b + (shared_k ? 0 : 9 * i);
        double Ka[9], Kb[9], Kai[9], Kbi[9], GK[9], Hraw[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) Ka[e] = ka[e], Kb[e] = kb[e];
        srk_homog_inv3(Ka, Kai);
        srk_homog_inv3(Kb, Kbi);
        srk_homog_mul3(cur.G, Ka, GK);
        srk_homog_mul3(Kbi, GK, Hraw);
        double sum[1] = { 0.0 };
        for (int64_t k = lane; k < n; k += HG_L) {
            double rec[5], xa[3];
            hg_record(rows + SRK_HOMOG_STRIP * k, rec);
            int in;
            double s2;
            srk_homog_term(cur, rec, f0, tau2, in, s2);
            if (in) sum[0] += srk_homog_sign_term(Kai, Kbi, Hraw, rec, f0, xa);
        }
        hg_merge<1>(sum);
        SrkHomogPlanes P;
        srk_homog_planes(Hraw, sum[0], P);
        int32_t a0 = 0, a1 = 0;
        for (int64_t k = lane; k < n; k += HG_L) {
            double rec[5], xa[3];
            hg_record(rows + SRK_HOMOG_STRIP * k, rec);
            int in;
            double s2;
            srk_homog_term(cur, rec, f0, tau2, in, s2);
            if (in) {
                srk_homog_sign_term(Kai, Kbi, Hraw, rec, f0, xa);
                a0 += srk_align_dot(P.N[0], xa) > 0.0;
                a1 += srk_align_dot(P.N[1], xa) > 0.0;
            }
        }
#pragma unroll
        for (int d = HG_L / 2; d >= 1; d >>= 1) {
            a0 += __shfl_xor(a0, d, HG_L);
            a1 += __shfl_xor(a1, d, HG_L);
        }
        const int64_t ahead[2] = { a0, a1 };
        srk_homog_finish(P, ahead, (int64_t)inl, R, T, N, fr);
#pragma unroll
        for (int e = 0; e < 9; ++e) H[e] = P.H[e];
        poses = P.n_poses;
        gap = P.gap;
    }
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) Gout[9 * i + e] = cur.G[e], Hout[9 * i + e] = H[e];
#pragma unroll
        for (int e = 0; e < 18; ++e) Rout[18 * i + e] = R[e];
#pragma unroll
        for (int e = 0; e < 6; ++e) Tout[6 * i + e] = T[e], Nout[6 * i + e] = N[e];
        n_poses[i] = poses;
        front[2 * i] = fr[0];
        front[2 * i + 1] = fr[1];
        double* l = homog + 8 * i;
        l[0] = bw >= 0 ? sqrt(best / (double)n) : none;
        l[1] = (double)n;
        l[2] = inl;
        l[3] = bw >= 0 ? hwin : none;
        l[4] = models;
        l[5] = (double)rounds;
        l[6] = bw >= 0 ? gap : none;
        l[7] = bw >= 0 ? (inl > 0.0 ? sqrt(ss / inl) : 0.0) : none; // a winner without inliers: nothing to average
        status[i] = n < 4 ? 1u : (bw < 0 ? 2u : 0u); // SRK_HOMOGRAPHY_FEW_POINTS, SRK_HOMOGRAPHY_NO_MODEL
    }
    if (inlier_out) {
        for (int64_t o = o0 + lane; o < o1; o += HG_L) {
            const double qo = q ? q[o] : 1.0;
            int in = 0;
            if (bw >= 0 && qo > 0.0) {
                const double rec[5] = { uv_a[2 * o], uv_a[2 * o + 1], uv_b[2 * o], uv_b[2 * o + 1], qo };
                double s2;
                srk_homog_term(cur, rec, f0, tau2, in, s2);
            }
            inlier_out[o] = (uint8_t)in;
        }
    }
}

void srk_launch_homog_gather(hipStream_t s, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                             double* strip, int64_t* count)
{
    if (n_pairs <= 0) return;
    const int32_t per = HG_BLOCK / HG_L;
    hipLaunchKernelGGL(k_homog_gather, dim3((unsigned)((n_pairs + per - 1) / per)), dim3(HG_BLOCK), 0, s, n_pairs, row_ptr, uv_a, uv_b, q, strip, count);
}

void srk_launch_homog_score(hipStream_t s, int32_t n_pairs, int32_t hypotheses, uint64_t seed, double tau, double f0, const int64_t* row_ptr,
                            const double* strip, const int64_t* count, double* slots)
{
    if (n_pairs <= 0) return;
    const int32_t per = HG_BLOCK / HG_L, waves = (hypotheses + HG_L - 1) / HG_L;
    const int64_t n_waves = (int64_t)n_pairs * waves;
    hipLaunchKernelGGL(k_homog_score, dim3((unsigned)((n_waves + per - 1) / per)), dim3(HG_BLOCK), 0, s, n_waves, waves, hypotheses, seed, tau * tau, f0,
                       row_ptr, strip, count, slots);
}

void srk_launch_homog_pick(hipStream_t s, int32_t n_pairs, int32_t hypotheses, double tau, double f0, int32_t refine_rounds, const int64_t* row_ptr,
                           const double* uv_a, const double* uv_b, const double* q, const double* strip, const int64_t* count, const double* K_a,
                           const double* K_b, int shared_k, const double* slots, double* G, double* H, int32_t* n_poses, double* R, double* T, double* N,
                           int32_t* front, double* homog, uint32_t* status, uint8_t* inlier_out)
{
    if (n_pairs <= 0) return;
    const int32_t per = HG_BLOCK / HG_L, waves = (hypotheses + HG_L - 1) / HG_L;
    hipLaunchKernelGGL(k_homog_pick, dim3((unsigned)((n_pairs + per - 1) / per)), dim3(HG_BLOCK), 0, s, n_pairs, waves, tau * tau, f0, refine_rounds,
                       row_ptr, uv_a, uv_b, q, strip, count, K_a, K_b, shared_k, slots, G, H, n_poses, R, T, N, front, homog, status, inlier_out);
}
