// srk_fund.hip -- the two-view fundamental matrix (srk_relate_uncalibrated), the device half.
//
// Hypothesise and verify with a seven-point sample and an eighth match that chooses among the cubic's roots, in the shape of
// srk_relate.hip and srk_homog.hip: every hypothesis of a pair reads the same matches, so a wave of the score is 64 hypotheses of
// one pair, one per lane, and the loop over the pair's matches has a wave-uniform index.
//   k_fund_gather  one wave per pair: the weighted matches (q > 0) compacted by the wave's ballot into a contiguous strip of
//                  64-byte records {uv_a, uv_b, q, 0, 0, 0} at row_ptr[i] + rank;
//   k_fund_solve   one lane per (pair, hypothesis): the sample, the 7 x 9 null space, the cubic and its real roots, the choice by
//                  the eighth match (srk_fund_math.hpp); one record per hypothesis: F, the eighth-match error, the roots, valid;
//   k_fund_score   one lane per (pair, hypothesis), a wave = 64 hypotheses of one pair: the MSAC score over the strip in ascending
//                  rank, one accumulator; the wave's best (score, h) by a fixed shuffle tree into the wave's slot;
//   k_fund_pick    one wave per pair: the slots in ascending wave order, the winner into F = U diag(1, sigma, 0) V^T, then up to
//                  refine_rounds Levenberg-Marquardt attempts with the whole wave (the inliers' 28 + 7 sums lane-strided and merged
//                  in a fixed tree, the 7 x 7 Cholesky step computed redundantly by every lane, a re-score in the score kernel's
//                  order, accepted only when strictly smaller), the outputs, and with inlier_out one pass at the final model.
// No LDS, no atomics, no workgroup barrier: a pair's bits depend on its own matches, the seed and the options alone.
#include "srk_fund_dev.hpp"
#include "srk_fund_math.hpp"

#define FD_BLOCK 256
#define FD_L SRK_FUND_LANES
static_assert(FD_L == 64, "a hypothesis wave is the hardware's");

__global__ __launch_bounds__(FD_BLOCK) void k_fund_gather(int32_t n_pairs, const int64_t* __restrict__ row_ptr, const double* __restrict__ uv_a,
                                                          const double* __restrict__ uv_b, const double* __restrict__ q, double* __restrict__ strip,
                                                          int64_t* __restrict__ count)
{
    const int lane = threadIdx.x & (FD_L - 1);
    const int64_t i = (int64_t)blockIdx.x * (FD_BLOCK / FD_L) + (threadIdx.x / FD_L);
    if (i >= n_pairs) return; // a whole wave: the lanes of a pair leave together
    const int64_t o0 = row_ptr[i], o1 = row_ptr[i + 1];
    int64_t base = 0;
    for (int64_t c0 = o0; c0 < o1; c0 += FD_L) {
        const int64_t o = c0 + lane;
        const bool w = o < o1 && (q == nullptr || q[o] > 0.0);
        const unsigned long long m = __ballot(w);
        if (w) { // the rank rule: the weighted matches in ascending o
            const int64_t rank = base + __popcll(m & ((1ull << lane) - 1ull));
            double2* e = reinterpret_cast<double2*>(strip + SRK_FUND_STRIP * (o0 + rank)); // rank <= o - o0: inside the pair's rows
            e[0] = make_double2(uv_a[2 * o], uv_a[2 * o + 1]);
            e[1] = make_double2(uv_b[2 * o], uv_b[2 * o + 1]);
            e[2] = make_double2(q ? q[o] : 1.0, 0.0);
            e[3] = make_double2(0.0, 0.0);
        }
        base += __popcll(m);
    }
    if (lane == 0) count[i] = base;
}

__global__ __launch_bounds__(FD_BLOCK) void k_fund_solve(int64_t n_hyp, int32_t hypotheses, uint64_t seed, double f0,
                                                         const int64_t* __restrict__ row_ptr, const double* __restrict__ strip,
                                                         const int64_t* __restrict__ count, double* __restrict__ hyp)
{
    const int64_t t = (int64_t)blockIdx.x * FD_BLOCK + threadIdx.x;
    if (t >= n_hyp) return; // no lane of this kernel talks to another
    const int64_t i = t / hypotheses;
    const int32_t h = (int32_t)(t % hypotheses);
    const int64_t n = count[i], o0 = row_ptr[i];
    double F[9], err8 = 0.0;
    int roots = 0, valid = 0;
#pragma unroll
    for (int e = 0; e < 9; ++e) F[e] = 0.0;
    if (n >= 8) {
        int64_t r[8];
        srk_fund_sample(seed, (uint32_t)h, n, r); // every rank is below n: inside the pair's strip
        double pa[21], pb[21];
        const double if0 = 1.0 / f0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const double* e = strip + SRK_FUND_STRIP * (o0 + r[k]);
            pa[3 * k] = e[0] * if0, pa[3 * k + 1] = e[1] * if0, pa[3 * k + 2] = 1.0;
            pb[3 * k] = e[2] * if0, pb[3 * k + 1] = e[3] * if0, pb[3 * k + 2] = 1.0;
        }
        const double* e = strip + SRK_FUND_STRIP * (o0 + r[7]);
        const double e8[4] = { e[0], e[1], e[2], e[3] };
        valid = srk_fund_hypothesis(pa, pb, e8, f0, F, err8, roots);
    }
    double2* rec = reinterpret_cast<double2*>(hyp + SRK_FUND_HYP * t); // 96 bytes a record: aligned to 16
    rec[0] = make_double2(F[0], F[1]);
    rec[1] = make_double2(F[2], F[3]);
    rec[2] = make_double2(F[4], F[5]);
    rec[3] = make_double2(F[6], F[7]);
    rec[4] = make_double2(F[8], err8);
    rec[5] = make_double2((double)roots, (double)valid);
}

__global__ __launch_bounds__(FD_BLOCK) void k_fund_score(int64_t n_waves, int32_t waves, int32_t hypotheses, double tau2, double f0,
                                                         const int64_t* __restrict__ row_ptr, const double* __restrict__ strip,
                                                         const int64_t* __restrict__ count, const double* __restrict__ hyp, double* __restrict__ slots)
{
    const int lane = threadIdx.x & (FD_L - 1);
    // the wave's number through the scalar unit, so that everything derived from it (the pair, its rows) is known to be uniform
    const int64_t w = (int64_t)blockIdx.x * (FD_BLOCK / FD_L) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / FD_L));
    if (w >= n_waves) return;
    const int64_t i = w / waves;
    const int32_t h = (int32_t)(w % waves) * FD_L + lane;
    const int64_t n = count[i], o0 = row_ptr[i];
    double* __restrict__ slot = slots + SRK_FUND_SLOT * w;

    double F[9];
    int valid = 0;
#pragma unroll
    for (int e = 0; e < 9; ++e) F[e] = 0.0;
    if (h < hypotheses) { // a lane past the last hypothesis has no record
        const double* rec = hyp + SRK_FUND_HYP * (i * hypotheses + h);
#pragma unroll
        for (int e = 0; e < 9; ++e) F[e] = rec[e];
        valid = rec[11] != 0.0;
    }
    double score = 0.0;
    int32_t inl = 0;
    if (__ballot(valid) != 0ull) { // uniform
        for (int64_t r = 0; r < n; ++r) { // ascending rank, one accumulator; the record's address is the same in every lane
            const double* e = strip + SRK_FUND_STRIP * (o0 + r);
            const double rec[5] = { e[0], e[1], e[2], e[3], e[4] };
            int in;
            double s2;
            score += srk_fund_term(F, rec, f0, tau2, in, s2);
            inl += in;
        }
    }
    double bs = valid ? score : INFINITY;
    int32_t bh = h;
#pragma unroll
    for (int d = FD_L / 2; d >= 1; d >>= 1) { // the wave's best: the smallest score, an equal score to the smaller h
        const double os = __shfl_down(bs, d, FD_L);
        const int32_t oh = __shfl_down(bh, d, FD_L);
        if (os < bs || (os == bs && oh < bh)) {
            bs = os;
            bh = oh;
        }
    }
    bs = __shfl(bs, 0, FD_L);
    bh = __shfl(bh, 0, FD_L);
    const int models = __popcll(__ballot(valid));
    if (bs < INFINITY) {
        if (h == bh) {
            slot[0] = score;
            slot[1] = (double)h;
            slot[2] = (double)inl;
            slot[3] = (double)models;
        }
    } else if (lane == 0) {
        slot[0] = INFINITY;
        slot[1] = slot[2] = 0.0;
        slot[3] = (double)models;
    }
}

// the lanes' sums merged in the wave's fixed tree, the total to every lane
template <int W> __device__ __forceinline__ void fd_merge(double* acc)
{
#pragma unroll
    for (int d = FD_L / 2; d >= 1; d >>= 1) {
#pragma unroll
        for (int e = 0; e < W; ++e) acc[e] += __shfl_down(acc[e], d, FD_L);
    }
#pragma unroll
    for (int e = 0; e < W; ++e) acc[e] = __shfl(acc[e], 0, FD_L);
}

__device__ __forceinline__ void fd_record(const double* e, double* rec)
{
    rec[0] = e[0], rec[1] = e[1], rec[2] = e[2], rec[3] = e[3], rec[4] = e[4];
}

// the score of F over the pair's n matches in the score kernel's order: ascending rank, one accumulator, in every lane alike
__device__ __forceinline__ double fd_score(const double* F, const double* rows, int64_t n, double f0, double tau2, int32_t& inl, double& ss)
{
    double sc = 0.0;
    inl = 0;
    ss = 0.0;
    for (int64_t r = 0; r < n; ++r) {
        double rec[5];
        fd_record(rows + SRK_FUND_STRIP * r, rec);
        int in;
        double s2;
        sc += srk_fund_term(F, rec, f0, tau2, in, s2);
        inl += in;
        ss += in ? s2 : 0.0;
    }
    return sc;
}

// the sums of a linearisation over the inliers of F: lane l takes ranks l, l + 64, .., the lanes merged in the fixed tree
__device__ __forceinline__ void fd_sums(const SrkFundRep& cur, const double* F, const double* rows, int64_t n, int lane, double f0, double tau2, double* acc)
{
    SrkFundLin lin;
    srk_fund_linearise(cur, lin);
#pragma unroll
    for (int e = 0; e < SRK_FUND_ACC; ++e) acc[e] = 0.0;
    for (int64_t k = lane; k < n; k += FD_L) {
        double rec[5];
        fd_record(rows + SRK_FUND_STRIP * k, rec);
        int in;
        double s2;
        srk_fund_term(F, rec, f0, tau2, in, s2);
        if (in) srk_fund_accumulate(acc, lin, rec, f0);
    }
    fd_merge<SRK_FUND_ACC>(acc);
}

__global__ __launch_bounds__(FD_BLOCK) void k_fund_pick(int32_t n_pairs, int32_t waves, int32_t hypotheses, double tau2, double f0, int32_t refine_rounds,
                                                        const int64_t* __restrict__ row_ptr, const double* __restrict__ uv_a,
                                                        const double* __restrict__ uv_b, const double* __restrict__ q, const double* __restrict__ strip,
                                                        const int64_t* __restrict__ count, const double* __restrict__ hyp, const double* __restrict__ slots,
                                                        double* __restrict__ Fout, double* __restrict__ Uout, double* __restrict__ Vout,
                                                        double* __restrict__ sigma_out, double* __restrict__ fund, double* __restrict__ info,
                                                        uint32_t* __restrict__ status, uint8_t* __restrict__ inlier_out)
{
    const int lane = threadIdx.x & (FD_L - 1);
    const int64_t i = (int64_t)blockIdx.x * (FD_BLOCK / FD_L) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / FD_L));
    if (i >= n_pairs) return;
    const int64_t o0 = row_ptr[i], o1 = row_ptr[i + 1], n = count[i];
    const double* fs = slots + SRK_FUND_SLOT * (i * waves);
    const double* rows = strip + SRK_FUND_STRIP * o0;
    double best = INFINITY, models = 0.0;
    int32_t bw = -1;
    for (int32_t w = 0; w < waves; ++w) { // ascending wave order = ascending h: an equal score stays with the smaller h
        const double s = fs[SRK_FUND_SLOT * w];
        models += fs[SRK_FUND_SLOT * w + 3];
        if (s < best) {
            best = s;
            bw = w;
        }
    }
    // "not a number" for the figures of a pair without a model, formed at run time: written as a constant it can end up as a 64-bit
    // scalar literal, which the gfx950 assembler encodes as zero
    const double none = sqrt(-1.0 - (double)n);
    SrkFundRep cur;
    srk_fund_identity(cur);
    double F[9], acc[SRK_FUND_ACC];
#pragma unroll
    for (int e = 0; e < 9; ++e) F[e] = 0.0;
#pragma unroll
    for (int e = 0; e < SRK_FUND_ACC; ++e) acc[e] = 0.0;
    double ss = 0.0, hwin = 0.0, err8 = 0.0, nroots = 0.0, cond = none;
    int32_t inl = 0, accepted = 0, used = 0;
    int have = 0;
    if (bw >= 0) {
        hwin = fs[SRK_FUND_SLOT * bw + 1];
        const double* rec = hyp + SRK_FUND_HYP * (i * hypotheses + (int64_t)hwin);
        double Fh[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) Fh[e] = rec[e];
        err8 = rec[9];
        nroots = rec[10];
        have = srk_fund_represent(Fh, cur);
    }
    if (have) {
        srk_fund_build(cur, F);
        srk_fund_sign(cur, F); // the current model is always the signed one: the sums belong to the U that is returned
        best = fd_score(F, rows, n, f0, tau2, inl, ss);
        double c = SRK_FUND_C0;
        int fresh = 1;
        for (int32_t attempt = 0; attempt < refine_rounds; ++attempt) { // every condition below is the same in every lane
            if (inl < SRK_FUND_MIN_INLIERS) break;
            if (fresh) fd_sums(cur, F, rows, n, lane, f0, tau2, acc);
            fresh = 0;
            int finite = 1;
#pragma unroll
            for (int e = 0; e < SRK_FUND_ACC; ++e) finite = finite && isfinite(acc[e]);
            if (!finite) break;
            ++used;
            double d[SRK_FUND_NV], Fc[9], sc = INFINITY, css = 0.0;
            int32_t cinl = 0;
            SrkFundRep cand;
            const int stepped = srk_fund_lm_step(acc, c, d);
            if (stepped) {
                srk_fund_move(cur, d, cand);
                srk_fund_build(cand, Fc);
                sc = fd_score(Fc, rows, n, f0, tau2, cinl, css);
            }
            const int last = stepped && fabs(sc - best) <= SRK_FUND_STOP * best;
            if (stepped && sc < best) { // only a strictly smaller score is accepted
                best = sc;
                inl = cinl;
                ss = css;
                cur = cand;
#pragma unroll
                for (int e = 0; e < 9; ++e) F[e] = Fc[e];
                srk_fund_sign(cur, F);
                c /= 10.0;
                ++accepted;
                fresh = 1;
            } else
                c *= 10.0;
            if (last) break;
        }
        if (fresh) fd_sums(cur, F, rows, n, lane, f0, tau2, acc); // the information at the result
        double A[SRK_FUND_NV][SRK_FUND_NV];
        srk_fund_full(acc, A);
        cond = srk_fund_cond1(A, none);
    } else
        srk_fund_identity(cur);
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) Fout[9 * i + e] = F[e], Uout[9 * i + e] = cur.U[e], Vout[9 * i + e] = cur.V[e];
        sigma_out[i] = cur.sigma;
        double* l = fund + 12 * i;
        l[0] = have ? sqrt(best / (double)n) : none;
        l[1] = (double)n;
        l[2] = (double)inl;
        l[3] = have ? hwin : none;
        l[4] = models;
        l[5] = have ? sqrt(err8) : none;
        l[6] = (double)accepted;
        l[7] = (double)used;
        l[8] = have ? (inl > 0 ? sqrt(ss / (double)inl) : 0.0) : none; // a winner without inliers: nothing to average
        l[9] = cur.sigma;
        l[10] = cond;
        l[11] = have ? nroots : 0.0;
        double A[SRK_FUND_NV][SRK_FUND_NV];
        srk_fund_full(acc, A);
#pragma unroll
        for (int a = 0; a < SRK_FUND_NV; ++a) {
#pragma unroll
            for (int b = 0; b < SRK_FUND_NV; ++b) info[49 * i + SRK_FUND_NV * a + b] = have ? A[a][b] : 0.0;
        }
        status[i] = n < 8 ? 1u : (have ? 0u : 2u); // SRK_FUNDAMENTAL_FEW_POINTS, SRK_FUNDAMENTAL_NO_MODEL
    }
    if (inlier_out) {
        for (int64_t o = o0 + lane; o < o1; o += FD_L) {
            const double qo = q ? q[o] : 1.0;
            int in = 0;
            if (have && qo > 0.0) {
                const double rec[5] = { uv_a[2 * o], uv_a[2 * o + 1], uv_b[2 * o], uv_b[2 * o + 1], qo };
                double s2;
                srk_fund_term(F, rec, f0, tau2, in, s2);
            }
            inlier_out[o] = (uint8_t)in;
        }
    }
}

void srk_launch_fund_gather(hipStream_t s, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                            double* strip, int64_t* count)
{
    if (n_pairs <= 0) return;
    const int32_t per = FD_BLOCK / FD_L;
    hipLaunchKernelGGL(k_fund_gather, dim3((unsigned)((n_pairs + per - 1) / per)), dim3(FD_BLOCK), 0, s, n_pairs, row_ptr, uv_a, uv_b, q, strip, count);
}

void srk_launch_fund_solve(hipStream_t s, int32_t n_pairs, int32_t hypotheses, uint64_t seed, double f0, const int64_t* row_ptr, const double* strip,
                           const int64_t* count, double* hyp)
{
    if (n_pairs <= 0) return;
    const int64_t n_hyp = (int64_t)n_pairs * hypotheses;
    hipLaunchKernelGGL(k_fund_solve, dim3((unsigned)((n_hyp + FD_BLOCK - 1) / FD_BLOCK)), dim3(FD_BLOCK), 0, s, n_hyp, hypotheses, seed, f0, row_ptr, strip,
                       count, hyp);
}

void srk_launch_fund_score(hipStream_t s, int32_t n_pairs, int32_t hypotheses, double tau, double f0, const int64_t* row_ptr, const double* strip,
                           const int64_t* count, const double* hyp, double* slots)
{
    if (n_pairs <= 0) return;
    const int32_t per = FD_BLOCK / FD_L, waves = (hypotheses + FD_L - 1) / FD_L;
    const int64_t n_waves = (int64_t)n_pairs * waves;
    hipLaunchKernelGGL(k_fund_score, dim3((unsigned)((n_waves + per - 1) / per)), dim3(FD_BLOCK), 0, s, n_waves, waves, hypotheses, tau * tau, f0, row_ptr,
                       strip, count, hyp, slots);
}

void srk_launch_fund_pick(hipStream_t s, int32_t n_pairs, int32_t hypotheses, double tau, double f0, int32_t refine_rounds, const int64_t* row_ptr,
                          const double* uv_a, const double* uv_b, const double* q, const double* strip, const int64_t* count, const double* hyp,
                          const double* slots, double* F, double* U, double* V, double* sigma, double* fund, double* info, uint32_t* status,
                          uint8_t* inlier_out)
{
    if (n_pairs <= 0) return;
    const int32_t per = FD_BLOCK / FD_L, waves = (hypotheses + FD_L - 1) / FD_L;
    hipLaunchKernelGGL(k_fund_pick, dim3((unsigned)((n_pairs + per - 1) / per)), dim3(FD_BLOCK), 0, s, n_pairs, waves, hypotheses, tau * tau, f0,
                       refine_rounds, row_ptr, uv_a, uv_b, q, strip, count, hyp, slots, F, U, V, sigma, fund, info, status, inlier_out);
}
