// srk_align.hip -- map alignment (srk_align_points, srk_ba_align), the device half.
//
// Hypothesise and verify with a three-point sample, in the shape of srk_locate.hip: every hypothesis of a set reads the same
// correspondences, so a wave is 64 hypotheses of one set, one per lane, and the loop over the set's correspondences has a
// wave-uniform index: a record is fetched once per wave (a scalar load) and every lane maps it under its own similarity.
//   k_align_gather  one wave per set: the weighted correspondences (q > 0) compacted by the wave's ballot into a contiguous strip
//                   of 64-byte records {a, b, q, 0} at row_ptr[i] + rank;
//   k_align_score   one lane per (set, hypothesis): the sample, Horn's triad (srk_align_math.hpp), then the MSAC score over the
//                   strip in ascending rank, one accumulator; the wave's best (score, h) by a fixed shuffle tree into the wave's
//                   slot, model included.  The hypothesis lives in registers only; the grid is sets x ceil(H / 64) waves;
//   k_align_pick    one wave per set: the slots in ascending wave order, then up to refine_rounds rounds of local optimisation with
//                   the whole wave (the inliers' weighted sums in two lane-strided passes merged in a fixed tree, the closed-form
//                   similarity computed redundantly by every lane, a re-score in the score kernel's order, accepted only when
//                   strictly smaller), the outputs, and with inlier_out one pass at the final model.
// No LDS, no atomics, no workgroup barrier: a set's bits depend on its own correspondences, the seed and the options alone.
#include "srk_align_dev.hpp"
#include "srk_align_math.hpp"

#define AL_BLOCK 256
#define AL_L SRK_ALIGN_LANES
static_assert(AL_L == 64, "a hypothesis wave is the hardware's");

__global__ __launch_bounds__(AL_BLOCK) void k_align_gather(int32_t n_sets, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ point,
                                                           const double* __restrict__ a, const double* __restrict__ b, const double* __restrict__ q,
                                                           double* __restrict__ strip, int64_t* __restrict__ count)
{
    const int lane = threadIdx.x & (AL_L - 1);
    const int64_t i = (int64_t)blockIdx.x * (AL_BLOCK / AL_L) + (threadIdx.x / AL_L);
    if (i >= n_sets) return; // a whole wave: the lanes of a set leave together
    const int64_t o0 = row_ptr[i], o1 = row_ptr[i + 1];
    int64_t base = 0;
    for (int64_t c0 = o0; c0 < o1; c0 += AL_L) {
        const int64_t o = c0 + lane;
        const bool w = o < o1 && (q == nullptr || q[o] > 0.0);
        const unsigned long long m = __ballot(w);
        if (w) { // the rank rule: the weighted correspondences in ascending o
            const int64_t rank = base + __popcll(m & ((1ull << lane) - 1ull));
            const double* x = a + 3 * (point ? (int64_t)point[o] : o);
            const double* y = b + 3 * o;
            double2* e = reinterpret_cast<double2*>(strip + SRK_ALIGN_STRIP * (o0 + rank)); // rank <= o - o0: inside the set's rows
            e[0] = make_double2(x[0], x[1]);
            e[1] = make_double2(x[2], y[0]);
            e[2] = make_double2(y[1], y[2]);
            e[3] = make_double2(q ? q[o] : 1.0, 0.0);
        }
        base += __popcll(m);
    }
    if (lane == 0) count[i] = base;
}

__global__ __launch_bounds__(AL_BLOCK) void k_align_score(int64_t n_waves, int32_t waves, int32_t hypotheses, uint64_t seed, double tau2, int with_scale,
                                                          const int64_t* __restrict__ row_ptr, const double* __restrict__ strip,
                                                          const int64_t* __restrict__ count, double* __restrict__ slots)
{
    const int lane = threadIdx.x & (AL_L - 1);
    // the wave's number through the scalar unit, so that everything derived from it (the set, its rows) is known to be uniform
    const int64_t w = (int64_t)blockIdx.x * (AL_BLOCK / AL_L) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / AL_L));
    if (w >= n_waves) return;
    const int64_t i = w / waves;
    const int32_t h = (int32_t)(w % waves) * AL_L + lane;
    const int64_t n = count[i], o0 = row_ptr[i];
    double* __restrict__ slot = slots + SRK_ALIGN_SLOT * w;

    SrkAlignModel m;
    int valid = 0;
    if (n >= 3) {
        // a lane past the last hypothesis works on a sample of its own and is dropped below
        int64_t r0, r1, r2;
        srk_align_sample(seed, (uint32_t)h, n, r0, r1, r2);
        const double* e0 = strip + SRK_ALIGN_STRIP * (o0 + r0);
        const double* e1 = strip + SRK_ALIGN_STRIP * (o0 + r1);
        const double* e2 = strip + SRK_ALIGN_STRIP * (o0 + r2);
        double a3[9], b3[9];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a3[c] = e0[c], a3[3 + c] = e1[c], a3[6 + c] = e2[c];
            b3[c] = e0[3 + c], b3[3 + c] = e1[3 + c], b3[6 + c] = e2[3 + c];
        }
        valid = srk_align_hypothesis(a3, b3, with_scale, m) && h < hypotheses;
    } else
        srk_align_identity(m);

    double score = 0.0, ss = 0.0;
    int32_t inl = 0;
    if (__ballot(valid) != 0ull) { // uniform
        double sR[9];
        srk_align_scaled(m, sR);
        for (int64_t r = 0; r < n; ++r) { // ascending rank, one accumulator; the record's address is the same in every lane
            const double* e = strip + SRK_ALIGN_STRIP * (o0 + r);
            const double x[3] = { e[0], e[1], e[2] }, y[3] = { e[3], e[4], e[5] };
            int in;
            double r2;
            score += srk_align_term(sR, m.t, x, y, e[6], tau2, in, r2);
            inl += in;
            ss += in ? r2 : 0.0;
        }
    }
    double bs = valid ? score : INFINITY;
    int32_t bh = h;
#pragma unroll
    for (int d = AL_L / 2; d >= 1; d >>= 1) { // the wave's best: the smallest score, an equal score to the smaller h
        const double os = __shfl_down(bs, d, AL_L);
        const int32_t oh = __shfl_down(bh, d, AL_L);
        if (os < bs || (os == bs && oh < bh)) {
            bs = os;
            bh = oh;
        }
    }
    bs = __shfl(bs, 0, AL_L);
    bh = __shfl(bh, 0, AL_L);
    const int models = __popcll(__ballot(valid));
    if (bs < INFINITY) {
        if (h == bh) {
            slot[0] = score;
            slot[1] = (double)h;
            slot[2] = (double)inl;
            slot[3] = (double)models;
            slot[4] = m.s;
            slot[5] = ss;
#pragma unroll
            for (int e = 0; e < 9; ++e) slot[6 + e] = m.R[e];
#pragma unroll
            for (int e = 0; e < 3; ++e) slot[15 + e] = m.t[e];
            slot[18] = slot[19] = 0.0;
        }
    } else if (lane == 0) {
        slot[0] = INFINITY;
#pragma unroll
        for (int e = 1; e < SRK_ALIGN_SLOT; ++e) slot[e] = 0.0;
    }
}

// the lanes' sums merged in the wave's fixed tree, the total to every lane
template <int W> __device__ __forceinline__ void al_merge(double* acc)
{
#pragma unroll
    for (int d = AL_L / 2; d >= 1; d >>= 1) {
#pragma unroll
        for (int e = 0; e < W; ++e) acc[e] += __shfl_down(acc[e], d, AL_L);
    }
#pragma unroll
    for (int e = 0; e < W; ++e) acc[e] = __shfl(acc[e], 0, AL_L);
}

__global__ __launch_bounds__(AL_BLOCK) void k_align_pick(int32_t n_sets, int32_t waves, double tau2, int with_scale, int32_t refine_rounds,
                                                         const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ point,
                                                         const double* __restrict__ a, const double* __restrict__ b, const double* __restrict__ q,
                                                         const double* __restrict__ strip, const int64_t* __restrict__ count,
                                                         const double* __restrict__ slots, double* __restrict__ scale, double* __restrict__ Rout,
                                                         double* __restrict__ tout, double* __restrict__ aligned, uint32_t* __restrict__ status,
                                                         uint8_t* __restrict__ inlier_out)
{
    const int lane = threadIdx.x & (AL_L - 1);
    const int64_t i = (int64_t)blockIdx.x * (AL_BLOCK / AL_L) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / AL_L));
    if (i >= n_sets) return;
    const int64_t o0 = row_ptr[i], o1 = row_ptr[i + 1], n = count[i];
    const double* fs = slots + SRK_ALIGN_SLOT * (i * waves);
    const double* rows = strip + SRK_ALIGN_STRIP * o0;
    double best = INFINITY, models = 0.0;
    int32_t bw = -1;
    for (int32_t w = 0; w < waves; ++w) { // ascending wave order = ascending h: an equal score stays with the smaller h
        const double s = fs[SRK_ALIGN_SLOT * w];
        models += fs[SRK_ALIGN_SLOT * w + 3];
        if (s < best) {
            best = s;
            bw = w;
        }
    }
    SrkAlignModel cur;
    srk_align_identity(cur);
    double inl = 0.0, ss = 0.0, hwin = NAN, gap = NAN;
    int32_t rounds = 0;
    if (bw >= 0) {
        const double* s = fs + SRK_ALIGN_SLOT * bw;
        hwin = s[1];
        inl = s[2];
        cur.s = s[4];
        ss = s[5];
#pragma unroll
        for (int e = 0; e < 9; ++e) cur.R[e] = s[6 + e];
#pragma unroll
        for (int e = 0; e < 3; ++e) cur.t[e] = s[15 + e];
        for (int32_t round = 0; round < refine_rounds; ++round) { // every condition below is the same in every lane
            double sR[9], acc[10];
            srk_align_scaled(cur, sR);
#pragma unroll
            for (int e = 0; e < 10; ++e) acc[e] = 0.0;
            int32_t cnt = 0;
            for (int64_t k = lane; k < n; k += AL_L) { // pass one: lane l takes ranks l, l + 64, ..
                const double* e = rows + SRK_ALIGN_STRIP * k;
                const double x[3] = { e[0], e[1], e[2] }, y[3] = { e[3], e[4], e[5] };
                int in;
                double r2;
                srk_align_term(sR, cur.t, x, y, e[6], tau2, in, r2);
                if (in) {
                    srk_align_pass_one(acc, x, y, e[6]);
                    ++cnt;
                }
            }
#pragma unroll
            for (int d = AL_L / 2; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, AL_L);
            if (cnt < 3) break;
            al_merge<7>(acc);
            const double am[3] = { acc[1] / acc[0], acc[2] / acc[0], acc[3] / acc[0] };
            const double bm[3] = { acc[4] / acc[0], acc[5] / acc[0], acc[6] / acc[0] };
#pragma unroll
            for (int e = 0; e < 10; ++e) acc[e] = 0.0;
            for (int64_t k = lane; k < n; k += AL_L) { // pass two: the same walk, centred
                const double* e = rows + SRK_ALIGN_STRIP * k;
                const double x[3] = { e[0], e[1], e[2] }, y[3] = { e[3], e[4], e[5] };
                int in;
                double r2;
                srk_align_term(sR, cur.t, x, y, e[6], tau2, in, r2);
                if (in) srk_align_pass_two(acc, x, y, e[6], am, bm);
            }
            al_merge<10>(acc);
            SrkAlignModel cand;
            double g;
            if (!srk_align_closed_form(acc, acc[9], am, bm, with_scale, cand, g)) break;
            srk_align_scaled(cand, sR);
            double sc = 0.0, css = 0.0;
            int32_t cinl = 0;
            for (int64_t r = 0; r < n; ++r) { // the score kernel's order: ascending rank, one accumulator, in every lane alike
                const double* e = rows + SRK_ALIGN_STRIP * r;
                const double x[3] = { e[0], e[1], e[2] }, y[3] = { e[3], e[4], e[5] };
                int in;
                double r2;
                sc += srk_align_term(sR, cand.t, x, y, e[6], tau2, in, r2);
                cinl += in;
                css += in ? r2 : 0.0;
            }
            if (!(sc < best)) break; // only a strictly smaller score is accepted
            best = sc;
            inl = (double)cinl;
            ss = css;
            cur = cand;
            gap = g;
            ++rounds;
        }
    }
    if (lane == 0) {
        scale[i] = cur.s;
#pragma unroll
        for (int e = 0; e < 9; ++e) Rout[9 * i + e] = cur.R[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) tout[3 * i + e] = cur.t[e];
        double* l = aligned + 8 * i;
        l[0] = bw >= 0 ? sqrt(best / (double)n) : NAN;
        l[1] = (double)n;
        l[2] = inl;
        l[3] = hwin;
        l[4] = models;
        l[5] = (double)rounds;
        l[6] = gap;
        l[7] = bw >= 0 ? sqrt(ss / inl) : NAN;
        status[i] = n < 3 ? 1u : (bw < 0 ? 2u : 0u); // SRK_ALIGN_FEW_POINTS, SRK_ALIGN_NO_MODEL
    }
    if (inlier_out) {
        double sR[9];
        srk_align_scaled(cur, sR);
        for (int64_t o = o0 + lane; o < o1; o += AL_L) {
            const double qo = q ? q[o] : 1.0;
            int in = 0;
            if (bw >= 0 && qo > 0.0) {
                const double* xs = a + 3 * (point ? (int64_t)point[o] : o);
                const double x[3] = { xs[0], xs[1], xs[2] }, y[3] = { b[3 * o], b[3 * o + 1], b[3 * o + 2] };
                double r2;
                srk_align_term(sR, cur.t, x, y, qo, tau2, in, r2);
            }
            inlier_out[o] = (uint8_t)in;
        }
    }
}

void srk_launch_align_gather(hipStream_t s, int32_t n_sets, const int64_t* row_ptr, const int32_t* point, const double* a, const double* b,
                             const double* q, double* strip, int64_t* count)
{
    if (n_sets <= 0) return;
    const int32_t per = AL_BLOCK / AL_L;
    hipLaunchKernelGGL(k_align_gather, dim3((unsigned)((n_sets + per - 1) / per)), dim3(AL_BLOCK), 0, s, n_sets, row_ptr, point, a, b, q, strip, count);
}

void srk_launch_align_score(hipStream_t s, int32_t n_sets, int32_t hypotheses, uint64_t seed, double tau, int with_scale, const int64_t* row_ptr,
                            const double* strip, const int64_t* count, double* slots)
{
    if (n_sets <= 0) return;
    const int32_t per = AL_BLOCK / AL_L, waves = (hypotheses + AL_L - 1) / AL_L;
    const int64_t n_waves = (int64_t)n_sets * waves;
    hipLaunchKernelGGL(k_align_score, dim3((unsigned)((n_waves + per - 1) / per)), dim3(AL_BLOCK), 0, s, n_waves, waves, hypotheses, seed, tau * tau,
                       with_scale, row_ptr, strip, count, slots);
}

void srk_launch_align_pick(hipStream_t s, int32_t n_sets, int32_t hypotheses, double tau, int with_scale, int32_t refine_rounds, const int64_t* row_ptr,
                           const int32_t* point, const double* a, const double* b, const double* q, const double* strip, const int64_t* count,
                           const double* slots, double* scale, double* R, double* t, double* aligned, uint32_t* status, uint8_t* inlier_out)
{
    if (n_sets <= 0) return;
    const int32_t per = AL_BLOCK / AL_L, waves = (hypotheses + AL_L - 1) / AL_L;
    hipLaunchKernelGGL(k_align_pick, dim3((unsigned)((n_sets + per - 1) / per)), dim3(AL_BLOCK), 0, s, n_sets, waves, tau * tau, with_scale, refine_rounds,
                       row_ptr, point, a, b, q, strip, count, slots, scale, R, t, aligned, status, inlier_out);
}
