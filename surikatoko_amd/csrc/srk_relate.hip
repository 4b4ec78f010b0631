// srk_relate.hip -- two-view relative pose (srk_relate_frames), the device half.
//
// Hypothesise and verify from 2D-2D matches.  Four kernels:
//   k_relate_gather  one wave per pair: the weighted matches (q > 0) compacted by the wave's ballot into a contiguous strip at
//                    row_ptr[i] + rank, so that the sampler reads rank r directly and the scoring loop reads aligned 64-byte records;
//   k_relate_solve   16 lanes per (pair, hypothesis), four hypotheses to a wave.  The 10 x 20 matrix of the cubic constraints does
//                    not fit one lane's registers, so lane r < 10 of the group builds and holds row r.  Gauss-Jordan finds the
//                    pivot by a shuffle reduction over the group, broadcasts the pivot row with __shfl(., lane, 16) and records
//                    the owning lane in place of an exchange.  det B(z) is formed by every lane; at each level of the derivative
//                    chain lane k owns interval k, and the roots found are ranked by ballot and shared by shuffles.  Each lane
//                    with a root of p forms its essential matrix and measures it at the sixth match; the group's minimum goes
//                    into the hypothesis' record;
//   k_relate_score   one lane per (pair, hypothesis), a wave = 64 hypotheses of one pair: the MSAC score over the strip in ascending
//                    rank, one accumulator, the record read at a wave-uniform address; the wave's best by a fixed shuffle tree;
//   k_relate_pick    one wave per pair: the slots in ascending wave order, the decomposition of the winner, the vote of its four
//                    poses over the pair's inliers with per-lane counts merged in a fixed tree, the outputs.
// No LDS, no atomics, no workgroup barrier: a pair's bits depend on its own matches, the seed and the hypothesis count alone.
#include "srk_relate_dev.hpp"
#include "srk_relate_math.hpp"

#define RL_BLOCK 256
#define RL_L SRK_RELATE_LANES
#define RL_G SRK_RELATE_GROUP
static_assert(RL_L == 64 && RL_G == 16, "a wave is the hardware's, a solve group a quarter of it");

__global__ __launch_bounds__(RL_BLOCK) void k_relate_gather(int32_t n_pairs, const int64_t* __restrict__ row_ptr, const double* __restrict__ uv_a,
                                                            const double* __restrict__ uv_b, const double* __restrict__ q,
                                                            double* __restrict__ strip, int64_t* __restrict__ count)
{
    const int lane = threadIdx.x & (RL_L - 1);
    const int64_t i = (int64_t)blockIdx.x * (RL_BLOCK / RL_L) + (threadIdx.x / RL_L);
    if (i >= n_pairs) return; // a whole wave: the lanes of a pair leave together
    const int64_t o0 = row_ptr[i], o1 = row_ptr[i + 1];
    int64_t base = 0;
    for (int64_t c0 = o0; c0 < o1; c0 += RL_L) {
        const int64_t o = c0 + lane;
        const bool w = o < o1 && (q == nullptr || q[o] > 0.0);
        const unsigned long long m = __ballot(w);
        if (w) { // the weighted matches in ascending o
            const int64_t rank = base + __popcll(m & ((1ull << lane) - 1ull));
            const double2 a = reinterpret_cast<const double2*>(uv_a)[o], b = reinterpret_cast<const double2*>(uv_b)[o];
            double2* e = reinterpret_cast<double2*>(strip + SRK_RELATE_STRIP * (o0 + rank)); // rank <= o - o0: inside the pair's rows
            e[0] = a;
            e[1] = b;
            e[2] = make_double2(q ? q[o] : 1.0, (double)(o - o0));
            e[3] = make_double2(0.0, 0.0);
        }
        base += __popcll(m);
    }
    if (lane == 0) count[i] = base;
}

// the smaller of (v, l) pairs over the 16 lanes of a group, an equal v to the smaller l; with `larger` the larger v.  The result
// is that of the group's lane 0, handed to all.
template <bool larger> __device__ __forceinline__ void rl_group_best(double& v, int& l)
{
#pragma unroll
    for (int d = RL_G / 2; d >= 1; d >>= 1) {
        const double ov = __shfl_down(v, d, RL_G);
        const int ol = __shfl_down(l, d, RL_G);
        if ((larger ? ov > v : ov < v) || (ov == v && ol < l)) {
            v = ov;
            l = ol;
        }
    }
    v = __shfl(v, 0, RL_G);
    l = __shfl(l, 0, RL_G);
}

// level D of the derivative chain: lane k of the group owns interval k between the roots of level D - 1 (held by the lanes that
// found them, in ascending order) and the bound
template <int D> __device__ __forceinline__ void rl_level(const double* p, double bound, int g, int shift, double& root, int& has)
{
    const unsigned mask = (unsigned)(__ballot(has) >> shift) & 0xffffu;
    const int n = __popc(mask);
    double lo = -bound, hi = bound;
#pragma unroll
    for (int s = 0; s < 10; ++s) {
        const double v = __shfl(root, s, RL_G);
        const bool bit = (mask >> s) & 1u;
        const int rk = __popc(mask & ((1u << s) - 1u));
        lo = (bit && rk == g - 1) ? v : lo;
        hi = (bit && rk == g) ? v : hi;
    }
    double r;
    const int f = srk_relate_interval<D>(p, lo, hi, r);
    has = g <= n && f;
    root = r;
}

__global__ __launch_bounds__(RL_BLOCK) void k_relate_solve(int64_t n_groups, int32_t hypotheses, uint64_t seed, double f0,
                                                           const int64_t* __restrict__ row_ptr, const double* __restrict__ strip,
                                                           const int64_t* __restrict__ count, const double* __restrict__ K_a,
                                                           const double* __restrict__ K_b, int shared_k, double* __restrict__ hyp)
{
    const int lane = threadIdx.x & (RL_L - 1), g = lane & (RL_G - 1), shift = lane & ~(RL_G - 1);
    const int64_t grp = (int64_t)blockIdx.x * (RL_BLOCK / RL_G) + (threadIdx.x / RL_G);
    // nothing below leaves early: a group past the end, or of a pair with too few matches, runs on zeros and stores nothing, so
    // that every shuffle and ballot sees all 64 lanes
    const bool exists = grp < n_groups;
    const int64_t i = exists ? grp / hypotheses : 0;
    const int32_t h = exists ? (int32_t)(grp % hypotheses) : 0;
    const int64_t n = exists ? count[i] : 0, o0 = exists ? row_ptr[i] : 0;
    const bool live = n >= 6;

    double kai[9], kbi[9], uva[12], uvb[12];
    {
        double ka[9], kb[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            ka[e] = live ? (shared_k ? K_a : K_a + 9 * i)[e] : ((e % 4 == 0) ? 1.0 : 0.0);
            kb[e] = live ? (shared_k ? K_b : K_b + 9 * i)[e] : ((e % 4 == 0) ? 1.0 : 0.0);
        }
        srk_relate_inverse3(ka, kai);
        srk_relate_inverse3(kb, kbi);
        int64_t r[6];
        srk_relate_sample(seed, (uint32_t)h, live ? n : 6, r);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double* e = strip + SRK_RELATE_STRIP * (o0 + r[k]); // r[k] < n: inside the pair's weighted matches
            uva[2 * k] = live ? e[0] : 0.0;
            uva[2 * k + 1] = live ? e[1] : 0.0;
            uvb[2 * k] = live ? e[2] : 0.0;
            uvb[2 * k + 1] = live ? e[3] : 0.0;
        }
    }
    double N[36];
    {
        double xa[15], xb[15];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            srk_relate_ray(kai, uva[2 * m], uva[2 * m + 1], f0, xa + 3 * m);
            srk_relate_ray(kbi, uvb[2 * m], uvb[2 * m + 1], f0, xb + 3 * m);
        }
        srk_relate_nullspace(xa, xb, N);
    }
    double row[20];
    srk_relate_row(N, g < 10 ? g : 9, row);

    // Gauss-Jordan on the left ten columns: the pivot of column c is the largest entry among the rows that own no column yet
    int mine = -1, owner[10];
#pragma unroll
    for (int c = 0; c < 10; ++c) {
        double bv = (g < 10 && mine < 0) ? fabs(row[c]) : -1.0;
        int p = g;
        rl_group_best<true>(bv, p);
        const double inv = 1.0 / __shfl(row[c], p, RL_G), f = row[c];
#pragma unroll
        for (int j = c; j < 20; ++j) {
            const double pj = __shfl(row[j], p, RL_G) * inv;
            row[j] = g == p ? pj : row[j] - f * pj;
        }
        mine = g == p ? c : mine;
        owner[c] = p;
    }
    double bx[12], by[12], b1[15], p[11];
    {
        double G4[10], G5[10], G6[10], G7[10], G8[10], G9[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            G4[j] = __shfl(row[10 + j], owner[4], RL_G);
            G5[j] = __shfl(row[10 + j], owner[5], RL_G);
            G6[j] = __shfl(row[10 + j], owner[6], RL_G);
            G7[j] = __shfl(row[10 + j], owner[7], RL_G);
            G8[j] = __shfl(row[10 + j], owner[8], RL_G);
            G9[j] = __shfl(row[10 + j], owner[9], RL_G);
        }
        srk_relate_bz(G4, G5, G6, G7, G8, G9, bx, by, b1);
    }
    srk_relate_detb(bx, by, b1, p);
    const double bound = srk_relate_bound(p);

    double root = 0.0;
    int has = 0;
    rl_level<1>(p, bound, g, shift, root, has);
    rl_level<2>(p, bound, g, shift, root, has);
    rl_level<3>(p, bound, g, shift, root, has);
    rl_level<4>(p, bound, g, shift, root, has);
    rl_level<5>(p, bound, g, shift, root, has);
    rl_level<6>(p, bound, g, shift, root, has);
    rl_level<7>(p, bound, g, shift, root, has);
    rl_level<8>(p, bound, g, shift, root, has);
    rl_level<9>(p, bound, g, shift, root, has);
    rl_level<10>(p, bound, g, shift, root, has);

    // the lanes hold the roots in ascending order: each forms its essential matrix and measures it at the sixth match
    double E[9], F[9];
    srk_relate_model(N, bx, by, b1, root, E);
    srk_relate_fundamental(kai, kbi, E, F);
    const double e6 = srk_relate_sampson(F, uva[10], uva[11], uvb[10], uvb[11], f0);
    double bv = (has && live && isfinite(e6)) ? e6 : INFINITY;
    int w = g;
    rl_group_best<false>(bv, w); // an equal error stays with the smaller root
    if (exists) {
        double* rec = hyp + SRK_RELATE_HYP * grp;
        if (bv < INFINITY) {
            if (g == w) {
#pragma unroll
                for (int e = 0; e < 9; ++e) {
                    rec[e] = F[e];
                    rec[9 + e] = E[e];
                }
                rec[18] = e6;
                rec[19] = 1.0;
            }
        } else if (g == 0) {
#pragma unroll
            for (int e = 0; e < SRK_RELATE_HYP; ++e) rec[e] = 0.0;
        }
    }
}

__global__ __launch_bounds__(RL_BLOCK) void k_relate_score(int64_t n_waves, int32_t waves, int32_t hypotheses, double tau2, double f0,
                                                           const int64_t* __restrict__ row_ptr, const double* __restrict__ strip,
                                                           const int64_t* __restrict__ count, const double* __restrict__ hyp,
                                                           double* __restrict__ slots)
{
    const int lane = threadIdx.x & (RL_L - 1);
    // the wave's number through the scalar unit, so that everything derived from it (the pair, its rows) is known to be uniform
    const int64_t w = (int64_t)blockIdx.x * (RL_BLOCK / RL_L) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / RL_L));
    if (w >= n_waves) return;
    const int64_t i = w / waves;
    const int32_t h = (int32_t)(w % waves) * RL_L + lane;
    const int64_t n = count[i], o0 = row_ptr[i];
    double* __restrict__ slot = slots + SRK_RELATE_SLOT * w;

    double F[9];
    int valid = 0;
    if (h < hypotheses) { // the record of a pair with too few matches says: no model
        const double* rec = hyp + SRK_RELATE_HYP * (i * hypotheses + h);
#pragma unroll
        for (int e = 0; e < 9; ++e) F[e] = rec[e];
        valid = rec[19] != 0.0;
    } else {
#pragma unroll
        for (int e = 0; e < 9; ++e) F[e] = 0.0;
    }
    double score = 0.0;
    int32_t inl = 0;
    if (__ballot(valid) != 0ull) { // uniform
        for (int64_t r = 0; r < n; ++r) { // ascending rank, one accumulator; the record's address is the same in every lane
            const double* e = strip + SRK_RELATE_STRIP * (o0 + r);
            int in;
            score += srk_relate_term(F, e[0], e[1], e[2], e[3], e[4], f0, tau2, in);
            inl += in;
        }
    }
    double bs = valid ? score : INFINITY;
    int32_t bh = h;
#pragma unroll
    for (int d = RL_L / 2; d >= 1; d >>= 1) { // the wave's best: the smallest score, an equal score to the smaller h
        const double os = __shfl_down(bs, d, RL_L);
        const int32_t oh = __shfl_down(bh, d, RL_L);
        if (os < bs || (os == bs && oh < bh)) {
            bs = os;
            bh = oh;
        }
    }
    bs = __shfl(bs, 0, RL_L);
    bh = __shfl(bh, 0, RL_L);
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

__global__ __launch_bounds__(RL_BLOCK) void k_relate_pick(int32_t n_pairs, int32_t waves, int32_t hypotheses, double tau2, double f0,
                                                          const int64_t* __restrict__ row_ptr, const double* __restrict__ q,
                                                          const double* __restrict__ strip, const int64_t* __restrict__ count,
                                                          const double* __restrict__ K_a, const double* __restrict__ K_b, int shared_k,
                                                          const double* __restrict__ hyp, const double* __restrict__ slots,
                                                          double* __restrict__ Rout, double* __restrict__ Tout, double* __restrict__ Eout,
                                                          double* __restrict__ related, uint32_t* __restrict__ status,
                                                          uint8_t* __restrict__ inlier_out)
{
    const int lane = threadIdx.x & (RL_L - 1);
    const int64_t i = (int64_t)blockIdx.x * (RL_BLOCK / RL_L) + (threadIdx.x / RL_L);
    if (i >= n_pairs) return;
    const int64_t o0 = row_ptr[i], o1 = row_ptr[i + 1], n = count[i];
    const double* fs = slots + SRK_RELATE_SLOT * (i * waves);
    double best = INFINITY, models = 0.0;
    int32_t bw = -1;
    for (int32_t w = 0; w < waves; ++w) { // ascending wave order = ascending h: an equal score stays with the smaller h
        const double s = fs[SRK_RELATE_SLOT * w];
        models += fs[SRK_RELATE_SLOT * w + 3];
        if (s < best) {
            best = s;
            bw = w;
        }
    }
    double R[9] = { 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0 }, T[3] = { 0.0, 0.0, 0.0 }, E[9] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    double l0 = NAN, l2 = 0.0, l3 = NAN, l5 = NAN, l6 = 0.0, l7 = NAN;
    if (inlier_out) { // the matches without weight, and every match of a pair without a model
        for (int64_t o = o0 + lane; o < o1; o += RL_L)
            if (bw < 0 || (q && !(q[o] > 0.0))) inlier_out[o] = 0;
    }
    if (bw >= 0) { // uniform
        const int64_t h = (int64_t)fs[SRK_RELATE_SLOT * bw + 1];
        const double* rec = hyp + SRK_RELATE_HYP * (i * hypotheses + h);
        double F[9], Ew[9], R1[9], R2[9], t[3], kai[9], kbi[9];
        {
            double ka[9], kb[9];
#pragma unroll
            for (int e = 0; e < 9; ++e) {
                F[e] = rec[e];
                Ew[e] = rec[9 + e];
                ka[e] = (shared_k ? K_a : K_a + 9 * i)[e];
                kb[e] = (shared_k ? K_b : K_b + 9 * i)[e];
            }
            srk_relate_inverse3(ka, kai);
            srk_relate_inverse3(kb, kbi);
        }
        srk_relate_decompose(Ew, R1, R2, t);
        int32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int64_t r = lane; r < n; r += RL_L) { // lane l takes the ranks l, l + 64, ...
            const double* e = strip + SRK_RELATE_STRIP * (o0 + r);
            const double ua = e[0], va = e[1], ub = e[2], vb = e[3];
            int in;
            srk_relate_term(F, ua, va, ub, vb, e[4], f0, tau2, in);
            if (inlier_out) inlier_out[o0 + (int64_t)e[5]] = (uint8_t)in;
            if (in) {
                double a[3], b[3], angle;
                srk_relate_ray(kai, ua, va, f0, a);
                srk_relate_ray(kbi, ub, vb, f0, b);
                if (srk_relate_front(R1, t, 1.0, a, b, angle)) ++c0, a0 += angle;
                if (srk_relate_front(R1, t, -1.0, a, b, angle)) ++c1, a1 += angle;
                if (srk_relate_front(R2, t, 1.0, a, b, angle)) ++c2, a2 += angle;
                if (srk_relate_front(R2, t, -1.0, a, b, angle)) ++c3, a3 += angle;
            }
        }
#pragma unroll
        for (int d = RL_L / 2; d >= 1; d >>= 1) { // the wave's tree
            c0 += __shfl_down(c0, d, RL_L);
            c1 += __shfl_down(c1, d, RL_L);
            c2 += __shfl_down(c2, d, RL_L);
            c3 += __shfl_down(c3, d, RL_L);
            a0 += __shfl_down(a0, d, RL_L);
            a1 += __shfl_down(a1, d, RL_L);
            a2 += __shfl_down(a2, d, RL_L);
            a3 += __shfl_down(a3, d, RL_L);
        }
        c0 = __shfl(c0, 0, RL_L), c1 = __shfl(c1, 0, RL_L), c2 = __shfl(c2, 0, RL_L), c3 = __shfl(c3, 0, RL_L);
        a0 = __shfl(a0, 0, RL_L), a1 = __shfl(a1, 0, RL_L), a2 = __shfl(a2, 0, RL_L), a3 = __shfl(a3, 0, RL_L);
        int c = 0, cc = c0; // the most matches in front, a tie to the earlier pose
        double ca = a0;
        if (c1 > cc) c = 1, cc = c1, ca = a1;
        if (c2 > cc) c = 2, cc = c2, ca = a2;
        if (c3 > cc) c = 3, cc = c3, ca = a3;
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = c < 2 ? R1[e] : R2[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) T[e] = (c & 1) ? -t[e] : t[e];
        srk_relate_essential(R, T, E);
        l0 = sqrt(best / (double)n);
        l2 = fs[SRK_RELATE_SLOT * bw + 2];
        l3 = (double)h;
        l5 = sqrt(rec[18]);
        l6 = (double)cc;
        l7 = ca / (double)cc;
    }
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            Rout[9 * i + e] = R[e];
            Eout[9 * i + e] = E[e];
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) Tout[3 * i + e] = T[e];
        double* l = related + 8 * i;
        l[0] = l0;
        l[1] = (double)n;
        l[2] = l2;
        l[3] = l3;
        l[4] = models;
        l[5] = l5;
        l[6] = l6;
        l[7] = l7;
        status[i] = n < 6 ? 1u : (bw < 0 ? 2u : 0u); // SRK_RELATE_FEW_POINTS, SRK_RELATE_NO_MODEL
    }
}

void srk_launch_relate_gather(hipStream_t s, int32_t n_pairs, const int64_t* row_ptr, const double* uv_a, const double* uv_b, const double* q,
                              double* strip, int64_t* count)
{
    if (n_pairs <= 0) return;
    const int32_t per = RL_BLOCK / RL_L;
    hipLaunchKernelGGL(k_relate_gather, dim3((unsigned)((n_pairs + per - 1) / per)), dim3(RL_BLOCK), 0, s, n_pairs, row_ptr, uv_a, uv_b, q, strip, count);
}

void srk_launch_relate_solve(hipStream_t s, int32_t n_pairs, int32_t hypotheses, uint64_t seed, double f0, const int64_t* row_ptr, const double* strip,
                             const int64_t* count, const double* K_a, const double* K_b, int shared_k, double* hyp)
{
    if (n_pairs <= 0) return;
    const int64_t per = RL_BLOCK / RL_G, n_groups = (int64_t)n_pairs * hypotheses;
    hipLaunchKernelGGL(k_relate_solve, dim3((unsigned)((n_groups + per - 1) / per)), dim3(RL_BLOCK), 0, s, n_groups, hypotheses, seed, f0, row_ptr, strip,
                       count, K_a, K_b, shared_k, hyp);
}

void srk_launch_relate_score(hipStream_t s, int32_t n_pairs, int32_t hypotheses, double tau, double f0, const int64_t* row_ptr, const double* strip,
                             const int64_t* count, const double* hyp, double* slots)
{
    if (n_pairs <= 0) return;
    const int32_t per = RL_BLOCK / RL_L, waves = (hypotheses + RL_L - 1) / RL_L;
    const int64_t n_waves = (int64_t)n_pairs * waves;
    hipLaunchKernelGGL(k_relate_score, dim3((unsigned)((n_waves + per - 1) / per)), dim3(RL_BLOCK), 0, s, n_waves, waves, hypotheses, tau * tau, f0, row_ptr,
                       strip, count, hyp, slots);
}

void srk_launch_relate_pick(hipStream_t s, int32_t n_pairs, int32_t hypotheses, double tau, double f0, const int64_t* row_ptr, const double* q,
                            const double* strip, const int64_t* count, const double* K_a, const double* K_b, int shared_k, const double* hyp,
                            const double* slots, double* R, double* T, double* E, double* related, uint32_t* status, uint8_t* inlier_out)
{
    if (n_pairs <= 0) return;
    const int32_t per = RL_BLOCK / RL_L, waves = (hypotheses + RL_L - 1) / RL_L;
    hipLaunchKernelGGL(k_relate_pick, dim3((unsigned)((n_pairs + per - 1) / per)), dim3(RL_BLOCK), 0, s, n_pairs, waves, hypotheses, tau * tau, f0, row_ptr, q,
                       strip, count, K_a, K_b, shared_k, hyp, slots, R, T, E, related, status, inlier_out);
}
