// srk_marg.hip -- marginalisation priors in information form (srk_ba_marginalization_prior), the device half.
//
// The factors that touch the marginalised landmarks P and the dropped frames D leave on the poses of the n = d + k slots (D
// first, then the kept frames K)
//     A_pose = U_F - sum_{l in P} W_l^T V_l^-1 W_l,     b_pose = u_F - sum_l W_l^T V_l^-1 g_l
// With V_l = L L^T the landmark sum is a Gram product: Z = [L^-1 W_l | L^-1 g_l] stacked over the landmarks is a tall, skinny
// strip [4 |P|][6 n + 1] and sum_l ... = Z^T Z.  k_marg_rows writes the strip from the current scene with the derivative
// kernels' own device functions (srk_jac_dev.hpp), k_marg_gram multiplies it with v_mfma_f64_16x16x4_f64, the row chunks of
// Z over the workgroups; k_marg_frame_sums and k_marg_reduce add what belongs to one slot or one entry in a fixed order.
// No atomics: the same scene gives the same bits.  Nothing here is launched by any other call.
#include "srk_marg_dev.hpp"
#include "srk_jac_dev.hpp"

typedef double double4_t __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ the strip
// the sum of v over the wave, the same bits in every lane (a + b and b + a are the same number)
__device__ __forceinline__ double mg_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// observation o of a landmark at X: geometry, the weight folded into s1, s2 as the derivative kernels fold it
template <bool ROBUST>
__device__ __forceinline__ double mg_obs(const double* __restrict__ c, const double X[3], double2 uv, const SrkLoss& loss, int64_t o, ObsGeom& g)
{
    obs_pqr(c, X[0], X[1], X[2], uv.x, uv.y, g);
    double w = 1.0;
    if constexpr (ROBUST) {
        double rho;
        srk_robust_wr(g.ex, g.ey, loss, srk_info(loss.q, o), w, rho);
        g.s1 *= w;
        g.s2 *= w;
    }
    return w;
}

template <bool ROBUST>
__global__ __launch_bounds__(256) void k_marg_rows(SrkDims d, const double* __restrict__ pts, const double* __restrict__ cam,
                                                   const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ obs_frame,
                                                   const double* __restrict__ obs_uv, SrkLoss loss, SrkMargTables a,
                                                   double* __restrict__ Z, double* __restrict__ stage, int32_t* __restrict__ skipped)
{
    const int lane = threadIdx.x & 63;
    const int64_t l = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= a.n_lm) return; // (a whole wave; the kernel has no workgroup barrier)
    const int64_t i = a.lm[l], o0 = row_ptr[i], o1 = row_ptr[i + 1];
    const double X[3] = { pts[3 * i], pts[3 * i + 1], pts[3 * i + 2] };
    // V_l (00 01 02 11 12 22) and g_l: the lanes' sums over their observations, then the wave's
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0;
    for (int64_t o = o0 + lane; o < o1; o += 64) {
        const double* c = cam + (int64_t)SRK_CAM_PACK * obs_frame[o];
        ObsGeom g;
        mg_obs<ROBUST>(c, X, reinterpret_cast<const double2*>(obs_uv)[o], loss, o, g);
        double Ap[3], Bp[3];
        point_ab(c, g, Ap, Bp);
        acc[0] += (Ap[0] * Ap[0] + Bp[0] * Bp[0]) * g.s2;
        acc[1] += (Ap[0] * Ap[1] + Bp[0] * Bp[1]) * g.s2;
        acc[2] += (Ap[0] * Ap[2] + Bp[0] * Bp[2]) * g.s2;
        acc[3] += (Ap[1] * Ap[1] + Bp[1] * Bp[1]) * g.s2;
        acc[4] += (Ap[1] * Ap[2] + Bp[1] * Bp[2]) * g.s2;
        acc[5] += (Ap[2] * Ap[2] + Bp[2] * Bp[2]) * g.s2;
        acc[6] += (g.ex * Ap[0] + g.ey * Bp[0]) * g.s1;
        acc[7] += (g.ex * Ap[1] + g.ey * Bp[1]) * g.s1;
        acc[8] += (g.ex * Ap[2] + g.ey * Bp[2]) * g.s1;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = mg_wave_sum(acc[k]);
    const int32_t pr = a.lm_prior[l];
    if (pr >= 0) { // 2 L into the block, 2 L (X - Xbar) into the gradient (k_prior_add)
        const int64_t n = a.n_priors;
        double dx[3], Lp[6];
#pragma unroll
        for (int e = 0; e < 3; ++e) dx[e] = X[e] - a.prior_val[e * n + pr];
#pragma unroll
        for (int e = 0; e < 6; ++e) Lp[e] = a.prior_val[(3 + e) * n + pr];
#pragma unroll
        for (int e = 0; e < 6; ++e) acc[e] += 2.0 * Lp[e];
        acc[6] += 2.0 * (Lp[0] * dx[0] + Lp[1] * dx[1] + Lp[2] * dx[2]);
        acc[7] += 2.0 * (Lp[1] * dx[0] + Lp[3] * dx[1] + Lp[4] * dx[2]);
        acc[8] += 2.0 * (Lp[2] * dx[0] + Lp[4] * dx[1] + Lp[5] * dx[2]);
    }
    // V = L L^T, undamped: the determinant test of the Schur passes, then the pivots (point_block_cholesky)
    const double e00 = acc[0], e01 = acc[1], e02 = acc[2], e11 = acc[3], e12 = acc[4], e22 = acc[5];
    const double det = e00 * (e11 * e22 - e12 * e12) + e01 * (e12 * e02 - e01 * e22) + e02 * (e01 * e12 - e11 * e02);
    const double l00 = sqrt(e00), i0 = 1 / l00;
    const double l10 = e01 * i0, l20 = e02 * i0;
    const double d1 = e11 - l10 * l10;
    const double l11 = sqrt(d1), i1 = 1 / l11;
    const double l21 = (e12 - l20 * l10) * i1;
    const double d2 = e22 - l20 * l20 - l21 * l21;
    const double l22 = sqrt(d2), i2 = 1 / l22;
    if (!(fabs(det) > 1e-12) || !(e00 > 0 && d1 > 0 && d2 > 0) || !isfinite(i0) || !isfinite(i1) || !isfinite(i2)) {
        if (lane == 0) skipped[l] = 1;
        return;
    }
    const double I10 = -l10 * i0 * i1, I21 = -l21 * i1 * i2, I20 = -(l20 * i0 + l21 * I10) * i2;
    const int32_t ncols = 6 * a.n_slots;
    double* zr = Z + (int64_t)SRK_MARG_ROWS * l * a.ldz;
    if (lane == 0) {
        zr[ncols] = i0 * acc[6];
        zr[a.ldz + ncols] = I10 * acc[6] + i1 * acc[7];
        zr[2 * a.ldz + ncols] = I20 * acc[6] + I21 * acc[7] + i2 * acc[8];
    }
    for (int64_t o = o0 + lane; o < o1; o += 64) {
        const int32_t f = obs_frame[o];
        const int32_t slot = a.frame_slot[f];
        const double* c = cam + (int64_t)SRK_CAM_PACK * f;
        ObsGeom g;
        const double w = mg_obs<ROBUST>(c, X, reinterpret_cast<const double2*>(obs_uv)[o], loss, o, g);
        if (w == 0.0 || slot < 0 || slot >= a.n_slots) continue; // a switched-off observation touches nothing
        double Ap[3], Bp[3], Af[10], Bf[10];
        point_ab(c, g, Ap, Bp);
        frame_ab(c, g, X[0], X[1], X[2], Af, Bf);
        double* z0 = zr + 6 * slot;
#pragma unroll
        for (int v = 0; v < 6; ++v) { // column v of W_o = (Ap Af^T + Bp Bf^T) s2 over the pose variables, then L^-1 W_o
            const double w0 = (Ap[0] * Af[4 + v] + Bp[0] * Bf[4 + v]) * g.s2;
            const double w1 = (Ap[1] * Af[4 + v] + Bp[1] * Bf[4 + v]) * g.s2;
            const double w2 = (Ap[2] * Af[4 + v] + Bp[2] * Bf[4 + v]) * g.s2;
            z0[v] = i0 * w0;
            z0[a.ldz + v] = I10 * w0 + i1 * w1;
            z0[2 * a.ldz + v] = I20 * w0 + I21 * w1 + i2 * w2;
        }
        double* st = stage + (a.lm_stage[l] + (o - o0)) * SRK_MARG_STAGE;
        int idx = 0;
#pragma unroll
        for (int v1 = 4; v1 < 10; ++v1)
#pragma unroll
            for (int v2 = v1; v2 < 10; ++v2) st[idx++] = (Af[v1] * Af[v2] + Bf[v1] * Bf[v2]) * g.s2;
#pragma unroll
        for (int v = 4; v < 10; ++v) st[17 + v] = (g.ex * Af[v] + g.ey * Bf[v]) * g.s1;
    }
}

void srk_launch_marg_rows(hipStream_t s, const SrkDims& d, const double* pts, const double* cam, const int64_t* row_ptr,
                          const int32_t* obs_frame, const double* obs_uv, const SrkLoss* loss, const SrkMargTables& t, double* Z,
                          double* stage, int32_t* skipped)
{
    if (t.n_lm <= 0) return;
    const dim3 grid((unsigned)((t.n_lm + 3) / 4)), block(256);
    if (loss && (loss->kind != SRK_LOSS_NONE || loss->q != nullptr))
        hipLaunchKernelGGL((k_marg_rows<true>), grid, block, 0, s, d, pts, cam, row_ptr, obs_frame, obs_uv, *loss, t, Z, stage, skipped);
    else
        hipLaunchKernelGGL((k_marg_rows<false>), grid, block, 0, s, d, pts, cam, row_ptr, obs_frame, obs_uv, SrkLoss{}, t, Z, stage, skipped);
}

// ------------------------------------------------------------------ the frames' own sums
// one workgroup per slot: thread t takes entry t & 31 of the staging rows slot_ptr + (t >> 5), + 8, ...; the eight partial sums
// of an entry are added in their order
__global__ __launch_bounds__(256) void k_marg_frame_sums(SrkMargTables a, const double* __restrict__ stage, double* __restrict__ Us)
{
    __shared__ double red[8][32];
    const int t = threadIdx.x, e = t & 31, c = t >> 5;
    const int32_t s = blockIdx.x;
    double v = 0;
    if (e < 27)
        for (int32_t p = a.slot_ptr[s] + c; p < a.slot_ptr[s + 1]; p += 8) v += stage[a.slot_ent[p] * SRK_MARG_STAGE + e];
    red[c][e] = v;
    __syncthreads();
    if (t < 27) Us[s * 27 + t] = ((red[0][t] + red[1][t]) + (red[2][t] + red[3][t])) + ((red[4][t] + red[5][t]) + (red[6][t] + red[7][t]));
}

void srk_launch_marg_frame_sums(hipStream_t s, const SrkMargTables& t, const double* stage, double* Us)
{
    if (t.n_slots <= 0) return;
    hipLaunchKernelGGL(k_marg_frame_sums, dim3((unsigned)t.n_slots), dim3(256), 0, s, t, stage, Us);
}

// ------------------------------------------------------------------ G = Z^T Z
// Workgroup (x, y): the rows [x rows_per_chunk, (x + 1) rows_per_chunk) of Z and tile row y of the lower block triangle of G,
// that is the 16 x 16 tiles (y, 0 .. y).  Four waves; wave w owns the tiles (y, w), (y, w + 4), (y, w + 8), (y, w + 12), one
// accumulator of v_mfma_f64_16x16x4_f64 each (the operand maps documented at k_cov_fwd: a = A[lane & 15][lane >> 4],
// b = B[lane & 15][lane >> 4], accumulator register reg = C[(lane >> 4) + 4 reg][lane & 15]).  Both operands are columns of Z read
// along its rows, so they come from the same LDS image of MG_KC rows: a = sZ[4 kk + (lane >> 4)][16 y + (lane & 15)].  A 32-lane
// half of a ds_read_b64 takes 16 consecutive doubles of two neighbouring rows: with a row stride of 16 (mod 32) doubles the two
// rows fall on the two halves of the 64 banks, conflict-free.  The rows ascend and the MFMA accumulates along them in order.
#define MG_KC 16
#define MG_LDS (SRK_MARG_LDZ_HOST + 16)
static_assert(MG_LDS % 32 == 16, "row stride of the LDS image: 16 (mod 32) doubles");

__global__ __launch_bounds__(256) void k_marg_gram(const double* __restrict__ Z, int64_t n_rows, int32_t ldz, int64_t rows_per_chunk,
                                                   double* __restrict__ part)
{
    __shared__ double sZ[MG_KC][MG_LDS];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int ti = blockIdx.y, ncol = 16 * (ti + 1);
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_chunk, r1 = r0 + rows_per_chunk < n_rows ? r0 + rows_per_chunk : n_rows;
    double4_t acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[s] = (double4_t){ 0, 0, 0, 0 };
    for (int64_t rb = r0; rb < r1; rb += MG_KC) {
        __syncthreads(); // the previous rows are consumed
        for (int e = t; e < MG_KC * ncol; e += 256) {
            const int r = e / ncol, c = e - r * ncol;
            sZ[r][c] = rb + r < r1 ? Z[(rb + r) * ldz + c] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < MG_KC / 4; ++kk) {
            const double av = sZ[4 * kk + lk][16 * ti + lr];
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if (wv + 4 * s <= ti) // (the same for every lane of the wave)
                    acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, sZ[4 * kk + lk][16 * (wv + 4 * s) + lr], acc[s], 0, 0, 0);
        }
    }
    double* out = part + (int64_t)blockIdx.x * ldz * ldz;
#pragma unroll
    for (int s = 0; s < 4; ++s)
        if (wv + 4 * s <= ti)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) out[(int64_t)(16 * ti + lk + 4 * reg) * ldz + 16 * (wv + 4 * s) + lr] = acc[s][reg];
}

void srk_launch_marg_gram(hipStream_t s, const double* Z, int64_t n_rows, int32_t ldz, int32_t n_chunks, int64_t rows_per_chunk, double* part)
{
    if (n_chunks <= 0 || ldz <= 0 || ldz > SRK_MARG_LDZ_HOST || ldz % 16) return;
    hipLaunchKernelGGL(k_marg_gram, dim3((unsigned)n_chunks, (unsigned)(ldz / 16)), dim3(256), 0, s, Z, n_rows, ldz, rows_per_chunk, part);
}

// ------------------------------------------------------------------ A = (U_F - G) / 2, b = (u_F - Z^T z) / 2
// one thread per entry (i, j <= i) of the lower triangle, row 6 n (the products with the last column of Z) included
__global__ __launch_bounds__(256) void k_marg_reduce(const double* __restrict__ part, int32_t n_chunks, int32_t ldz, int32_t ncols,
                                                     const double* __restrict__ Us, double* __restrict__ A, double* __restrict__ b)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int32_t i = (int32_t)(idx / ncols), j = (int32_t)(idx - (int64_t)i * ncols);
    if (i > ncols || j > i) return;
    double g = 0;
    for (int32_t c = 0; c < n_chunks; ++c) g += part[(int64_t)c * ldz * ldz + (int64_t)i * ldz + j];
    if (i == ncols) {
        b[j] = 0.5 * (Us[(j / 6) * 27 + 21 + j % 6] - g);
        return;
    }
    double u = 0;
    if (i / 6 == j / 6) {
        const int lo = j % 6, hi = i % 6; // entry (lo, hi) of the upper triangle, row by row
        u = Us[(i / 6) * 27 + 6 * lo - lo * (lo - 1) / 2 + hi - lo];
    }
    const double v = 0.5 * (u - g);
    A[(int64_t)i * ncols + j] = v;
    A[(int64_t)j * ncols + i] = v;
}

void srk_launch_marg_reduce(hipStream_t s, const double* part, int32_t n_chunks, int32_t ldz, int32_t n_slots, const double* Us, double* A,
                            double* b)
{
    const int32_t ncols = 6 * n_slots;
    if (ncols <= 0) return;
    const int64_t n = (int64_t)(ncols + 1) * ncols;
    hipLaunchKernelGGL(k_marg_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, n_chunks, ldz, ncols, Us, A, b);
}
