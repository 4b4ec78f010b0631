// srk_cov.hip -- marginal covariances of frames and landmarks after a solve (srk_ba_phase_covariance).
//
// H = [[V, W], [W^T, U]] is the Gauss-Newton Hessian the LM loop builds, S = L L^T its Schur complement onto the frame
// variables, factorised by the single-chain solver (srk_chol.hip): the strictly lower 64 x 64 tiles of L in S, the inverses of
// the diagonal tiles in dinv.
//   frame j:     (H^-1)_jj = Y^T Y,            Y = L^-1 E_j   (E_j: the unit columns of the frame's variables)
//   landmark i:  (H^-1)_ii = V^-1 + Z^T Z,     Z = L^-1 B_i   (B_i: rows W_o^T V^-1 at the frames of its observations)
// One primitive serves both: a forward substitution with many right-hand sides (k_cov_fwd), fed by k_cov_rhs and followed
// by the small Gram products of k_cov_gram.  A workgroup of k_cov_fwd owns SRK_COV_CB columns from the first tile row to the
// last and reads nothing but L and the rows it wrote itself: no flags, no spins, no atomics, a fixed summation order.
// Variables that do not move (gauge, constant frames, padding) get no unit column and no row of B: S holds identity rows
// there, so every entry of their rows and columns comes out as an exact zero.
// Cross-covariances (srk_ba_phase_cross_covariance; section 17) are products between two column groups of the same Y:
// frame a, frame b: Y_a^T Y_b; landmark i, frame j: -Z_i^T Y_j; landmark i, landmark k: Z_i^T Z_k (k_cov_cross, at the end).
#include "srk_cov.hpp"

typedef double double4_t __attribute__((ext_vector_type(4)));

#define CV_NB 64
#define CV_LDSP (CV_NB + 2) // padded LDS row: conflict-free ds_read_b64 for the MFMA operand map (as in srk_chol.hip)

// plane of Af[fv] / Bf[fv] of the stored rank-2 factors (srk_dev.hpp: SRK_WF_*), or -1 where the factor is structurally zero
__device__ __forceinline__ int cv_af_plane(int fv) { return fv >= 4 ? SRK_WF_AF4 + fv - 4 : (fv == 0 ? SRK_WF_AF0 : (fv == 2 ? SRK_WF_G : -1)); }
__device__ __forceinline__ int cv_bf_plane(int fv) { return fv >= 4 ? SRK_WF_BF4 + fv - 4 : (fv == 1 ? SRK_WF_BF1 : (fv == 3 ? SRK_WF_G : -1)); }

// inverse of the damped 3 x 3 landmark block E = V with diagonal * (1 + c), as its six distinct entries
// { 00, 01, 02, 11, 12, 22 }; the determinant test is the one of the Schur and back-substitution passes
__device__ __forceinline__ bool cv_point_inverse(const double* __restrict__ Vg, int64_t Ns, int64_t pt, double c, double inv[6])
{
    const double e00 = Vg[0 * Ns + pt] * (1 + c), e01 = Vg[1 * Ns + pt], e02 = Vg[2 * Ns + pt];
    const double e11 = Vg[3 * Ns + pt] * (1 + c), e12 = Vg[4 * Ns + pt], e22 = Vg[5 * Ns + pt] * (1 + c);
    const double c00 = e11 * e22 - e12 * e12;
    const double c01 = e12 * e02 - e01 * e22;
    const double c02 = e01 * e12 - e11 * e02;
    const double det = e00 * c00 + e01 * c01 + e02 * c02;
    if (!(fabs(det) > 1e-12)) return false;
    const double id = 1 / det;
    inv[0] = c00 * id;
    inv[1] = c01 * id;
    inv[2] = c02 * id;
    inv[3] = (e00 * e22 - e02 * e02) * id;
    inv[4] = (e01 * e02 - e00 * e12) * id;
    inv[5] = (e00 * e11 - e01 * e01) * id;
    return true;
}

// ------------------------------------------------------------------ right-hand sides
// one workgroup of 64 threads per selected block
template <typename WT, int FV>
__global__ __launch_bounds__(64) void k_cov_rhs(SrkDims d, double c, const SrkCovGroup* __restrict__ grp, const int64_t* __restrict__ row_ptr,
                                                const int32_t* __restrict__ obs_frame, const WT* __restrict__ W,
                                                const double* __restrict__ Vg, const uint8_t* __restrict__ free_var,
                                                double* __restrict__ Y, int64_t ncp, int* __restrict__ info)
{
    const SrkCovGroup g = grp[blockIdx.x];
    const int t = threadIdx.x;
    if (!g.is_point) {
        if (t < FV) {
            const int64_t var = FV * g.idx + t;
            if (free_var[var]) Y[var * ncp + g.col0 + t] = 1.0;
        }
        return;
    }
    double iv[6];
    if (!cv_point_inverse(Vg, d.Ns, g.idx, c, iv)) {
        if (t == 0) atomicOr(info, 1);
        return;
    }
    const double Vi[3][3] = { { iv[0], iv[1], iv[2] }, { iv[1], iv[3], iv[4] }, { iv[2], iv[4], iv[5] } };
    const int64_t r0 = row_ptr[g.idx], nobs = row_ptr[g.idx + 1] - r0;
    constexpr int off = 10 - FV; // FV = 6: the frame variables are [Tx Ty Tz Wx Wy Wz], variables 4..9 of the full layout
    for (int64_t e = t; e < nobs * FV; e += 64) {
        const int64_t o = r0 + e / FV;
        const int v = (int)(e % FV);
        const int64_t var = FV * (int64_t)obs_frame[o] + v;
        if (!free_var[var]) continue;
        const int pa = cv_af_plane(v + off), pb = cv_bf_plane(v + off);
        const double af = pa >= 0 ? (double)W[(int64_t)pa * d.Os + o] : 0.0, bf = pb >= 0 ? (double)W[(int64_t)pb * d.Os + o] : 0.0;
        double w[3]; // column v of W_o: W[pv][v] = Ap[pv] Af[v] + Bp[pv] Bf[v]
#pragma unroll
        for (int pv = 0; pv < 3; ++pv)
            w[pv] = (double)W[(int64_t)(SRK_WF_AP + pv) * d.Os + o] * af + (double)W[(int64_t)(SRK_WF_BP + pv) * d.Os + o] * bf;
#pragma unroll
        for (int a = 0; a < 3; ++a) Y[var * ncp + g.col0 + a] = (w[0] * Vi[0][a] + w[1] * Vi[1][a]) + w[2] * Vi[2][a];
    }
}

void srk_launch_cov_rhs(hipStream_t s, const SrkDims& d, double c, const SrkCovGroup* grp, int32_t n_grp, const int64_t* row_ptr,
                        const int32_t* obs_frame, const double* W, const double* Vg, const uint8_t* free_var, double* Y, int64_t ncp,
                        int* info)
{
    if (n_grp <= 0) return;
    const dim3 grid((unsigned)n_grp), block(64);
    if (d.w_f32) {
        const float* Wf = reinterpret_cast<const float*>(W);
        if (d.fv == 6) hipLaunchKernelGGL((k_cov_rhs<float, 6>), grid, block, 0, s, d, c, grp, row_ptr, obs_frame, Wf, Vg, free_var, Y, ncp, info);
        else hipLaunchKernelGGL((k_cov_rhs<float, 10>), grid, block, 0, s, d, c, grp, row_ptr, obs_frame, Wf, Vg, free_var, Y, ncp, info);
    } else {
        if (d.fv == 6) hipLaunchKernelGGL((k_cov_rhs<double, 6>), grid, block, 0, s, d, c, grp, row_ptr, obs_frame, W, Vg, free_var, Y, ncp, info);
        else hipLaunchKernelGGL((k_cov_rhs<double, 10>), grid, block, 0, s, d, c, grp, row_ptr, obs_frame, W, Vg, free_var, Y, ncp, info);
    }
}

// ------------------------------------------------------------------ forward substitution with many right-hand sides
// Workgroup b owns the columns [64 b, 64 b + 64) of Y and walks the tile rows d = blk_first[b] .. n_tiles - 1:
//     Y_d = Dinv_d (B_d - sum_{j < d} L_dj Y_j),   j from max(col_begin[d] / 64, blk_first[b])   (everything left of it is zero)
// Four waves; wave w owns the rows [16 w, 16 w + 16) of the 64 x 64 result, four 16 x 16 accumulators of
// v_mfma_f64_16x16x4_f64 (a = A[lane & 15][lane >> 4], b = B[lane & 15][lane >> 4], accumulator register
// reg = C[(lane >> 4) + 4 reg][lane & 15]).  The left operand is a tile of L (or Dinv_d) as it lies in memory, sA[row][k]; the
// right operand is the tile of Y TRANSPOSED in LDS, sB[column][k], so both are read along k.  The rows a workgroup reads
// back from Y are rows it stored itself, behind a workgroup barrier; L and dinv are only read.  j ascends and the MFMA
// accumulates along k in order: the same L gives the same bits.
__global__ __launch_bounds__(256) void k_cov_fwd(int64_t ld, const double* __restrict__ L, const double* __restrict__ dinv,
                                                 const int64_t* __restrict__ col_begin, int n_tiles, const int32_t* __restrict__ blk_first,
                                                 double* Y, int64_t ncp)
{
    __shared__ double sA[CV_NB][CV_LDSP];
    __shared__ double sB[CV_NB][CV_LDSP];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int64_t c0 = (int64_t)blockIdx.x * SRK_COV_CB;
    const int d0 = blk_first[blockIdx.x];
    for (int dt = d0; dt < n_tiles; ++dt) {
        double4_t acc[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = (double4_t){ 0, 0, 0, 0 };
        int jb = (int)(col_begin[dt] / CV_NB);
        if (jb < d0) jb = d0;
        for (int j = jb; j < dt; ++j) {
            __syncthreads(); // the previous tile's operands are consumed; the rows of Y stored so far are visible
#pragma unroll 4
            for (int i = 0; i < 16; ++i) {
                const int e = t + 256 * i, r = e >> 6, k = e & 63;
                sA[r][k] = L[((int64_t)CV_NB * dt + r) * ld + (int64_t)CV_NB * j + k];
                sB[k][r] = Y[((int64_t)CV_NB * j + r) * ncp + c0 + k];
            }
            __syncthreads();
#pragma unroll 4
            for (int kk = 0; kk < CV_NB / 4; ++kk) {
                const double a = sA[16 * wv + lr][4 * kk + lk];
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sB[16 * s + lr][4 * kk + lk], acc[s], 0, 0, 0);
            }
        }
        __syncthreads();
        // T = B_d - sum (transposed into sB), Dinv_d into sA
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const int e = t + 256 * i, r = e >> 6, k = e & 63;
            sA[r][k] = dinv[(int64_t)dt * CV_NB * CV_NB + r * CV_NB + k];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int m = 16 * wv + lk + 4 * reg, n = 16 * s + lr;
                sB[n][m] = Y[((int64_t)CV_NB * dt + m) * ncp + c0 + n] - acc[s][reg];
            }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = (double4_t){ 0, 0, 0, 0 };
        for (int kk = 0; kk < 4 * (wv + 1); ++kk) { // Dinv_d is lower triangular: the rows of wave w end at column 16 w + 15
            const double a = sA[16 * wv + lr][4 * kk + lk];
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sB[16 * s + lr][4 * kk + lk], acc[s], 0, 0, 0);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int m = 16 * wv + lk + 4 * reg, n = 16 * s + lr;
                Y[((int64_t)CV_NB * dt + m) * ncp + c0 + n] = acc[s][reg];
            }
    }
}

void srk_launch_cov_fwd(hipStream_t s, int64_t ld, const double* L, const double* dinv, const int64_t* col_begin, int32_t n_tiles,
                        const int32_t* blk_first, double* Y, int64_t ncp)
{
    if (ncp <= 0) return;
    hipLaunchKernelGGL(k_cov_fwd, dim3((unsigned)(ncp / SRK_COV_CB)), dim3(256), 0, s, ld, L, dinv, col_begin, (int)n_tiles, blk_first, Y, ncp);
}

// ------------------------------------------------------------------ Gram products
// one workgroup per selected block: thread t sums the rows first_row + t, + 256, ... of the g (g + 1) / 2 products, the 64
// partial sums of a wave are combined by a shuffle tree and the four waves' sums in wave order: a fixed order
__global__ __launch_bounds__(256) void k_cov_gram(SrkDims d, double c, const SrkCovGroup* __restrict__ grp, const double* __restrict__ Vg,
                                                  const double* __restrict__ Y, int64_t ncp, int64_t n_rows, double* __restrict__ out)
{
    __shared__ double sp[4][55];
    const SrkCovGroup g = grp[blockIdx.x];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int n = g.ncols;
    double acc[55];
#pragma unroll
    for (int p = 0; p < 55; ++p) acc[p] = 0;
    for (int64_t r = g.first_row + t; r < n_rows; r += 256) {
        const double* yr = Y + r * ncp + g.col0;
        double y[10];
#pragma unroll
        for (int a = 0; a < 10; ++a) y[a] = a < n ? yr[a] : 0.0;
        int p = 0;
#pragma unroll
        for (int a = 0; a < 10; ++a)
#pragma unroll
            for (int b = a; b < 10; ++b, ++p) acc[p] = fma(y[a], y[b], acc[p]);
    }
#pragma unroll
    for (int p = 0; p < 55; ++p) {
        double v = acc[p];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) sp[wv][p] = v;
    }
    __syncthreads();
    if (t < 55) {
        // pair index p of the 10-wide enumeration -> (a, b)
        int a = 0, rem = t;
        while (rem >= 10 - a) { rem -= 10 - a; ++a; }
        const int b = a + rem;
        if (b < n) {
            double v = (sp[0][t] + sp[1][t]) + (sp[2][t] + sp[3][t]);
            if (g.is_point) {
                double iv[6];
                if (cv_point_inverse(Vg, d.Ns, g.idx, c, iv)) v += iv[a == 0 ? b : (a == 1 ? 2 + b : 5)];
            }
            double* o = out + (int64_t)blockIdx.x * 100;
            o[a * n + b] = v;
            o[b * n + a] = v;
        }
    }
}

void srk_launch_cov_gram(hipStream_t s, const SrkDims& d, double c, const SrkCovGroup* grp, int32_t n_grp, const double* Vg,
                         const double* Y, int64_t ncp, int64_t n_rows, double* out)
{
    if (n_grp <= 0) return;
    hipLaunchKernelGGL(k_cov_gram, dim3((unsigned)n_grp), dim3(256), 0, s, d, c, grp, Vg, Y, ncp, n_rows, out);
}

// ------------------------------------------------------------------ cross products between two blocks
// one workgroup per pair (p, q) of column groups of the same Y: the NP x NQ product Y_p^T Y_q over the rows
// [max(first_row_p, first_row_q), n_rows) -- above that row one of the two groups holds exact zeros.  The summation scheme is
// k_cov_gram's (thread t the rows r0 + t, + 256, ...; one fma per product; a shuffle tree per wave; the four waves' sums as
// k_cov_gram adds them), so a pair (p, p) gives the bits of the marginal block and (q, p) the transpose of (p, q).  One
// instantiation per shape keeps the NP NQ accumulators in registers.  A landmark x frame block is negated
// ((H^-1)_ij = -Z_i^T Y_j); a landmark with itself adds V^-1.
template <int NP, int NQ>
__global__ __launch_bounds__(256) void k_cov_cross(SrkDims d, double c, const SrkCovGroup* __restrict__ grp, const SrkCovPair* __restrict__ pairs,
                                                   const double* __restrict__ Vg, const double* __restrict__ Y, int64_t ncp, int64_t n_rows,
                                                   double* __restrict__ out)
{
    __shared__ double sp[4][NP * NQ];
    const SrkCovPair pr = pairs[blockIdx.x];
    const SrkCovGroup gp = grp[pr.p], gq = grp[pr.q];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    double acc[NP * NQ];
#pragma unroll
    for (int e = 0; e < NP * NQ; ++e) acc[e] = 0;
    const int64_t r0 = gp.first_row > gq.first_row ? gp.first_row : gq.first_row;
    for (int64_t r = r0 + t; r < n_rows; r += 256) {
        const double* yp = Y + r * ncp + gp.col0;
        const double* yq = Y + r * ncp + gq.col0;
        double a[NP], b[NQ];
#pragma unroll
        for (int i = 0; i < NP; ++i) a[i] = yp[i];
#pragma unroll
        for (int j = 0; j < NQ; ++j) b[j] = yq[j];
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
            for (int j = 0; j < NQ; ++j) acc[i * NQ + j] = fma(a[i], b[j], acc[i * NQ + j]);
    }
#pragma unroll
    for (int e = 0; e < NP * NQ; ++e) {
        double v = acc[e];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) sp[wv][e] = v;
    }
    __syncthreads();
    if (t < NP * NQ) {
        const int i = t / NQ, j = t % NQ;
        double v = (sp[0][t] + sp[1][t]) + (sp[2][t] + sp[3][t]);
        if (NP == 3 && NQ == 3 && pr.p == pr.q) {
            double iv[6];
            const int lo = i < j ? i : j, hi = i < j ? j : i;
            if (cv_point_inverse(Vg, d.Ns, gp.idx, c, iv)) v += iv[lo == 0 ? hi : (lo == 1 ? 2 + hi : 5)];
        }
        if (NP == 3 && NQ != 3) v = -v;
        out[(int64_t)blockIdx.x * 100 + t] = v;
    }
}

template <int NP, int NQ>
static void cov_cross_launch(hipStream_t s, const SrkDims& d, double c, const SrkCovGroup* grp, const SrkCovPair* pairs, int32_t n, const double* Vg,
                             const double* Y, int64_t ncp, int64_t n_rows, double* out)
{
    if (n <= 0) return;
    hipLaunchKernelGGL((k_cov_cross<NP, NQ>), dim3((unsigned)n), dim3(256), 0, s, d, c, grp, pairs, Vg, Y, ncp, n_rows, out);
}

void srk_launch_cov_cross(hipStream_t s, const SrkDims& d, double c, const SrkCovGroup* grp, const SrkCovPair* pairs, int32_t n_ff, int32_t n_pf,
                          int32_t n_pp, const double* Vg, const double* Y, int64_t ncp, int64_t n_rows, double* out)
{
    if (d.fv == 6) {
        cov_cross_launch<6, 6>(s, d, c, grp, pairs, n_ff, Vg, Y, ncp, n_rows, out);
        cov_cross_launch<3, 6>(s, d, c, grp, pairs + n_ff, n_pf, Vg, Y, ncp, n_rows, out + 100 * (int64_t)n_ff);
    } else {
        cov_cross_launch<10, 10>(s, d, c, grp, pairs, n_ff, Vg, Y, ncp, n_rows, out);
        cov_cross_launch<3, 10>(s, d, c, grp, pairs + n_ff, n_pf, Vg, Y, ncp, n_rows, out + 100 * (int64_t)n_ff);
    }
    cov_cross_launch<3, 3>(s, d, c, grp, pairs + n_ff + n_pf, n_pp, Vg, Y, ncp, n_rows, out + 100 * ((int64_t)n_ff + n_pf));
}
