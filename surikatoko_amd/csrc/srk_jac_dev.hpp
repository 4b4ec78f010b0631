// srk_jac_dev.hpp -- the per-observation device functions of the derivative kernels (srk_ba_kernels.hip): the geometry of one
// observation, its robust / information weight and the closed-form A, B vectors of the landmark and frame variables.  They live
// here so that srk_marg.hip recomputes an observation's blocks with the very functions k_jac_* use.
#pragma once
#include "srk_dev.hpp"

// ------------------------------------------------------------------ per-observation geometry
struct ObsGeom {
    double p, q, r;
    double ex, ey;    // p/r - u/f0 , q/r - v/f0
    double s1, s2;    // 2/r^2 , 2/r^4
};

__device__ __forceinline__ void obs_pqr(const double* __restrict__ c, double X0, double X1, double X2, double u,
                                        double v, ObsGeom& g)
{
    double xc0 = c[0] * X0 + c[1] * X1 + c[2] * X2 + c[9];
    double xc1 = c[3] * X0 + c[4] * X1 + c[5] * X2 + c[10];
    double xc2 = c[6] * X0 + c[7] * X1 + c[8] * X2 + c[11];
    g.p = c[12] * xc0 + c[13] * xc1 + c[14] * xc2;
    g.q = c[15] * xc0 + c[16] * xc1 + c[17] * xc2;
    g.r = c[18] * xc0 + c[19] * xc1 + c[20] * xc2;
    // one IEEE reciprocal; p/r, q/r, 2/r^2, 2/r^4 and u/f0 become multiplies (<= 1-2 ulp from the divided forms)
    double ir = 1.0 / g.r;
    double if0 = c[46];
    g.ex = g.p * ir - u * if0;
    g.ey = g.q * ir - v * if0;
    double ir2 = ir * ir;
    g.s1 = 2 * ir2;
    g.s2 = g.s1 * ir2;
}

// (w, rho) of one observation from its residual: s = ex^2 + ey^2, rho(s) its term of the objective, w = rho'(s) its IRLS
// weight.  Every robust kernel that forms an observation's contribution calls this once, so V, U, W and the gradient all
// see the same w.  Below the threshold (Huber s <= d^2) w is exactly 1 and rho is s itself: the kernels fold w (and
// sqrt(w)) into scale factors they multiply anyway, and a multiply by 1.0 is exact, so a threshold above every residual
// reproduces the plain kernels' values bit for bit.
__device__ __forceinline__ void srk_rho_w(double s, const SrkLoss& L, double& w, double& rho)
{
    w = 1.0;
    rho = s;
    if (L.kind == SRK_LOSS_HUBER) {
        if (s > L.d2) {
            const double rs = sqrt(s);
            w = L.d / rs;
            rho = 2.0 * L.d * rs - L.d2;
        }
    } else if (L.kind == SRK_LOSS_CAUCHY) {
        const double t = s / L.d2;
        w = 1.0 / (1.0 + t);
        rho = L.d2 * log1p(t);
    }
}

// ---- per-observation information (srk_ba_set_observation_information): observation o carries q_o >= 0,
// its whitened squared residual is q s, its term of the objective rho(q s) and its weight in the normal equations
// w_eff = q rho'(q s).  The robust instantiations read q from SrkLoss::q (internal observation order; k_jac_frames from
// SrkLoss::qf, the frame-major order); a null pointer is q = 1.  Kind SRK_LOSS_NONE with a pointer is a valid robust-side
// instantiation: rho the identity, w_eff = q.  The kernels use w_eff exactly where they used w, so q = 1 changes no bit
// (1.0 * s and 1.0 * w are exact) and q = 0 gives exact zeros: sqrt(0) on the stored factors, 0 on the sums.
__device__ __forceinline__ double srk_info(const double* __restrict__ q, int64_t o) { return q ? q[o] : 1.0; }
__device__ __forceinline__ void srk_robust_wr(double ex, double ey, const SrkLoss& L, double qi, double& w, double& rho)
{
    srk_rho_w(qi * (ex * ex + ey * ey), L, w, rho);
    w *= qi;
}

// A_v = r p'_v - p r'_v , B_v = r q'_v - q r'_v for the three landmark variables (:1450-1455)
__device__ __forceinline__ void point_ab(const double* __restrict__ c, const ObsGeom& g, double A[3], double B[3])
{
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        double gp = c[21 + v], gq = c[24 + v], gr = c[27 + v];
        A[v] = g.r * gp - g.p * gr;
        B[v] = g.r * gq - g.q * gr;
    }
}

// the ten frame variables [fx fy u0 v0 Tx Ty Tz Wx Wy Wz] (:1457-1525)
__device__ __forceinline__ void frame_ab(const double* __restrict__ c, const ObsGeom& g, double X0, double X1,
                                         double X2, double A[10], double B[10])
{
    double gp_fx = c[42] * g.p - c[43] * g.r;
    double gq_fy = c[44] * g.q - c[45] * g.r;
    double g_uv = c[46] * g.r;
    A[0] = g.r * gp_fx; B[0] = 0;
    A[1] = 0;           B[1] = g.r * gq_fy;
    A[2] = g.r * g_uv;  B[2] = 0;
    A[3] = 0;           B[3] = g.r * g_uv;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double gp = -c[33 + k], gq = -c[36 + k], gr = -c[39 + k];
        A[4 + k] = g.r * gp - g.p * gr;
        B[4 + k] = g.r * gq - g.q * gr;
    }
    double t0 = X0 - c[30], t1 = X1 - c[31], t2 = X2 - c[32];
    // cross(rot, t)
    double cp[3], cq[3], cr[3];
    cp[0] = c[34] * t2 - c[35] * t1; cp[1] = c[35] * t0 - c[33] * t2; cp[2] = c[33] * t1 - c[34] * t0;
    cq[0] = c[37] * t2 - c[38] * t1; cq[1] = c[38] * t0 - c[36] * t2; cq[2] = c[36] * t1 - c[37] * t0;
    cr[0] = c[40] * t2 - c[41] * t1; cr[1] = c[41] * t0 - c[39] * t2; cr[2] = c[39] * t1 - c[40] * t0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        A[7 + k] = g.r * cp[k] - g.p * cr[k];
        B[7 + k] = g.r * cq[k] - g.q * cr[k];
    }
}
