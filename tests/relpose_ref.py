"""Relative-pose factors between frames (srk_ba_set_relative_pose_factors) stated with the oracle's entry points.

Factor k between frames a != b measures Z_k ~ R_a R_b^T and z_k ~ R_a (C_b - C_a), C_j = -R_j^T T_j:

    e_t = R_a (C_b - C_a) - z_k,   e_r = Log(Z_k^T R_a R_b^T),   E = (what E is without factors) + sum_k e^T L_k e,  e = [e_t; e_r]

The oracle's gradient and blocks carry the factor 2 (first_deriv / second_deriv in oracle/ba_oracle.c), so a factor adds
2 J_a^T L J_a and 2 J_b^T L J_b to the pose part (variables 4..9 of ten) of U_a and U_b, 2 J_a^T L e and 2 J_b^T L e to the two
frame gradients, and the block 2 J_a^T L J_b couples the two frames in the reduced camera system, undamped and outside the
Schur complement.  The Jacobians are those of orc.apply_corrections: [Tx Ty Tz] is added to the centre, the rotation correction
multiplies the direct rotation R^T from the left and leaves the centre alone.  With d = C_b - C_a and J = Jr^-1(e_r):

    d e_t / d(T_a, W_a, T_b, W_b) = -R_a, R_a [d]x, R_a, 0        d e_r / d(...) = 0, -J R_b, 0, J R_b

Log and Jr^-1 are those of tests/so3_ref.py (mpmath; no formula shared with the kernels).  Everything else here is numpy on
factors that are already in the coordinates of the scene they are used with.  The step forms the
damped reduced camera system densely over all 10 M frame variables (constant_ref.schur), adds the couplings, restricts it to
the free variables and solves (constant_ref.solve) -- with the gauge kept as well, because orc.two_phase has no place for a
block between two frames.  The LM loop is lm_ref.loop.
"""
import numpy as np

import constant_ref as kref
import lm_ref
import prior_ref as pref
import so3_ref as so3

TRI = [(r, c) for r in range(6) for c in range(r, 6)]  # the 21 entries of the upper triangle, row by row


def full(info21):
    """[n][21] (upper triangle row by row, order [t; r]) -> [n][6][6]"""
    a = np.asarray(info21, dtype=np.float64).reshape(-1, 21)
    L = np.zeros((a.shape[0], 6, 6))
    for k, (r, c) in enumerate(TRI):
        L[:, r, c] = a[:, k]
        L[:, c, r] = a[:, k]
    return L


def tri21(L):
    L = np.asarray(L, dtype=np.float64).reshape(-1, 6, 6)
    return np.ascontiguousarray(np.stack([L[:, r, c] for r, c in TRI], axis=1))


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def log_so3(M):
    """rotation vector of the rotation M, angle in [0, pi] (tests/so3_ref.py: mpmath, nothing shared with the kernels)"""
    return so3.log(M)


def jr_inv(phi):
    """inverse right Jacobian of SO(3): Log(Exp(phi) Exp(d)) = phi + Jr^-1(phi) d + O(d^2) (tests/so3_ref.py)"""
    return so3.jr_inv(phi)


class Factors:
    """a, b [n] (a != b, any order inside a pair), Z [n][3][3], z [n][3], info [n][6][6]"""

    def __init__(self, a=None, b=None, Z=None, z=None, info=None):
        self.a = np.zeros(0, np.int32) if a is None else np.asarray(a, dtype=np.int32).ravel().copy()
        self.b = np.zeros(0, np.int32) if b is None else np.asarray(b, dtype=np.int32).ravel().copy()
        n = self.a.size
        self.Z = np.zeros((0, 3, 3)) if Z is None else np.asarray(Z, dtype=np.float64).reshape(n, 3, 3).copy()
        self.z = np.zeros((0, 3)) if z is None else np.asarray(z, dtype=np.float64).reshape(n, 3).copy()
        self.info = np.zeros((0, 6, 6)) if info is None else np.asarray(info, dtype=np.float64).reshape(n, 6, 6).copy()
        assert self.b.size == n and np.all(self.a != self.b)

    @property
    def n(self):
        return self.a.size

    def copy(self):
        return Factors(self.a, self.b, self.Z, self.z, self.info)

    def sorted(self):
        """the same factors in the order the setter asks for: by (min, max) of the pair"""
        key = np.lexsort((np.maximum(self.a, self.b), np.minimum(self.a, self.b)))
        return Factors(self.a[key], self.b[key], self.Z[key], self.z[key], self.info[key])

    def set_on(self, gpu):
        gpu.set_relative_pose_factors(np.stack([self.a, self.b], axis=1), self.Z, self.z, info=tri21(self.info))


def poses(so):
    R = np.asarray(so.cam_R, dtype=np.float64).reshape(-1, 3, 3)
    return R, pref.centres(so)


def relative_pose(so, a, b):
    """(Z, z) of the pair as the scene's poses have it: Z = R_a R_b^T, z = R_a (C_b - C_a)"""
    R, Cn = poses(so)
    return R[a] @ R[b].T, R[a] @ (Cn[b] - Cn[a])


def residuals(fac, so):
    """[n][6]: e_t, e_r"""
    R, Cn = poses(so)
    e = np.zeros((fac.n, 6))
    for k in range(fac.n):
        a, b = int(fac.a[k]), int(fac.b[k])
        e[k, :3] = R[a] @ (Cn[b] - Cn[a]) - fac.z[k]
        # (R_a R_b^T first, as relative_pose forms it: Z^T Z is then symmetric to the bit and a zero residual exactly zero)
        e[k, 3:] = log_so3(fac.Z[k].T @ (R[a] @ R[b].T))
    return e


def energy(fac, so):
    e = residuals(fac, so)
    return float(np.einsum("na,nab,nb->", e, fac.info, e))


def jacobians(fac, so):
    """(e [n][6], J_a [n][6][6], J_b [n][6][6]) over the pose variables [Tx Ty Tz Wx Wy Wz] of the two frames"""
    R, Cn = poses(so)
    e = residuals(fac, so)
    Ja, Jb = np.zeros((fac.n, 6, 6)), np.zeros((fac.n, 6, 6))
    for k in range(fac.n):
        a, b = int(fac.a[k]), int(fac.b[k])
        J = jr_inv(e[k, 3:])
        Ja[k, :3, :3] = -R[a]
        Ja[k, :3, 3:] = R[a] @ skew(Cn[b] - Cn[a])
        Ja[k, 3:, 3:] = -J @ R[b]
        Jb[k, :3, :3] = R[a]
        Jb[k, 3:, 3:] = J @ R[b]
    return e, Ja, Jb


def add_terms(blocks, so, fac):
    """the (gradE, V, U, W) given plus the factors' terms in the frame blocks and frame gradients (copies)"""
    gradE, V, U, W = blocks[:4]
    N = so.N
    g, U = gradE.copy(), U.copy()
    e, Ja, Jb = jacobians(fac, so)
    gf = g[3 * N:].reshape(-1, 10)
    for k in range(fac.n):
        L = fac.info[k]
        for j, J in ((int(fac.a[k]), Ja[k]), (int(fac.b[k]), Jb[k])):
            U[j, 4:, 4:] += 2.0 * J.T @ L @ J
            gf[j, 4:] += 2.0 * J.T @ L @ e[k]
    return g, V, U, W


def couplings(fac, so):
    """[n][6][6]: 2 J_a^T L J_b, the block (a, b) of the reduced camera system over the pose variables"""
    _, Ja, Jb = jacobians(fac, so)
    return 2.0 * np.einsum("nxa,nxy,nyb->nab", Ja, fac.info, Jb)


def add_couplings(S, fac, so):
    """S [10M][10M] (both triangles) plus the coupling blocks; a switched-off factor adds zeros"""
    Cb = couplings(fac, so)
    for k in range(fac.n):
        a, b = int(fac.a[k]), int(fac.b[k])
        S[10 * a + 4:10 * a + 10, 10 * b + 4:10 * b + 10] += Cb[k]
        S[10 * b + 4:10 * b + 10, 10 * a + 4:10 * a + 10] += Cb[k].T
    return S


def normalised(fac, nrm):
    """the factors in the normalised world X_n = s (R0 X + T0): Z and the rotation part of L as they are, z_n = s z,
    L_tt / s^2, L_tr / s (numpy; the library's host map is compared against this in tests/test_relpose_cpu.py)"""
    s = float(nrm.world_scale)
    out = fac.copy()
    out.z = s * fac.z
    D = np.diag([1 / s] * 3 + [1.0] * 3)
    out.info = np.einsum("ab,nbc,cd->nad", D, fac.info, D)
    return out


def step(orc, f0, so, c, fac, keep_gauge, fv=10, fconst=None, pconst=None, want_system=False, derivatives=None, pri=None):
    """one attempt at damping c on the normalised oracle scene so with the factors fac (and the position priors pri) in so's
    coordinates.  Returns a dict: ok, corr (10-variable layout), fixed, the restricted g, V, U, W, blocks (before any
    restriction), S / rhs over all 10 M frame variables (rows and columns of fixed variables are not meaningful) and, with
    want_system, dc_exact and d_solver as constant_ref.step_restricted gives them."""
    fconst = np.zeros(so.M, dtype=bool) if fconst is None else fconst
    pconst = np.zeros(so.N, dtype=bool) if pconst is None else pconst
    base = orc.derivatives(f0, so) if derivatives is None else derivatives(so)
    blocks = base[:4] if pri is None else pref.add_terms(base[:4], so, pri)
    blocks = add_terms(blocks, so, fac)
    out = step_restricted(so, kref.restrict_all(so, blocks, fconst, pconst, fv), c, fac, fconst, keep_gauge, fv, want_system)
    out["blocks"] = blocks
    return out


def step_restricted(so, restricted, c, fac, fconst, keep_gauge, fv=10, want_system=False):
    g, V, U, W = restricted
    fixed = kref.fixed_vars(so.M, fconst, keep_gauge, fv)
    S, rhs, Einv = kref.schur(so, g, V, U, W, c)
    add_couplings(S, fac, so)
    ok, corr = kref.solve(so, g, W, S, rhs, Einv, fixed)
    out = dict(g=g, V=V, U=U, W=W, fixed=fixed, S=S, rhs=rhs, ok=ok, corr=corr)
    if want_system:
        x = kref.refined_solution(S, rhs, fixed)
        out.update(dc_exact=x, d_solver=kref.rel_err(corr[3 * so.N:][~fixed], x[~fixed]) if np.any(~fixed) else 0.0)
    return out


def compute_inplace(orc, f0, so, fac_world, keep_gauge=1, fv=10, fconst=None, pconst=None, allowed_err_change=None,
                    max_hessian_factor=None, max_iterations=0, obs_energy=None, derivatives=None):
    """lm_ref.loop around the step with factors.  fac_world: the factors in the coordinates of so as given; so is changed in
    place (normalised, optimised, normalisation reverted; constant blocks restored bit for bit).  Returns (rc, report)."""
    rep = lm_ref.Report()
    fconst = np.zeros(so.M, dtype=bool) if fconst is None else fconst
    pconst = np.zeros(so.N, dtype=bool) if pconst is None else pconst
    before = (so.points[pconst].copy(), so.cam_R[fconst].copy(), so.cam_T[fconst].copy())
    ok, nrm = orc.normalize(so)
    if not ok:
        return 1, rep
    fac = normalised(fac_world, nrm)
    held = (so.points[pconst].copy(), so.cam_R[fconst].copy(), so.cam_T[fconst].copy())

    def total():
        return (obs_energy(so) if obs_energy else orc.reproj_error(f0, so)[0]) + energy(fac, so)

    def prepare():
        base = orc.derivatives(f0, so) if derivatives is None else derivatives(so)
        return kref.restrict_all(so, add_terms(base[:4], so, fac), fconst, pconst, fv)

    def solve(restricted, c):
        res = step_restricted(so, restricted, c, fac, fconst, keep_gauge, fv)
        return res["ok"], res["corr"]

    def apply(corr):
        orc.apply_corrections(so, corr)
        so.points[pconst], so.cam_R[fconst], so.cam_T[fconst] = held

    rc = lm_ref.loop(rep, so, energy=total, prepare=prepare, solve=solve, apply=apply, allowed_err_change=allowed_err_change,
                     max_hessian_factor=max_hessian_factor, max_iterations=max_iterations)
    orc.revert(so, nrm)
    so.points[pconst], so.cam_R[fconst], so.cam_T[fconst] = before
    return rc, rep
