"""Cross-covariances between blocks (srk_ba_phase_cross_covariance / srk_ba_cross_covariances) and relative-pose covariances
(srk_ba_relative_pose_covariances) stated with the oracle's entry points, on top of tests/covariance_ref.py.

With H = [[V, W], [W^T, U]] the damped Hessian of covariance_ref, S its reduced camera system over the free frame variables and
T_i = E_i^-1 W_i (3 x the variables of the frames that see landmark i):

    (H^-1)_frame a, frame b        =  (S^-1)_ab
    (H^-1)_landmark i, frame j     = -T_i (S^-1)_{frames of i, j}
    (H^-1)_landmark i, landmark k  =  T_i (S^-1)_{frames of i, frames of k} T_k^T      (+ E_i^-1 for i = k)

and every block with a variable that does not move is zero there.  SchurInverse computes the full S_free^-1 through
covariance_ref.spd_inverse (the landmarks added in order, or reversed: the reference's own rounding noise), DenseInverse the
inverse of the full Hessian over all 3N + 10M variables for tiny scenes; both are read through the same three accessors.

relative_pose_covariance() propagates the joint covariance of the pose variables of two frames through
relpose_ref.jacobians with the factor's (Z, z) set to the scene's current relative pose, so that Jr^-1 = I.
"""
import numpy as np

import constant_ref as kref
import covariance_ref as vref
import relpose_ref as rref

EPS = vref.EPS


class Inverse:
    """the blocks of H^-1 of one case at one damping: ff(a, b) [fv][fv], pf(i, j) [3][fv], pp(i, k) [3][3]; cond = the scaled
    condition number of the free part of S (None on the dense route)"""

    def __init__(self, so, fv, pconst, cond):
        self.so, self.fv, self.off, self.pconst, self.cond = so, fv, 10 - fv, np.asarray(pconst, dtype=bool), cond

    def _fcols(self, j):
        return np.arange(10 * j + self.off, 10 * j + 10)

    def frame_diag(self, j):
        return np.diag(self.ff(j, j)).copy()

    def point_diag(self, i):
        return np.diag(self.pp(i, i)).copy()


class SchurInverse(Inverse):
    def __init__(self, so, restricted, c, fv, fconst, pconst, keep_gauge, fac=None, reverse=False):
        g, V, U, W = restricted
        fixed = kref.fixed_vars(so.M, fconst, keep_gauge, fv)
        if reverse:
            S, Einv = vref.schur_reversed(so, g, V, U, W, c)
        else:
            S, _, Einv = kref.schur(so, g, V, U, W, c)
        if fac is not None:
            rref.add_couplings(S, fac, so)
        free = np.flatnonzero(~fixed)
        self.Sinv = np.zeros_like(S)
        cond = 1.0
        if free.size:
            inv, cond = vref.spd_inverse(S[np.ix_(free, free)])
            self.Sinv[np.ix_(free, free)] = inv
        super().__init__(so, fv, pconst, cond)
        self.Einv, self.W = Einv, W
        self.fr = np.asarray(so.obs_frame).astype(np.int64)
        self.rp = np.asarray(so.row_ptr)

    def _T(self, i):
        """(E_i^-1 W_i [3][10 n_obs], the columns of S it multiplies)"""
        o0, o1 = int(self.rp[i]), int(self.rp[i + 1])
        cols = (10 * self.fr[o0:o1, None] + np.arange(10)[None, :]).reshape(-1)
        return self.Einv[i] @ self.W[o0:o1].transpose(1, 0, 2).reshape(3, -1), cols

    def ff(self, a, b):
        return self.Sinv[np.ix_(self._fcols(a), self._fcols(b))].copy()

    def pf(self, i, j):
        if self.pconst[i]:
            return np.zeros((3, self.fv))
        T, cols = self._T(i)
        return -T @ self.Sinv[np.ix_(cols, self._fcols(j))]

    def pp(self, i, k):
        if self.pconst[i] or self.pconst[k]:
            return np.zeros((3, 3))
        Ti, ci = self._T(i)
        Tk, ck = self._T(k)
        B = Ti @ self.Sinv[np.ix_(ci, ck)] @ Tk.T
        if i == k:
            B = self.Einv[i] + B
            B = 0.5 * (B + B.T)
        return B


class DenseInverse(Inverse):
    """the same blocks from the inverse of the full damped Hessian over all 3N + 10M variables (tiny scenes only); the
    assembly is covariance_ref.dense_blocks'"""

    def __init__(self, so, restricted, c, fv, fconst, pconst, keep_gauge, fac=None):
        g, V, U, W = restricted
        N, M = so.N, so.M
        n = 3 * N + 10 * M
        H = np.zeros((n, n))
        fr = np.asarray(so.obs_frame).astype(np.int64)
        pt = kref.obs_points(so)
        for i in range(N):
            E = V[i].copy()
            E[np.arange(3), np.arange(3)] *= 1 + c
            H[3 * i:3 * i + 3, 3 * i:3 * i + 3] = E
        Sf = np.zeros((10 * M, 10 * M))
        for j in range(M):
            G = U[j].copy()
            G[np.arange(10), np.arange(10)] *= 1 + c
            Sf[10 * j:10 * j + 10, 10 * j:10 * j + 10] = G
        if fac is not None:
            rref.add_couplings(Sf, fac, so)
        H[3 * N:, 3 * N:] = Sf
        for o in range(len(fr)):
            i, j = int(pt[o]), int(fr[o])
            H[3 * i:3 * i + 3, 3 * N + 10 * j:3 * N + 10 * j + 10] = W[o]
            H[3 * N + 10 * j:3 * N + 10 * j + 10, 3 * i:3 * i + 3] = W[o].T
        fixed = np.concatenate([np.repeat(pconst, 3), kref.fixed_vars(M, fconst, keep_gauge, fv)])
        free = np.flatnonzero(~fixed)
        self.Hinv = np.zeros_like(H)
        inv, _ = vref.spd_inverse(H[np.ix_(free, free)])
        self.Hinv[np.ix_(free, free)] = inv
        super().__init__(so, fv, pconst, None)
        self.N3 = 3 * N

    def ff(self, a, b):
        return self.Hinv[np.ix_(self.N3 + self._fcols(a), self.N3 + self._fcols(b))].copy()

    def pf(self, i, j):
        return self.Hinv[np.ix_(np.arange(3 * i, 3 * i + 3), self.N3 + self._fcols(j))].copy()

    def pp(self, i, k):
        return self.Hinv[np.ix_(np.arange(3 * i, 3 * i + 3), np.arange(3 * k, 3 * k + 3))].copy()


def blocks(inv, ff, pf, pp):
    """the three arrays the library returns for the pairs ff [n][2] (a, b), pf [n][2] (landmark, frame), pp [n][2]"""
    fv = inv.fv
    FF = np.array([inv.ff(int(a), int(b)) for a, b in ff]).reshape(-1, fv, fv)
    PF = np.array([inv.pf(int(i), int(j)) for i, j in pf]).reshape(-1, 3, fv)
    PP = np.array([inv.pp(int(i), int(k)) for i, k in pp]).reshape(-1, 3, 3)
    return FF, PF, PP


def diagonals(inv, ff, pf, pp):
    """per pair the reference's marginal diagonals of its two blocks: ([n][fv], [n][fv]), ([n][3], [n][fv]), ([n][3], [n][3])"""
    fd, pd = {}, {}

    def f(j):
        if int(j) not in fd:
            fd[int(j)] = inv.frame_diag(int(j))
        return fd[int(j)]

    def p(i):
        if int(i) not in pd:
            pd[int(i)] = inv.point_diag(int(i))
        return pd[int(i)]

    fv = inv.fv
    return ((np.array([f(a) for a, _ in ff]).reshape(-1, fv), np.array([f(b) for _, b in ff]).reshape(-1, fv)),
            (np.array([p(i) for i, _ in pf]).reshape(-1, 3), np.array([f(j) for _, j in pf]).reshape(-1, fv)),
            (np.array([p(i) for i, _ in pp]).reshape(-1, 3), np.array([p(k) for _, k in pp]).reshape(-1, 3)))


def cross_err(a, b, dp, dq):
    """max |a - b| / sqrt(ref_pp,ii ref_qq,jj) over the blocks a, b [n][np][nq] (b the reference) with the marginal diagonals
    dp [n][np], dq [n][nq]; an entry whose denominator is 0 must be an exact 0"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not a.size:
        return 0.0
    assert a.shape == b.shape
    den = np.sqrt(np.abs(dp))[:, :, None] * np.sqrt(np.abs(dq))[:, None, :]
    mask = den == 0
    assert np.all(a[mask] == 0), "an entry of a variable that does not move is not an exact zero"
    return float((np.abs(a - b) / np.where(mask, 1.0, den)).max())


def max_offdiagonal_correlation(b, dp, dq, offdiag):
    """the largest |correlation| in the reference blocks b of the pairs flagged offdiag (p != q)"""
    b = np.asarray(b, dtype=np.float64)
    offdiag = np.asarray(offdiag, dtype=bool)
    if not b.size or not offdiag.any():
        return 0.0
    den = np.sqrt(np.abs(dp))[:, :, None] * np.sqrt(np.abs(dq))[:, None, :]
    r = np.abs(b) / np.where(den == 0, np.inf, den)
    return float(r[offdiag].max())


def relative_pose_jacobians(so, a, b):
    """(J_a, J_b) [6][6] of [e_t; e_r] over the pose variables of a and b at zero residual: relpose_ref.jacobians with the
    factor's (Z, z) set to the scene's current relative pose"""
    Z, z = rref.relative_pose(so, a, b)
    fac = rref.Factors([a], [b], Z[None], z[None], np.eye(6)[None])
    e, Ja, Jb = rref.jacobians(fac, so)
    assert np.abs(e[0, :3]).max() == 0 and np.abs(e[0, 3:]).max() < 1e-7  # Jr^-1 = I to rounding
    return Ja[0], Jb[0]


def relative_pose_covariance(inv, so, a, b):
    """Sigma_rel [6][6] (order [t; r]) of the pair in the units of so: J_a S_aa J_a^T + J_a S_ab J_b^T + J_b S_ba J_a^T + J_b S_bb J_b^T over
    the pose variables (with ten variables a frame the last six: the marginal over the intrinsics is the sub-block)"""
    Ja, Jb = relative_pose_jacobians(so, a, b)
    o = inv.fv - 6
    Saa, Sab, Sbb = inv.ff(a, a)[o:, o:], inv.ff(a, b)[o:, o:], inv.ff(b, b)[o:, o:]
    J = np.concatenate([Ja, Jb], axis=1)
    S = np.block([[Saa, Sab], [Sab.T, Sbb]])
    R = J @ S @ J.T
    return 0.5 * (R + R.T)


def maps(nrm, fv):
    """(D_frame [fv][fv], D_point [3][3]) of the map from the normalised scene X_n = s (R0 X + T0) to the caller's coordinates:
    D_frame = diag(I (the intrinsics, ten variables only), R0^T / s, R0^T), D_point = R0^T / s"""
    R0 = np.array(list(nrm.R0), dtype=np.float64).reshape(3, 3)
    s = float(nrm.world_scale)
    D = np.zeros((fv, fv))
    off = fv - 6
    D[:off, :off] = np.eye(off)
    D[off:off + 3, off:off + 3] = R0.T / s
    D[off + 3:, off + 3:] = R0.T
    return D, R0.T / s


def revert(nrm, FF, PF, PP):
    """cross blocks of the normalised scene in the caller's coordinates (numpy): D_p Sigma D_q^T"""
    FF, PF, PP = (np.asarray(x, dtype=np.float64) for x in (FF, PF, PP))
    fv = FF.shape[-1] if FF.size else (PF.shape[-1] if PF.size else 6)
    D, Dp = maps(nrm, fv)
    return (np.einsum("ab,nbc,dc->nad", D, FF.reshape(-1, fv, fv), D), np.einsum("ab,nbc,dc->nad", Dp, PF.reshape(-1, 3, fv), D),
            np.einsum("ab,nbc,dc->nad", Dp, PP.reshape(-1, 3, 3), Dp))


def mapped_errors(got, ref, diags, nrm, fv):
    """cross_err of blocks in the caller's coordinates: got against the mapped reference revert(nrm, ref).  An error of
    b sqrt(S_kk S_ll) on every entry of a block becomes at most b g_i g_j on entry (i, j) of D_p S D_q^T with g = |D| sqrt(diag S),
    so g^2 stands where the marginal diagonal stands in the normalised scene (the same number when D is diagonal)"""
    D, Dp = maps(nrm, fv)
    out = []
    for g, r, (dp, dq), (Da, Db) in zip(got, revert(nrm, *ref), diags, ((D, D), (Dp, D), (Dp, Dp))):
        out.append(cross_err(g, r, (np.sqrt(np.abs(dp)) @ np.abs(Da).T) ** 2, (np.sqrt(np.abs(dq)) @ np.abs(Db).T) ** 2))
    return tuple(out)


def relative_pose_to_caller(nrm, R):
    """Sigma_rel of the normalised scene in the caller's units: tt / s^2, tr / s, rr (no R0: z and Z do not change under a
    rigid motion of the world)"""
    s = float(nrm.world_scale)
    D = np.diag([1 / s] * 3 + [1.0] * 3)
    return D @ np.asarray(R, dtype=np.float64) @ D
