"""Marginal covariances (srk_ba_phase_covariance / srk_ba_covariances) stated with the oracle's entry points.

The blocks (gradE, V, U, W) are the oracle's, with the prior terms (prior_ref.add_terms), the factor terms and couplings
(relpose_ref.add_terms / add_couplings) and the constant blocks and fixed intrinsics restricted (constant_ref.restrict_all)
exactly as the step tests build them: H = [[V, W], [W^T, U]] is the Gauss-Newton Hessian of the objective in the factor-2
convention, V and the diagonal of the frame part carrying (1 + c).  With S the reduced camera system over the free frame
variables (constant_ref.schur, constant_ref.fixed_vars)

    (H^-1)_frame j     = (S^-1)_jj
    (H^-1)_landmark i  = E_i^-1 + E_i^-1 W_i S^-1 W_i^T E_i^-1,   E_i = V_i with (1 + c) on the diagonal

and every variable that does not move has covariance 0.  The free part of S is scaled to a unit diagonal before a
Cholesky-based inverse: LU on the unscaled matrix (np.linalg.inv) is three orders of magnitude less accurate on the
ten-variable cases.  Two more routes check this one: the Schur sum with the landmarks added in reverse order (the
reference's own rounding noise), and the inverse of the full Hessian over all 3N + 10M variables (tiny scenes).

Blocks are returned in the library's layout: frame blocks [M][fv][fv], landmark blocks [N][3][3], in the (normalised) scene's
variables.  revert() is the map to the caller's coordinates, scaled() the factor 2 (sigma / f0)^2.
"""
import numpy as np

import constant_ref as kref
import prior_ref as pref
import relpose_ref as rref

EPS = float(np.finfo(np.float64).eps)


def blocks_of(orc, f0, so, fv, fconst=None, pconst=None, pri=None, fac=None, derivatives=None):
    """the restricted (g, V, U, W) of the normalised oracle scene so, priors and factors (in so's coordinates) included"""
    fconst = np.zeros(so.M, dtype=bool) if fconst is None else fconst
    pconst = np.zeros(so.N, dtype=bool) if pconst is None else pconst
    base = orc.derivatives(f0, so) if derivatives is None else derivatives(so)
    blocks = base[:4]
    if pri is not None:
        blocks = pref.add_terms(blocks, so, pri)
    if fac is not None:
        blocks = rref.add_terms(blocks, so, fac)
    return kref.restrict_all(so, blocks, fconst, pconst, fv)


def schur_reversed(so, g, V, U, W, c):
    """constant_ref.schur with the landmarks added in reverse order (S only)"""
    N, M = so.N, so.M
    fr = np.asarray(so.obs_frame).astype(np.int64)
    rp = np.asarray(so.row_ptr)
    S = np.zeros((10 * M, 10 * M))
    E = V.copy()
    E[:, np.arange(3), np.arange(3)] *= 1 + c
    Einv = np.linalg.inv(E)
    for i in range(N - 1, -1, -1):
        o0, o1 = int(rp[i]), int(rp[i + 1])
        if o1 == o0:
            continue
        cols = (10 * fr[o0:o1, None] + np.arange(10)[None, :]).reshape(-1)
        F = W[o0:o1].transpose(1, 0, 2).reshape(3, -1)
        S[np.ix_(cols, cols)] -= (F.T @ Einv[i]) @ F
    for j in range(M - 1, -1, -1):
        G = U[j].copy()
        G[np.arange(10), np.arange(10)] *= 1 + c
        S[10 * j:10 * j + 10, 10 * j:10 * j + 10] += G
    return S, Einv


def spd_inverse(A):
    """(inverse, condition number of the diagonally scaled matrix) of a symmetric positive definite A: scaled to a unit
    diagonal, Cholesky, the triangular inverse squared.  Raises np.linalg.LinAlgError when A is not positive definite."""
    A = 0.5 * (A + A.T)
    d = np.sqrt(np.diag(A))
    if not np.all(d > 0):
        raise np.linalg.LinAlgError("non-positive diagonal")
    As = A / d[:, None] / d[None, :]
    L = np.linalg.cholesky(As)
    Li = np.linalg.solve(L, np.eye(A.shape[0]))
    return (Li.T @ Li) / d[:, None] / d[None, :], float(np.linalg.cond(As))


def covariance_blocks(so, restricted, c, fv, fconst, pconst, keep_gauge, fac=None, reverse=False):
    """(frame blocks [M][fv][fv], landmark blocks [N][3][3], scaled condition number of the free part of S) of the inverse of
    the damped Hessian; fixed variables and constant landmarks zero"""
    g, V, U, W = restricted
    N, M = so.N, so.M
    fixed = kref.fixed_vars(M, fconst, keep_gauge, fv)
    if reverse:
        S, Einv = schur_reversed(so, g, V, U, W, c)
    else:
        S, _, Einv = kref.schur(so, g, V, U, W, c)
    if fac is not None:
        rref.add_couplings(S, fac, so)
    free = np.flatnonzero(~fixed)
    Sinv = np.zeros_like(S)
    cond = 1.0
    if free.size:
        inv, cond = spd_inverse(S[np.ix_(free, free)])
        Sinv[np.ix_(free, free)] = inv
    off = 10 - fv
    FB = np.stack([Sinv[10 * j + off:10 * j + 10, 10 * j + off:10 * j + 10] for j in range(M)])
    fr = np.asarray(so.obs_frame).astype(np.int64)
    rp = np.asarray(so.row_ptr)
    PB = np.zeros((N, 3, 3))
    for i in range(N):
        if pconst[i]:
            continue
        o0, o1 = int(rp[i]), int(rp[i + 1])
        cols = (10 * fr[o0:o1, None] + np.arange(10)[None, :]).reshape(-1)
        F = W[o0:o1].transpose(1, 0, 2).reshape(3, -1)
        T = Einv[i] @ F
        PB[i] = Einv[i] + T @ Sinv[np.ix_(cols, cols)] @ T.T
    return FB, 0.5 * (PB + PB.transpose(0, 2, 1)), cond


def dense_blocks(so, restricted, c, fv, fconst, pconst, keep_gauge, fac=None):
    """the same blocks from the inverse of the full damped Hessian over all 3N + 10M variables (tiny scenes only)"""
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
    Hinv = np.zeros_like(H)
    inv, _ = spd_inverse(H[np.ix_(free, free)])
    Hinv[np.ix_(free, free)] = inv
    off = 10 - fv
    FB = np.stack([Hinv[3 * N + 10 * j + off:3 * N + 10 * j + 10, 3 * N + 10 * j + off:3 * N + 10 * j + 10] for j in range(M)])
    PB = np.stack([Hinv[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in range(N)])
    return FB, PB


def block_err(a, b):
    """per block max |a - b| / sqrt(ref_aa ref_bb) (b the reference), the maximum over the blocks; rows and columns the
    reference holds zeros for must be exact zeros"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not a.size:
        return 0.0
    d = np.sqrt(np.abs(np.einsum("nii->ni", b)))
    zero = d == 0
    mask = zero[:, :, None] | zero[:, None, :]
    assert np.all(a[mask] == 0), "an entry of a fixed variable is not an exact zero"
    den = np.where(mask, 1.0, d[:, :, None] * d[:, None, :])
    return float((np.abs(a - b) / den).max())


def revert(nrm, FB, PB):
    """blocks of the normalised scene X_n = s (R0 X + T0) in the caller's coordinates (numpy): landmarks R0^T Sigma R0 / s^2,
    frames D Sigma D^T with D = diag(I (the intrinsics, ten variables only), R0^T / s, R0^T)"""
    R0 = np.array(list(nrm.R0), dtype=np.float64).reshape(3, 3)
    s = float(nrm.world_scale)
    FB, PB = np.asarray(FB, dtype=np.float64), np.asarray(PB, dtype=np.float64)
    fv = FB.shape[-1] if FB.size else 6
    D = np.zeros((fv, fv))
    off = fv - 6
    D[:off, :off] = np.eye(off)
    D[off:off + 3, off:off + 3] = R0.T / s
    D[off + 3:, off + 3:] = R0.T
    return np.einsum("ab,nbc,dc->nad", D, FB, D), np.einsum("ba,nbc,cd->nad", R0, PB, R0) / (s * s)


def scaled(f0, sigma_pixels, FB, PB):
    k = 2.0 * (float(sigma_pixels) / float(f0)) ** 2
    return k * np.asarray(FB), k * np.asarray(PB)
