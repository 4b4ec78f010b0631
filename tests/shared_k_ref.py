"""Shared-intrinsics bundle adjustment (intrinsic groups) stated with the oracle's entry points.

Every frame f belongs to a group g(f); each group has one [fx fy u0 v0].  P (10M -> 6M + 4G) maps a frame's pose variables
[Tx Ty Tz Wx Wy Wz] (variables 4..9) to 6 f + v and its intrinsic variable k (0..3) to 6M + 4 g(f) + k.  P touches only
camera variables, so the landmark Schur complement commutes with it: S_sh(c) = P^T S10(c) P and rhs_sh = P^T rhs10, with
S10(c), rhs10 the oracle's damped reduced system (gauge rows removed).  The step solves S_sh, expands dc10 = P dc_sh and
back-substitutes the points with the oracle's blocks; each group's K takes the additions of bundle-adj-kanatani.cpp:2025-2033.
The LM loop is lm_ref.loop, with K among the saved arrays: the trial K is kept on accept.
The closed-form frame derivatives are the derivatives of the error only with K(2,2) = f0 (test_oracle_fd_checkers.py), so the
library and this yardstick work on every frame's K scaled by f0 / K(2,2) (the same projections): per_frame_scene, to_caller.
"""
import numpy as np

import calibrated_ref as cref
import lm_ref
import robust_ref as rref


def shared_index(M, groups):
    """full 10-variable index (10 M) -> shared index (6 M + 4 G)"""
    groups = np.asarray(groups)
    f = np.arange(10 * M) // 10
    v = np.arange(10 * M) % 10
    return np.where(v >= 4, 6 * f + v - 4, 6 * M + 4 * groups[f] + np.minimum(v, 3))


def aggregation(M, groups, comp=1):
    """P as a dense [10M - 7, 6M + 4G] matrix over the oracle's reduced rows (gauge rows removed)"""
    G = int(np.max(groups)) + 1
    red = cref.reduced_full_index(M, comp)
    sh = shared_index(M, groups)
    Pm = np.zeros((10 * M - 7, 6 * M + 4 * G))
    keep = red >= 0
    Pm[red[keep], sh[keep]] = 1.0
    return Pm


def fold(S10, rhs10, M, groups, comp=1):
    """S_sh = P^T S10 P and rhs_sh = P^T rhs10; the gauge rows and columns come out zero"""
    Pm = aggregation(M, groups, comp)
    return Pm.T @ S10 @ Pm, Pm.T @ rhs10


def gauge_mask(M, groups, comp=1):
    """True for the shared variables the gauge fixes (frame 0's pose, frame 1's translation component comp)"""
    G = int(np.max(groups)) + 1
    m = np.zeros(6 * M + 4 * G, dtype=bool)
    m[0:6] = True
    m[6 + comp] = True
    return m


def expand(dc_sh, M, groups):
    """dc10 = P dc_sh: [6M + 4G] -> [10M]"""
    return dc_sh[shared_index(M, groups)]


def backsub(gradE, V, W, row_ptr, obs_frame, dc10, c):
    """the point corrections of the two-phase step for given camera corrections dc10: (V_i with its diagonal scaled by
    1 + c) dx_i = -(g_i + sum_o W_o dc10_frame(o))"""
    N = V.shape[0]
    dx = np.zeros((N, 3))
    dcf = dc10.reshape(-1, 10)
    for i in range(N):
        Vd = V[i].copy()
        Vd[np.diag_indices(3)] *= 1 + c
        r = gradE[3 * i:3 * i + 3].copy()
        for o in range(row_ptr[i], row_ptr[i + 1]):
            r += W[o] @ dcf[obs_frame[o]]
        dx[i] = -np.linalg.solve(Vd, r)
    return dx.reshape(-1)


def step(orc, f0, so, groups, c, kind=None, delta=None):
    """one shared-intrinsics attempt at damping c on the (normalised) oracle scene so (per-frame K).  Returns a dict with
    ok, S / rhs (shared layout, gauge rows and columns zero), dc_sh, corr ([3N + 6M + 4G]), corr10 ([3N + 10M]) and the
    oracle's blocks."""
    N, M = so.N, so.M
    if kind is None:
        gradE, V, U, W = orc.derivatives(f0, so)
    else:  # a robust loss: the IRLS-weighted blocks of robust_ref
        gradE, V, U, W, _ = rref.derivatives(f0, so, kind, delta)
    ok, _, S10, rhs10 = orc.two_phase(so, gradE, V, U, W, c, want_system=True)
    S, rhs = fold(S10, rhs10, M, groups)
    free = ~gauge_mask(M, groups)
    dc = np.zeros(S.shape[0])
    dc[free] = np.linalg.solve(S[np.ix_(free, free)], rhs[free])
    dc10 = expand(dc, M, groups)
    dx = backsub(gradE, V, W, so.row_ptr, so.obs_frame, dc10, c)
    return dict(ok=ok, S=S, rhs=rhs, dc=dc, corr=np.concatenate([dx, dc]), corr10=np.concatenate([dx, dc10]),
                gradE=gradE, V=V, U=U, W=W)


def folded_gradient(gradE, N, M, groups):
    """P^T of the 10-variable gradient: [3N + 6M + 4G]"""
    G = int(np.max(groups)) + 1
    out = np.zeros(3 * N + 6 * M + 4 * G)
    out[:3 * N] = gradE[:3 * N]
    np.add.at(out, 3 * N + shared_index(M, groups), gradE[3 * N:])
    return out


def apply_k(K, dc_sh, M, groups):
    """per-frame K [M][9] with every group's corrections added (bundle-adj-kanatani.cpp:2025-2033)"""
    K = K.reshape(-1, 9).copy()
    for f in range(M):
        b = 6 * M + 4 * groups[f]
        K[f, 0] += dc_sh[b]
        K[f, 4] += dc_sh[b + 1]
        K[f, 2] += dc_sh[b + 2]
        K[f, 5] += dc_sh[b + 3]
    return K


def per_frame_scene(orc, sc, f0):
    """the oracle scene with one K per frame (the groups' K expanded), each scaled so that K(2,2) = f0"""
    K = np.repeat(sc.K.reshape(-1, 9), sc.M, axis=0) if sc.shared_k else sc.K.reshape(-1, 9).copy()
    K = K * (f0 / K[:, 8:9])
    return orc.Scene(sc.points, sc.cam_R, sc.cam_T, K, 0, sc.row_ptr, sc.obs_frame, sc.obs_uv)


def to_caller(K, k22):
    """K with K(2,2) = f0 (rows of 9) -> the caller's convention K(2,2) = k22"""
    K = np.asarray(K, dtype=np.float64).reshape(-1, 9)
    return K * (k22 / K[:, 8:9])


def compute_inplace(orc, f0, so, groups, allowed_err_change=None, max_hessian_factor=None, max_iterations=0):
    """lm_ref.loop around the shared-intrinsics step, which forms its derivatives at every attempt; so (per frame K) is
    changed in place: normalised, optimised, K of every group updated, normalisation reverted.  Returns (rc, report):
    rc 0 = true, 1 = false."""
    rep = lm_ref.Report()
    ok, nrm = orc.normalize(so)
    if not ok:
        return 1, rep
    groups = np.asarray(groups)

    def solve(_, c):
        out = step(orc, f0, so, groups, c)
        return out["ok"] and bool(np.all(np.isfinite(out["corr"]))), out

    def apply(out):
        orc.apply_corrections(so, out["corr10"])
        so.K[:] = apply_k(so.K, out["dc"], so.M, groups)

    rc = lm_ref.loop(rep, so, energy=lambda: orc.reproj_error(f0, so)[0], prepare=lambda: None, solve=solve, apply=apply,
                     allowed_err_change=allowed_err_change, max_hessian_factor=max_hessian_factor,
                     max_iterations=max_iterations, saved=("points", "cam_R", "cam_T", "K"))
    orc.revert(so, nrm)
    return rc, rep
