"""Constant parameter blocks (srk_ba_set_constant_blocks) stated with the oracle's entry points.

The oracle's blocks restricted to the free blocks: a constant frame's U block becomes the identity, its columns of W and its
gradient zero; a constant landmark's V block becomes the identity, its rows of W and its gradient zero.  The two-phase step
multiplies the diagonal by (1 + c) (bundle-adj-kanatani.cpp:1819,1831), so a constant block's row of the damped system is
(1 + c) on the diagonal against a zero right-hand side: its correction is exactly 0 and the rest is the step of the problem
in the free blocks alone.

keep_gauge = 1: the restricted blocks go to orc.two_phase, which removes the seven gauge rows itself.
keep_gauge = 0: no gauge row is removed, which the oracle has no entry point for: schur() forms
S = G (1 + c on the diagonal) - sum_i W_i^T (V_i (1 + c on the diagonal))^-1 W_i and
rhs = sum_i W_i^T (V_i (1 + c))^-1 g_i - g_f over all 10 M frame variables in numpy, and solve() solves it densely.
(With the gauge rows dropped this is orc.two_phase's system: tests/test_constant_cpu.py.)

The LM loop is lm_ref.loop.
"""
import numpy as np

import calibrated_ref as cref
import lm_ref


def flags(sel, n):
    """index list or boolean mask -> boolean mask of length n (None: nothing constant)"""
    out = np.zeros(n, dtype=bool)
    if sel is None:
        return out
    a = np.asarray(sel)
    if a.dtype == np.bool_:
        assert a.size == n
        return a.copy()
    out[a.astype(np.int64)] = True
    return out


def obs_points(so):
    return np.repeat(np.arange(so.N), np.diff(np.asarray(so.row_ptr)))


def restrict(gradE, V, U, W, so, fconst, pconst):
    """the oracle's blocks (10-variable layout) with the flagged frames and landmarks made constants (copies)"""
    N = so.N
    g, V, U, W = gradE.copy(), V.copy(), U.copy(), W.copy()
    fr = np.asarray(so.obs_frame)
    pt = obs_points(so)
    U[fconst] = np.eye(10)
    V[pconst] = np.eye(3)
    W[fconst[fr]] = 0
    W[pconst[pt]] = 0
    g[3 * N:].reshape(-1, 10)[fconst] = 0
    g[:3 * N].reshape(-1, 3)[pconst] = 0
    return g, V, U, W


def gauge_vars(M, comp=1):
    """the seven gauge variables among the 10 M frame variables (bundle-adj-kanatani.cpp:539-563)"""
    out = np.zeros(10 * M, dtype=bool)
    out[4:10] = True
    out[14 + comp] = True
    return out


def fixed_vars(M, fconst, keep_gauge, fv=10):
    """mask over the 10 M frame variables: the ones that do not move (constant frames, the gauge, with fv = 6 the intrinsics)"""
    fx = np.repeat(fconst, 10)
    if keep_gauge:
        fx = fx | gauge_vars(M)
    if fv == 6:
        fx = fx | np.tile(np.arange(10) < 4, M)
    return fx


def schur(so, g, V, U, W, c):
    """the damped reduced camera system over all 10 M frame variables, and the damped point-block inverses"""
    N, M = so.N, so.M
    fr = np.asarray(so.obs_frame).astype(np.int64)
    rp = np.asarray(so.row_ptr)
    n = 10 * M
    S = np.zeros((n, n))
    rhs = np.zeros(n)
    for j in range(M):
        G = U[j].copy()
        G[np.arange(10), np.arange(10)] *= 1 + c
        S[10 * j:10 * j + 10, 10 * j:10 * j + 10] = G
    rhs -= g[3 * N:]
    E = V.copy()
    E[:, np.arange(3), np.arange(3)] *= 1 + c
    Einv = np.linalg.inv(E)
    for i in range(N):
        o0, o1 = int(rp[i]), int(rp[i + 1])
        if o1 == o0:
            continue
        cols = (10 * fr[o0:o1, None] + np.arange(10)[None, :]).reshape(-1)
        F = W[o0:o1].transpose(1, 0, 2).reshape(3, -1)  # 3 x (10 * observations)
        T = F.T @ Einv[i]
        S[np.ix_(cols, cols)] -= T @ F
        rhs[cols] += T @ g[3 * i:3 * i + 3]
    return S, rhs, Einv


def solve(so, g, W, S, rhs, Einv, fixed):
    """frame corrections from the free rows of (S, rhs), dense; landmark corrections by back-substitution
    (bundle-adj-kanatani.cpp:1919-1960).  Returns (ok, corrections [3N + 10M])"""
    N, M = so.N, so.M
    free = np.flatnonzero(~fixed)
    dc = np.zeros(10 * M)
    if free.size:
        A = S[np.ix_(free, free)]
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            return False, np.zeros(3 * N + 10 * M)
        dc[free] = np.linalg.solve(L.T, np.linalg.solve(L, rhs[free]))
    fr = np.asarray(so.obs_frame).astype(np.int64)
    pt = obs_points(so)
    acc = np.zeros((N, 3))
    np.add.at(acc, pt, np.einsum("opf,of->op", W, dc.reshape(M, 10)[fr]))
    dx = -np.einsum("nab,nb->na", Einv, acc + g[:3 * N].reshape(N, 3))
    corr = np.concatenate([dx.reshape(-1), dc])
    return bool(np.all(np.isfinite(corr))), corr


def refined_solution(S, rhs, fixed):
    """the exact solution of the free rows of (S, rhs) to working precision (iterative refinement with long-double
    residuals, as tests/test_gpu_parity.py measures the oracle's own Householder QR against): [10 M], zeros at fixed"""
    free = np.flatnonzero(~fixed)
    x = np.zeros(S.shape[0])
    if not free.size:
        return x
    A, b = S[np.ix_(free, free)], rhs[free]
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    y = np.linalg.solve(A, b)
    for _ in range(6):
        y = y + np.linalg.solve(A, (bl - Al @ y.astype(np.longdouble)).astype(np.float64))
    x[free] = y
    return x


def rel_err(a, b):
    den = max(float(np.abs(b).max()) if b.size else 0.0, 1e-300)
    return float(np.abs(a - b).max() / den) if a.size else 0.0


def step_blocks(orc, so, blocks, c, fconst, pconst, keep_gauge, fv=10, want_system=False, skyline=False):
    """one attempt at damping c from the blocks (gradE, V, U, W) of the normalised oracle scene so.  Returns a dict: ok, corr
    (10-variable layout), fixed (mask over the 10 M frame variables), the restricted blocks g, V, U, W and, with want_system,
    S [10M, 10M] / rhs [10M] in the full frame-variable indexing (rows and columns of fixed variables are not meaningful),
    dc_exact (the exact solution of that system) and d_solver (the distance of corr's frame part from it)."""
    return step_restricted(orc, so, restrict_all(so, blocks, fconst, pconst, fv), c, fconst, keep_gauge, fv, want_system, skyline)


def restrict_all(so, blocks, fconst, pconst, fv=10):
    """restrict(), and with fv = 6 the intrinsics made constants as well (calibrated_ref.restrict)"""
    g, V, U, W = restrict(*blocks[:4], so, fconst, pconst)
    if fv == 6:
        g, V, U, W = cref.restrict(g, V, U, W, so.N)
    return g, V, U, W


def step_restricted(orc, so, restricted, c, fconst, keep_gauge, fv=10, want_system=False, skyline=False):
    """step_blocks from blocks that restrict_all has restricted already (an LM iteration restricts once for all its attempts)"""
    N, M = so.N, so.M
    g, V, U, W = restricted
    fixed = fixed_vars(M, fconst, keep_gauge, fv)
    out = dict(g=g, V=V, U=U, W=W, fixed=fixed)
    if keep_gauge:
        if want_system:
            ok, corr, Sr, rr = orc.two_phase(so, g, V, U, W, c, want_system=True)
            red = cref.reduced_full_index(M)
            keep = red >= 0
            S = np.zeros((10 * M, 10 * M))
            S[np.ix_(keep, keep)] = Sr[np.ix_(red[keep], red[keep])]
            rhs = np.zeros(10 * M)
            rhs[keep] = rr[red[keep]]
            out.update(S=S, rhs=rhs)
        elif skyline:  # the oracle's skyline Cholesky instead of its Householder QR (long LM runs), as calibrated_ref offers
            ok, corr = orc.two_phase_skyline(so, g, V, U, W, c)
        else:
            ok, corr = orc.two_phase(so, g, V, U, W, c)
    else:
        S, rhs, Einv = schur(so, g, V, U, W, c)
        ok, corr = solve(so, g, W, S, rhs, Einv, fixed)
        out.update(S=S, rhs=rhs)
    out.update(ok=ok, corr=corr)
    if want_system:
        # d_solver: how far the route's own solver (the oracle's Householder QR, or numpy's Cholesky) is from the exact
        # solution of its system; the comparisons allow max(tolerance, 4 d_solver), as tests/test_gpu_parity.py does
        x = refined_solution(out["S"], out["rhs"], fixed)
        out.update(dc_exact=x, d_solver=rel_err(corr[3 * N:][~fixed], x[~fixed]) if np.any(~fixed) else 0.0)
    return out


def step(orc, f0, so, c, fconst, pconst, keep_gauge, fv=10, want_system=False, derivatives=None):
    """as step_blocks, the blocks taken from orc.derivatives (or from derivatives(so), e.g. weighted ones)"""
    blocks = orc.derivatives(f0, so) if derivatives is None else derivatives(so)
    out = step_blocks(orc, so, blocks[:4], c, fconst, pconst, keep_gauge, fv, want_system)
    out["blocks"] = blocks
    return out


def to_layout(x10, N, M, fv):
    """[3N + 10M] -> the library's [3N + fv M]"""
    return x10 if fv == 10 else cref.compact_corrections(x10, N, M)


def frame_var_index(M, fv):
    """full frame variable (10 M) of each of the library's fv M frame variables"""
    return (10 * np.arange(M)[:, None] + (10 - fv) + np.arange(fv)[None, :]).reshape(-1)


def system_check(S, fixed, bound=1e10):
    """the condition every compared case must meet: the free part of S is positive definite (np.linalg.cholesky succeeds)
    and its condition number after symmetric diagonal scaling is below `bound`.  Returns that condition number."""
    free = np.flatnonzero(~fixed)
    if not free.size:
        return 1.0
    A = S[np.ix_(free, free)]
    A = 0.5 * (A + A.T)
    d = np.sqrt(np.diag(A))
    assert np.all(d > 0)
    A = A / d[:, None] / d[None, :]
    np.linalg.cholesky(A)
    cond = float(np.linalg.cond(A))
    assert cond < bound, cond
    return cond


def compute_inplace(orc, f0, so, fconst, pconst, keep_gauge, fv=10, allowed_err_change=None, max_hessian_factor=None,
                    max_iterations=0, skyline=False):
    """lm_ref.loop around the constant-block step; so is changed in place (normalised, optimised, normalisation reverted; the
    constant blocks' values restored bit for bit from before the normalisation, as srk_ba_compute_inplace leaves them).
    skyline (keep_gauge = 1 only): the oracle's skyline Cholesky instead of its Householder QR.  Returns (rc, report):
    rc 0 = true, 1 = false."""
    rep = lm_ref.Report()
    before = (so.points[pconst].copy(), so.cam_R[fconst].copy(), so.cam_T[fconst].copy())
    ok, nrm = orc.normalize(so)
    if not ok:
        return 1, rep
    held = (so.points[pconst].copy(), so.cam_R[fconst].copy(), so.cam_T[fconst].copy())

    def solve(restricted, c):
        res = step_restricted(orc, so, restricted, c, fconst, keep_gauge, fv, skyline=skyline)
        return res["ok"], res["corr"]

    def apply(corr):
        orc.apply_corrections(so, corr)
        so.points[pconst], so.cam_R[fconst], so.cam_T[fconst] = held  # a zero correction leaves a block as it is

    rc = lm_ref.loop(rep, so, energy=lambda: orc.reproj_error(f0, so)[0],
                     prepare=lambda: restrict_all(so, orc.derivatives(f0, so), fconst, pconst, fv), solve=solve, apply=apply,
                     allowed_err_change=allowed_err_change, max_hessian_factor=max_hessian_factor,
                     max_iterations=max_iterations)
    orc.revert(so, nrm)
    so.points[pconst], so.cam_R[fconst], so.cam_T[fconst] = before
    return rc, rep
