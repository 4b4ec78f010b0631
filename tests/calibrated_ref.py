"""Calibrated bundle adjustment (fixed intrinsics, six pose variables per frame) stated with the oracle's entry points.

The 10-variable damped system of the oracle restricted to the pose and point variables: in every frame's 10 x 10 block of U
the intrinsic rows and columns are zeroed and their diagonal set to 1, the intrinsic columns of W and the intrinsic entries
of gradE are zeroed.  The two-phase step multiplies the diagonal by (1 + c) (bundle-adj-kanatani.cpp:1819,1831), so the
intrinsic corrections come out exactly 0 and the rest is the calibrated step; the compact reduced system is the oracle's
with the intrinsic rows and columns removed (V is point-only, so that is the Schur complement of the 6-variable Hessian).
The LM loop is lm_ref.loop.
"""
import numpy as np

import lm_ref

FV = 6
INTR = slice(0, 4)  # [fx fy u0 v0] of the 10-variable layout


def restrict(gradE, V, U, W, N):
    """the oracle's blocks with the intrinsics made constants (copies)"""
    g, U, W = gradE.copy(), U.copy(), W.copy()
    U[:, INTR, :] = 0
    U[:, :, INTR] = 0
    for k in range(4):
        U[:, k, k] = 1.0
    W[:, :, INTR] = 0
    gf = g[3 * N:].reshape(-1, 10)
    gf[:, INTR] = 0
    return g, V, U, W


def reduced_full_index(M, comp=1):
    """full frame variable (10 M) -> row of the oracle's 10M - 7 system, or -1 (gauge), bundle-adj-kanatani.cpp:539-563"""
    red = np.full(10 * M, -1, dtype=np.int64)
    r = 0
    for fi in range(10 * M):
        if 4 <= fi <= 9 or fi == 14 + comp:
            continue
        red[fi] = r
        r += 1
    return red


def compact_to_reduced(M, comp=1):
    """compact variable (6 M, gauge rows included) -> row of the oracle's 10M - 7 system, or -1 (gauge-fixed)"""
    red = reduced_full_index(M, comp)
    full = (10 * np.arange(M)[:, None] + 4 + np.arange(FV)[None, :]).reshape(-1)
    return red[full]


def compact_corrections(corr, N, M):
    """[3N + 10M] corrections -> [3N + 6M]"""
    return np.concatenate([corr[:3 * N], corr[3 * N:].reshape(M, 10)[:, 4:].reshape(-1)])


def expand_corrections(corr6, N, M):
    """[3N + 6M] -> [3N + 10M] with zero intrinsic corrections"""
    f = np.zeros((M, 10))
    f[:, 4:] = corr6[3 * N:].reshape(M, FV)
    return np.concatenate([corr6[:3 * N], f.reshape(-1)])


def solve_blocks(orc, so, blocks, c, out, fv=10, want_system=False, skyline=False, sel_rows=None):
    """the tail of every step(): the oracle's two-phase solve of the blocks (gradE, V, U, W; with fv = 6 restricted) at damping
    c, by its skyline Cholesky (sel_rows: rows of the inverse, in the fv layout) or its Householder QR.  Adds to out: ok,
    corr10, corr (fv layout), with sel_rows rows, with want_system S / rhs in the oracle's 10M - 7 numbering (fv = 10) or
    the compact 6M one with zero gauge rows and columns (fv = 6)."""
    N, M = so.N, so.M
    if skyline:
        sel = sel_rows
        if fv == 6 and sel_rows is not None:
            sel = compact_to_reduced(M)[np.asarray(sel_rows)]
        res = orc.two_phase_skyline(so, *blocks, c, sel_rows=sel)
        ok, corr = res[0], res[1]
        if sel is not None:
            out["rows"] = res[2]
    elif want_system:
        ok, corr, S, rhs = orc.two_phase(so, *blocks, c, want_system=True)
        if fv == 6:
            idx = compact_to_reduced(M)
            keep = idx >= 0
            n = FV * M
            Sc = np.zeros((n, n))
            Sc[np.ix_(keep, keep)] = S[np.ix_(idx[keep], idx[keep])]
            rc = np.zeros(n)
            rc[keep] = rhs[idx[keep]]
            S, rhs = Sc, rc
        out.update(S=S, rhs=rhs)
    else:
        ok, corr = orc.two_phase(so, *blocks, c)
    out.update(ok=ok, corr10=corr, corr=compact_corrections(corr, N, M) if fv == 6 else corr)
    return out


def step(orc, f0, so, c, want_system=False, skyline=False, sel_rows=None):
    """one calibrated attempt at damping c on the (normalised) oracle scene so.  Returns a dict with ok, corr (compact),
    corr10 (10-variable layout, intrinsics 0), the compact blocks, and with want_system the compact system S / rhs
    (gauge rows and columns zero)."""
    N, M = so.N, so.M
    gradE, V, U, W = orc.derivatives(f0, so)
    out = dict(gradE10=gradE, U10=U, W10=W, V=V,
               grad=np.concatenate([gradE[:3 * N], gradE[3 * N:].reshape(M, 10)[:, 4:].reshape(-1)]),
               U=U[:, 4:, 4:].copy(), W=W[:, :, 4:].copy())
    return solve_blocks(orc, so, restrict(gradE, V, U, W, N), c, out, FV, want_system, skyline, sel_rows)


def compute_inplace(orc, f0, so, allowed_err_change=None, max_hessian_factor=None, max_iterations=0, skyline=False):
    """lm_ref.loop around the calibrated step; so is changed in place (normalised, optimised, normalisation reverted).
    skyline: the oracle's skyline Cholesky instead of its Householder QR (large scenes).  Returns (rc, report): rc 0 = true,
    1 = false."""
    rep = lm_ref.Report()
    ok, nrm = orc.normalize(so)
    if not ok:
        return 1, rep
    two_phase = orc.two_phase_skyline if skyline else orc.two_phase
    rc = lm_ref.loop(rep, so, energy=lambda: orc.reproj_error(f0, so)[0],
                     prepare=lambda: restrict(*orc.derivatives(f0, so), so.N),
                     solve=lambda blocks, c: two_phase(so, *blocks, c),
                     apply=lambda corr: orc.apply_corrections(so, corr),
                     allowed_err_change=allowed_err_change, max_hessian_factor=max_hessian_factor,
                     max_iterations=max_iterations)
    orc.revert(so, nrm)
    return rc, rep
