"""Calibrated bundle adjustment (fixed intrinsics, six pose variables per frame) stated with the oracle's entry points.

The 10-variable damped system of the oracle restricted to the pose and point variables: in every frame's 10 x 10 block of U
the intrinsic rows and columns are zeroed and their diagonal set to 1, the intrinsic columns of W and the intrinsic entries
of gradE are zeroed.  The two-phase step multiplies the diagonal by (1 + c) (bundle-adj-kanatani.cpp:1819,1831), so the
intrinsic corrections come out exactly 0 and the rest is the calibrated step; the compact reduced system is the oracle's
with the intrinsic rows and columns removed (V is point-only, so that is the Schur complement of the 6-variable Hessian).
The LM loop restates bundle-adj-kanatani.cpp:720-893 with the decisions of orc_compute_inplace.
"""
import numpy as np

import lm_trajectory as lt

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


def step(orc, f0, so, c, want_system=False, skyline=False, sel_rows=None):
    """one calibrated attempt at damping c on the (normalised) oracle scene so.  Returns a dict with ok, corr (compact),
    corr10 (10-variable layout, intrinsics 0), the compact blocks, and with want_system the compact system S / rhs
    (gauge rows and columns zero)."""
    N, M = so.N, so.M
    gradE, V, U, W = orc.derivatives(f0, so)
    g, V, Ur, Wr = restrict(gradE, V, U, W, N)
    out = dict(gradE10=gradE, U10=U, W10=W, V=V,
               grad=np.concatenate([gradE[:3 * N], gradE[3 * N:].reshape(M, 10)[:, 4:].reshape(-1)]),
               U=U[:, 4:, 4:].copy(), W=W[:, :, 4:].copy())
    idx = compact_to_reduced(M)
    if skyline:
        sel = None if sel_rows is None else idx[np.asarray(sel_rows)]
        res = orc.two_phase_skyline(so, g, V, Ur, Wr, c, sel_rows=sel)
        ok, corr = res[0], res[1]
        if sel is not None:
            out["rows"] = res[2]
    elif want_system:
        ok, corr, S, rhs = orc.two_phase(so, g, V, Ur, Wr, c, want_system=True)
        keep = idx >= 0
        n = FV * M
        Sc = np.zeros((n, n))
        Sc[np.ix_(keep, keep)] = S[np.ix_(idx[keep], idx[keep])]
        rc = np.zeros(n)
        rc[keep] = rhs[idx[keep]]
        out.update(S=Sc, rhs=rc)
    else:
        ok, corr = orc.two_phase(so, g, V, Ur, Wr, c)
    out.update(ok=ok, corr10=corr, corr=compact_corrections(corr, N, M))
    return out


class Report:
    pass


def compute_inplace(orc, f0, so, allowed_err_change=None, max_hessian_factor=None, max_iterations=0, skyline=False):
    """the LM loop of bundle-adj-kanatani.cpp:720-893 (as orc_compute_inplace) around the calibrated step; so is changed in
    place (normalised, optimised, normalisation reverted).  skyline: the oracle's skyline Cholesky instead of its
    Householder QR (large scenes).  Returns (rc, report): rc 0 = true, 1 = false."""
    rep = Report()
    rep.status, rep.iterations, rep.attempts = 0, 0, 0
    rep.attempts_per_iteration = []
    rep.log = lt.AttemptLog().arrays()
    log = lt.AttemptLog()
    ok, nrm = orc.normalize(so)
    if not ok:
        return 1, rep
    N, M = so.N, so.M
    hessian_factor = float(np.float32(0.0001))  # :723 float literal
    err_value, _ = orc.reproj_error(f0, so)
    rep.err_initial = rep.err_final = err_value
    result_true = False
    done = False
    if allowed_err_change is not None and err_value < allowed_err_change:
        rep.status, result_true, done = 1, True, True
    while not done:
        if max_iterations > 0 and rep.iterations >= max_iterations:
            rep.status, result_true = 5, False
            break
        gradE, V, U, W = orc.derivatives(f0, so)
        g, V, Ur, Wr = restrict(gradE, V, U, W, N)
        bak = (so.points.copy(), so.cam_R.copy(), so.cam_T.copy())
        have_prev, err_new_prev, decrease, n_att = False, 0.0, 0, 0
        while not decrease:
            rep.attempts += 1
            n_att += 1
            if skyline:
                suc, corr = orc.two_phase_skyline(so, g, V, Ur, Wr, hessian_factor)
            else:
                suc, corr = orc.two_phase(so, g, V, Ur, Wr, hessian_factor)
            if not suc:
                log.add(rep.iterations, hessian_factor, np.nan, err_value, lt.SOLVE_FAILED)
                decrease = 2
                break
            orc.apply_corrections(so, corr)
            err_new, _ = orc.reproj_error(f0, so)
            if err_new - err_value < 0:
                log.add(rep.iterations, hessian_factor, err_new, err_value, lt.ACCEPTED)
                decrease = 1
                break
            so.points[:], so.cam_R[:], so.cam_T[:] = bak
            if have_prev and allowed_err_change is not None and abs(err_new - err_new_prev) < allowed_err_change:
                log.add(rep.iterations, hessian_factor, err_new, err_value, lt.CONVERGED)
                decrease = 3
                break
            used = hessian_factor
            hessian_factor *= 10
            if max_hessian_factor is not None and hessian_factor > max_hessian_factor:
                log.add(rep.iterations, used, err_new, err_value, lt.CAP_OVERFLOW)
                decrease = 2
                break
            log.add(rep.iterations, used, err_new, err_value, lt.REJECTED)
            err_new_prev, have_prev = err_new, True
        rep.attempts_per_iteration.append(n_att)
        if decrease != 1:
            rep.status = 3 if decrease == 2 else 4
            result_true = False
            break
        rep.iterations += 1
        change = err_new - err_value
        rep.err_final = err_new
        if allowed_err_change is not None and abs(change) < allowed_err_change:
            rep.status, result_true = 2, True
            break
        err_value = err_new
        hessian_factor /= 10
    rep.hessian_factor = hessian_factor
    rep.log = log.arrays()
    orc.revert(so, nrm)
    return (0 if result_true else 1), rep
