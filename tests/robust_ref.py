"""Robust bundle adjustment (srk_ba_set_robust_loss) stated with the oracle's entry points.

Per observation o the residual (ex, ey) = (p/r - u/f0, q/r - v/f0) and its Jacobian over the 3 + 10 variables of the
observation's landmark and frame (the library's variable order) are formed in numpy: d(p/r)/dv = (r p'_v - p r'_v) / r^2 =
A_v / r^2, and likewise B_v / r^2 for q/r (bundle-adj-kanatani.cpp:1450-1525).  With s = ex^2 + ey^2, rho the loss and
w = rho'(s), the weighted Gauss-Newton blocks are  V, U, W = sum_o w_o 2 J_o^T J_o  and the gradient sum_o w_o 2 J_o^T e_o,
the exact gradient of E = sum_o rho(s_o).  At w = 1 these are the oracle's orc_derivatives.  The step is the oracle's own
two_phase / two_phase_skyline on those blocks; the LM loop restates bundle-adj-kanatani.cpp:720-893 on E.  Fixed intrinsics
(FV = 6): the blocks restricted with calibrated_ref.restrict.
"""
import numpy as np

import lm_trajectory as lt

import calibrated_ref as cref

NONE, HUBER, CAUCHY = 0, 1, 2
KINDS = {None: NONE, "huber": HUBER, "cauchy": CAUCHY}
CHUNK = 1 << 18  # observations a block of numpy work takes (bounded memory on the large scenes)


def rho_w(s, kind, d):
    """(rho(s), w = rho'(s)) elementwise; d = delta / f0"""
    s = np.asarray(s, dtype=np.float64)
    if kind == NONE:
        return s.copy(), np.ones_like(s)
    d2 = d * d
    if kind == HUBER:
        rs = np.sqrt(s)
        out = s > d2
        rho = np.where(out, 2.0 * d * rs - d2, s)
        w = np.where(out, d / np.where(out, rs, 1.0), 1.0)
        return rho, w
    if kind == CAUCHY:
        t = s / d2
        return d2 * np.log1p(t), 1.0 / (1.0 + t)
    raise ValueError(kind)


def _frames_K(so):
    K = np.asarray(so.K, dtype=np.float64).reshape(-1, 3, 3)
    return np.repeat(K, so.M, axis=0) if (so.shared_k or K.shape[0] == 1) else K


def _obs_points(so):
    return np.repeat(np.arange(so.N), np.diff(np.asarray(so.row_ptr)))


def residuals(f0, so, sl=slice(None)):
    """(ex, ey) of observations sl, formed as the error pass forms them (divisions)"""
    R = so.cam_R.reshape(-1, 3, 3)
    T = so.cam_T.reshape(-1, 3)
    K = _frames_K(so)
    pt = _obs_points(so)[sl]
    fr = np.asarray(so.obs_frame)[sl]
    X = so.points.reshape(-1, 3)[pt]
    xc = np.einsum("oab,ob->oa", R[fr], X) + T[fr]
    pqr = np.einsum("oab,ob->oa", K[fr], xc)
    uv = so.obs_uv.reshape(-1, 2)[sl]
    return pqr[:, 0] / pqr[:, 2] - uv[:, 0] / f0, pqr[:, 1] / pqr[:, 2] - uv[:, 1] / f0


def energy(f0, so, kind=NONE, delta=None):
    """E = sum_o rho(s_o) (delta in pixels)"""
    d = (delta / f0) if kind != NONE else 0.0
    e = 0.0
    for a in range(0, so.O, CHUNK):
        ex, ey = residuals(f0, so, slice(a, min(a + CHUNK, so.O)))
        e += float(rho_w(ex * ex + ey * ey, kind, d)[0].sum())
    return e


def weights(f0, so, kind=NONE, delta=None):
    """w_o of every observation (caller's order)"""
    ex, ey = residuals(f0, so)
    return rho_w(ex * ex + ey * ey, kind, (delta / f0) if kind != NONE else 0.0)[1]


def jacobian(f0, so, sl=slice(None)):
    """per observation of sl: ex, ey, A [n, 13], B [n, 13], r -- the library's closed forms (point variables, then the ten
    frame variables [fx fy u0 v0 Tx Ty Tz Wx Wy Wz]); d ex / dv = A_v / r^2, d ey / dv = B_v / r^2"""
    R = so.cam_R.reshape(-1, 3, 3)
    T = so.cam_T.reshape(-1, 3)
    K = _frames_K(so)
    pt = _obs_points(so)[sl]
    fr = np.asarray(so.obs_frame)[sl]
    X = so.points.reshape(-1, 3)[pt]
    Rf, Kf = R[fr], K[fr]
    xc = np.einsum("oab,ob->oa", Rf, X) + T[fr]
    pqr = np.einsum("oab,ob->oa", Kf, xc)
    p, q, r = pqr[:, 0], pqr[:, 1], pqr[:, 2]
    uv = so.obs_uv.reshape(-1, 2)[sl]
    ex, ey = p / r - uv[:, 0] / f0, q / r - uv[:, 1] / f0
    KR = np.einsum("oab,obc->oac", Kf, Rf)
    n = len(p)
    A = np.zeros((n, 13))
    B = np.zeros((n, 13))
    # landmark: A_v = r (KR)[0][v] - p (KR)[2][v]
    A[:, :3] = r[:, None] * KR[:, 0, :] - p[:, None] * KR[:, 2, :]
    B[:, :3] = r[:, None] * KR[:, 1, :] - q[:, None] * KR[:, 2, :]
    fx, fy, u0, v0 = Kf[:, 0, 0], Kf[:, 1, 1], Kf[:, 0, 2], Kf[:, 1, 2]
    rot1 = fx[:, None] * Rf[:, 0, :] + u0[:, None] * Rf[:, 2, :]
    rot2 = fy[:, None] * Rf[:, 1, :] + v0[:, None] * Rf[:, 2, :]
    rot3 = f0 * Rf[:, 2, :]
    A[:, 3] = r * (p / fx - u0 / (f0 * fx) * r)
    B[:, 4] = r * (q / fy - v0 / (f0 * fy) * r)
    A[:, 5] = r * (r / f0)
    B[:, 6] = r * (r / f0)
    A[:, 7:10] = -(r[:, None] * rot1 - p[:, None] * rot3)
    B[:, 7:10] = -(r[:, None] * rot2 - q[:, None] * rot3)
    td = -np.einsum("oba,ob->oa", Rf, T[fr])  # direct translation -(R^T T)
    t = X - td
    cp, cq, cr = np.cross(rot1, t), np.cross(rot2, t), np.cross(rot3, t)
    A[:, 10:13] = r[:, None] * cp - p[:, None] * cr
    B[:, 10:13] = r[:, None] * cq - q[:, None] * cr
    return ex, ey, A, B, r


def derivatives(f0, so, kind=NONE, delta=None):
    """weighted (gradE [3N + 10M], V [N,3,3], U [M,10,10], W [O,3,10]) in the oracle's layout, and the weights"""
    N, M, O = so.N, so.M, so.O
    d = (delta / f0) if kind != NONE else 0.0
    gradE = np.zeros(3 * N + 10 * M)
    V = np.zeros((N, 3, 3))
    U = np.zeros((M, 10, 10))
    W = np.zeros((O, 3, 10))
    wts = np.zeros(O)
    pt_all = _obs_points(so)
    for a in range(0, O, CHUNK):
        sl = slice(a, min(a + CHUNK, O))
        ex, ey, A, B, r = jacobian(f0, so, sl)
        _, w = rho_w(ex * ex + ey * ey, kind, d)
        wts[sl] = w
        ir2 = 1.0 / (r * r)
        Jx, Jy = A * ir2[:, None], B * ir2[:, None]  # d ex / dv, d ey / dv
        g = 2.0 * w[:, None] * (ex[:, None] * Jx + ey[:, None] * Jy)
        H = 2.0 * w[:, None, None] * (Jx[:, :, None] * Jx[:, None, :] + Jy[:, :, None] * Jy[:, None, :])
        pt = pt_all[sl]
        fr = np.asarray(so.obs_frame)[sl]
        np.add.at(gradE, (3 * pt[:, None] + np.arange(3)[None, :]), g[:, :3])
        np.add.at(gradE, (3 * N + 10 * fr[:, None] + np.arange(10)[None, :]), g[:, 3:])
        np.add.at(V, pt, H[:, :3, :3])
        np.add.at(U, fr, H[:, 3:, 3:])
        W[sl] = H[:, :3, 3:]
    return gradE, V, U, W, wts


def step(orc, f0, so, c, kind=NONE, delta=None, fv=10, want_system=False, skyline=False, sel_rows=None):
    """one robust attempt at damping c on the (normalised) oracle scene so, the blocks at the current scene.  Returns a dict:
    ok, corr (fv layout), corr10, the weighted blocks (gradE, V, U, W in the 10-variable layout), weights; with want_system
    the system S / rhs of the oracle's 10M - 7 numbering (fv = 10) or the compact 6M one (fv = 6)."""
    N, M = so.N, so.M
    gradE, V, U, W, wts = derivatives(f0, so, kind, delta)
    out = dict(gradE=gradE, V=V, U=U, W=W, weights=wts)
    g, Ur, Wr = gradE, U, W
    if fv == 6:
        g, V, Ur, Wr = cref.restrict(gradE, V, U, W, N)
    if skyline:
        sel = sel_rows
        if fv == 6 and sel_rows is not None:
            sel = cref.compact_to_reduced(M)[np.asarray(sel_rows)]
        res = orc.two_phase_skyline(so, g, V, Ur, Wr, c, sel_rows=sel)
        ok, corr = res[0], res[1]
        if sel is not None:
            out["rows"] = res[2]
    elif want_system:
        ok, corr, S, rhs = orc.two_phase(so, g, V, Ur, Wr, c, want_system=True)
        if fv == 6:
            idx = cref.compact_to_reduced(M)
            keep = idx >= 0
            n = 6 * M
            Sc = np.zeros((n, n))
            Sc[np.ix_(keep, keep)] = S[np.ix_(idx[keep], idx[keep])]
            rc = np.zeros(n)
            rc[keep] = rhs[idx[keep]]
            S, rhs = Sc, rc
        out.update(S=S, rhs=rhs)
    else:
        ok, corr = orc.two_phase(so, g, V, Ur, Wr, c)
    out.update(ok=ok, corr10=corr, corr=cref.compact_corrections(corr, N, M) if fv == 6 else corr)
    return out


class Report:
    pass


def compute_inplace(orc, f0, so, kind=NONE, delta=None, allowed_err_change=None, max_hessian_factor=None, max_iterations=0,
                    fv=10, skyline=False, normalize=True):
    """the LM loop of bundle-adj-kanatani.cpp:720-893 (as orc_compute_inplace) on E = sum rho(s) with the IRLS step; so is
    changed in place (normalised, optimised, normalisation reverted unless normalize=False).  Returns (rc, report) with
    report.errors = E after every accepted iteration and report.attempts_per_iteration."""
    rep = Report()
    rep.status, rep.iterations, rep.attempts = 0, 0, 0
    rep.attempts_per_iteration, rep.errors = [], []
    rep.log = lt.AttemptLog().arrays()
    log = lt.AttemptLog()
    nrm = None
    if normalize:
        ok, nrm = orc.normalize(so)
        if not ok:
            return 1, rep
    N = so.N
    hessian_factor = float(np.float32(0.0001))  # :723 float literal
    err_value = energy(f0, so, kind, delta)
    rep.err_initial = rep.err_final = err_value
    result_true = False
    done = False
    if allowed_err_change is not None and err_value < allowed_err_change:
        rep.status, result_true, done = 1, True, True
    while not done:
        if max_iterations > 0 and rep.iterations >= max_iterations:
            rep.status, result_true = 5, False
            break
        gradE, V, U, W, _ = derivatives(f0, so, kind, delta)
        if fv == 6:
            gradE, V, U, W = cref.restrict(gradE, V, U, W, N)
        bak = (so.points.copy(), so.cam_R.copy(), so.cam_T.copy())
        have_prev, err_new_prev, decrease, n_att = False, 0.0, 0, 0
        while not decrease:
            rep.attempts += 1
            n_att += 1
            if skyline:
                suc, corr = orc.two_phase_skyline(so, gradE, V, U, W, hessian_factor)
            else:
                suc, corr = orc.two_phase(so, gradE, V, U, W, hessian_factor)
            if not suc:
                log.add(rep.iterations, hessian_factor, np.nan, err_value, lt.SOLVE_FAILED)
                decrease = 2
                break
            orc.apply_corrections(so, corr)
            err_new = energy(f0, so, kind, delta)
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
        rep.errors.append(err_new)
        if allowed_err_change is not None and abs(change) < allowed_err_change:
            rep.status, result_true = 2, True
            break
        err_value = err_new
        hessian_factor /= 10
    rep.hessian_factor = hessian_factor
    rep.log = log.arrays()
    if nrm is not None:
        orc.revert(so, nrm)
    return (0 if result_true else 1), rep


def inject_outliers(sc, frac, lo_pix, hi_pix, seed):
    """move a fraction of the observations (chosen at a fixed seed) by lo..hi pixels in a random direction, in place;
    returns the indices (caller's order)"""
    rng = np.random.RandomState(seed)
    O = int(sc.row_ptr[-1])
    idx = np.sort(rng.choice(O, size=int(round(frac * O)), replace=False))
    ang = rng.uniform(0, 2 * np.pi, size=len(idx))
    mag = rng.uniform(lo_pix, hi_pix, size=len(idx))
    uv = sc.obs_uv.reshape(-1, 2)
    uv[idx, 0] += mag * np.cos(ang)
    uv[idx, 1] += mag * np.sin(ang)
    return idx
