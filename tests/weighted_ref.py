"""Bundle adjustment with per-observation information (srk_ba_set_observation_information) stated with
the oracle's entry points: tests/robust_ref.py with q.

Observation o carries q_o >= 0; with s = ex^2 + ey^2 its whitened squared residual is q s, the objective
E = sum_o rho(q_o s_o) (rho the identity without a loss) and the weight of its Gauss-Newton blocks and gradient terms
w_eff = q rho'(q s): V, U, W = sum_o w_eff 2 J_o^T J_o and the gradient sum_o w_eff 2 J_o^T e_o, the exact gradient of E.
The residuals, Jacobians and rho are robust_ref's; the step is the oracle's own two_phase / two_phase_skyline on those
blocks; the LM loop restates bundle-adj-kanatani.cpp:720-893 on E.  At q = 1 every function here gives robust_ref's values
bit for bit (1.0 * x is exact).
"""
import numpy as np

import lm_trajectory as lt

import calibrated_ref as cref
import robust_ref as rr
from robust_ref import NONE, HUBER, CAUCHY, CHUNK, Report  # noqa: F401


def _d(f0, kind, delta):
    return (delta / f0) if kind != NONE else 0.0


def energy(f0, so, q, kind=NONE, delta=None):
    """E = sum_o rho(q_o s_o) (delta in pixels)"""
    q = np.asarray(q, dtype=np.float64)
    e = 0.0
    for a in range(0, so.O, CHUNK):
        sl = slice(a, min(a + CHUNK, so.O))
        ex, ey = rr.residuals(f0, so, sl)
        e += float(rr.rho_w(q[sl] * (ex * ex + ey * ey), kind, _d(f0, kind, delta))[0].sum())
    return e


def weights(f0, so, q, kind=NONE, delta=None):
    """the loss's factor rho'(q_o s_o) of every observation (caller's order): what srk_ba_observation_weights returns"""
    ex, ey = rr.residuals(f0, so)
    return rr.rho_w(np.asarray(q, dtype=np.float64) * (ex * ex + ey * ey), kind, _d(f0, kind, delta))[1]


def derivatives(f0, so, q, kind=NONE, delta=None):
    """weighted (gradE [3N + 10M], V [N,3,3], U [M,10,10], W [O,3,10]) in the oracle's layout, and the loss's factors
    rho'(q s); the blocks carry w_eff = q rho'(q s)"""
    N, M, O = so.N, so.M, so.O
    q = np.asarray(q, dtype=np.float64)
    d = _d(f0, kind, delta)
    gradE = np.zeros(3 * N + 10 * M)
    V = np.zeros((N, 3, 3))
    U = np.zeros((M, 10, 10))
    W = np.zeros((O, 3, 10))
    wts = np.zeros(O)
    pt_all = rr._obs_points(so)
    for a in range(0, O, CHUNK):
        sl = slice(a, min(a + CHUNK, O))
        ex, ey, A, B, r = rr.jacobian(f0, so, sl)
        _, wl = rr.rho_w(q[sl] * (ex * ex + ey * ey), kind, d)
        wts[sl] = wl
        w = q[sl] * wl
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


def step(orc, f0, so, c, q, kind=NONE, delta=None, fv=10, want_system=False, skyline=False, sel_rows=None):
    """one attempt at damping c on the (normalised) oracle scene so, as robust_ref.step with the information q"""
    N, M = so.N, so.M
    gradE, V, U, W, wts = derivatives(f0, so, q, kind, delta)
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


def compute_inplace(orc, f0, so, q, kind=NONE, delta=None, allowed_err_change=None, max_hessian_factor=None, max_iterations=0,
                    fv=10, skyline=False, normalize=True):
    """the LM loop of bundle-adj-kanatani.cpp:720-893 on E = sum rho(q s), as robust_ref.compute_inplace"""
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
    err_value = energy(f0, so, q, kind, delta)
    rep.err_initial = rep.err_final = err_value
    result_true = False
    done = False
    if allowed_err_change is not None and err_value < allowed_err_change:
        rep.status, result_true, done = 1, True, True
    while not done:
        if max_iterations > 0 and rep.iterations >= max_iterations:
            rep.status, result_true = 5, False
            break
        gradE, V, U, W, _ = derivatives(f0, so, q, kind, delta)
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
            err_new = energy(f0, so, q, kind, delta)
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


def make_information(sc, seed, zero_frac=0.03):
    """seeded information for a scene: log-uniform in [0.25, 4]; then about zero_frac of the observations set to 0, at most
    one per landmark and only in landmarks with at least four observations (so every landmark keeps >= 3 positive ones)"""
    rng = np.random.RandomState(seed)
    rp = np.asarray(sc.row_ptr)
    O = int(rp[-1])
    q = np.exp(rng.uniform(np.log(0.25), np.log(4.0), size=O))
    cnt = np.diff(rp)
    cand = np.flatnonzero(cnt >= 4)
    n_zero = min(len(cand), int(round(zero_frac * O)))
    for i in rng.choice(cand, size=n_zero, replace=False):
        q[rp[i] + rng.randint(cnt[i])] = 0.0
    return q


def remove_observations(sc, drop):
    """a copy of the scene sc without the observations flagged in drop (caller's order)"""
    keep = ~np.asarray(drop, dtype=bool)
    rp = np.asarray(sc.row_ptr)
    kept = np.concatenate([[0], np.cumsum(keep)])
    return type(sc)(sc.points.copy(), sc.cam_R.copy(), sc.cam_T.copy(), sc.K.copy(), sc.shared_k, kept[rp].astype(np.int64),
                    np.asarray(sc.obs_frame)[keep], np.asarray(sc.obs_uv).reshape(-1, 2)[keep])
