"""Robust bundle adjustment (srk_ba_set_robust_loss) stated with the oracle's entry points.

Per observation o the residual (ex, ey) = (p/r - u/f0, q/r - v/f0) and its Jacobian over the 3 + 10 variables of the
observation's landmark and frame (the library's variable order) are formed in numpy: d(p/r)/dv = (r p'_v - p r'_v) / r^2 =
A_v / r^2, and likewise B_v / r^2 for q/r (bundle-adj-kanatani.cpp:1450-1525).  With s = ex^2 + ey^2, rho the loss and
w = rho'(s), the weighted Gauss-Newton blocks are  V, U, W = sum_o w_o 2 J_o^T J_o  and the gradient sum_o w_o 2 J_o^T e_o,
the exact gradient of E = sum_o rho(s_o).  At w = 1 these are the oracle's orc_derivatives.  The step is the oracle's own
two_phase / two_phase_skyline on those blocks (calibrated_ref.solve_blocks); the LM loop is lm_ref.loop on E.  Fixed intrinsics
(FV = 6): the blocks restricted with calibrated_ref.restrict.

Every function takes an optional per-observation information q (tests/weighted_ref.py): s becomes q s and the weight of the
blocks q rho'(q s).  q = None is unit information; 1.0 * x is exact, so the values are those without q bit for bit.
"""
import numpy as np

import calibrated_ref as cref
import lm_ref

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


def _information(so, q):
    return np.ones(so.O) if q is None else np.asarray(q, dtype=np.float64)


def energy(f0, so, kind=NONE, delta=None, q=None):
    """E = sum_o rho(q_o s_o) (delta in pixels; q = None: unit information, 1.0 * s is exact)"""
    d = (delta / f0) if kind != NONE else 0.0
    q = _information(so, q)
    e = 0.0
    for a in range(0, so.O, CHUNK):
        sl = slice(a, min(a + CHUNK, so.O))
        ex, ey = residuals(f0, so, sl)
        e += float(rho_w(q[sl] * (ex * ex + ey * ey), kind, d)[0].sum())
    return e


def weights(f0, so, kind=NONE, delta=None, q=None):
    """the loss's factor w_o = rho'(q_o s_o) of every observation (caller's order)"""
    ex, ey = residuals(f0, so)
    return rho_w(_information(so, q) * (ex * ex + ey * ey), kind, (delta / f0) if kind != NONE else 0.0)[1]


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


def derivatives(f0, so, kind=NONE, delta=None, q=None):
    """weighted (gradE [3N + 10M], V [N,3,3], U [M,10,10], W [O,3,10]) in the oracle's layout, and the loss's factors
    rho'(q s); the blocks carry w_eff = q rho'(q s)"""
    N, M, O = so.N, so.M, so.O
    d = (delta / f0) if kind != NONE else 0.0
    q = _information(so, q)
    gradE = np.zeros(3 * N + 10 * M)
    V = np.zeros((N, 3, 3))
    U = np.zeros((M, 10, 10))
    W = np.zeros((O, 3, 10))
    wts = np.zeros(O)
    pt_all = _obs_points(so)
    for a in range(0, O, CHUNK):
        sl = slice(a, min(a + CHUNK, O))
        ex, ey, A, B, r = jacobian(f0, so, sl)
        _, wl = rho_w(q[sl] * (ex * ex + ey * ey), kind, d)
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


def step(orc, f0, so, c, kind=NONE, delta=None, fv=10, want_system=False, skyline=False, sel_rows=None, q=None):
    """one robust attempt at damping c on the (normalised) oracle scene so, the blocks at the current scene.  Returns a dict:
    ok, corr (fv layout), corr10, the weighted blocks (gradE, V, U, W in the 10-variable layout), weights; with want_system
    the system S / rhs of the oracle's 10M - 7 numbering (fv = 10) or the compact 6M one (fv = 6)."""
    gradE, V, U, W, wts = derivatives(f0, so, kind, delta, q)
    out = dict(gradE=gradE, V=V, U=U, W=W, weights=wts)
    blocks = cref.restrict(gradE, V, U, W, so.N) if fv == 6 else (gradE, V, U, W)
    return cref.solve_blocks(orc, so, blocks, c, out, fv, want_system, skyline, sel_rows)


def compute_inplace(orc, f0, so, kind=NONE, delta=None, allowed_err_change=None, max_hessian_factor=None, max_iterations=0,
                    fv=10, skyline=False, normalize=True, q=None):
    """lm_ref.loop on E = sum rho(q s) with the IRLS step; so is changed in place (normalised, optimised, normalisation
    reverted unless normalize=False).  Returns (rc, report) with report.errors = E after every accepted iteration and
    report.attempts_per_iteration."""
    rep = lm_ref.Report()
    nrm = None
    if normalize:
        ok, nrm = orc.normalize(so)
        if not ok:
            return 1, rep
    two_phase = orc.two_phase_skyline if skyline else orc.two_phase

    def prepare():
        blocks = derivatives(f0, so, kind, delta, q)[:4]
        return cref.restrict(*blocks, so.N) if fv == 6 else blocks

    rc = lm_ref.loop(rep, so, energy=lambda: energy(f0, so, kind, delta, q), prepare=prepare,
                     solve=lambda blocks, c: two_phase(so, *blocks, c),
                     apply=lambda corr: orc.apply_corrections(so, corr),
                     allowed_err_change=allowed_err_change, max_hessian_factor=max_hessian_factor,
                     max_iterations=max_iterations)
    if nrm is not None:
        orc.revert(so, nrm)
    return rc, rep


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
