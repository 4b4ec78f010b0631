"""The numpy yardstick of two-view pose refinement (srk_refine_pairs): a straightforward statement of the
problem, independent of the kernel's order of operations (sums by numpy over all matches at once, solves by LAPACK, F from
numpy.linalg.inv through relate_ref.fundamental, the Sampson distance of relate_ref.sampson).

Per pair: E_pair = sum rho(q s), s = r^2 the squared Sampson distance in pixels under F = K_b^-T [T]x R K_a^-1, the five variables
d = [w; beta] with R <- R Exp(w)^T and T <- (T + B beta) / |T + B beta|, H = sum q w J^T J, g = sum q w J r, Levenberg-Marquardt
with the project's damping rule."""
import numpy as np

import relate_ref
import robust_ref
from resect_ref import C0, CAUCHY, EPS, HUBER, NONE, cond1_scaled, newton_step, scaled, so3_exp  # noqa: F401

FEW_POINTS, DEGENERATE, NOT_CONVERGED = 1, 2, 8
skew = relate_ref.skew


def basis(T):
    """B [3][2] = [b1 b2]: k the index of the smallest |T_k| (a tie: the smaller k), b1 = e_k x T normalised, b2 = T x b1"""
    k = int(np.argmin(np.abs(T)))                 # argmin returns the first of equal entries
    b1 = np.cross(np.eye(3)[k], T)
    b1 /= np.linalg.norm(b1)
    return np.column_stack([b1, np.cross(T, b1)])


def move(R, T, d):
    """the pose moved by d = [w; beta]"""
    t = T + basis(T) @ d[3:]
    return R @ so3_exp(d[:3]).T, t / np.linalg.norm(t)


def signed_residuals(f0, uva, uvb, Ka, Kb, R, T):
    """r [n] in pixels: p_b^T F p_a over the root of the four squared line entries; r^2 is relate_ref.sampson"""
    F = relate_ref.fundamental(skew(T) @ R, Ka, Kb)
    pa = np.column_stack([uva, np.full(len(uva), f0)])
    pb = np.column_stack([uvb, np.full(len(uvb), f0)])
    la, lb = pa @ F.T, pb @ F
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sum(pb * la, axis=1) / np.sqrt(la[:, 0] ** 2 + la[:, 1] ** 2 + lb[:, 0] ** 2 + lb[:, 1] ** 2)


def jacobian(f0, uva, uvb, Ka, Kb, R, T):
    """J [n][5] = dr / d[w; beta], analytic: dE/dw_i = -[T]x R [e_i]x, dE/dbeta_j = [b_j]x R, and the quotient rule on
    r = e / sqrt(den), den = |S F p_a|^2 + |S F^T p_b|^2 with S the first two rows of the identity"""
    n = len(uva)
    Kai, KbiT = np.linalg.inv(Ka), np.linalg.inv(Kb).T
    F = KbiT @ skew(T) @ R @ Kai
    pa = np.column_stack([uva, np.full(n, f0)])
    pb = np.column_stack([uvb, np.full(n, f0)])
    la, lb = pa @ F.T, pb @ F
    e = np.sum(pb * la, axis=1)
    den = la[:, 0] ** 2 + la[:, 1] ** 2 + lb[:, 0] ** 2 + lb[:, 1] ** 2
    B = basis(T)
    dE = [-skew(T) @ R @ skew(np.eye(3)[i]) for i in range(3)] + [skew(B[:, j]) @ R for j in range(2)]
    J = np.zeros((n, 5))
    for k in range(5):
        dF = KbiT @ dE[k] @ Kai
        dla, dlb = pa @ dF.T, pb @ dF
        de = np.sum(pb * dla, axis=1)
        dden = 2.0 * (la[:, 0] * dla[:, 0] + la[:, 1] * dla[:, 1] + lb[:, 0] * dlb[:, 0] + lb[:, 1] * dlb[:, 1])
        J[:, k] = de / np.sqrt(den) - 0.5 * e * dden / den ** 1.5
    return J


def terms(f0, uva, uvb, q, Ka, Kb, R, T, kind=NONE, delta=None):
    """E, H [5][5], g [5] and the robust weights w [n] over the matches with q > 0 (w = 0 elsewhere)"""
    n = len(uva)
    q = np.ones(n) if q is None else np.asarray(q, dtype=np.float64)
    on = q > 0
    with np.errstate(all="ignore"):
        r = signed_residuals(f0, uva, uvb, Ka, Kb, R, T)
        s = relate_ref.sampson(relate_ref.fundamental(skew(T) @ R, Ka, Kb), uva, uvb, f0)
        rho, w = robust_ref.rho_w(q * s, kind, delta if kind != NONE else 0.0)
        J = jacobian(f0, uva, uvb, Ka, Kb, R, T)
    w = np.where(on, w, 0.0)
    qw = (q * w)[on]
    H = np.einsum("o,oi,oj->ij", qw, J[on], J[on])
    g = np.einsum("o,oi,o->i", qw, J[on], r[on])
    return float(rho[on].sum()), H, g, w


def in_front(f0, uva, uvb, Ka, Kb, R, T):
    """per match: the point nearest to both rays lies at a positive distance along both (relate_ref.depths: least squares)"""
    if len(uva) == 0:
        return np.zeros(0, bool)
    return np.all(relate_ref.depths(R, T, relate_ref.rays(Ka, uva, f0), relate_ref.rays(Kb, uvb, f0)) > 0.0, axis=1)


def refine_pair(f0, uva, uvb, q, Ka, Kb, R0, T0, attempts=10, rel_change=1e-9, kind=NONE, delta=None):
    """One pair.  Returns a dict: R, T, E (= [T]x R), quality [6], info [5][5], basis [2][3], status, w [n], E_pair, E0, log (one
    (accepted, E_cur, E_cand) per attempt), H, g."""
    n_obs = len(uva)
    qq = np.ones(n_obs) if q is None else np.asarray(q, dtype=np.float64)
    on = qq > 0
    n = int(np.count_nonzero(on))
    R, T = np.array(R0, dtype=np.float64), np.array(T0, dtype=np.float64)
    Ep, H, g, w = terms(f0, uva, uvb, qq, Ka, Kb, R, T, kind, delta)
    out = dict(E0=Ep, log=[])
    if n < 5:
        out.update(R=R, T=T, E=skew(T) @ R, quality=np.array([np.nan, n, np.nan, np.nan, np.nan, 0.0]), info=np.zeros((5, 5)), basis=basis(T).T,
                   status=FEW_POINTS, w=w, E_pair=Ep, H=H, g=g)
        return out
    c, capped, used = C0, attempts > 0, 0
    for _ in range(attempts):
        used += 1
        cand = None
        try:
            A = H + c * np.diag(np.diag(H))
            np.linalg.cholesky(A)
            d = np.linalg.solve(A, -g)
            if np.all(np.isfinite(d)):
                Rn, Tn = move(R, T, d)
                cand = terms(f0, uva, uvb, qq, Ka, Kb, Rn, Tn, kind, delta)
        except np.linalg.LinAlgError:
            pass
        if cand is not None and cand[0] < Ep:
            out["log"].append((True, Ep, cand[0]))
            stop = Ep - cand[0] < rel_change * Ep
            R, T = Rn, Tn
            Ep, H, g, w = cand
            c /= 10.0
            if stop:
                capped = False
                break
        else:
            out["log"].append((False, Ep, np.nan if cand is None else cand[0]))
            c *= 10.0
    status = 0
    with np.errstate(all="ignore"):
        try:
            np.linalg.cholesky(scaled(H))
            cond = cond1_scaled(H)
        except np.linalg.LinAlgError:
            cond = np.nan
    if not np.isfinite(cond) or not np.isfinite(Ep) or not np.all(np.isfinite(H)):
        status |= DEGENERATE
    if capped:
        status |= NOT_CONVERGED
    front = int(np.count_nonzero(in_front(f0, uva[on], uvb[on], Ka, Kb, R, T)))
    out.update(R=R, T=T, E=skew(T) @ R, quality=np.array([np.sqrt(Ep / n), n, w.sum() / n, cond, front, used]), info=H / (f0 * f0),
               basis=basis(T).T, status=status, w=w, E_pair=Ep, H=H, g=g)
    return out
