"""The numpy yardstick of batched camera resection (srk_resect_frames): a straightforward statement of the
problem, independent of the kernel's order of operations (sums by numpy over all observations at once, solves by LAPACK).

Per frame: E = sum rho(q s), s = |pi(K (R X + T)) - uv|^2 in pixels^2, the six variables [t; w] with C <- C + t and
R^T <- Exp(w) R^T, H = sum q w J^T J, g = sum q w J^T e, Levenberg-Marquardt with the project's damping rule."""
import numpy as np

import robust_ref

EPS = 2.0 ** -52
NONE, HUBER, CAUCHY = 0, 1, 2
FEW_POINTS, DEGENERATE, BEHIND, NOT_CONVERGED = 1, 2, 4, 8
C0 = 1e-4


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=np.float64)


def so3_exp(w):
    w = np.asarray(w, dtype=np.float64)
    t = np.linalg.norm(w)
    W = skew(w)
    if t < 1e-6:
        return np.eye(3) + W + 0.5 * (W @ W)
    return np.eye(3) + np.sin(t) / t * W + 2.0 * (np.sin(0.5 * t) / t) ** 2 * (W @ W)


def angle_between(Ra, Rb):
    """the rotation angle of Ra Rb^T from its skew part (never acos)"""
    D = Ra @ Rb.T
    s = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(np.linalg.norm(s), 0.5 * (np.trace(D) - 1.0)))


def centre(R, T):
    return -R.T @ T


def move(R, T, d):
    """the pose moved by d = [t; w]"""
    C = centre(R, T) + d[:3]
    Rn = (so3_exp(d[3:]) @ R.T).T
    return Rn, -Rn @ C


def residuals(f0, uv, X, K, R, T):
    """e [n][2] in pixels, the depths, and the camera-frame points"""
    xc = X @ R.T + T
    pqr = xc @ K.T
    e = f0 * pqr[:, :2] / pqr[:, 2:3] - uv
    return e, xc[:, 2], xc


def terms(f0, uv, X, q, K, R, T, kind=NONE, delta=None):
    """E, H [6][6], g [6], the robust weights w [n] and the depths, over the observations with q > 0 (w = 0 elsewhere)"""
    n = len(uv)
    q = np.ones(n) if q is None else np.asarray(q, dtype=np.float64)
    on = q > 0
    e, depth, xc = residuals(f0, uv, X, K, R, T)
    rho, w = robust_ref.rho_w(q * (e * e).sum(axis=1), kind, delta if kind != NONE else 0.0)
    w = np.where(on, w, 0.0)
    # d pi / d x_cam, then d x_cam / d [t; w] = R [-I | [X - C]x]
    pqr = xc @ K.T
    p, qq, r = pqr[:, 0], pqr[:, 1], pqr[:, 2]
    dpi = np.zeros((n, 2, 3))
    dpi[:, 0, 0] = dpi[:, 1, 1] = f0 / r
    dpi[:, 0, 2], dpi[:, 1, 2] = -f0 * p / r ** 2, -f0 * qq / r ** 2
    A = dpi @ (K @ R)                                     # d pi / d X, [n][2][3]
    D = X - centre(R, T)
    S = np.zeros((n, 3, 3))                               # [X - C]x
    S[:, 0, 1], S[:, 0, 2], S[:, 1, 0], S[:, 1, 2], S[:, 2, 0], S[:, 2, 1] = -D[:, 2], D[:, 1], D[:, 2], -D[:, 0], -D[:, 1], D[:, 0]
    J = np.concatenate([-A, A @ S], axis=2)
    qw = q * w
    H = np.einsum("o,oai,oaj->ij", qw, J, J)
    g = np.einsum("o,oai,oa->i", qw, J, e)
    return float(rho[on].sum()), H, g, w, depth[on]


def scaled(H):
    d = 1.0 / np.sqrt(np.diag(H))
    return H * np.outer(d, d)


def cond1_scaled(H):
    Hs = scaled(H)
    return float(np.linalg.norm(Hs, 1) * np.linalg.norm(np.linalg.inv(Hs), 1))


def cond2_scaled(H):
    return float(np.linalg.cond(scaled(H), 2))


def newton_step(H, g):
    """|H_s^-1 g_s|: the remaining Newton step in the Jacobi-scaled variables"""
    d = 1.0 / np.sqrt(np.diag(H))
    return float(np.linalg.norm(np.linalg.solve(scaled(H), g * d)))


def resect_frame(f0, uv, X, q, K, R0, T0, attempts=10, rel_change=1e-9, kind=NONE, delta=None):
    """One frame (uv [n][2], X [n][3] the landmarks of its observations).  Returns a dict: R, T, quality [6], info [6][6], status,
    w [n], E, E0, log (one (accepted, E_cur, E_cand) per attempt), H, g."""
    n_obs = len(uv)
    qq = np.ones(n_obs) if q is None else np.asarray(q, dtype=np.float64)
    n = int(np.count_nonzero(qq > 0))
    R, T = np.array(R0, dtype=np.float64), np.array(T0, dtype=np.float64)
    E, H, g, w, depth = terms(f0, uv, X, qq, K, R, T, kind, delta)
    out = dict(E0=E, log=[])
    if n < 3:
        out.update(R=R, T=T, quality=np.array([np.nan, n, np.nan, np.nan, np.nan, 0.0]), info=np.zeros((6, 6)), status=FEW_POINTS, w=w, E=E,
                   H=H, g=g)
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
                with np.errstate(all="ignore"):
                    cand = terms(f0, uv, X, qq, K, Rn, Tn, kind, delta)
        except np.linalg.LinAlgError:
            pass
        if cand is not None and cand[0] < E:
            out["log"].append((True, E, cand[0]))
            stop = E - cand[0] < rel_change * E
            R, T = Rn, Tn
            E, H, g, w, depth = cand
            c /= 10.0
            if stop:
                capped = False
                break
        else:
            out["log"].append((False, E, np.nan if cand is None else cand[0]))
            c *= 10.0
    status = 0
    with np.errstate(all="ignore"):
        try:
            np.linalg.cholesky(scaled(H))
            cond = cond1_scaled(H)
        except np.linalg.LinAlgError:
            cond = np.nan
    if not np.isfinite(cond) or not np.isfinite(E) or not np.all(np.isfinite(H)):
        status |= DEGENERATE
    if not depth.min() > 0:
        status |= BEHIND
    if capped:
        status |= NOT_CONVERGED
    out.update(R=R, T=T, quality=np.array([np.sqrt(E / n), n, w.sum() / n, cond, depth.min(), used]), info=H / (f0 * f0), status=status, w=w,
               E=E, H=H, g=g)
    return out
