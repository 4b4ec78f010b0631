"""The yardstick of batched triangulation, numpy only: the linear system of
Triangulate3DPointByLeastSquares (obs-geom.cpp:679-727) solved by numpy.linalg.qr (Householder), the refinement loop restated
step for step, the quality figures and the status bits.  Nothing here comes from the code under test."""
import numpy as np

FEW_VIEWS, DEGENERATE, BEHIND, LOW_PARALLAX, NOT_CONVERGED = 1, 2, 4, 8, 16
EPS = np.finfo(np.float64).eps


def proj_mats(R, T, K):
    """P = K [R | T] per frame: [M][3][4]; K [M][3][3] or one 3 x 3"""
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    T = np.asarray(T, dtype=np.float64).reshape(-1, 3)
    K = np.broadcast_to(np.asarray(K, dtype=np.float64).reshape(-1, 3, 3), R.shape)
    return np.concatenate([K @ R, (K @ T[:, :, None])], axis=2)


def system_from_P(f0, uv, P, q=None):
    """A [2 n][3], b [2 n] of one track: rows x p2 - f0 p0 and y p2 - f0 p1, scaled by sqrt(q)"""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3, 4)
    rows = np.empty((2 * len(uv), 4))
    rows[0::2] = uv[:, :1] * P[:, 2] - f0 * P[:, 0]
    rows[1::2] = uv[:, 1:] * P[:, 2] - f0 * P[:, 1]
    if q is not None:
        rows *= np.repeat(np.sqrt(np.asarray(q, dtype=np.float64)), 2)[:, None]
    return rows[:, :3], -rows[:, 3]


def system_from_KRT(f0, uv, R, T, K, q=None):
    """the same system with the rows written out from K, R, T (no P formed): row = x (k2 R) - f0 (k0 R), ..."""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    A, b = np.empty((2 * len(uv), 3)), np.empty(2 * len(uv))
    for i, (m, r, t, k) in enumerate(zip(uv, R, T, K)):
        for e in range(2):
            w = m[e] * k[2] - f0 * k[e]   # the combination of K's rows
            A[2 * i + e] = w @ r
            b[2 * i + e] = -(w @ t)
    if q is not None:
        s = np.repeat(np.sqrt(np.asarray(q, dtype=np.float64)), 2)
        A, b = A * s[:, None], b * s
    return A, b


def solve_linear(A, b):
    """X from the Householder QR of A; (X, R)"""
    Q, Rf = np.linalg.qr(A)
    with np.errstate(all="ignore"):
        X = np.linalg.solve(Rf, Q.T @ b) if np.all(np.diag(Rf) != 0) else np.full(3, np.nan)
    return X, Rf


def cond2(A):
    s = np.linalg.svd(A, compute_uv=False)
    return s[0] / s[-1] if s[-1] > 0 else np.inf


def project(f0, P, X):
    """pixels of X in every frame of P: [n][2], and the third homogeneous coordinate"""
    h = P[:, :, :3] @ X + P[:, :, 3]
    return f0 * h[:, :2] / h[:, 2:], h


def energy_terms(f0, uv, P, q, X):
    """E = sum q |uv - pi|^2, H = sum q J^T J, g = sum q J^T (pi - uv) at X"""
    pix, h = project(f0, P, X)
    e = pix - uv
    J = f0 * (h[:, 2, None, None] * P[:, :2, :3] - h[:, :2, None] * P[:, None, 2, :3]) / (h[:, 2] ** 2)[:, None, None]
    E = float(np.sum(q * np.sum(e * e, axis=1)))
    H = np.einsum("n,nij,nik->jk", q, J, J)
    g = np.einsum("n,nij,ni->j", q, J, e)
    return E, H, g


def refine(f0, uv, P, q, X0, attempts, rel_change):
    """The refinement loop: damping factor 1e-4, x 10 on a rejected attempt, / 10 on an accepted one; an attempt solves
    (H + c diag H) d = -g and is accepted iff E decreases; stops when an accepted attempt changes E by less than rel_change E.
    Returns X, E, hit_cap and the log [(accepted, X tried)]."""
    X = np.array(X0, dtype=np.float64)
    E, H, g = energy_terms(f0, uv, P, q, X)
    c, log = 1e-4, []
    for _ in range(attempts):
        try:
            with np.errstate(all="ignore"):
                d = np.linalg.solve(H + c * np.diag(np.diag(H)), -g)
            stepped = bool(np.all(np.isfinite(d))) and bool(np.all(np.linalg.eigvalsh(H + c * np.diag(np.diag(H))) > 0))
        except np.linalg.LinAlgError:
            stepped, d = False, np.zeros(3)
        Xn = X + d
        with np.errstate(all="ignore"):
            En, Hn, gn = energy_terms(f0, uv, P, q, Xn) if stepped else (np.inf, H, g)
        if stepped and En < E:
            log.append((True, Xn))
            dE, bound = E - En, rel_change * E
            X, E, H, g = Xn, En, Hn, gn
            c /= 10.0
            if dE < bound:
                return X, E, False, log
        else:
            log.append((False, Xn))
            c *= 10.0
    return X, E, attempts > 0, log


def ray_angles_deg(uv, R, K, f0):
    """angle between the viewing ray of every observation and that of the first, degrees"""
    m = np.concatenate([uv, np.full((len(uv), 1), f0)], axis=1)
    rays = np.einsum("nji,nj->ni", R, np.linalg.solve(K, m[:, :, None])[:, :, 0])
    a = rays[0]
    return np.degrees(np.arctan2(np.linalg.norm(np.cross(np.broadcast_to(a, rays.shape), rays), axis=1), rays @ a))


def triangulate_track(f0, frame, uv, R, T, K, q=None, refine_attempts=0, refine_rel_change=0.0, min_parallax_deg=0.0):
    """one track through the whole definition: X, quality [4], status, and the refinement log"""
    frame = np.asarray(frame, dtype=np.int64)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    T = np.asarray(T, dtype=np.float64).reshape(-1, 3)
    K = np.broadcast_to(np.asarray(K, dtype=np.float64).reshape(-1, 3, 3), R.shape)
    w = np.ones(len(frame)) if q is None else np.asarray(q, dtype=np.float64)
    keep = w > 0
    frame, uv, w = frame[keep], uv[keep], w[keep]
    n = len(frame)
    if n < 2:
        return np.full(3, np.nan), np.array([np.nan, 0.0, np.nan, n]), FEW_VIEWS, []
    P = proj_mats(R[frame], T[frame], K[frame])
    A, b = system_from_P(f0, uv, P, w)
    X, Rf = solve_linear(A, b)
    status, log = 0, []
    solved = bool(np.all(np.isfinite(X))) and bool(np.all(np.isfinite(np.diag(Rf))))
    if not solved:
        status |= DEGENERATE
    elif refine_attempts > 0:
        X, _, hit, log = refine(f0, uv, P, w, X, refine_attempts, refine_rel_change)
        if hit:
            status |= NOT_CONVERGED
    with np.errstate(all="ignore"):
        E = energy_terms(f0, uv, P, w, X)[0]
        depth = R[frame][:, 2] @ X + T[frame][:, 2]
        cond1 = np.linalg.cond(Rf, 1) if solved else np.inf
    angle = float(ray_angles_deg(uv, R[frame], K[frame], f0).max())
    if not np.all(depth > 0):
        status |= BEHIND
    if min_parallax_deg > 0 and not angle >= min_parallax_deg:
        status |= LOW_PARALLAX
    return X, np.array([np.sqrt(E / n), angle, cond1, n]), status, log
