"""A numpy yardstick for resection without a start pose (srk_locate_frames): the counter-based sampler, P3P
by Grunert's quartic with numpy.roots and a least-squares alignment of the three points, the choice by the fourth point, the
truncated (MSAC) score and the pick.  Written from the formulas, not from the library's code: the quartic is solved by the
eigenvalues of its companion matrix and the pose comes from an SVD, where the library has closed forms and an orthonormal frame."""
import numpy as np

FEW_POINTS, NO_MODEL = 1, 2
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix(seed, h, k):
    z = (seed + GOLDEN * (4 * h + k + 1)) & M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample(seed, h, n):
    """the four distinct ranks of hypothesis h among n weighted observations"""
    picks = []
    for k in range(4):
        r = (mix(seed, h, k) * (n - k)) >> 64
        for s in sorted(picks):
            if r >= s:
                r += 1
        picks.append(r)
    return picks


def bearings(K, uv, f0):
    m = np.column_stack([uv, np.full(len(uv), f0)])
    b = m @ np.linalg.inv(K).T
    return b / np.linalg.norm(b, axis=1, keepdims=True)


def project(f0, K, R, T, X):
    """pixels and depths of the landmarks X [n][3] under x_cam = R X + T"""
    xc = X @ R.T + T
    pqr = xc @ K.T
    with np.errstate(divide="ignore", invalid="ignore"):
        return f0 * pqr[:, :2] / pqr[:, 2:3], xc[:, 2]


def align(X, Q):
    """the rigid motion (R, T) with Q = R X + T in the least-squares sense (three points: exact when the distances agree)"""
    cx, cq = X.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((Q - cq).T @ (X - cx))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return R, cq - R @ cx


def p3p(X, b):
    """all poses (R, T) that put the three landmarks X [3][3] on the rays b [3][3]: Grunert's quartic in v = s3 / s1.  Returns
    (poses, fragile): fragile says that a root of the quartic is nearly double, where `real` is decided by rounding."""
    a2, b2, c2 = np.sum((X[1] - X[2]) ** 2), np.sum((X[0] - X[2]) ** 2), np.sum((X[0] - X[1]) ** 2)
    ca, cb, cg = b[1] @ b[2], b[0] @ b[2], b[0] @ b[1]
    k1, k2 = (a2 - c2) / b2, c2 / b2
    N = np.array([k1 - 1.0, -2.0 * k1 * cb, 1.0 + k1])           # u = N(v) / D(v)
    D = np.array([-2.0 * ca, 2.0 * cg])
    W = np.array([1.0, -2.0 * cb, 1.0])                          # 1 + v^2 - 2 v cos(beta)
    D2 = np.polymul(D, D)
    quartic = np.polyadd(np.polysub(np.polyadd(D2, np.polymul(N, N)), 2.0 * cg * np.polymul(N, D)), -k2 * np.polymul(W, D2))
    if not np.all(np.isfinite(quartic)) or quartic[0] == 0.0:
        return [], True
    roots = np.roots(quartic)
    fragile = False
    for i, r in enumerate(roots):
        if 0.0 < abs(r.imag) < 1e-6 * max(1.0, abs(r)):
            fragile = True
        for s in roots[i + 1:]:
            if r.imag == 0.0 and s.imag == 0.0 and abs(r - s) < 1e-6 * max(1.0, abs(r)):
                fragile = True
    poses = []
    for r in roots:
        if r.imag != 0.0:
            continue
        v = r.real
        with np.errstate(all="ignore"):
            u = np.polyval(N, v) / np.polyval(D, v)
            s1 = np.sqrt(b2 / np.polyval(W, v))
        if not (np.isfinite(u) and np.isfinite(s1)):
            continue
        Q = np.stack([s1 * b[0], u * s1 * b[1], v * s1 * b[2]])
        R, T = align(X, Q)
        if np.all(np.isfinite(R)) and np.all(np.isfinite(T)):
            poses.append((R, T))
    return poses, fragile


def hypothesis(f0, K, X4, uv4):
    """the pose of a sample of four (landmarks X4 [4][3], pixels uv4 [4][2]): P3P on the first three, poses with a non-positive
    depth at any of the four dropped, the smallest squared pixel error at the fourth wins.  (R, T, e4 squared, fragile) or None."""
    b = bearings(K, uv4[:3], f0)
    poses, fragile = p3p(X4[:3], b)
    best = None
    for R, T in poses:
        px, depth = project(f0, K, R, T, X4)
        if not np.all(depth > 0):
            if np.any(np.abs(depth) < 1e-9 * np.abs(depth).max()):
                fragile = True
            continue
        e4 = float(np.sum((px[3] - uv4[3]) ** 2))
        if np.isfinite(e4) and (best is None or e4 < best[2]):
            best = (R, T, e4)
    return (None if best is None else best + (fragile,)), fragile


def score_terms(f0, K, R, T, X, uv, q, tau):
    """min(q s, tau^2) per observation (depth <= 0 counts tau^2), and the inlier flags"""
    px, depth = project(f0, K, R, T, X)
    with np.errstate(invalid="ignore"):
        z = q * np.sum((px - uv) ** 2, axis=1)
        inl = (depth > 0) & (z < tau * tau)
    return np.where(inl, z, tau * tau), inl, z


def locate_frame(f0, uv, X, q, K, hypotheses=256, tau=4.0, seed=1):
    """One frame.  uv [m][2], X [m][3] the landmarks of its observations, q [m] or None.  Returns a dict: R, T, located [6],
    status, inliers [m] (bool), scores [hypotheses] (inf without a pose), fragile (a decision of some hypothesis hangs on
    rounding), hyp (the poses)."""
    m = len(uv)
    q = np.ones(m) if q is None else np.asarray(q, dtype=np.float64)
    on = np.flatnonzero(q > 0)
    n = len(on)
    nan = float("nan")
    out = dict(R=np.eye(3), T=np.zeros(3), located=np.array([nan, n, 0, nan, 0, nan]), status=0, inliers=np.zeros(m, bool),
               scores=np.full(hypotheses, np.inf), fragile=False, hyp=[None] * hypotheses)
    if n < 4:
        out["status"] = FEW_POINTS
        return out
    Xw, uvw, qw = X[on], uv[on], q[on]
    for h in range(hypotheses):
        r = sample(seed, h, n)
        hyp, fragile = hypothesis(f0, K, Xw[r], uvw[r])
        out["fragile"] |= fragile
        if hyp is None:
            continue
        out["hyp"][h] = hyp
        out["scores"][h] = score_terms(f0, K, hyp[0], hyp[1], Xw, uvw, qw, tau)[0].sum()
    valid = int(np.count_nonzero(np.isfinite(out["scores"])))
    out["located"][4] = valid
    if valid == 0:
        out["status"] = NO_MODEL
        return out
    h = int(np.argmin(out["scores"]))            # the first of equal scores
    R, T, e4, _ = out["hyp"][h]
    _, inl, _ = score_terms(f0, K, R, T, Xw, uvw, qw, tau)
    out["R"], out["T"] = R, T
    out["inliers"][on] = inl
    out["located"] = np.array([np.sqrt(out["scores"][h] / n), n, np.count_nonzero(inl), h, valid, np.sqrt(e4)])
    return out


def ransac_hypotheses(outlier_ratio, success_probability, sample_size=4):
    """RansacIterationsCount: ceil(log(1 - p) / log(1 - (1 - e)^s))"""
    if outlier_ratio == 0:
        return 1
    return int(np.ceil(np.log(1.0 - success_probability) / np.log(1.0 - (1.0 - outlier_ratio) ** sample_size)))


def pose_distance(R, T, R2, T2, depth):
    """(rotation angle between the two poses in radians, distance of the camera centres over the depth)"""
    c = (np.trace(R @ R2.T) - 1.0) / 2.0
    s = np.linalg.norm(R @ R2.T - R2 @ R.T) / (2.0 * np.sqrt(2.0))
    return float(np.arctan2(s, c)), float(np.linalg.norm(R.T @ T - R2.T @ T2) / depth)
