"""A numpy yardstick for the two-view fundamental matrix by another route than the library's: the sampler
integer for integer, the null space of the 7 x 9 matrix from numpy's SVD, the cubic from `det` at four abscissae with polyfit and
numpy.roots, the representation from numpy's SVD, the attempts with a central-difference Jacobian of the residual in the seven
variables and numpy.linalg.solve, the same acceptance rule and the same 1e-9 stop.  Nothing here is compiled."""
import math

import numpy as np

MASK = (1 << 64) - 1
C0 = 1e-4
STOP = 1e-9
MIN_INLIERS = 8
DEPENDENT = 1e-10   # the yardstick's own rule for seven dependent rows: the seventh singular value at most this share of the first
# (noise-free planar samples show 2e-16, general ones 1e-4 to 1e-2: the library's pivot rule and this one agree on both)
EXACT_FIT = 1e-12   # (1e-6 px)^2 per match: a score below it is an exact fit
# A score is a sum of at most 200 terms, so two routes to it differ by some 200 eps = 4e-14 relative.  A decision whose margin is within
# TIE of zero is rounding's: either arm is right.
TIE = 1e-12


def mix(seed, h, k):
    z = (seed + 0x8EBC6AF09C88C6E3 * (8 * h + k + 1)) & MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def sample(seed, h, n):
    """eight distinct ranks below n: draw k is uniform among the n - k ranks not yet picked"""
    picks = []
    for k in range(8):
        r = (mix(seed, h, k) * (n - k)) >> 64
        for s in sorted(picks):
            if r >= s:
                r += 1
        picks.append(r)
    return picks


def ransac_hypotheses(share, confidence, sample_size=7):
    return int(math.ceil(math.log(1.0 - confidence) / math.log(1.0 - (1.0 - share) ** sample_size)))


def homog(uv, f0):
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    return np.column_stack([uv, np.full(len(uv), float(f0))])


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def canonical(F):
    """norm 1, the entry of largest magnitude positive (a tie: the first row by row)"""
    F = np.asarray(F, dtype=np.float64).reshape(3, 3)
    F = F / np.linalg.norm(F)
    k = int(np.argmax(np.abs(F).reshape(-1)))
    return -F if F.reshape(-1)[k] < 0 else F


def true_fundamental(R, T, Ka, Kb):
    """K_b^-T [T]x R K_a^-1 for p = (u, v, f0), norm 1 and signed"""
    return canonical(np.linalg.inv(Kb).T @ skew(T) @ R @ np.linalg.inv(Ka))


def sampson(F, uva, uvb, f0):
    """s [n], the squared Sampson distance in pixels"""
    pa, pb = homog(uva, f0), homog(uvb, f0)
    l, m = pa @ F.T, pb @ F
    e = np.sum(pb * l, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return e * e / (l[:, 0] ** 2 + l[:, 1] ** 2 + m[:, 0] ** 2 + m[:, 1] ** 2)


def seven_point(uva, uvb, f0):
    """the matrices (norm 1) of the real roots of det(F1 + z F2) for seven matches, and the seventh singular value over the first;
    no matrices when the rows are dependent"""
    a, b = homog(uva, f0) / f0, homog(uvb, f0) / f0
    A = np.einsum("ni,nj->nij", b, a).reshape(7, 9)
    _, s, Vt = np.linalg.svd(A)
    ratio = s[6] / s[0]
    if not ratio > DEPENDENT:
        return [], ratio
    F1, F2 = Vt[7].reshape(3, 3), Vt[8].reshape(3, 3)
    if abs(np.linalg.det(F1)) > abs(np.linalg.det(F2)):
        F1, F2 = F2, F1
    zs = np.array([-1.0, 0.0, 1.0, 2.0])
    coeff = np.polyfit(zs, [np.linalg.det(F1 + z * F2) for z in zs], 3)
    out = []
    for z in sorted(np.roots(coeff), key=lambda r: r.real):
        if abs(z.imag) <= 1e-7 * (1.0 + abs(z.real)):
            G = F1 + z.real * F2
            out.append(G / np.linalg.norm(G))
    return out, ratio


def hypothesis(a8, b8, f0):
    """the model of a sample of eight matches: (F, squared eighth-match error, real roots) or (None, None, 0)"""
    Fs, _ = seven_point(a8[:7], b8[:7], f0)
    best = None
    for F in Fs:
        s = float(sampson(F, a8[7:], b8[7:], f0)[0])
        if np.isfinite(s) and (best is None or s < best[1]):
            best = (F, s)
    return (None, None, 0) if best is None else (best[0], best[1], len(Fs))


def judge(F, uva, uvb, q, f0, tau):
    """score, inlier mask, the inliers' sum of s, and the distance of the nearest q s from tau^2 in pixels squared"""
    s = sampson(F, uva, uvb, f0)
    w = q * s
    with np.errstate(invalid="ignore"):
        inl = w < tau * tau
    edge = np.abs(np.where(np.isfinite(w), w, np.inf) - tau * tau).min() if len(w) else np.inf
    return float(np.where(inl, w, tau * tau).sum()), inl, float(s[inl].sum()), float(edge)


def so3_exp(w):
    t = np.linalg.norm(w)
    if t == 0.0:
        return np.eye(3)
    k = skew(np.asarray(w) / t)
    return np.eye(3) + math.sin(t) * k + (1.0 - math.cos(t)) * (k @ k)


def represent(F):
    """U, V proper and sigma in [0, 1] with F ~ U diag(1, sigma, 0) V^T, from numpy's SVD"""
    U, s, Vt = np.linalg.svd(F)
    V = Vt.T.copy()
    if np.linalg.det(U) < 0:
        U[:, 2] = -U[:, 2]
    if np.linalg.det(V) < 0:
        V[:, 2] = -V[:, 2]
    return U, V, s[1] / s[0]


def build(U, V, sigma):
    return (np.outer(U[:, 0], V[:, 0]) + sigma * np.outer(U[:, 1], V[:, 1])) / math.sqrt(1.0 + sigma * sigma)


def moved(U, V, sigma, d):
    U, V, sigma = U @ so3_exp(d[:3]), V @ so3_exp(d[3:6]), sigma + d[6]
    if sigma < 0:
        sigma, U = -sigma, U @ np.diag([1.0, -1.0, -1.0])
    if sigma > 1:
        P = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])
        sigma, U, V = 1.0 / sigma, U @ P, V @ P
    return U, V, sigma


def residual(U, V, sigma, d, uva, uvb, q, f0):
    """sqrt(q) times the signed Sampson distance in pixels at the model moved by d"""
    F = build(*moved(U, V, sigma, d))
    pa, pb = homog(uva, f0), homog(uvb, f0)
    l, m = pa @ F.T, pb @ F
    return np.sqrt(q) * np.sum(pb * l, axis=1) / np.sqrt(l[:, 0] ** 2 + l[:, 1] ** 2 + m[:, 0] ** 2 + m[:, 1] ** 2)


def normal_equations(U, V, sigma, uva, uvb, q, f0, step=1e-6):
    """H = J^T J and g = J^T r of the given matches, J by central differences"""
    r = residual(U, V, sigma, np.zeros(7), uva, uvb, q, f0)
    J = np.zeros((len(r), 7))
    for k in range(7):
        d = np.zeros(7)
        d[k] = step
        J[:, k] = (residual(U, V, sigma, d, uva, uvb, q, f0) - residual(U, V, sigma, -d, uva, uvb, q, f0)) / (2.0 * step)
    return J.T @ J, J.T @ r


def cond1(H):
    """cond_1 of the Jacobi-scaled H, NaN when it is not positive definite"""
    d = np.diag(H)
    if not np.all(d > 0):
        return np.nan
    Hs = H / np.sqrt(np.outer(d, d))
    try:
        np.linalg.cholesky(Hs)
    except np.linalg.LinAlgError:
        return np.nan
    return float(np.linalg.norm(Hs, 1) * np.linalg.norm(np.linalg.inv(Hs), 1))


def score_all(f0, uva, uvb, q, hypotheses, seed, tau):
    """every hypothesis' model and score of one pair: what pick() needs"""
    uva, uvb = np.asarray(uva, float).reshape(-1, 2), np.asarray(uvb, float).reshape(-1, 2)
    keep = np.ones(len(uva), bool) if q is None else np.asarray(q) > 0
    w = np.ones(int(keep.sum())) if q is None else np.asarray(q, float)[keep]
    a, b = uva[keep], uvb[keep]
    n = len(a)
    models, scores = [None] * hypotheses, np.full(hypotheses, np.inf)
    if n >= 8:
        for h in range(hypotheses):
            r = sample(seed, h, n)
            F, e8, roots = hypothesis(a[r], b[r], f0)
            if F is not None:
                models[h] = (F, e8, roots)
                scores[h] = judge(F, a, b, w, f0, tau)[0]
    return dict(f0=f0, a=a, b=b, w=w, keep=keep, tau=tau, n=n, models=models, scores=scores)


def pick(A, hypotheses, refine_rounds, winner=None):
    """the yardstick's result of a pair at a hypothesis count (a prefix of the same hypotheses): the winner, the attempts, the
    outputs.  y["trail"] holds, per attempt, (candidate score - current score) / current score; y["at"](h) is the result had
    hypothesis h won (eight or nine matches draw orderings of the same few samples again and again, whose scores tie to rounding)."""
    n, keep = A["n"], A["keep"]
    scores = A["scores"][:hypotheses]
    n_models = int(np.isfinite(scores).sum())
    nan = np.nan
    if n < 8 or n_models == 0:
        return dict(status=1 if n < 8 else 2, F=np.zeros((3, 3)), U=np.eye(3), V=np.eye(3), sigma=0.0, info=np.zeros((7, 7)),
                    fund=np.array([nan, n, 0, nan, n_models, nan, 0, 0, nan, 0, nan, 0]), inliers=np.zeros(len(keep), np.uint8), scores=scores,
                    trail=[], edge=np.inf)
    a, b, w, f0, tau = A["a"], A["b"], A["w"], A["f0"], A["tau"]
    h = int(np.argmin(scores)) if winner is None else int(winner)
    Fh, e8, roots = A["models"][h]
    U, V, sigma = represent(Fh)
    F = build(U, V, sigma)
    best, inl, ss, edge = judge(F, a, b, w, f0, tau)
    start = best
    c, accepted, used, trail = C0, 0, 0, []
    for _ in range(refine_rounds):
        if inl.sum() < MIN_INLIERS:
            break
        H, g = normal_equations(U, V, sigma, a[inl], b[inl], w[inl], f0)
        if not (np.all(np.isfinite(H)) and np.all(np.isfinite(g))):
            break
        used += 1
        sc, stepped = np.inf, False
        try:
            np.linalg.cholesky(H + c * np.diag(np.diag(H)))
            d = np.linalg.solve(H + c * np.diag(np.diag(H)), -g)
            stepped = bool(np.all(np.isfinite(d)))
        except np.linalg.LinAlgError:
            pass
        if stepped:
            cand = moved(U, V, sigma, d)
            Fc = build(*cand)
            sc, cinl, css, cedge = judge(Fc, a, b, w, f0, tau)
            trail.append((sc - best) / best if best > 0 else 0.0)
        last = stepped and abs(sc - best) <= STOP * best
        if stepped and sc < best:
            (U, V, sigma), F, best, inl, ss, edge = cand, Fc, sc, cinl, css, min(edge, cedge)
            c /= 10.0
            accepted += 1
        else:
            c *= 10.0
        if last:
            break
    H, _ = normal_equations(U, V, sigma, a[inl], b[inl], w[inl], f0) if inl.any() else (np.zeros((7, 7)), None)
    flags = np.zeros(len(keep), np.uint8)
    flags[np.flatnonzero(keep)[inl]] = 1
    k = int(np.argmax(np.abs(F).reshape(-1)))
    if F.reshape(-1)[k] < 0:
        F, U = -F, U @ np.diag([-1.0, -1.0, 1.0])
    n_inl = int(inl.sum())
    return dict(status=0, F=F, U=U, V=V, sigma=sigma, info=H, inliers=flags, scores=scores, trail=trail, edge=edge, start=start,
                at=lambda hh: pick(A, hypotheses, refine_rounds, hh),
                fund=np.array([math.sqrt(best / n), n, n_inl, h, n_models, math.sqrt(e8), accepted, used, math.sqrt(ss / max(n_inl, 1)), sigma,
                               cond1(H), roots]))


def relate_uncalibrated(f0, uva, uvb, q, hypotheses, seed, tau, refine_rounds):
    return pick(score_all(f0, uva, uvb, q, hypotheses, seed, tau), hypotheses, refine_rounds)
