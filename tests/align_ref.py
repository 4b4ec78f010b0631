"""The numpy yardstick of map alignment: the same counter-based sampler, Horn's triad hypothesis and the MSAC
score as the kernels, and a local optimisation by Umeyama's SVD route (numpy.linalg.svd with the determinant sign), which is
independent of the device's quaternion-Jacobi route.  Slow and plain on purpose."""
import numpy as np

MASK = (1 << 64) - 1
ODD = 0xA0761D6478BD642F
FEW_POINTS, NO_MODEL = 1, 2


def mix(seed, h, k):
    z = (seed + ODD * (4 * h + k + 1)) & MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def sample(seed, h, n):
    """three distinct ranks below n: draw k is umulhi64(mix, n - k), bumped past the earlier picks in ascending order"""
    picks = []
    for k in range(3):
        r = (mix(seed & MASK, h, k) * (n - k)) >> 64
        for s in sorted(picks):
            if r >= s:
                r += 1
        picks.append(r)
    return picks


def triad(p):
    d1, d2 = p[1] - p[0], p[2] - p[0]
    c = np.cross(d1, d2)
    ok = np.isfinite(c @ c) and c @ c > 1e-12 * (d1 @ d1) * (d2 @ d2)
    if not ok:
        return None
    e1, e3 = d1 / np.linalg.norm(d1), c / np.linalg.norm(c)
    return np.column_stack([e1, np.cross(e3, e1), e3])


def hypothesis(a3, b3, with_scale):
    """(s, R, t) of a sample of three, or None"""
    A, B = triad(a3), triad(b3)
    if A is None or B is None:
        return None
    R = B @ A.T
    am, bm = a3.mean(0), b3.mean(0)
    s = np.sqrt(((b3 - bm) ** 2).sum() / ((a3 - am) ** 2).sum()) if with_scale else 1.0
    t = bm - s * R @ am
    if not (np.isfinite(s) and s > 0 and np.all(np.isfinite(t)) and np.all(np.isfinite(R))):
        return None
    return s, R, t


def terms(model, a, b, q, tau):
    """(the terms min(q r^2, tau^2), the inlier flags, q r^2, r^2) of every correspondence"""
    s, R, t = model
    r2 = ((b - (s * a @ R.T + t)) ** 2).sum(1)
    z = q * r2
    inl = z < tau * tau
    return np.where(inl, z, tau * tau), inl, z, r2


def umeyama(a, b, w, with_scale):
    """the weighted least-squares similarity by the SVD route: (s, R, t), and the eigenvalue gap of Horn's matrix from the
    singular values (lambda1 = s1 + s2 + d s3, lambda2 = s1 - s2 - d s3)"""
    W = w.sum()
    am, bm = (w[:, None] * a).sum(0) / W, (w[:, None] * b).sum(0) / W
    da, db = a - am, b - bm
    M = (w[:, None] * db).T @ da
    U, S, Vt = np.linalg.svd(M)
    d = 1.0 if np.linalg.det(U @ Vt) > 0 else -1.0
    D = np.diag([1.0, 1.0, d])
    R = U @ D @ Vt
    va = (w * (da ** 2).sum(1)).sum()
    s = (S[0] + S[1] + d * S[2]) / va if with_scale else 1.0
    lam1 = S[0] + S[1] + d * S[2]
    gap = 2.0 * (S[1] + d * S[2]) / abs(lam1)
    return (s, R, bm - s * R @ am), gap


def align_set(a, b, q, hypotheses, tau, seed, with_scale=True, refine_rounds=2):
    """One set.  A dict: status, s, R, t, aligned [8], inliers [n_obs] (bool), scores [hypotheses]; and under "stage" the same of the
    hypothesis stage alone (refine_rounds = 0).  edge: the smallest |q r^2 / tau^2 - 1| at any model whose inliers were taken;
    margin: the smallest relative distance between a candidate's score and the score it had to beat."""
    a, b = np.asarray(a, float).reshape(-1, 3), np.asarray(b, float).reshape(-1, 3)
    q = np.ones(len(a)) if q is None else np.asarray(q, float)
    on = np.flatnonzero(q > 0)
    n = len(on)
    A, Bt, Q = a[on], b[on], q[on]
    scores = np.full(hypotheses, np.inf)

    def result(status, model, aligned, inl):
        flags = np.zeros(len(a), bool)
        if inl is not None:
            flags[on] = inl
        return dict(status=status, s=model[0], R=model[1], t=model[2], aligned=np.array(aligned, float), inliers=flags, scores=scores)
    none = (1.0, np.eye(3), np.zeros(3))
    nan = np.nan
    if n < 3:
        out = result(FEW_POINTS, none, [nan, n, 0, nan, 0, 0, nan, nan], None)
        out["stage"] = out
        return out
    models = {}
    for h in range(hypotheses):
        r = sample(seed, h, n)
        m = hypothesis(A[r], Bt[r], with_scale)
        if m is None:
            continue
        models[h] = m
        scores[h] = terms(m, A, Bt, Q, tau)[0].sum()
    if not models:
        out = result(NO_MODEL, none, [nan, n, 0, nan, 0, 0, nan, nan], None)
        out["stage"] = out
        return out
    win = int(np.argmin(scores))      # the first of equal scores: the smaller h
    cur, best = models[win], scores[win]

    def summary(model, score, rounds, gap):
        _, inl, _, r2 = terms(model, A, Bt, Q, tau)
        k = int(inl.sum())
        return result(0, model, [np.sqrt(score / n), n, k, win, len(models), rounds, gap, np.sqrt(r2[inl].sum() / k) if k else nan], inl)
    stage = summary(cur, best, 0, nan)
    rounds, gap = 0, nan
    edge = [np.abs(terms(cur, A, Bt, Q, tau)[2] / (tau * tau) - 1.0).min()]     # how near a correspondence comes to the threshold
    margin = []                                                                # how near a candidate's score comes to the best
    for _ in range(refine_rounds):
        inl = terms(cur, A, Bt, Q, tau)[1]
        if inl.sum() < 3:
            break
        cand, g = umeyama(A[inl], Bt[inl], Q[inl], with_scale)
        if not (np.isfinite(cand[0]) and cand[0] > 0 and np.all(np.isfinite(cand[1])) and np.all(np.isfinite(cand[2]))):
            break
        sc = terms(cand, A, Bt, Q, tau)[0].sum()
        margin.append(abs(sc - best) / best if best > 0 else np.inf)
        if not sc < best:
            break
        cur, best, gap, rounds = cand, sc, g, rounds + 1
        edge.append(np.abs(terms(cur, A, Bt, Q, tau)[2] / (tau * tau) - 1.0).min())
    out = summary(cur, best, rounds, gap)
    out["stage"] = stage
    out["edge"], out["margin"] = float(min(edge)), float(min(margin + [np.inf]))
    stage["edge"], stage["margin"] = float(edge[0]), np.inf
    return out


def score_at(model, a, b, q, tau):
    """the score of a set at a model: over the weighted correspondences"""
    a, b = np.asarray(a, float).reshape(-1, 3), np.asarray(b, float).reshape(-1, 3)
    q = np.ones(len(a)) if q is None else np.asarray(q, float)
    on = q > 0
    return float(terms(model, a[on], b[on], q[on], tau)[0].sum())


def distance(model, ref, b):
    """the distance of two similarities: the largest of the rotation angle, |s / s_ref - 1| and |t - t_ref| over the largest |b|"""
    s, R, t = model
    s0, R0, t0 = ref
    D = np.asarray(R).reshape(3, 3) @ np.asarray(R0).reshape(3, 3).T
    angle = np.arctan2(np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]) / 2.0, (np.trace(D) - 1.0) / 2.0)
    big = max(float(np.linalg.norm(np.asarray(b, float).reshape(-1, 3), axis=1).max()) if np.size(b) else 1.0, 1e-300)
    return float(max(abs(angle), abs(s / s0 - 1.0), np.linalg.norm(np.asarray(t) - np.asarray(t0)) / big))
