"""A numpy yardstick for two-view relative pose (srk_relate_frames): the counter-based sampler, integer for
integer, and everything after it by another route than the library's.  The five-point solve takes the null space from an SVD,
eliminates the ten cubic constraints with the cubic monomials in front (numpy.linalg.solve) and reads the solutions off the
eigenvectors of the action matrix of x (Stewenius), where the library forms det B(z) after Nister and brackets its roots; the pose
comes from the SVD of E and a linear triangulation, where the library has closed forms.  Written from the formulas."""
import itertools

import numpy as np

FEW_POINTS, NO_MODEL = 1, 2
M64 = (1 << 64) - 1
STREAM = 0xD1B54A32D192ED03


def mix(seed, h, k):
    z = (seed + STREAM * (8 * h + k + 1)) & M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample(seed, h, n):
    """the six distinct ranks of hypothesis h among n weighted matches"""
    picks = []
    for k in range(6):
        r = (mix(seed, h, k) * (n - k)) >> 64
        for s in sorted(picks):
            if r >= s:
                r += 1
        picks.append(r)
    return picks


def ransac_hypotheses(e, p, s):
    return int(np.ceil(np.log(1.0 - p) / np.log(1.0 - (1.0 - e) ** s)))


def rays(K, uv, f0):
    m = np.column_stack([uv, np.full(len(uv), f0)])
    b = m @ np.linalg.inv(K).T
    return b / np.linalg.norm(b, axis=1, keepdims=True)


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def fundamental(E, Ka, Kb):
    return np.linalg.inv(Kb).T @ E @ np.linalg.inv(Ka)


def sampson(F, uva, uvb, f0):
    """the squared Sampson distances in pixels of the matches under F"""
    pa = np.column_stack([uva, np.full(len(uva), f0)])
    pb = np.column_stack([uvb, np.full(len(uvb), f0)])
    la, lb = pa @ F.T, pb @ F
    e = np.sum(pb * la, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return e * e / (la[:, 0] ** 2 + la[:, 1] ** 2 + lb[:, 0] ** 2 + lb[:, 1] ** 2)


# ---- polynomials in (x, y, z) of degree <= 3 as arrays [..., 4, 4, 4] over the exponents
def _linear(c):
    """c [..., 4] = the coefficients of x, y, z, 1"""
    p = np.zeros(c.shape[:-1] + (4, 4, 4))
    p[..., 1, 0, 0], p[..., 0, 1, 0], p[..., 0, 0, 1], p[..., 0, 0, 0] = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    return p


def _times_linear(p, c):
    """p times the linear polynomial c [..., 4]"""
    s = (Ellipsis, None, None, None)
    out = p * c[..., 3][s]
    out[..., 1:, :, :] += p[..., :-1, :, :] * c[..., 0][s]
    out[..., :, 1:, :] += p[..., :, :-1, :] * c[..., 1][s]
    out[..., :, :, 1:] += p[..., :, :, :-1] * c[..., 2][s]
    return out


CUBIC = [e for e in itertools.product(range(4), repeat=3) if sum(e) == 3]                     # ten monomials of degree 3
BASIS = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def five_point(xa, xb, polished=True):
    """all essential matrices of five pairs of rays, batched: xa, xb [H][5][3].  Returns (E [H][10][3][3], real [H][10], fragile
    [H]): real marks the solutions, fragile the samples with an eigenvalue whose imaginary part is small but not rounding."""
    H = len(xa)
    N, cons = constraints(xa, xb)
    left = np.stack([cons[(Ellipsis,) + m] for m in CUBIC], axis=-1)
    right = np.stack([cons[(Ellipsis,) + m] for m in BASIS], axis=-1)
    E = np.zeros((H, 10, 3, 3))
    real = np.zeros((H, 10), bool)
    fragile = np.zeros(H, bool)
    for h in range(H):
        try:
            G = np.linalg.solve(left[h], right[h])                         # cubic monomial = -G (basis)
        except np.linalg.LinAlgError:
            fragile[h] = True
            continue
        if not np.all(np.isfinite(G)):
            continue
        act = np.zeros((10, 10))                                           # x times the basis, in the basis
        for r, m in enumerate(BASIS):
            t = (m[0] + 1, m[1], m[2])
            if t in BASIS:
                act[r, BASIS.index(t)] = 1.0
            else:
                act[r] = -G[CUBIC.index(t)]
        w, v = np.linalg.eig(act)
        for k in range(10):
            im = abs(w[k].imag)
            if im > 1e-9 * (1.0 + abs(w[k])):
                fragile[h] |= im < 1e-5 * (1.0 + abs(w[k]))
                continue
            vec = (v[:, k] / v[9, k]).real
            Ek = vec[6] * N[h, 0] + vec[7] * N[h, 1] + vec[8] * N[h, 2] + N[h, 3]
            if np.all(np.isfinite(Ek)):
                E[h, k] = polish(Ek, N[h]) if polished else (Ek * np.sqrt(2.0) / np.linalg.norm(Ek)).reshape(3, 3)
                real[h, k] = True
    return (E, real, fragile) if polished else (E, real, fragile, N)


def _residual(E):
    return np.concatenate([(2.0 * E @ E.T @ E - np.trace(E @ E.T) * E).ravel(), [np.linalg.det(E)]])


def polish(Ek, N):
    """Newton steps on the constraints over the unit sphere of the null space (least squares of the ten constraints and c . c = 1):
    the eigenvector of the action matrix carries the error of the elimination, the solution itself is usually well conditioned"""
    c = N @ Ek
    c /= np.linalg.norm(c)
    for _ in range(4):
        E = (c @ N).reshape(3, 3)
        r = np.concatenate([_residual(E), [0.5 * (c @ c - 1.0)]])
        J = np.zeros((11, 4))
        for k in range(4):
            D = N[k].reshape(3, 3)
            S = D @ E.T
            J[:9, k] = (2.0 * (S + S.T) @ E + 2.0 * E @ E.T @ D - 2.0 * np.trace(S) * E - np.trace(E @ E.T) * D).ravel()
        J[9] = [np.sum(_cofactor(E) * N[k].reshape(3, 3)) for k in range(4)]
        J[10] = c
        step = np.linalg.lstsq(J, r, rcond=None)[0]
        if not np.all(np.isfinite(step)):
            break
        c = c - step
    E = (c @ N).reshape(3, 3)
    return E * np.sqrt(2.0) / np.linalg.norm(E)


def _cofactor(E):
    return np.array([np.cross(E[1], E[2]), np.cross(E[2], E[0]), np.cross(E[0], E[1])])


def constraints(xa, xb):
    """(N [H][4][9], the ten cubic constraints [H][10][4][4][4]) of five pairs of rays, batched"""
    H = len(xa)
    A = (xb[:, :, :, None] * xa[:, :, None, :]).reshape(H, 5, 9)
    N = np.linalg.svd(A)[2][:, 5:, :]                                      # [H][4][9]: E = x N0 + y N1 + z N2 + N3
    lin = np.moveaxis(N, 1, 2).reshape(H, 3, 3, 4)                        # entry (i, j): its four coefficients
    e = _linear(lin)                                                       # [H][3][3][4][4][4]
    eet = sum(_times_linear(e[:, :, None, m], lin[:, None, :, m]) for m in range(3))           # (E E^T)[i][k]
    tr = eet[:, 0, 0] + eet[:, 1, 1] + eet[:, 2, 2]
    cons = [2.0 * sum(_times_linear(eet[:, i, k], lin[:, k, j]) for k in range(3)) - _times_linear(tr, lin[:, i, j]) for i in range(3) for j in range(3)]
    minor = lambda a, b, c, d: _times_linear(e[:, 1, a], lin[:, 2, b]) - _times_linear(e[:, 1, c], lin[:, 2, d])  # noqa: E731
    det = _times_linear(minor(1, 2, 2, 1), lin[:, 0, 0]) - _times_linear(minor(0, 2, 2, 0), lin[:, 0, 1]) + _times_linear(minor(0, 1, 1, 0), lin[:, 0, 2])
    return N, np.stack(cons + [det], axis=1)


def decompose(E):
    """the four poses (R, T) of an essential matrix by its SVD"""
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    return [(R, s * U[:, 2]) for R in (U @ W @ Vt, U @ W.T @ Vt) for s in (1.0, -1.0)]


def depths(R, T, a, b):
    """the distances along the rays a [n][3] (frame a) and b (frame b) of the points nearest to both: least squares of
    depth_b b = depth_a R a + T"""
    ar = a @ R.T
    out = np.zeros((len(a), 2))
    for i in range(len(a)):
        out[i] = np.linalg.lstsq(np.column_stack([-ar[i], b[i]]), T, rcond=None)[0]
    return out


def pick_pose(E, a, b):
    """the pose of E with the most matches in front of both cameras: (R, T, count, mean parallax)"""
    best = None
    for R, T in decompose(E):
        front = np.all(depths(R, T, a, b) > 0.0, axis=1)
        if best is None or front.sum() > best[2]:
            ar = a[front] @ R.T
            ang = np.arctan2(np.linalg.norm(np.cross(ar, b[front]), axis=1), np.sum(ar * b[front], axis=1))
            best = (R, T, int(front.sum()), float(ang.mean()) if front.any() else np.nan)
    return best


def score_all(f0, Ka, Kb, uva, uvb, q, hypotheses, seed, tau):
    """every hypothesis of one pair: its model, its sixth-match error and its score.  A hypothesis is a function of (seed, h) and
    the pair alone, so the result at a smaller count is a prefix (pick)."""
    n_obs = len(uva)
    q = np.ones(n_obs) if q is None else np.asarray(q, float)
    on = np.flatnonzero(q > 0)
    n = len(on)
    a = dict(f0=f0, Ka=Ka, Kb=Kb, n_obs=n_obs, on=on, n=n, tau=tau, scores=np.full(hypotheses, np.inf), e6=np.full(hypotheses, np.nan),
             chosen=[None] * hypotheses, fragile=np.zeros(hypotheses, bool))
    if n < 6:
        return a
    ua, ub, w = uva[on], uvb[on], q[on]
    ra, rb = rays(Ka, ua, f0), rays(Kb, ub, f0)
    picks = np.array([sample(seed, h, n) for h in range(hypotheses)])
    with np.errstate(all="ignore"):
        Es, real, a["fragile"], N = five_point(ra[picks[:, :5]], rb[picks[:, :5]], polished=False)
    for h in range(hypotheses):
        best = np.inf
        for k in np.flatnonzero(real[h]):
            F = fundamental(Es[h, k], Ka, Kb)
            e6 = sampson(F, ua[picks[h, 5:6]], ub[picks[h, 5:6]], f0)[0]
            if np.isfinite(e6) and e6 < best:
                best, a["chosen"][h] = e6, k
        if a["chosen"][h] is None:
            continue
        E = polish(Es[h, a["chosen"][h]].ravel(), N[h])         # the choice is made among the eigenvectors, the chosen one is polished
        F = fundamental(E, Ka, Kb)
        a["chosen"][h] = (E, F)
        a["e6"][h] = sampson(F, ua[picks[h, 5:6]], ub[picks[h, 5:6]], f0)[0]
        s = w * sampson(a["chosen"][h][1], ua, ub, f0)
        a["scores"][h] = np.sum(np.where(s < tau * tau, s, tau * tau))
    a.update(ua=ua, ub=ub, w=w, ra=ra, rb=rb)
    return a


def pick(a, hypotheses):
    """the result of one pair at a hypothesis count, as include/srk_ba.h states it.  Returns a dict: status, R, T, E, related [8],
    inliers [n_obs], scores [hypotheses], fragile (a decision of some hypothesis hung on rounding), margin (the distance of the
    nearest weighted error from tau^2), at (h -> the same dict with hypothesis h as the winner)."""
    n, tau2 = a["n"], a["tau"] ** 2
    scores = a["scores"][:hypotheses]
    models = int(np.isfinite(scores).sum())

    def at(h):
        out = dict(status=0, R=np.eye(3), T=np.zeros(3), E=np.zeros((3, 3)), inliers=np.zeros(a["n_obs"], np.uint8), scores=scores,
                   fragile=bool(a["fragile"][:hypotheses].any()), related=np.array([np.nan, n, 0, np.nan, models, np.nan, 0, np.nan]), at=at)
        if n < 6 or models == 0:
            out["status"] = FEW_POINTS if n < 6 else NO_MODEL
            return out
        E, F = a["chosen"][h]
        s = a["w"] * sampson(F, a["ua"], a["ub"], a["f0"])
        inl = s < tau2
        out["inliers"][a["on"]] = inl
        out["margin"] = float(np.min(np.abs(s - tau2)))
        R, T, front, parallax = pick_pose(E, a["ra"][inl], a["rb"][inl])
        out.update(R=R, T=T, E=skew(T) @ R)
        out["related"] = np.array([np.sqrt(scores[h] / n), n, inl.sum(), h, models, np.sqrt(a["e6"][h]), front, parallax])
        return out
    return at(int(np.argmin(scores)) if models else 0)


def relate(f0, Ka, Kb, uva, uvb, q, hypotheses, seed, tau):
    """one pair at one hypothesis count"""
    return pick(score_all(f0, Ka, Kb, uva, uvb, q, hypotheses, seed, tau), hypotheses)


def rotation_angle(Ra, Rb):
    c = 0.5 * (np.trace(Ra.T @ Rb) - 1.0)
    return float(np.arccos(np.clip(c, -1.0, 1.0))) if abs(c) < 0.999999 else float(np.linalg.norm(Ra - Rb) / np.sqrt(2.0))


def direction_angle(Ta, Tb):
    return float(np.arctan2(np.linalg.norm(np.cross(Ta, Tb)), Ta @ Tb))


def essential_distance(E, Et):
    """min over the sign of the Frobenius distance between two essential matrices scaled to norm sqrt(2)"""
    a = E * np.sqrt(2.0) / np.linalg.norm(E)
    b = Et * np.sqrt(2.0) / np.linalg.norm(Et)
    return float(min(np.linalg.norm(a - b), np.linalg.norm(a + b)))
