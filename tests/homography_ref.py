"""A numpy yardstick for the two-view homography by another route than the library's: the sampler integer for
integer, the four-point model from the SVD null space of the 8 x 9 DLT matrix with Hartley normalisation, the score from the
formula, the rounds as a Gauss-Newton over the nine entries of G by lstsq with the scale direction projected out, the same inlier
re-selection and acceptance rule, and the decomposition through numpy's SVD.  Nothing here is compiled."""
import math

import numpy as np

MASK = (1 << 64) - 1
COLLINEAR = 1e-9
DET = 1e-12
GAP = 1e-10
# A score is a sum of at most 200 terms, so two routes to it differ by some 200 eps = 4e-14 relative.  A candidate's score within TIE
# (25 times that) of the score it has to beat: rounding decides, either way is right.  From CLEAR on (250 times) the decision is
# clear; the cases keep out of the band between the two.
TIE = 1e-12
CLEAR = 1e-11
EXACT_FIT = 1e-12   # (1e-6 px)^2 per match, the bound a model is held to: a score below it is an exact fit


def mix(seed, h, k):
    z = (seed + 0xE7037ED1A0B428DB * (4 * h + k + 1)) & MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def sample(seed, h, n):
    """four distinct ranks below n: draw k is uniform among the n - k ranks not yet picked"""
    picks = []
    for k in range(4):
        r = (mix(seed, h, k) * (n - k)) >> 64
        for s in sorted(picks):
            if r >= s:
                r += 1
        picks.append(r)
    return picks


def ransac_hypotheses(share, confidence, sample_size):
    return int(math.ceil(math.log(1.0 - confidence) / math.log(1.0 - (1.0 - share) ** sample_size)))


def homog(uv, f0):
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    return np.column_stack([uv, np.full(len(uv), float(f0))])


def project(G, uv, f0):
    y = homog(uv, f0) @ G.T
    with np.errstate(divide="ignore", invalid="ignore"):
        return f0 * y[:, :2] / y[:, 2:3], y[:, 2]


def _hartley(uv):
    c = uv.mean(axis=0)
    s = math.sqrt(2.0) / max(np.sqrt(((uv - c) ** 2).sum(axis=1)).mean(), 1e-300)
    return np.array([[s, 0.0, -s * c[0]], [0.0, s, -s * c[1]], [0.0, 0.0, 1.0]])


def triple_margin(p):
    """the smallest |det| / (product of the column norms) over the four triples of the homogeneous points p [4][3]"""
    out = np.inf
    for skip in range(4):
        t = np.delete(p, skip, axis=0)
        out = min(out, abs(np.linalg.det(t)) / np.prod(np.linalg.norm(t, axis=1)))
    return out


def dlt_model(uva, uvb, f0):
    """G (norm 1, (G p_a0)_3 > 0) of four matches by the DLT, or None by the library's rules; and the sample's collinearity margin"""
    pa, pb = homog(uva, f0), homog(uvb, f0)
    margin = min(triple_margin(pa), triple_margin(pb))
    if not margin > COLLINEAR:
        return None, margin
    Ta, Tb = _hartley(uva), _hartley(uvb)
    a = np.column_stack([uva, np.ones(4)]) @ Ta.T
    b = np.column_stack([uvb, np.ones(4)]) @ Tb.T
    rows = []
    for x, y in zip(a, b):
        rows.append(np.concatenate([np.zeros(3), -y[2] * x, y[1] * x]))
        rows.append(np.concatenate([y[2] * x, np.zeros(3), -y[0] * x]))
    Gn = np.linalg.svd(np.array(rows))[2][-1].reshape(3, 3)
    # normalised pixels (u, v, 1) -> homogeneous pixels (u, v, f0)
    S = np.diag([1.0, 1.0, 1.0 / f0])
    G = np.diag([1.0, 1.0, f0]) @ np.linalg.inv(Tb) @ Gn @ Ta @ S
    G /= np.linalg.norm(G)
    z = pa @ G[2]
    if not (np.all(z > 0) or np.all(z < 0)) or not np.all(np.isfinite(G)):
        return None, margin
    if z[0] < 0:
        G = -G
    if not abs(np.linalg.det(G)) > DET:
        return None, margin
    return G, margin


def errors(G, uva, uvb, f0):
    """s [n], the symmetric transfer error in pixels squared, and the mask of the matches in front of both images"""
    fwd, zf = project(G, uva, f0)
    Gi = np.linalg.inv(G)
    bwd, zb = project(Gi, uvb, f0)
    with np.errstate(invalid="ignore"):
        s = ((fwd - uvb) ** 2).sum(axis=1) + ((bwd - uva) ** 2).sum(axis=1)
        front = (zf > 0) & (zb * 1.0 > 0) & np.isfinite(s)
    return s, front


def judge(G, uva, uvb, q, f0, tau):
    """score, inlier mask, the inliers' sum of s, and the distance of the nearest q s from tau^2 (relative)"""
    s, front = errors(G, uva, uvb, f0)
    w = q * s
    inl = front & (w < tau * tau)
    edge = np.abs(np.where(front, w, np.inf) / (tau * tau) - 1.0).min() if len(w) else np.inf
    return float(np.where(inl, w, tau * tau).sum()), inl, float(s[inl].sum()), float(edge)


def gauss_newton_step(G, uva, uvb, q, f0):
    """one step on the symmetric transfer error of the given matches over the nine entries of G: lstsq (the scale direction is its
    null space), then the multiple of G taken out that makes tr(G^-1 dG) = 0, the library's traceless update"""
    pa, pb = homog(uva, f0), homog(uvb, f0)
    Gi = np.linalg.inv(G)
    rows, res = [], []
    for a, b, ua, ub, w in zip(pa, pb, uva, uvb, np.sqrt(q)):
        y, x = G @ a, Gi @ b
        dy = f0 / y[2] * np.array([[1.0, 0.0, -y[0] / y[2]], [0.0, 1.0, -y[1] / y[2]]])
        dx = f0 / x[2] * np.array([[1.0, 0.0, -x[0] / x[2]], [0.0, 1.0, -x[1] / x[2]]])
        # d(G a) / dG_ij = a_j e_i;  d(Gi b) = -Gi dG x
        Jf = np.einsum("ri,j->rij", dy, a).reshape(2, 9)
        Jb = -np.einsum("ri,j->rij", dx @ Gi, x).reshape(2, 9)
        rows += [w * Jf, w * Jb]
        res += [w * (f0 * y[:2] / y[2] - ub), w * (f0 * x[:2] / x[2] - ua)]
    d = np.linalg.lstsq(np.vstack(rows), -np.concatenate(res), rcond=1e-12)[0].reshape(3, 3)
    d -= np.trace(Gi @ d) / 3.0 * G
    Gn = G + d
    return Gn / np.linalg.norm(Gn)


def nearest_rotation(M):
    U, _, Vt = np.linalg.svd(M)
    return U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt


def decompose(H, xa, xb, q=None):
    """H = R + (T/d) N^T through numpy's SVD: (H normalised and signed, gap, [(R, T, N, front)]) with the candidate that has more
    rays in front first; one candidate (R, 0, 0, 0) when gap <= GAP"""
    q = np.ones(len(xa)) if q is None else q
    sv = np.linalg.svd(H, compute_uv=False)
    H = H / sv[1]
    if (q * np.einsum("ni,ij,nj->n", xb, H, xa)).sum() < 0:
        H = -H
    _, s, Vt = np.linalg.svd(H)
    w = s ** 2
    gap = w[0] - w[2]
    if not gap > GAP:
        return H, gap, [(nearest_rotation(H), np.zeros(3), np.zeros(3), 0)]
    v1, v2, v3 = Vt[0], Vt[1], Vt[2]
    if np.linalg.det(Vt) < 0:
        v3 = -v3
    out = []
    for sg in (1.0, -1.0):
        u = (math.sqrt(max(1.0 - w[2], 0.0)) * v1 + sg * math.sqrt(max(w[0] - 1.0, 0.0)) * v3) / math.sqrt(gap)
        N = np.cross(v2, u)
        U = np.column_stack([v2, u, N])
        W = np.column_stack([H @ v2, H @ u, np.cross(H @ v2, H @ u)])
        R = nearest_rotation(W @ U.T)
        ahead = int((xa @ N > 0).sum())
        if 2 * ahead < len(xa):
            N, ahead = -N, len(xa) - ahead
        out.append((R, (H - R) @ N, N, ahead))
    if out[1][3] > out[0][3]:
        out.reverse()
    return H, gap, out


def score_all(f0, Ka, Kb, uva, uvb, q, hypotheses, seed, tau):
    """every hypothesis' model and score of one pair: what pick() needs"""
    uva, uvb = np.asarray(uva, float).reshape(-1, 2), np.asarray(uvb, float).reshape(-1, 2)
    keep = np.ones(len(uva), bool) if q is None else np.asarray(q) > 0
    w = np.ones(int(keep.sum())) if q is None else np.asarray(q, float)[keep]
    a, b = uva[keep], uvb[keep]
    n = len(a)
    models, scores, margin = [None] * hypotheses, np.full(hypotheses, np.inf), np.inf
    if n >= 4:
        for h in range(hypotheses):
            r = sample(seed, h, n)
            G, m = dlt_model(a[r], b[r], f0)
            margin = min(margin, abs(math.log10(max(m, 1e-300) / COLLINEAR)))
            if G is not None:
                models[h] = G
                scores[h] = judge(G, a, b, w, f0, tau)[0]
    return dict(f0=f0, Ka=np.asarray(Ka, float).reshape(3, 3), Kb=np.asarray(Kb, float).reshape(3, 3), a=a, b=b, w=w, keep=keep, tau=tau, n=n,
                models=models, scores=scores, collinear_margin=margin)


def _finish(A, G, h, n_models, rounds, score, inl, ss, edge):
    """the outputs at a model"""
    keep, n = A["keep"], A["n"]
    flags = np.zeros(len(keep), np.uint8)
    flags[np.flatnonzero(keep)[inl]] = 1
    Kai, Kbi = np.linalg.inv(A["Ka"]), np.linalg.inv(A["Kb"])
    xa, xb = homog(A["a"][inl], A["f0"]) @ Kai.T, homog(A["b"][inl], A["f0"]) @ Kbi.T
    H, gap, poses = decompose(Kbi @ G @ A["Ka"], xa, xb, A["w"][inl])
    return dict(status=0, G=G, H=H, poses=poses, n_poses=len(poses), inliers=flags, edge=edge, gap=gap,
                homog=np.array([math.sqrt(score / n), n, int(inl.sum()), h, n_models, rounds, gap, math.sqrt(ss / max(int(inl.sum()), 1))]))


def pick(A, hypotheses, refine_rounds):
    """the yardstick's result of a pair at a hypothesis count (a prefix of the same hypotheses): the winner, the rounds, the outputs.
    y["at"](h, rounds) is the result had hypothesis h won and `rounds` rounds been accepted; y["trail"] the rounds' candidates with
    their margins (relative decrease of the score they had to beat)."""
    n, keep = A["n"], A["keep"]
    scores = A["scores"][:hypotheses]
    n_models = int(np.isfinite(scores).sum())
    if n < 4 or n_models == 0:
        return dict(status=1 if n < 4 else 2, homog=np.array([np.nan, n, 0, np.nan, n_models, 0, np.nan, np.nan]), inliers=np.zeros(len(keep), np.uint8),
                    scores=scores, n_poses=0)

    def walk(h, stop_at=None):
        """the rounds from hypothesis h.  Returns (result, trail, allowed round counts).  The walk goes on through a rejection
        that is a tie, so that a result exists for either decision; stop_at: the round count to report."""
        a, b, w, f0, tau = A["a"], A["b"], A["w"], A["f0"], A["tau"]
        G = A["models"][h]
        best, inl, ss, edge = judge(G, a, b, w, f0, tau)
        states = [(G, best, inl, ss, edge)]
        trail, own = [], None
        for k in range(refine_rounds):
            if inl.sum() < 4:
                break
            try:
                cand = gauss_newton_step(G, a[inl], b[inl], w[inl], f0)
            except np.linalg.LinAlgError:
                break
            if not np.all(np.isfinite(cand)) or not abs(np.linalg.det(cand)) > DET:
                break
            sc, cinl, css, cedge = judge(cand, a, b, w, f0, tau)
            # below the floor every score is the rounding of an exact fit: a tie
            margin = 0.0 if max(best, sc) < EXACT_FIT * n else (best - sc) / best
            trail.append(margin)
            if not sc < best and own is None:
                own = k          # the yardstick's own walk stops here
            if margin < -TIE:
                break            # clearly no better: the rounds stop on either side
            G, best, inl, ss, edge = cand, sc, cinl, css, cedge
            states.append((G, sc, inl, ss, edge))
        if own is None:
            own = len(states) - 1
        # states[r] exists when every round before r was accepted clearly or was a tie; r rounds are a right answer when the
        # walk ended there or round r itself was a tie
        allowed = [r for r in range(len(states)) if r == len(states) - 1 or abs(trail[r]) <= TIE]
        r = own if stop_at is None else stop_at
        G, sc, inl, ss, edge = states[r]
        out = _finish(A, G, h, n_models, r, sc, inl, ss, min(s[4] for s in states[:r + 1]))
        return out, trail, allowed

    h = int(np.argmin(scores))
    y, trail, allowed = walk(h)
    y.update(scores=scores, trail=trail, allowed=allowed, walk=walk)
    y["at"] = lambda hh, rr: walk(hh, rr)[0]
    return y


def relate_homography(f0, Ka, Kb, uva, uvb, q, hypotheses, seed, tau, refine_rounds):
    return pick(score_all(f0, Ka, Kb, uva, uvb, q, hypotheses, seed, tau), hypotheses, refine_rounds)


def corner_distance(G, G0, f0, width=640.0, height=480.0):
    """the largest distance in pixels between the images of the four corners of a frame under two homographies"""
    c = np.array([[0.0, 0.0], [width, 0.0], [0.0, height], [width, height]])
    return float(np.sqrt(((project(G, c, f0)[0] - project(G0, c, f0)[0]) ** 2).sum(axis=1)).max())
