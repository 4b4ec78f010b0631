"""Marginalisation priors (srk_ba_marginalization_prior) stated with the existing yardsticks.

Numpy on a scene that is already in the coordinates it is used with (the normalised world of an upload).  The involved factors F
of dropping the frames D and the landmarks P are selected as include/srk_ba.h states them; their dense Gauss-Newton model over
(landmarks of P, D, K) is built from robust_ref.derivatives (the library's closed forms with information and loss weights; the
observations outside F get information 0, which makes their blocks exact zeros), prior_ref.add_terms, relpose_ref.add_terms /
add_couplings and jointprior_ref.add_terms / add_couplings; the landmarks are eliminated with constant_ref.schur at c = 0 and the
dropped frames with numpy.linalg.  Everything carries the yardsticks' factor 2 until the last line of system(), which halves it.
"""
import numpy as np

import constant_ref as kref
import jointprior_ref as jr
import prior_ref as pref
import relpose_ref as rr
import robust_ref as rob


def select(so, D, P, q=None, fac=None, sets=None):
    """(selected landmarks [bool N], single [count of landmarks of P with fewer than two weighted observations], kept frames K
    ascending, involved factors [indices], involved sets [indices]); raises ValueError for the observation refusal"""
    rp = np.asarray(so.row_ptr)
    fr = np.asarray(so.obs_frame).astype(np.int64)
    O = int(rp[-1])
    q = np.ones(O) if q is None else np.asarray(q, dtype=np.float64)
    pt = np.repeat(np.arange(so.N), np.diff(rp))
    inD = np.zeros(so.M, dtype=bool)
    inD[np.asarray(D, dtype=np.int64)] = True
    inP = np.zeros(so.N, dtype=bool)
    inP[np.asarray(P, dtype=np.int64)] = True
    if np.any(inD[fr] & (q > 0) & ~inP[pt]):
        raise ValueError("a weighted observation in a dropped frame whose landmark stays")
    nw = np.bincount(pt[q > 0], minlength=so.N)
    sel = inP & (nw >= 2)
    touched = np.zeros(so.M, dtype=bool)
    touched[fr[sel[pt] & (q > 0)]] = True
    facs = [k for k in range(fac.n)] if fac is not None else []
    facs = [k for k in facs if (inD[fac.a[k]] or inD[fac.b[k]]) and np.any(fac.info[k] != 0)]
    for k in facs:
        touched[[fac.a[k], fac.b[k]]] = True
    sts = [g for g, s in enumerate(sets.sets) if np.any(inD[s["frames"]]) and np.any(s["info"] != 0)] if sets is not None else []
    for g in sts:
        touched[sets.sets[g]["frames"]] = True
    return sel, int((inP & ~sel).sum()), np.flatnonzero(touched & ~inD), facs, sts


def system(f0, so, D, P, q=None, kind=rob.NONE, delta=None, pri=None, fac=None, sets=None):
    """dict: K, idx (the 10 M-layout variables of the slots, D first), A0 / b0 (observations and landmark priors, P eliminated),
    A1 / b1 (plus the priors on centres of D, the involved factors and sets), skipped (landmarks of P left out), cond_V (the
    largest scaled condition number of a used V_l)"""
    N, M = so.N, so.M
    rp = np.asarray(so.row_ptr)
    O = int(rp[-1])
    D = np.asarray(D, dtype=np.int64).reshape(-1)
    qf = np.ones(O) if q is None else np.asarray(q, dtype=np.float64).copy()
    sel, single, K, facs, sts = select(so, D, P, qf, fac, sets)
    pt = np.repeat(np.arange(N), np.diff(rp))
    qf[~sel[pt]] = 0.0
    g, V, U, W, _ = rob.derivatives(f0, so, kind, delta, qf)
    if pri is not None and pri.pidx.size:
        keep = sel[pri.pidx]
        g, V, U, W = pref.add_terms((g, V, U, W), so, pref.Priors(pri.pidx[keep], pri.ppos[keep], pri.pinfo[keep]))
    # a landmark whose undamped block is not positive definite is left out altogether, as the kernel leaves it out
    bad = np.zeros(N, dtype=bool)
    cond_V = 1.0
    for i in np.flatnonzero(sel):
        try:
            np.linalg.cholesky(V[i])
            ok = abs(np.linalg.det(V[i])) > 1e-12
        except np.linalg.LinAlgError:
            ok = False
        bad[i] = not ok
        if ok:
            d = np.sqrt(np.diag(V[i]))
            cond_V = max(cond_V, float(np.linalg.cond(V[i] / d[:, None] / d[None, :])))
    if bad.any():
        qf[bad[pt]] = 0.0
        g, V, U, W, _ = rob.derivatives(f0, so, kind, delta, qf)
        if pri is not None and pri.pidx.size:
            keep = (sel & ~bad)[pri.pidx]
            g, V, U, W = pref.add_terms((g, V, U, W), so, pref.Priors(pri.pidx[keep], pri.ppos[keep], pri.pinfo[keep]))
    used = sel & ~bad
    V = V.copy()
    V[~used] = np.eye(3)
    S, rhs, _ = kref.schur(so, g, V, U, W, 0.0)
    slots = np.concatenate([D, K]).astype(np.int64)
    idx = (10 * slots[:, None] + 4 + np.arange(6)[None, :]).reshape(-1)
    S0, r0 = S[np.ix_(idx, idx)], rhs[idx]
    # the host's terms: zero blocks plus the priors on centres of D, the involved factors and sets
    blocks = (np.zeros(3 * N + 10 * M), np.zeros((N, 3, 3)), np.zeros((M, 10, 10)), np.zeros((O, 3, 10)))
    Sc = np.zeros((10 * M, 10 * M))
    if pri is not None and pri.fidx.size:
        keep = np.isin(pri.fidx, D)
        blocks = pref.add_terms(blocks, so, pref.Priors(fidx=pri.fidx[keep], fpos=pri.fpos[keep], finfo=pri.finfo[keep]))
    if facs:
        sub = rr.Factors(fac.a[facs], fac.b[facs], fac.Z[facs], fac.z[facs], fac.info[facs])
        blocks = rr.add_terms(blocks, so, sub)
        rr.add_couplings(Sc, sub, so)
    if sts:
        sub = jr.Sets([sets.sets[g] for g in sts])
        blocks = jr.add_terms(blocks, so, sub)
        jr.add_couplings(Sc, sub, so)
    for j in range(M):
        Sc[10 * j:10 * j + 10, 10 * j:10 * j + 10] += blocks[2][j]
    S1 = S0 + Sc[np.ix_(idx, idx)]
    r1 = r0 - blocks[0][3 * N:][idx]
    # the scales of the comparisons: a variable's own block before anything is eliminated (the d_k of the S comparisons of the
    # other GPU tests), and the energy of F (|b_i| <= sqrt(A_ii E_F) by Cauchy-Schwarz)
    U0 = 0.5 * np.concatenate([np.diag(U[j])[4:] for j in slots])
    U1 = U0 + 0.5 * np.diag(Sc)[idx]
    E0 = rob.energy(f0, so, kind, delta, qf)
    if pri is not None and pri.pidx.size:
        keep = used[pri.pidx]
        E0 += pref.energy(pref.Priors(pri.pidx[keep], pri.ppos[keep], pri.pinfo[keep]), so)[0]
    E1 = E0
    if pri is not None and pri.fidx.size:
        keep = np.isin(pri.fidx, D)
        E1 += pref.energy(pref.Priors(fidx=pri.fidx[keep], fpos=pri.fpos[keep], finfo=pri.finfo[keep]), so)[1]
    if facs:
        E1 += rr.energy(rr.Factors(fac.a[facs], fac.b[facs], fac.Z[facs], fac.z[facs], fac.info[facs]), so)
    if sts:
        E1 += jr.energy(jr.Sets([sets.sets[g] for g in sts]), so)
    return dict(K=K, slots=slots, idx=idx, A0=0.5 * S0, b0=-0.5 * r0, A1=0.5 * S1, b1=-0.5 * r1, skipped=single + int(bad.sum()),
                used=used, cond_V=cond_V, factors=facs, sets=sts, U0=U0, U1=U1, E0=E0, E1=E1)


def scaled_cond(A):
    """condition number of a symmetric positive definite block after symmetric diagonal scaling"""
    A = 0.5 * (A + A.T)
    d = np.sqrt(np.diag(A))
    return float(np.linalg.cond(A / d[:, None] / d[None, :]))


def eliminate(A, b, d):
    """(Lam, eta) of eliminating the first 6 d variables: the Schur complement onto the rest"""
    nd = 6 * d
    if nd == 0:
        return 0.5 * (A + A.T), b.copy()
    X = np.linalg.solve(A[:nd, :nd], np.concatenate([A[:nd, nd:], b[:nd, None]], axis=1))
    Lam = A[nd:, nd:] - A[nd:, :nd] @ X[:, :-1]
    return 0.5 * (Lam + Lam.T), b[nd:] - A[nd:, :nd] @ X[:, -1]


def energy(Lam, eta, x):
    return float(x @ Lam @ x + 2.0 * eta @ x)
