"""Joint Gaussian pose priors over sets of frames (srk_ba_set_joint_pose_priors) stated with the oracle's entry points.

Set g holds k frames (strictly ascending), each with a linearisation pose (Rbar_i, Cbar_i), a mean m (6 k) and a symmetric
positive semi-definite information matrix L (6 k x 6 k; variable order frame by frame, [t; r] inside a frame).  With R_i the
world -> camera rotation and C_i = -R_i^T T_i the centre:

    r_i = [C_i - Cbar_i; Log(R_i^T Rbar_i)],   E = (what E is without the priors) + sum_g (r_g - m_g)^T L_g (r_g - m_g)

The oracle's gradient and blocks carry the factor 2 (first_deriv / second_deriv in oracle/ba_oracle.c), so a set adds
2 J_i^T L_ii J_i to the pose part (variables 4..9 of ten) of U_i, 2 J_i^T (L (r - m))_i to the frame gradient, and the block
2 J_i^T L_ij J_j couples frames i and j in the reduced camera system, undamped and outside the Schur complement.  The Jacobians
are those of orc.apply_corrections: [Tx Ty Tz] is added to the centre, the rotation correction multiplies the direct rotation
R^T from the left and leaves the centre alone, so J_i = diag(I, Jl^-1(r_r,i)) with Jl^-1(phi) = I - [phi]x / 2 + k [phi]x^2.

Everything here is numpy on sets that are already in the coordinates of the scene they are used with.  The step is that of
tests/relpose_ref.py (constant_ref.schur plus couplings, restricted to the free variables); relative-pose factors and position
priors may be given beside the sets.  The LM loop is lm_ref.loop.
"""
import numpy as np

import constant_ref as kref
import lm_ref
import prior_ref as pref
import relpose_ref as rr
import so3_ref as so3


def jl_inv(phi):
    """inverse left Jacobian of SO(3): Log(Exp(d) Exp(phi)) = phi + Jl^-1(phi) d + O(d^2) (tests/so3_ref.py)"""
    return so3.jl_inv(phi)


class Sets:
    """a list of sets: frames [k], R [k][3][3], C [k][3], mean [6k], info [6k][6k]"""

    def __init__(self, sets=()):
        self.sets = []
        for s in sets:
            fr = np.asarray(s["frames"], dtype=np.int32).ravel().copy()
            k = fr.size
            m = s.get("mean")
            self.sets.append(dict(frames=fr, R=np.asarray(s["R"], dtype=np.float64).reshape(k, 3, 3).copy(),
                                  C=np.asarray(s["C"], dtype=np.float64).reshape(k, 3).copy(),
                                  mean=np.zeros(6 * k) if m is None else np.asarray(m, dtype=np.float64).reshape(6 * k).copy(),
                                  info=np.asarray(s["info"], dtype=np.float64).reshape(6 * k, 6 * k).copy()))
            assert np.all(np.diff(fr) > 0)

    @property
    def n(self):
        return len(self.sets)

    def copy(self):
        return Sets(self.sets)

    def frames(self):
        return np.unique(np.concatenate([s["frames"] for s in self.sets])) if self.sets else np.zeros(0, np.int32)

    def set_on(self, gpu, keep_gauge=1):
        gpu.set_joint_pose_priors(self.sets, keep_gauge=bool(keep_gauge))


def linearised_at(so, frames, info, mean=None):
    """one set over the given frames, linearised at the scene's current poses"""
    R, Cn = rr.poses(so)
    fr = np.asarray(frames, dtype=np.int32)
    return dict(frames=fr, R=R[fr].copy(), C=Cn[fr].copy(), mean=mean, info=info)


def residual(s, so):
    """r - m [6k] of one set"""
    R, Cn = rr.poses(so)
    k = s["frames"].size
    r = np.zeros(6 * k)
    for i, j in enumerate(s["frames"]):
        r[6 * i:6 * i + 3] = Cn[j] - s["C"][i]
        r[6 * i + 3:6 * i + 6] = rr.log_so3(R[j].T @ s["R"][i])
    return r - s["mean"]


def residuals(sets, so):
    return [residual(s, so) for s in sets.sets]


def energy(sets, so):
    return float(sum(r @ s["info"] @ r for s, r in zip(sets.sets, residuals(sets, so))))


def jacobian(s, so):
    """(r - m [6k], J [6k][6k] block diagonal) of one set over the pose variables [Tx Ty Tz Wx Wy Wz] of its frames"""
    e = residual(s, so)
    k = s["frames"].size
    J = np.zeros((6 * k, 6 * k))
    for i in range(k):
        J[6 * i:6 * i + 3, 6 * i:6 * i + 3] = np.eye(3)
        J[6 * i + 3:6 * i + 6, 6 * i + 3:6 * i + 6] = jl_inv(e[6 * i + 3:6 * i + 6] + s["mean"][6 * i + 3:6 * i + 6])
    return e, J


def add_terms(blocks, so, sets):
    """the (gradE, V, U, W) given plus the sets' terms in the frame blocks and frame gradients (copies)"""
    gradE, V, U, W = blocks[:4]
    g, U = gradE.copy(), U.copy()
    gf = g[3 * so.N:].reshape(-1, 10)
    for s in sets.sets:
        e, J = jacobian(s, so)
        H = 2.0 * J.T @ s["info"] @ J
        gs = 2.0 * J.T @ (s["info"] @ e)
        for i, j in enumerate(s["frames"]):
            U[j, 4:, 4:] += H[6 * i:6 * i + 6, 6 * i:6 * i + 6]
            gf[j, 4:] += gs[6 * i:6 * i + 6]
    return g, V, U, W


def coupled_pairs(s):
    """the slot pairs (i, j), i > j, whose 6 x 6 block of L is not all zeros"""
    k = s["frames"].size
    return [(i, j) for i in range(1, k) for j in range(i) if np.any(s["info"][6 * i:6 * i + 6, 6 * j:6 * j + 6] != 0)]


def frame_pairs(sets):
    """the unordered frame pairs the sets couple, (lo, hi), each once"""
    out = set()
    for s in sets.sets:
        if not np.any(s["info"] != 0):
            continue
        for i, j in coupled_pairs(s):
            out.add((int(s["frames"][j]), int(s["frames"][i])))
    return sorted(out)


def couplings(sets, so):
    """[(frame a, frame b, 2 J_a^T L_ab J_b)]: the blocks (a, b) of the reduced camera system over the pose variables"""
    out = []
    for s in sets.sets:
        _, J = jacobian(s, so)
        H = 2.0 * J.T @ s["info"] @ J
        for i, j in coupled_pairs(s):
            out.append((int(s["frames"][i]), int(s["frames"][j]), H[6 * i:6 * i + 6, 6 * j:6 * j + 6]))
    return out


def add_couplings(S, sets, so):
    """S [10M][10M] (both triangles) plus the coupling blocks"""
    for a, b, Cb in couplings(sets, so):
        S[10 * a + 4:10 * a + 10, 10 * b + 4:10 * b + 10] += Cb
        S[10 * b + 4:10 * b + 10, 10 * a + 4:10 * a + 10] += Cb.T
    return S


def normalised(sets, nrm):
    """the sets in the normalised world X_n = s (R0 X + T0): Cbar_n = s (R0 Cbar + T0), Rbar_n = Rbar R0^T, m_n = D m,
    L_n = D^-T L D^-1 with D = diag(s R0, R0) per frame (numpy; the library's host map is compared against this)"""
    s = float(nrm.world_scale)
    R0 = np.array(list(nrm.R0)).reshape(3, 3)
    T0 = np.array(list(nrm.T0))
    out = []
    for st in sets.sets:
        k = st["frames"].size
        D = np.zeros((6 * k, 6 * k))
        for i in range(k):
            D[6 * i:6 * i + 3, 6 * i:6 * i + 3] = s * R0
            D[6 * i + 3:6 * i + 6, 6 * i + 3:6 * i + 6] = R0
        Di = np.linalg.inv(D)
        L = Di.T @ st["info"] @ Di
        out.append(dict(frames=st["frames"], R=st["R"] @ R0.T, C=s * (st["C"] @ R0.T + T0), mean=D @ st["mean"], info=0.5 * (L + L.T)))
    return Sets(out)


def step(orc, f0, so, c, sets, keep_gauge, fv=10, fconst=None, pconst=None, want_system=False, derivatives=None, pri=None, fac=None):
    """one attempt at damping c on the normalised oracle scene so with the sets (and the relative-pose factors fac and the
    position priors pri) in so's coordinates.  Returns the dict of relpose_ref.step."""
    fconst = np.zeros(so.M, dtype=bool) if fconst is None else fconst
    pconst = np.zeros(so.N, dtype=bool) if pconst is None else pconst
    base = orc.derivatives(f0, so) if derivatives is None else derivatives(so)
    blocks = base[:4] if pri is None else pref.add_terms(base[:4], so, pri)
    if fac is not None:
        blocks = rr.add_terms(blocks, so, fac)
    blocks = add_terms(blocks, so, sets)
    out = step_restricted(so, kref.restrict_all(so, blocks, fconst, pconst, fv), c, sets, fconst, keep_gauge, fv, want_system, fac)
    out["blocks"] = blocks
    return out


def step_restricted(so, restricted, c, sets, fconst, keep_gauge, fv=10, want_system=False, fac=None):
    g, V, U, W = restricted
    fixed = kref.fixed_vars(so.M, fconst, keep_gauge, fv)
    S, rhs, Einv = kref.schur(so, g, V, U, W, c)
    if fac is not None:
        rr.add_couplings(S, fac, so)
    add_couplings(S, sets, so)
    ok, corr = kref.solve(so, g, W, S, rhs, Einv, fixed)
    out = dict(g=g, V=V, U=U, W=W, fixed=fixed, S=S, rhs=rhs, ok=ok, corr=corr)
    if want_system:
        x = kref.refined_solution(S, rhs, fixed)
        out.update(dc_exact=x, d_solver=kref.rel_err(corr[3 * so.N:][~fixed], x[~fixed]) if np.any(~fixed) else 0.0)
    return out


def compute_inplace(orc, f0, so, sets_world, keep_gauge=1, fv=10, fconst=None, pconst=None, allowed_err_change=None,
                    max_hessian_factor=None, max_iterations=0):
    """lm_ref.loop around the step with sets.  sets_world: the sets in the coordinates of so as given; so is changed in place
    (normalised, optimised, normalisation reverted; constant blocks restored bit for bit).  Returns (rc, report)."""
    rep = lm_ref.Report()
    fconst = np.zeros(so.M, dtype=bool) if fconst is None else fconst
    pconst = np.zeros(so.N, dtype=bool) if pconst is None else pconst
    before = (so.points[pconst].copy(), so.cam_R[fconst].copy(), so.cam_T[fconst].copy())
    ok, nrm = orc.normalize(so)
    if not ok:
        return 1, rep
    sets = normalised(sets_world, nrm)
    held = (so.points[pconst].copy(), so.cam_R[fconst].copy(), so.cam_T[fconst].copy())

    def total():
        return orc.reproj_error(f0, so)[0] + energy(sets, so)

    def prepare():
        return kref.restrict_all(so, add_terms(orc.derivatives(f0, so)[:4], so, sets), fconst, pconst, fv)

    def solve(restricted, c):
        res = step_restricted(so, restricted, c, sets, fconst, keep_gauge, fv)
        return res["ok"], res["corr"]

    def apply(corr):
        orc.apply_corrections(so, corr)
        so.points[pconst], so.cam_R[fconst], so.cam_T[fconst] = held

    rc = lm_ref.loop(rep, so, energy=total, prepare=prepare, solve=solve, apply=apply, allowed_err_change=allowed_err_change,
                     max_hessian_factor=max_hessian_factor, max_iterations=max_iterations)
    orc.revert(so, nrm)
    so.points[pconst], so.cam_R[fconst], so.cam_T[fconst] = before
    return rc, rep
