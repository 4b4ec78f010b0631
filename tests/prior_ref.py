"""Gaussian position priors (srk_ba_set_position_priors) stated with the oracle's entry points.

The objective is E = (the oracle's reprojection sum, or the robust / weighted energy of the existing refs)
+ sum_i (X_i - Xbar_i)^T L_i (X_i - Xbar_i) + sum_j (C_j - Cbar_j)^T L_j (C_j - Cbar_j), C_j = -R_j^T T_j.  The oracle's gradient
and blocks are the first derivatives and the Gauss-Newton second derivatives of E with the factor 2 (first_deriv /
second_deriv in oracle/ba_oracle.c), so a landmark prior adds 2 L to V_i and 2 L (X_i - Xbar_i) to the landmark's gradient, a
frame prior 2 L to the [Tx Ty Tz] part of U_j (variables 4..6 of ten: orc.apply_corrections adds the translation correction
to the direct translation -R^T T, the centre, and the rotation update leaves it alone) and 2 L (C_j - Cbar_j) to those gradient
entries.  Everything here is numpy on priors that are already in the coordinates of the scene they are used with.

The step is then the one of tests/constant_ref.py: orc.two_phase with the gauge kept, its dense numpy Schur complement over
all 10 M frame variables without it.  The LM loop is lm_ref.loop.
"""
import numpy as np

import constant_ref as kref
import lm_ref


def full(info6):
    """[n][6] (xx xy xz yy yz zz) -> [n][3][3]"""
    a = np.asarray(info6, dtype=np.float64).reshape(-1, 6)
    L = np.zeros((a.shape[0], 3, 3))
    for k, (r, c) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        L[:, r, c] = a[:, k]
        L[:, c, r] = a[:, k]
    return L


def six(L):
    L = np.asarray(L, dtype=np.float64).reshape(-1, 3, 3)
    return np.stack([L[:, 0, 0], L[:, 0, 1], L[:, 0, 2], L[:, 1, 1], L[:, 1, 2], L[:, 2, 2]], axis=1)


class Priors:
    """landmark priors (pidx [n], ppos [n][3], pinfo [n][3][3]) and frame-centre priors (fidx, fpos, finfo), indices ascending"""

    def __init__(self, pidx=None, ppos=None, pinfo=None, fidx=None, fpos=None, finfo=None):
        self.pidx = np.zeros(0, np.int64) if pidx is None else np.asarray(pidx, dtype=np.int64).ravel()
        self.ppos = np.zeros((0, 3)) if ppos is None else np.asarray(ppos, dtype=np.float64).reshape(-1, 3).copy()
        self.pinfo = np.zeros((0, 3, 3)) if pinfo is None else np.asarray(pinfo, dtype=np.float64).reshape(-1, 3, 3).copy()
        self.fidx = np.zeros(0, np.int32) if fidx is None else np.asarray(fidx, dtype=np.int32).ravel()
        self.fpos = np.zeros((0, 3)) if fpos is None else np.asarray(fpos, dtype=np.float64).reshape(-1, 3).copy()
        self.finfo = np.zeros((0, 3, 3)) if finfo is None else np.asarray(finfo, dtype=np.float64).reshape(-1, 3, 3).copy()
        assert self.pidx.size == self.ppos.shape[0] == self.pinfo.shape[0]
        assert self.fidx.size == self.fpos.shape[0] == self.finfo.shape[0]
        assert np.all(np.diff(self.pidx) > 0) and np.all(np.diff(self.fidx) > 0)

    def copy(self):
        return Priors(self.pidx, self.ppos, self.pinfo, self.fidx, self.fpos, self.finfo)

    def set_on(self, gpu, keep_gauge):
        """hand the priors to a surikatoko_amd.BundleAdjustmentKanatani, information given directly"""
        gpu.set_position_priors(points=(self.pidx, self.ppos, {"info": six(self.pinfo)}) if self.pidx.size else None,
                                frames=(self.fidx, self.fpos, {"info": six(self.finfo)}) if self.fidx.size else None,
                                keep_gauge=bool(keep_gauge))


def normalised(pri, nrm):
    """the priors in the normalised world X_n = s (R0 X + T0) of an orc / sa Normalizer: pos_n = s (R0 pos + T0),
    L_n = R0 L R0^T / s^2 (numpy; the library's host map is compared against this in tests/test_prior_cpu.py)"""
    R0 = np.array(list(nrm.R0), dtype=np.float64).reshape(3, 3)
    T0 = np.array(list(nrm.T0), dtype=np.float64)
    s = float(nrm.world_scale)
    out = pri.copy()
    out.ppos = s * (pri.ppos @ R0.T + T0)
    out.fpos = s * (pri.fpos @ R0.T + T0)
    out.pinfo = np.einsum("ab,nbc,dc->nad", R0, pri.pinfo, R0) / (s * s)
    out.finfo = np.einsum("ab,nbc,dc->nad", R0, pri.finfo, R0) / (s * s)
    return out


def centres(so):
    """C_j = -R_j^T T_j"""
    R = np.asarray(so.cam_R).reshape(-1, 3, 3)
    T = np.asarray(so.cam_T).reshape(-1, 3)
    return -np.einsum("jba,jb->ja", R, T)


def offsets(pri, so):
    """(X - Xbar [n][3], C - Cbar [n][3]) of scene so (any scene object with points, cam_R, cam_T)"""
    return np.asarray(so.points).reshape(-1, 3)[pri.pidx] - pri.ppos, centres(so)[pri.fidx] - pri.fpos


def energy(pri, so):
    """(landmark prior sum, frame prior sum)"""
    dp, df = offsets(pri, so)
    return float(np.einsum("na,nab,nb->", dp, pri.pinfo, dp)), float(np.einsum("na,nab,nb->", df, pri.finfo, df))


def add_terms(blocks, so, pri):
    """the oracle's (gradE, V, U, W) plus the prior terms (copies; W is untouched: a prior adds no coupling)"""
    gradE, V, U, W = blocks[:4]
    N = so.N
    g, V, U = gradE.copy(), V.copy(), U.copy()
    dp, df = offsets(pri, so)
    V[pri.pidx] += 2.0 * pri.pinfo
    g[:3 * N].reshape(-1, 3)[pri.pidx] += 2.0 * np.einsum("nab,nb->na", pri.pinfo, dp)
    U[pri.fidx, 4:7, 4:7] += 2.0 * pri.finfo
    g[3 * N:].reshape(-1, 10)[pri.fidx, 4:7] += 2.0 * np.einsum("nab,nb->na", pri.finfo, df)
    return g, V, U, W


def step(orc, f0, so, c, pri, keep_gauge, fv=10, fconst=None, pconst=None, want_system=False, derivatives=None):
    """one attempt at damping c on the normalised oracle scene so with the priors pri (in so's coordinates): the dict of
    constant_ref.step_blocks, plus blocks = the (gradE, V, U, W) with the prior terms, before any restriction"""
    fconst = np.zeros(so.M, dtype=bool) if fconst is None else fconst
    pconst = np.zeros(so.N, dtype=bool) if pconst is None else pconst
    base = orc.derivatives(f0, so) if derivatives is None else derivatives(so)
    blocks = add_terms(base[:4], so, pri)
    out = kref.step_blocks(orc, so, blocks, c, fconst, pconst, keep_gauge, fv, want_system)
    out["blocks"] = blocks
    return out


def compute_inplace(orc, f0, so, pri_world, keep_gauge, fv=10, allowed_err_change=None, max_hessian_factor=None,
                    max_iterations=0, obs_energy=None, derivatives=None):
    """lm_ref.loop around the step with priors.  pri_world: the priors in the coordinates of so as given; so is changed in
    place (normalised, optimised, normalisation reverted).  Returns (rc, report): rc 0 = true, 1 = false."""
    rep = lm_ref.Report()
    ok, nrm = orc.normalize(so)
    if not ok:
        return 1, rep
    pri = normalised(pri_world, nrm)
    fconst, pconst = np.zeros(so.M, dtype=bool), np.zeros(so.N, dtype=bool)

    def total():
        e = obs_energy(so) if obs_energy else orc.reproj_error(f0, so)[0]
        return e + sum(energy(pri, so))

    def prepare():
        base = orc.derivatives(f0, so) if derivatives is None else derivatives(so)
        return kref.restrict_all(so, add_terms(base[:4], so, pri), fconst, pconst, fv)

    def solve(restricted, c):
        res = kref.step_restricted(orc, so, restricted, c, fconst, keep_gauge, fv)
        return res["ok"], res["corr"]

    rc = lm_ref.loop(rep, so, energy=total, prepare=prepare, solve=solve, apply=lambda corr: orc.apply_corrections(so, corr),
                     allowed_err_change=allowed_err_change, max_hessian_factor=max_hessian_factor,
                     max_iterations=max_iterations)
    orc.revert(so, nrm)
    return rc, rep
