"""Bundle adjustment with per-observation information (srk_ba_set_observation_information) stated with
the oracle's entry points: tests/robust_ref.py with q.

Observation o carries q_o >= 0; with s = ex^2 + ey^2 its whitened squared residual is q s, the objective
E = sum_o rho(q_o s_o) (rho the identity without a loss) and the weight of its Gauss-Newton blocks and gradient terms
w_eff = q rho'(q s): V, U, W = sum_o w_eff 2 J_o^T J_o and the gradient sum_o w_eff 2 J_o^T e_o, the exact gradient of E.
The bodies are robust_ref's, which take q as their last argument; the functions here put it where the callers of this
module pass it.  At q = 1 every function here gives robust_ref's values bit for bit (1.0 * x is exact).
"""
import numpy as np

import robust_ref as rr
from robust_ref import NONE, HUBER, CAUCHY, CHUNK  # noqa: F401


def energy(f0, so, q, kind=NONE, delta=None):
    """E = sum_o rho(q_o s_o) (delta in pixels)"""
    return rr.energy(f0, so, kind, delta, q)


def weights(f0, so, q, kind=NONE, delta=None):
    """the loss's factor rho'(q_o s_o) of every observation (caller's order): what srk_ba_observation_weights returns"""
    return rr.weights(f0, so, kind, delta, q)


def derivatives(f0, so, q, kind=NONE, delta=None):
    """weighted (gradE [3N + 10M], V [N,3,3], U [M,10,10], W [O,3,10]) in the oracle's layout, and the loss's factors
    rho'(q s); the blocks carry w_eff = q rho'(q s)"""
    return rr.derivatives(f0, so, kind, delta, q)


def step(orc, f0, so, c, q, kind=NONE, delta=None, fv=10, want_system=False, skyline=False, sel_rows=None):
    """one attempt at damping c on the (normalised) oracle scene so, as robust_ref.step with the information q"""
    return rr.step(orc, f0, so, c, kind, delta, fv, want_system, skyline, sel_rows, q)


def compute_inplace(orc, f0, so, q, kind=NONE, delta=None, allowed_err_change=None, max_hessian_factor=None, max_iterations=0,
                    fv=10, skyline=False, normalize=True):
    """the LM loop on E = sum rho(q s), as robust_ref.compute_inplace"""
    return rr.compute_inplace(orc, f0, so, kind, delta, allowed_err_change, max_hessian_factor, max_iterations, fv, skyline,
                              normalize, q)


def make_information(sc, seed, zero_frac=0.03):
    """seeded information for a scene: log-uniform in [0.25, 4]; then about zero_frac of the observations set to 0, at most
    one per landmark and only in landmarks with at least four observations (so every landmark keeps >= 3 positive ones)"""
    rng = np.random.RandomState(seed)
    rp = np.asarray(sc.row_ptr)
    O = int(rp[-1])
    q = np.exp(rng.uniform(np.log(0.25), np.log(4.0), size=O))
    cnt = np.diff(rp)
    cand = np.flatnonzero(cnt >= 4)
    n_zero = min(len(cand), int(round(zero_frac * O)))
    for i in rng.choice(cand, size=n_zero, replace=False):
        q[rp[i] + rng.randint(cnt[i])] = 0.0
    return q


def remove_observations(sc, drop):
    """a copy of the scene sc without the observations flagged in drop (caller's order)"""
    keep = ~np.asarray(drop, dtype=bool)
    rp = np.asarray(sc.row_ptr)
    kept = np.concatenate([[0], np.cumsum(keep)])
    return type(sc)(sc.points.copy(), sc.cam_R.copy(), sc.cam_T.copy(), sc.K.copy(), sc.shared_k, kept[rp].astype(np.int64),
                    np.asarray(sc.obs_frame)[keep], np.asarray(sc.obs_uv).reshape(-1, 2)[keep])
