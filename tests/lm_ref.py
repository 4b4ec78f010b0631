"""The Levenberg-Marquardt loop of bundle-adj-kanatani.cpp:720-893 with the decisions of orc_compute_inplace, once.

The yardsticks (calibrated_ref, robust_ref / weighted_ref, shared_k_ref, constant_ref, prior_ref) differ in their energy, in
the blocks an iteration prepares, in how one attempt is solved and applied and in what a rejected attempt restores; the
damping schedule, the four exits, the attempt log and the report are the same and are here.  Each compute_inplace normalises
the scene, hands loop() those pieces and reverts the normalisation.  tests/test_lm_ref_cpu.py holds loop() against the C
oracle's own loop bit for bit.
"""
import numpy as np

import lm_trajectory as lt


class Report:
    """what every yardstick's compute_inplace returns beside rc; errors = the energy after every accepted iteration"""

    def __init__(self):
        self.status, self.iterations, self.attempts = 0, 0, 0
        self.attempts_per_iteration, self.errors = [], []
        self.log = lt.AttemptLog().arrays()


def loop(rep, so, energy, prepare, solve, apply, allowed_err_change=None, max_hessian_factor=None, max_iterations=0,
         saved=("points", "cam_R", "cam_T")):
    """runs on the (normalised) scene so in place and fills rep; returns rc: 0 = true, 1 = false.
    energy() -> the error of so as it stands; prepare() -> whatever one iteration computes once for all its attempts;
    solve(prepared, c) -> (ok, step) at damping c; apply(step) moves so by it; saved: the arrays of so a rejected attempt
    restores."""
    log = lt.AttemptLog()
    hessian_factor = float(np.float32(0.0001))  # :723 float literal
    err_value = energy()
    rep.err_initial = rep.err_final = err_value
    result_true = False
    done = False
    if allowed_err_change is not None and err_value < allowed_err_change:
        rep.status, result_true, done = 1, True, True
    while not done:
        if max_iterations > 0 and rep.iterations >= max_iterations:
            rep.status, result_true = 5, False
            break
        prepared = prepare()
        bak = [getattr(so, name).copy() for name in saved]
        have_prev, err_new_prev, decrease, n_att = False, 0.0, 0, 0
        while not decrease:
            rep.attempts += 1
            n_att += 1
            suc, step = solve(prepared, hessian_factor)
            if not suc:
                log.add(rep.iterations, hessian_factor, np.nan, err_value, lt.SOLVE_FAILED)
                decrease = 2
                break
            apply(step)
            err_new = energy()
            if err_new - err_value < 0:
                log.add(rep.iterations, hessian_factor, err_new, err_value, lt.ACCEPTED)
                decrease = 1
                break
            for name, b in zip(saved, bak):
                getattr(so, name)[:] = b
            if have_prev and allowed_err_change is not None and abs(err_new - err_new_prev) < allowed_err_change:
                log.add(rep.iterations, hessian_factor, err_new, err_value, lt.CONVERGED)
                decrease = 3
                break
            used = hessian_factor
            hessian_factor *= 10
            if max_hessian_factor is not None and hessian_factor > max_hessian_factor:
                log.add(rep.iterations, used, err_new, err_value, lt.CAP_OVERFLOW)
                decrease = 2
                break
            log.add(rep.iterations, used, err_new, err_value, lt.REJECTED)
            err_new_prev, have_prev = err_new, True
        rep.attempts_per_iteration.append(n_att)
        if decrease != 1:
            rep.status = 3 if decrease == 2 else 4
            result_true = False
            break
        rep.iterations += 1
        change = err_new - err_value
        rep.err_final = err_new
        rep.errors.append(err_new)
        if allowed_err_change is not None and abs(change) < allowed_err_change:
            rep.status, result_true = 2, True
            break
        err_value = err_new
        hessian_factor /= 10
    rep.hessian_factor = hessian_factor
    rep.log = log.arrays()
    return 0 if result_true else 1
