"""Attempt-by-attempt comparison of a Levenberg-Marquardt run with a reference loop.

The reference loops (oracle.compute_inplace(..., want_log=True) and lm_ref.loop, the one Python loop behind the
compute_inplace of calibrated_ref, robust_ref, weighted_ref, shared_k_ref, constant_ref and prior_ref) record every attempt in
one format, a dict of equal-length numpy arrays:

  iteration  int64    accepted iterations before this attempt (the iteration the attempt belongs to)
  factor     float64  the damping factor (hessian_factor) the attempt used
  err_trial  float64  its trial error; NaN when the step solve failed
  err_value  float64  the error it was judged against (the current scene's)
  outcome    int32    ACCEPTED, REJECTED, CONVERGED ("err converged to limit value"), CAP_OVERFLOW or SOLVE_FAILED (both
                      "hessian overflow")

The library logs accepted iterations only (BundleAdjustmentKanatani.iteration_log(): attempts, err, hessian_factor, the
factor of the accepted attempt).  assert_same_trajectory folds the reference log into accepted iterations and compares the
two iteration by iteration: the same number of attempts, the same factor bit for bit (both sides start at float32(1e-4)
and multiply or divide by 10 in the same order) and the accepted error within a tolerance.
"""
import numpy as np

REJECTED, ACCEPTED, CONVERGED, CAP_OVERFLOW, SOLVE_FAILED = 0, 1, 2, 3, 4
OUTCOME_NAMES = {REJECTED: "rejected", ACCEPTED: "accepted", CONVERGED: "converged", CAP_OVERFLOW: "cap overflow",
                 SOLVE_FAILED: "solve failed"}
FIELDS = ("iteration", "factor", "err_trial", "err_value", "outcome")

# A decision is a rounding-level tie when the reference's margin (err_value - err_trial) / err_value is below this: the
# library's error sums agree with the oracle's to about 1e-12, so such a decision may legitimately go the other way.
TIE_MARGIN = 1e-10


class AttemptLog:
    """what a Python reference loop fills, attempt by attempt"""

    def __init__(self):
        self._rows = []

    def add(self, iteration, factor, err_trial, err_value, outcome):
        self._rows.append((int(iteration), float(factor), float(err_trial), float(err_value), int(outcome)))

    def arrays(self):
        cols = list(zip(*self._rows)) if self._rows else [()] * 5
        return {"iteration": np.asarray(cols[0], dtype=np.int64), "factor": np.asarray(cols[1], dtype=np.float64),
                "err_trial": np.asarray(cols[2], dtype=np.float64), "err_value": np.asarray(cols[3], dtype=np.float64),
                "outcome": np.asarray(cols[4], dtype=np.int32)}


def margins(log, sel=slice(None)):
    """(err_value - err_trial) / err_value of the attempts sel: positive = accepted by that much"""
    ev = np.asarray(log["err_value"][sel], dtype=np.float64)
    et = np.asarray(log["err_trial"][sel], dtype=np.float64)
    return (ev - et) / ev


def fold(log):
    """the accepted iterations of a reference log: dict of arrays attempts, err, hessian_factor (as iteration_log())"""
    acc = np.flatnonzero(log["outcome"] == ACCEPTED)
    it = log["iteration"]
    attempts = np.array([int(np.count_nonzero(it == k)) for k in range(len(acc))], dtype=np.int64)
    return {"attempts": attempts, "err": log["err_trial"][acc].astype(np.float64),
            "hessian_factor": log["factor"][acc].astype(np.float64)}


def check_log_consistent(log, rep, max_hessian_factor=None):
    """the invariants a reference log must satisfy against its own report (rep: the loop's report)"""
    n = len(log["outcome"])
    assert n == rep.attempts, (n, rep.attempts)
    it, out, fac = log["iteration"], log["outcome"], log["factor"]
    acc = np.flatnonzero(out == ACCEPTED)
    assert len(acc) == rep.iterations, (len(acc), rep.iterations)
    # attempts are grouped by iteration, in order; every iteration but possibly the last ends in its accepted attempt
    assert np.all(np.diff(it) >= 0) and (n == 0 or it[0] == 0)
    assert np.array_equal(it[acc], np.arange(len(acc)))
    terminal = np.flatnonzero(np.isin(out, (CONVERGED, CAP_OVERFLOW, SOLVE_FAILED)))
    assert len(terminal) <= 1 and (len(terminal) == 0 or terminal[0] == n - 1), terminal
    errs = log["err_trial"][acc]
    assert np.all(np.diff(errs) < 0), "accepted errors must strictly decrease"
    if len(acc):
        assert errs[-1] == rep.err_final, (errs[-1], rep.err_final)
        assert np.array_equal(log["err_value"][acc[1:]], errs[:-1])
    if n:
        assert log["err_value"][0] == rep.err_initial
    # the damping factor: float32(1e-4), x10 after a rejection (the capped one included), /10 after an acceptance unless
    # it ended the run on "small relative err change" (status 2), in this order
    c = float(np.float32(1e-4))
    for k in range(n):
        assert fac[k] == c, (k, fac[k], c)
        if out[k] == ACCEPTED and not (k == n - 1 and rep.status == 2):
            c /= 10
        elif out[k] in (REJECTED, CAP_OVERFLOW):
            c *= 10
    if n and out[-1] == CAP_OVERFLOW:
        assert max_hessian_factor is not None and fac[-1] * 10 > max_hessian_factor
    assert c == rep.hessian_factor, (c, rep.hessian_factor)
    for k in np.flatnonzero(out == REJECTED):
        assert not (log["err_trial"][k] - log["err_value"][k] < 0)
    for k in np.flatnonzero(out == SOLVE_FAILED):
        assert np.isnan(log["err_trial"][k])


def first_difference(gpu_log, ref_log, err_rel, n_iter=None, err_abs=0.0):
    """(index of the first accepted iteration where the two runs differ, reason) or (None, None)"""
    ref = fold(ref_log)
    n_gpu, n_ref = len(gpu_log["attempts"]), len(ref["attempts"])
    n = min(n_gpu, n_ref) if n_iter is None else min(n_iter, n_gpu, n_ref)
    for i in range(n):
        ga, ra = int(gpu_log["attempts"][i]), int(ref["attempts"][i])
        if ga != ra:
            return i, f"attempts {ga} (library) != {ra} (reference)"
        gf, rf = float(gpu_log["hessian_factor"][i]), float(ref["hessian_factor"][i])
        if gf != rf:
            return i, f"hessian_factor {gf!r} (library) != {rf!r} (reference)"
        ge, re_ = float(gpu_log["err"][i]), float(ref["err"][i])
        if not abs(ge - re_) <= max(err_rel * abs(re_), err_abs):
            return i, f"accepted err {ge!r} (library) vs {re_!r} (reference): rel {abs(ge - re_) / abs(re_):.3e} > {err_rel:g}"
    if n_iter is None and n_gpu != n_ref:
        return n, f"{n_gpu} accepted iterations (library) != {n_ref} (reference)"
    if n_iter is not None and n < n_iter:
        return n, f"fewer than {n_iter} accepted iterations: library {n_gpu}, reference {n_ref}"
    return None, None


def _describe(ref_log, i):
    sel = np.flatnonzero(ref_log["iteration"] == i)
    if not len(sel):
        return f"the reference has no attempt in iteration {i}"
    rows = [f"factor {ref_log['factor'][k]:.3g} err_trial {ref_log['err_trial'][k]!r} err_value {ref_log['err_value'][k]!r} "
            f"margin {margins(ref_log, k):+.3e} ({OUTCOME_NAMES[int(ref_log['outcome'][k])]})" for k in sel]
    return f"reference attempts of iteration {i}:\n  " + "\n  ".join(rows)


def decisive_margin(gpu_log, ref_log, i):
    """the reference's margin at the first decision the library took differently in accepted iteration i: the attempt the
    library accepted where the reference rejected it, or the reference's accepted attempt where the library rejected it"""
    sel = np.flatnonzero(ref_log["iteration"] == i)
    n_gpu = int(gpu_log["attempts"][i]) if i < len(gpu_log["attempts"]) else len(sel) + 1
    k = sel[min(n_gpu, len(sel)) - 1]
    return float(margins(ref_log, k))


def assert_same_trajectory(gpu_log, ref_log, err_rel, n_iter=None, gpu_attempts=None, allow_tie_fork=False, err_abs=0.0):
    """Iteration by iteration: the same attempt count, the same hessian_factor (exactly) and the accepted error within
    max(err_rel * |reference|, err_abs) (as pytest.approx).  n_iter: compare only the first n_iter accepted iterations.  gpu_attempts: the library report's
    attempt count, which must equal the reference log's length (this covers a failed last iteration, which neither
    iteration log shows).  allow_tie_fork: the runs may part at a rounding-level tie (reference margin < TIE_MARGIN at the
    decision that differs); everything before it must agree and nothing after it is compared.  Returns the index of the
    accepted iteration where the runs part, or None."""
    i, why = first_difference(gpu_log, ref_log, err_rel, n_iter, err_abs)
    if i is not None:
        ref = fold(ref_log)
        if allow_tie_fork and i < len(ref["attempts"]) and i < len(gpu_log["attempts"]) and \
                int(gpu_log["attempts"][i]) != int(ref["attempts"][i]):
            m = decisive_margin(gpu_log, ref_log, i)
            if abs(m) < TIE_MARGIN:
                return i
            why += f"; the reference's margin at the differing decision is {m:+.3e}, not a tie (< {TIE_MARGIN:g})"
        raise AssertionError(f"LM trajectories differ at accepted iteration {i}: {why}\n{_describe(ref_log, i)}")
    if gpu_attempts is not None and n_iter is None:
        assert int(gpu_attempts) == len(ref_log["outcome"]), \
            f"attempts {int(gpu_attempts)} (library report) != {len(ref_log['outcome'])} (reference log)\n" + \
            _describe(ref_log, len(gpu_log["attempts"]))
    return None
