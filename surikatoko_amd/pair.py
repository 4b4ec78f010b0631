"""Two-view pose refinement on the device (include/srk_ba.h): per pair a Levenberg-Marquardt loop on the
robust Sampson error of all its matches over the five degrees of freedom of (R, unit T), one wave a pair, from a start pose
(refine_pairs) or chained behind relate without leaving the device (relate_frames(..., refine=dict(...))), and the map from a
refined pair to the relative-pose factor the adjuster takes (relative_pose_factor)."""
import ctypes as C
from collections import namedtuple

import numpy as np

from ._lib import PairOptions, lib
from .resect import LOSS_KINDS

# the bits of `status`
PAIR_FEW_POINTS = 1       # fewer than five matches with q > 0: the pose is the start
PAIR_DEGENERATE = 2       # the scaled H at the result is not positive definite, or something is not finite
PAIR_NOT_CONVERGED = 8    # the loop used all its attempts
PAIR_STATUS_NAMES = {PAIR_FEW_POINTS: "FEW_POINTS", PAIR_DEGENERATE: "DEGENERATE", PAIR_NOT_CONVERGED: "NOT_CONVERGED"}

# R [n][3][3], T [n][3] (unit): x_b ~ R x_a + T; E [n][3][3] = [T]x R; quality [n][6] (RMS robust Sampson error in pixels, weighted
# matches, mean robust weight, cond_1 of the scaled H, matches in front of both cameras, attempts used); info [n][5][5] = H / f0^2
# over [w; beta]; basis [n][2][3] = b1, b2 at the result; status [n]; weights [O] or None
PairResult = namedtuple("PairResult", "R T E quality info basis status weights")


def pair_status_names(status):
    """the names of the bits set in one status word"""
    return [name for bit, name in PAIR_STATUS_NAMES.items() if int(status) & bit]


def default_pair_options():
    """srk_pair_default_options as a dict"""
    o = PairOptions()
    lib().srk_pair_default_options(C.byref(o))
    return dict(attempts=o.attempts, rel_change=o.rel_change, loss_kind=o.loss_kind, loss_delta_pixels=o.loss_delta_pixels, inliers_only=o.inliers_only)


def _d(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def pair_options(attempts=10, rel_change=1e-9, loss=None, delta=None, inliers_only=False):
    """the options as the C ABI takes them; loss None, "huber" or "cauchy" (or 0, 1, 2) with delta in pixels"""
    if loss not in LOSS_KINDS:
        raise ValueError(f"pair: unknown loss {loss!r}")
    return PairOptions(int(attempts), float(rel_change), LOSS_KINDS[loss], 0.0 if delta is None else float(delta), int(inliers_only))


def pair_outputs(n, n_obs, want_weights):
    return (np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros((n, 3, 3)), np.zeros((n, 6)), np.zeros((n, 5, 5)), np.zeros((n, 2, 3)),
            np.zeros(n, np.uint32), np.zeros(n_obs) if want_weights else None)


def _start_args(row_ptr, uv_a, uv_b, K_a, K_b, R0, T0, q):
    from .relate import relate_pair_args
    n, rp, a, b, w, Ka, Kb, shared_k = relate_pair_args(row_ptr, uv_a, uv_b, q, K_a, K_b)
    R = np.ascontiguousarray(R0, dtype=np.float64).reshape(-1, 9)
    T = np.ascontiguousarray(T0, dtype=np.float64).reshape(-1, 3)
    if R.shape[0] != n or T.shape[0] != n:
        raise ValueError("pair: row_ptr, R0 and T0 disagree about the number of pairs")
    keep = (rp, a, b, w, Ka, Kb, R, T)   # the arrays the pointers below point into
    return n, max(int(rp.max()), 0), [C.c_int32(n), _d(rp), _d(a), _d(b), _d(w), _d(Ka), _d(Kb), C.c_int(int(shared_k)), _d(R), _d(T)], keep


def refine_pairs(ba, f0, row_ptr, uv_a, uv_b, K_a, K_b, R0, T0, q=None, attempts=10, rel_change=1e-9, loss=None, delta=None, want_weights=False):
    """srk_refine_pairs: pairs in CSR form (row_ptr [n + 1], uv_a, uv_b [O][2] pixels of the two images, q [O] information or None),
    the intrinsics of the two cameras ([n][3][3] each, or one 3 x 3 each for all) and the start poses R0 [n][3][3], T0 [n][3]
    (unit).  loss None, "huber" or "cauchy" with delta in pixels; attempts 0 evaluates only.  Returns a PairResult; with
    want_weights its weights [O] are the robust weights at the result.  An uploaded scene of `ba` is left untouched."""
    n, n_obs, args, _keep = _start_args(row_ptr, uv_a, uv_b, K_a, K_b, R0, T0, q)
    opts = pair_options(attempts, rel_change, loss, delta)
    out = pair_outputs(n, n_obs, want_weights)
    ba._raise(lib().srk_refine_pairs(C.c_void_p(ba._h), C.c_double(f0), *args, C.byref(opts), *[_d(a) for a in out]))
    return PairResult(*out)


def last_kernel_ms(ba):
    """device ms of the refinement's kernels in the last refine_pairs / relate_frames(..., refine=) call on this handle"""
    return float(lib().srk_ba_pair_kernel_ms(C.c_void_p(ba._h)))


def check_pairs(row_ptr, uv_a, uv_b, K_a, K_b, R0, T0, q=None, attempts=10, rel_change=1e-9, loss=None, delta=None, inliers_only=0):
    """srk_pair_check_pairs (host only): None, or the text of the refusal"""
    _n, _n_obs, args, _keep = _start_args(row_ptr, uv_a, uv_b, K_a, K_b, R0, T0, q)
    opts = PairOptions(int(attempts), float(rel_change), LOSS_KINDS.get(loss, loss), 0.0 if delta is None else float(delta), int(inliers_only))
    why = C.c_char_p()
    rc = lib().srk_pair_check_pairs(*args, C.byref(opts), C.byref(why))
    return None if rc == 0 else why.value.decode()


def host_pair(f0, uv_a, uv_b, K_a, K_b, R0, T0, q=None, attempts=10, rel_change=1e-9, loss=None, delta=None, want_weights=False):
    """srk_pair_host_pair (host only): one pair in the kernel's own order of operations.  Returns (PairResult of one pair, g [5]
    at the result, log [attempts used][3] of (accepted, E_cur, E_cand))."""
    a = np.ascontiguousarray(uv_a, dtype=np.float64).reshape(-1, 2)
    b = np.ascontiguousarray(uv_b, dtype=np.float64).reshape(-1, 2)
    w = None if q is None else np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    Ka, Kb = np.ascontiguousarray(K_a, dtype=np.float64).reshape(9), np.ascontiguousarray(K_b, dtype=np.float64).reshape(9)
    R, T = np.ascontiguousarray(R0, dtype=np.float64).reshape(9), np.ascontiguousarray(T0, dtype=np.float64).reshape(3)
    if b.shape[0] != a.shape[0] or (w is not None and w.size != a.shape[0]):
        raise ValueError("pair: the match arrays disagree about their length")
    opts = pair_options(attempts, rel_change, loss, delta)
    out = pair_outputs(1, a.shape[0], want_weights)
    grad, log, count = np.zeros(5), np.zeros((max(int(attempts), 1), 3)), C.c_int32(0)
    rc = lib().srk_pair_host_pair(C.c_int64(a.shape[0]), _d(a), _d(b), _d(w), _d(Ka), _d(Kb), C.c_double(f0), _d(R), _d(T), C.byref(opts),
                                  *[_d(x) for x in out[:6]], _d(out[7]), _d(grad), _d(log), C.byref(count))
    if rc < 0:
        raise ValueError("pair: the checks refuse the pair")
    return PairResult(*out[:6], np.array([rc], np.uint32), out[7]), grad, log[:count.value]


def relative_pose_factor(R, T, info, basis, baseline):
    """srk_pair_factor (host only): from one refined pair to the measurement and information that set_relative_pose_factors takes
    for the frames (a, b), at the baseline length the caller knows: (rel_R [3][3] = R^T, rel_t [3] = -baseline R^T T, info21 [21], the
    upper triangle of the 6 x 6 information over [t; r]).  The information has rank 5 at most: its null direction [rel_t; 0] is
    the scale, which two views do not see."""
    Rc, Tc = np.ascontiguousarray(R, dtype=np.float64).reshape(9), np.ascontiguousarray(T, dtype=np.float64).reshape(3)
    Lc, Bc = np.ascontiguousarray(info, dtype=np.float64).reshape(25), np.ascontiguousarray(basis, dtype=np.float64).reshape(6)
    out = (np.zeros((3, 3)), np.zeros(3), np.zeros(21))
    if lib().srk_pair_factor(_d(Rc), _d(Tc), _d(Lc), _d(Bc), C.c_double(baseline), *[_d(x) for x in out]) != 0:
        raise ValueError("srk_pair_factor: bad argument")
    return out
