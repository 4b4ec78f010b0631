"""Batched camera resection with robust pose refinement on the device (include/srk_ba.h): the pose of many
frames at once from 2D-3D correspondences with known landmarks and a predicted pose each, by Levenberg-Marquardt on the
reprojection error with an optional Huber or Cauchy loss, one wave per frame."""
import ctypes as C

import numpy as np

from ._lib import ResectOptions, lib

# the bits of `status`
RESECT_FEW_POINTS = 1      # fewer than three observations with q > 0: the pose is the start
RESECT_DEGENERATE = 2      # the scaled H at the result is not positive definite, or something is not finite
RESECT_BEHIND = 4          # a weighted observation at depth <= 0 at the result
RESECT_NOT_CONVERGED = 8   # the loop used all its attempts
RESECT_STATUS_NAMES = {RESECT_FEW_POINTS: "FEW_POINTS", RESECT_DEGENERATE: "DEGENERATE", RESECT_BEHIND: "BEHIND",
                       RESECT_NOT_CONVERGED: "NOT_CONVERGED"}
LOSS_KINDS = {None: 0, "none": 0, "huber": 1, "cauchy": 2, 0: 0, 1: 1, 2: 2}


def resect_status_names(status):
    """the names of the bits set in one status word"""
    return [name for bit, name in RESECT_STATUS_NAMES.items() if int(status) & bit]


def default_resect_options():
    """srk_resect_default_options as a dict: attempts, rel_change, loss_kind, loss_delta_pixels"""
    o = ResectOptions()
    lib().srk_resect_default_options(C.byref(o))
    return dict(attempts=o.attempts, rel_change=o.rel_change, loss_kind=o.loss_kind, loss_delta_pixels=o.loss_delta_pixels)


def _d(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def resect_options(attempts, rel_change, loss, delta):
    if loss not in LOSS_KINDS:
        raise ValueError(f"resect: unknown loss {loss!r}")
    return ResectOptions(int(attempts), float(rel_change), LOSS_KINDS[loss], 0.0 if delta is None else float(delta))


def resect_frame_args(row_ptr, point, uv, q, K, R0, T0):
    """the frame arrays as the C ABI takes them: (n_frames, row_ptr, point, uv, q or None, K, shared_k, R0, T0); the lengths are
    checked here, the values by the library"""
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64).reshape(-1)
    pt = np.ascontiguousarray(point, dtype=np.int32).reshape(-1)
    m = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
    w = None if q is None else np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    if rp.size < 1:
        raise ValueError("resect: row_ptr needs at least one entry")
    n = rp.size - 1
    n_obs = max(int(rp.max()), 0)
    if pt.size < n_obs or m.shape[0] < n_obs or (w is not None and w.size < n_obs):
        raise ValueError("resect: the observation arrays are shorter than row_ptr says")
    R = np.ascontiguousarray(R0, dtype=np.float64).reshape(-1, 9)
    T = np.ascontiguousarray(T0, dtype=np.float64).reshape(-1, 3)
    Kc = np.ascontiguousarray(K, dtype=np.float64).reshape(-1, 9)
    shared_k = Kc.shape[0] == 1 and n != 1
    if R.shape[0] != n or T.shape[0] != n or (not shared_k and Kc.shape[0] != n):
        raise ValueError("resect: row_ptr, K, R0 and T0 disagree about the number of frames")
    return n, rp, pt, m, w, Kc, shared_k, R, T


def _outputs(n, n_obs, want_weights):
    return (np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros((n, 6)), np.zeros((n, 6, 6)), np.zeros(n, np.uint32),
            np.zeros(n_obs) if want_weights else None)


def _result(out, want_weights):
    return out if want_weights else out[:5]


def resect_frames(ba, f0, row_ptr, point, uv, X, K, R0, T0, q=None, attempts=10, rel_change=1e-9, loss=None, delta=None, want_weights=False):
    """srk_resect_frames: frames in CSR form (row_ptr [n + 1], point [O] into X [N][3], uv [O][2] pixels, q [O] information or
    None), K ([n][3][3], or one 3 x 3 for all) and the predicted inverse poses R0 [n][3][3], T0 [n][3].  loss None, "huber" or
    "cauchy" with delta in pixels.  Returns R [n][3][3], T [n][3], quality [n][6] (RMS reprojection error in pixels, weighted
    observations, mean robust weight, cond_1 of the scaled H, smallest depth, attempts used), info [n][6][6] (H / f0^2, the units
    of set_joint_pose_priors) and status [n] (RESECT_* bits); with want_weights also the robust weights [O] at the result.  An
    uploaded scene of `ba` is left untouched."""
    n, rp, pt, m, w, Kc, shared_k, R, T = resect_frame_args(row_ptr, point, uv, q, K, R0, T0)
    Xc = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
    opts = resect_options(attempts, rel_change, loss, delta)
    out = _outputs(n, max(int(rp.max()), 0), want_weights)
    ba._raise(lib().srk_resect_frames(C.c_void_p(ba._h), C.c_double(f0), C.c_int32(n), _d(rp), _d(pt), _d(m), _d(w), C.c_int64(Xc.shape[0]),
                                      _d(Xc), _d(Kc), C.c_int(int(shared_k)), _d(R), _d(T), C.byref(opts), *[_d(a) for a in out]))
    return _result(out, want_weights)


def last_kernel_ms(ba):
    """device ms of the kernels of the last resect_frames / ba.resect call on this handle (an event pair)"""
    return float(lib().srk_ba_resect_kernel_ms(C.c_void_p(ba._h)))


def check_frames(row_ptr, point, uv, X, K, R0, T0, q=None, attempts=10, rel_change=1e-9, loss=None, delta=None):
    """srk_resect_check_frames (host only): None, or the text of the refusal"""
    n, rp, pt, m, w, Kc, shared_k, R, T = resect_frame_args(row_ptr, point, uv, q, K, R0, T0)
    Xc = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
    opts = ResectOptions(int(attempts), float(rel_change), LOSS_KINDS.get(loss, loss), 0.0 if delta is None else float(delta))
    why = C.c_char_p()
    rc = lib().srk_resect_check_frames(C.c_int32(n), _d(rp), _d(pt), _d(m), _d(w), C.c_int64(Xc.shape[0]), _d(Xc), _d(Kc), C.c_int(int(shared_k)),
                                       _d(R), _d(T), C.byref(opts), C.byref(why))
    return None if rc == 0 else why.value.decode()


def revert(nrm, R, T, info=None):
    """srk_resect_revert (host only): results of the normalised scene in the caller's coordinates (copies)"""
    Rc = np.array(R, dtype=np.float64).reshape(-1, 3, 3)
    Tc = np.array(T, dtype=np.float64).reshape(-1, 3)
    Lc = None if info is None else np.array(info, dtype=np.float64).reshape(-1, 6, 6)
    if lib().srk_resect_revert(C.byref(nrm), C.c_int32(Rc.shape[0]), _d(Rc), _d(Tc), _d(Lc)) != 0:
        raise ValueError("srk_resect_revert: bad argument")
    return Rc, Tc, Lc
