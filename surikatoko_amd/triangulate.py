"""Batched landmark triangulation and refinement on the device (include/srk_ba.h): the linear system of
Triangulate3DPointByLeastSquares (obs-geom.cpp:679-727) for many ragged tracks at once, solved by a streaming Givens QR, and an
optional Levenberg-Marquardt refinement of the reprojection error per landmark."""
import ctypes as C

import numpy as np

from ._lib import TriOptions, lib

# the bits of `status`
TRI_FEW_VIEWS = 1       # fewer than two observations with q > 0: X is NaN
TRI_DEGENERATE = 2      # a zero or non-finite diagonal of the factor, or a non-finite X
TRI_BEHIND = 4          # depth <= 0 in some weighted frame
TRI_LOW_PARALLAX = 8    # quality[:, 1] < min_parallax_deg
TRI_NOT_CONVERGED = 16  # the refinement used all its attempts
TRI_STATUS_NAMES = {TRI_FEW_VIEWS: "FEW_VIEWS", TRI_DEGENERATE: "DEGENERATE", TRI_BEHIND: "BEHIND", TRI_LOW_PARALLAX: "LOW_PARALLAX",
                    TRI_NOT_CONVERGED: "NOT_CONVERGED"}


def tri_status_names(status):
    """the names of the bits set in one status word"""
    return [name for bit, name in TRI_STATUS_NAMES.items() if int(status) & bit]


def default_tri_options():
    """srk_tri_default_options as a dict: refine_attempts, refine_rel_change, min_parallax_deg"""
    o = TriOptions()
    lib().srk_tri_default_options(C.byref(o))
    return dict(refine_attempts=o.refine_attempts, refine_rel_change=o.refine_rel_change, min_parallax_deg=o.min_parallax_deg)


def _d(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def tri_track_args(row_ptr, frame, uv, q):
    """the track arrays as the C ABI takes them: (n_tracks, row_ptr, frame, uv, q or None); the lengths are checked here, the
    values by the library"""
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64).reshape(-1)
    fr = np.ascontiguousarray(frame, dtype=np.int32).reshape(-1)
    m = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
    w = None if q is None else np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    if rp.size < 1:
        raise ValueError("triangulate: row_ptr needs at least one entry")
    n_obs = max(int(rp.max()), 0)
    if fr.size < n_obs or m.shape[0] < n_obs or (w is not None and w.size < n_obs):
        raise ValueError("triangulate: the observation arrays are shorter than row_ptr says")
    return rp.size - 1, rp, fr, m, w


def tri_options(refine_attempts, refine_rel_change, min_parallax_deg):
    """a TriOptions, or None (linear only, no parallax gate) when nothing is asked for"""
    if not refine_attempts and not min_parallax_deg:
        return None
    return TriOptions(int(refine_attempts), float(refine_rel_change), float(min_parallax_deg))


def triangulate_tracks(ba, f0, row_ptr, frame, uv, cam_R, cam_T, K, q=None, refine_attempts=0, refine_rel_change=1e-9, min_parallax_deg=0.0,
                       shared_k=None):
    """srk_triangulate_tracks: tracks in CSR form (row_ptr [n + 1], frame [O], uv [O][2] pixels, q [O] information or None) over
    caller-given inverse poses cam_R [M][3][3], cam_T [M][3] and K ([M][3][3], or one 3 x 3 for all).  Returns X [n][3], quality
    [n][4] (RMS reprojection error in pixels, largest ray angle to the first weighted view in degrees, cond_1 of the triangular
    factor, weighted observations) and status [n] (TRI_* bits).  An uploaded scene of `ba` is left untouched."""
    n, rp, fr, m, w = tri_track_args(row_ptr, frame, uv, q)
    R = np.ascontiguousarray(cam_R, dtype=np.float64).reshape(-1, 9)
    T = np.ascontiguousarray(cam_T, dtype=np.float64).reshape(-1, 3)
    Kc = np.ascontiguousarray(K, dtype=np.float64).reshape(-1, 9)
    if shared_k is None:
        shared_k = Kc.shape[0] == 1 and R.shape[0] != 1
    if T.shape[0] != R.shape[0] or (not shared_k and Kc.shape[0] != R.shape[0]):
        raise ValueError("triangulate_tracks: cam_R, cam_T and K disagree about the number of frames")
    X, quality, status = np.zeros((n, 3)), np.zeros((n, 4)), np.zeros(n, np.uint32)
    opts = tri_options(refine_attempts, refine_rel_change, min_parallax_deg)
    ba._raise(lib().srk_triangulate_tracks(C.c_void_p(ba._h), C.c_double(f0), C.c_int64(n), _d(rp), _d(fr), _d(m), _d(w), C.c_int32(R.shape[0]),
                                           _d(R), _d(T), _d(Kc), C.c_int(int(bool(shared_k))), None if opts is None else C.byref(opts), _d(X),
                                           _d(quality), _d(status)))
    return X, quality, status


def last_kernel_ms(ba):
    """device ms of the kernels of the last triangulate_tracks / ba.triangulate call on this handle (an event pair)"""
    return float(lib().srk_ba_triangulate_kernel_ms(C.c_void_p(ba._h)))


def check_tracks(row_ptr, frame, uv, n_frames, q=None, refine_attempts=0, refine_rel_change=1e-9, min_parallax_deg=0.0):
    """srk_tri_check_tracks (host only): None, or the text of the refusal"""
    n, rp, fr, m, w = tri_track_args(row_ptr, frame, uv, q)
    opts = tri_options(refine_attempts, refine_rel_change, min_parallax_deg)
    why = C.c_char_p()
    rc = lib().srk_tri_check_tracks(C.c_int64(n), _d(rp), _d(fr), _d(m), _d(w), C.c_int32(n_frames), None if opts is None else C.byref(opts),
                                    C.byref(why))
    return None if rc == 0 else why.value.decode()


def revert_points(nrm, X):
    """srk_tri_revert_points (host only): points of the normalised scene in the caller's coordinates (a copy)"""
    out = np.array(X, dtype=np.float64).reshape(-1, 3)
    if lib().srk_tri_revert_points(C.byref(nrm), C.c_int64(out.shape[0]), _d(out)) != 0:
        raise ValueError("srk_tri_revert_points: bad argument")
    return out
