"""Resection without a start pose on the device (include/srk_ba.h): the pose of many frames at once from
2D-3D correspondences with known landmarks, wrong matches among them and no prediction, by P3P hypotheses from a counter-based
sampler, each scored on every observation (a wave is 64 hypotheses of one frame), optionally handed to the refinement of
resect.py without leaving the device."""
import ctypes as C
from collections import namedtuple

import numpy as np

from ._lib import LocateOptions, lib
from .resect import resect_options

# the bits of `located_status`
LOCATE_FEW_POINTS = 1   # fewer than four observations with q > 0
LOCATE_NO_MODEL = 2     # no sample gave a pose with positive depths
LOCATE_STATUS_NAMES = {LOCATE_FEW_POINTS: "FEW_POINTS", LOCATE_NO_MODEL: "NO_MODEL"}

# R [n][3][3], T [n][3]: the refined poses with refine, else the located ones; located [n][6] (RMS truncated error in pixels, weighted
# observations, inliers, winning hypothesis, hypotheses with a pose, the winning sample's fourth-point error in pixels);
# located_status [n]; inliers [O] uint8 or None; quality, info, status, weights: those of resect_frames, None without refine
LocateResult = namedtuple("LocateResult", "R T located located_status inliers quality info status weights")


def locate_status_names(status):
    """the names of the bits set in one located_status word"""
    return [name for bit, name in LOCATE_STATUS_NAMES.items() if int(status) & bit]


def default_locate_options():
    """srk_locate_default_options as a dict: hypotheses, inlier_pixels, seed"""
    o = LocateOptions()
    lib().srk_locate_default_options(C.byref(o))
    return dict(hypotheses=o.hypotheses, inlier_pixels=o.inlier_pixels, seed=o.seed)


def ransac_hypotheses(outlier_ratio, success_probability, sample_size=4):
    """srk_ransac_hypotheses (the reference's RansacIterationsCount): the samples of `sample_size` that reach, with the given
    probability, one without a wrong match"""
    k = int(lib().srk_ransac_hypotheses(C.c_int(int(sample_size)), C.c_double(outlier_ratio), C.c_double(success_probability)))
    if k < 1:
        raise ValueError("ransac_hypotheses: outlier_ratio outside [0, 1), success_probability outside (0, 1) or an empty sample")
    return k


def _d(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def locate_frame_args(row_ptr, point, uv, q, K):
    """the frame arrays as the C ABI takes them: (n_frames, row_ptr, point, uv, q or None, K, shared_k); the lengths are checked
    here, the values by the library"""
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64).reshape(-1)
    pt = np.ascontiguousarray(point, dtype=np.int32).reshape(-1)
    m = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
    w = None if q is None else np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    if rp.size < 1:
        raise ValueError("locate: row_ptr needs at least one entry")
    n = rp.size - 1
    n_obs = max(int(rp.max()), 0)
    if pt.size < n_obs or m.shape[0] < n_obs or (w is not None and w.size < n_obs):
        raise ValueError("locate: the observation arrays are shorter than row_ptr says")
    Kc = np.ascontiguousarray(K, dtype=np.float64).reshape(-1, 9)
    shared_k = Kc.shape[0] == 1 and n != 1
    if not shared_k and Kc.shape[0] != n:
        raise ValueError("locate: row_ptr and K disagree about the number of frames")
    return n, rp, pt, m, w, Kc, shared_k


def _options(hypotheses, inlier_pixels, seed, refine):
    lo = LocateOptions(int(hypotheses), float(inlier_pixels), int(seed) & ((1 << 64) - 1))
    if refine is None:
        return lo, None
    unknown = set(refine) - {"attempts", "rel_change", "loss", "delta"}
    if unknown:
        raise ValueError(f"locate: unknown refine option(s) {sorted(unknown)}")
    return lo, resect_options(refine.get("attempts", 10), refine.get("rel_change", 1e-9), refine.get("loss"), refine.get("delta"))


def _prepare(row_ptr, point, uv, K, q, hypotheses, inlier_pixels, seed, refine, want_inliers, want_weights):
    """(the frames' arguments, the arguments K .. refine, the output arrays) of the two entry points"""
    n, rp, pt, m, w, Kc, shared_k = locate_frame_args(row_ptr, point, uv, q, K)
    lo, ro = _options(hypotheses, inlier_pixels, seed, refine)
    out = _outputs(n, max(int(rp.max()), 0), ro is not None, want_inliers, want_weights)
    keep = (rp, pt, m, w, Kc, lo, ro)   # the arrays the pointers below point into
    return ([C.c_int32(n), _d(rp), _d(pt), _d(m), _d(w)], [_d(Kc), C.c_int(int(shared_k)), C.byref(lo), None if ro is None else C.byref(ro)], out,
            keep)


def locate_frames(ba, f0, row_ptr, point, uv, X, K, q=None, hypotheses=256, inlier_pixels=4.0, seed=1, refine=None, want_inliers=False,
                  want_weights=False):
    """srk_locate_frames: frames in CSR form (row_ptr [n + 1], point [O] into X [N][3], uv [O][2] pixels, q [O] information or
    None) and K ([n][3][3], or one 3 x 3 for all); no predicted pose.  `hypotheses` samples per frame (1 .. 4096; ransac_hypotheses
    gives the count for an outlier ratio), inlier_pixels the truncation of the score and the inlier test, seed the sampler's.
    refine None, or a dict of resect_frames' options (attempts, rel_change, loss, delta): the located poses are then refined on the
    device.  Returns a LocateResult; with want_inliers its inliers [O] mark the observations within inlier_pixels of the located
    pose, with want_weights (and refine) its weights are the robust weights at the refined pose.  An uploaded scene of `ba` is
    left untouched."""
    Xc = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
    frames, hyp, out, _keep = _prepare(row_ptr, point, uv, K, q, hypotheses, inlier_pixels, seed, refine, want_inliers, want_weights)
    ba._raise(lib().srk_locate_frames(C.c_void_p(ba._h), C.c_double(f0), *frames, C.c_int64(Xc.shape[0]), _d(Xc), *hyp, *[_d(a) for a in out]))
    return LocateResult(*out)


def _outputs(n, n_obs, refined, want_inliers, want_weights):
    return (np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros((n, 6)), np.zeros(n, np.uint32), np.zeros(n_obs, np.uint8) if want_inliers else None,
            np.zeros((n, 6)) if refined else None, np.zeros((n, 6, 6)) if refined else None, np.zeros(n, np.uint32) if refined else None,
            np.zeros(n_obs) if refined and want_weights else None)


def last_kernel_ms(ba):
    """device ms of the kernels of the last locate_frames / ba.locate call on this handle, and of its hypothesis-and-score kernel alone"""
    return float(lib().srk_ba_locate_kernel_ms(C.c_void_p(ba._h))), float(lib().srk_ba_locate_score_ms(C.c_void_p(ba._h)))


def check_frames(row_ptr, point, uv, X, K, q=None, hypotheses=256, inlier_pixels=4.0, seed=1, refine=None):
    """srk_locate_check_frames (host only): None, or the text of the refusal"""
    n, rp, pt, m, w, Kc, shared_k = locate_frame_args(row_ptr, point, uv, q, K)
    Xc = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
    lo, ro = _options(hypotheses, inlier_pixels, seed, refine)
    why = C.c_char_p()
    rc = lib().srk_locate_check_frames(C.c_int32(n), _d(rp), _d(pt), _d(m), _d(w), C.c_int64(Xc.shape[0]), _d(Xc), _d(Kc), C.c_int(int(shared_k)),
                                       C.byref(lo), None if ro is None else C.byref(ro), C.byref(why))
    return None if rc == 0 else why.value.decode()
