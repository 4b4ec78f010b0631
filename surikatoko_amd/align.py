"""Map alignment on the device (include/srk_ba.h): the similarity b ~ s R a + t between sets of corresponding
3D points, wrong correspondences among them, by three-point hypotheses from a counter-based sampler, each scored on every
correspondence (a wave is 64 hypotheses of one set), the winner refined by rounds of a closed-form weighted least-squares
similarity on its inliers.  The 3D-3D member of the family: relate is 2D-2D, locate is 2D-3D."""
import ctypes as C
from collections import namedtuple

import numpy as np

from ._lib import AlignOptions, lib
from .locate import ransac_hypotheses  # noqa: F401  (sample_size=3 gives the count for an outlier ratio)

# the bits of `status`
ALIGN_FEW_POINTS = 1   # fewer than three correspondences with q > 0
ALIGN_NO_MODEL = 2     # no sample gave a similarity
ALIGN_STATUS_NAMES = {ALIGN_FEW_POINTS: "FEW_POINTS", ALIGN_NO_MODEL: "NO_MODEL"}

# s [n], R [n][3][3], t [n][3]: b ~ s R a + t; aligned [n][8] (RMS truncated distance, weighted correspondences, inliers, winning
# hypothesis, hypotheses with a model, rounds accepted, the eigenvalue gap of the last accepted closed form, the inliers' RMS
# distance); status [n]; inliers [O] uint8 or None
AlignResult = namedtuple("AlignResult", "s R t aligned status inliers")


def align_status_names(status):
    """the names of the bits set in one status word"""
    return [name for bit, name in ALIGN_STATUS_NAMES.items() if int(status) & bit]


def default_align_options():
    """srk_align_default_options as a dict; inlier_distance is 0 there, which every call refuses: it has no sensible default"""
    o = AlignOptions()
    lib().srk_align_default_options(C.byref(o))
    return dict(hypotheses=o.hypotheses, inlier_distance=o.inlier_distance, seed=o.seed, with_scale=bool(o.with_scale), refine_rounds=o.refine_rounds)


def _d(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _options(hypotheses, inlier_distance, seed, with_scale, refine_rounds):
    return AlignOptions(int(hypotheses), 0.0 if inlier_distance is None else float(inlier_distance), int(seed) & ((1 << 64) - 1), int(bool(with_scale)),
                        int(refine_rounds))


def _outputs(n, n_obs, want_inliers):
    return (np.zeros(n), np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros((n, 8)), np.zeros(n, np.uint32), np.zeros(n_obs, np.uint8) if want_inliers else None)


def align_set_args(row_ptr, a, b, q):
    """the set arrays as the C ABI takes them: (n_sets, n_obs, row_ptr, a, b, q or None); the lengths are checked here, the values
    by the library"""
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64).reshape(-1)
    x = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3)
    y = np.ascontiguousarray(b, dtype=np.float64).reshape(-1, 3)
    w = None if q is None else np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    if rp.size < 1:
        raise ValueError("align: row_ptr needs at least one entry")
    n_obs = max(int(rp.max()), 0)
    if x.shape[0] < n_obs or y.shape[0] < n_obs or (w is not None and w.size < n_obs):
        raise ValueError("align: the correspondence arrays are shorter than row_ptr says")
    return rp.size - 1, n_obs, rp, x, y, w


def align_points(ba, row_ptr, a, b, q=None, hypotheses=256, inlier_distance=None, seed=1, with_scale=True, refine_rounds=2, want_inliers=False):
    """srk_align_points: sets in CSR form (row_ptr [n + 1], a, b [O][3], q [O] information or None).  `hypotheses` samples per set
    (1 .. 4096; ransac_hypotheses(share, p, sample_size=3) gives the count for an outlier ratio), inlier_distance (required, in the
    units of b) the truncation of the score and the inlier test, seed the sampler's, with_scale False for a rigid motion,
    refine_rounds rounds of local optimisation (0 .. 16).  Returns an AlignResult; with want_inliers its inliers [O] mark the
    correspondences within inlier_distance of the returned model.  An uploaded scene of `ba` is left untouched."""
    n, n_obs, rp, x, y, w = align_set_args(row_ptr, a, b, q)
    opts = _options(hypotheses, inlier_distance, seed, with_scale, refine_rounds)
    out = _outputs(n, n_obs, want_inliers)
    ba._raise(lib().srk_align_points(C.c_void_p(ba._h), C.c_int32(n), _d(rp), _d(x), _d(y), _d(w), C.byref(opts), *[_d(o) for o in out]))
    return AlignResult(*out)


def last_kernel_ms(ba):
    """device ms of the kernels of the last align_points / ba.align call on this handle, and of its hypothesis-and-score kernel alone"""
    return float(lib().srk_ba_align_kernel_ms(C.c_void_p(ba._h))), float(lib().srk_ba_align_score_ms(C.c_void_p(ba._h)))


def check_sets(row_ptr, a, b, q=None, hypotheses=256, inlier_distance=None, seed=1, with_scale=True, refine_rounds=2, point=None, n_points=0):
    """srk_align_check_sets (host only): None, or the text of the refusal.  With point (and n_points) the sources are landmarks of a
    map, as in ba.align, and a may be None."""
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64).reshape(-1)
    x = None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3)
    y = np.ascontiguousarray(b, dtype=np.float64).reshape(-1, 3)
    w = None if q is None else np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    pt = None if point is None else np.ascontiguousarray(point, dtype=np.int32).reshape(-1)
    n_obs = max(int(rp.max()), 0) if rp.size else 0
    if rp.size < 1 or y.shape[0] < n_obs or any(v is not None and v.shape[0] < n_obs for v in (x, w, pt)):
        raise ValueError("align: the correspondence arrays are shorter than row_ptr says")
    opts = _options(hypotheses, inlier_distance, seed, with_scale, refine_rounds)
    out = _outputs(rp.size - 1, n_obs, False)
    why = C.c_char_p()
    rc = lib().srk_align_check_sets(C.c_int32(rp.size - 1), _d(rp), _d(pt), C.c_int64(int(n_points)), _d(x), _d(y), _d(w), C.byref(opts),
                                    *[_d(o) for o in out[:5]], C.byref(why))
    return None if rc == 0 else why.value.decode()


def host_set(a, b, q=None, hypotheses=256, inlier_distance=None, seed=1, with_scale=True, refine_rounds=2):
    """srk_align_host_set (host only): one set in the kernels' own order of operations, as an AlignResult of one set"""
    x = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3)
    y = np.ascontiguousarray(b, dtype=np.float64).reshape(-1, 3)
    w = None if q is None else np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    if y.shape[0] != x.shape[0] or (w is not None and w.size != x.shape[0]):
        raise ValueError("align: the correspondence arrays disagree about their length")
    opts = _options(hypotheses, inlier_distance, seed, with_scale, refine_rounds)
    out = _outputs(1, x.shape[0], True)
    rc = lib().srk_align_host_set(C.c_int64(x.shape[0]), _d(x), _d(y), _d(w), C.byref(opts), _d(out[0]), _d(out[1]), _d(out[2]), _d(out[3]), _d(out[5]))
    if rc < 0:
        raise ValueError("align: the checks refuse the set")
    out[4][0] = rc
    return AlignResult(*out)


def apply_similarity(s, R, t, points=None, cam_R=None, cam_T=None):
    """srk_similarity_apply (host only): copies of points [N][3] and of the inverse poses cam_R [M][3][3], cam_T [M][3]
    (x_cam = R_c X + T_c) under X' = s R X + t: R_c' = R_c R^T, T_c' = s T_c - R_c' t, so every projection is unchanged.  Returns
    (points, cam_R, cam_T), None where None was given."""
    Rm = np.ascontiguousarray(R, dtype=np.float64).reshape(9)
    tv = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
    X = None if points is None else np.array(points, dtype=np.float64, order="C").reshape(-1, 3)
    if (cam_R is None) != (cam_T is None):
        raise ValueError("apply_similarity: cam_R and cam_T go together")
    cR = None if cam_R is None else np.array(cam_R, dtype=np.float64, order="C").reshape(-1, 3, 3)
    cT = None if cam_T is None else np.array(cam_T, dtype=np.float64, order="C").reshape(-1, 3)
    if cR is not None and cR.shape[0] != cT.shape[0]:
        raise ValueError("apply_similarity: cam_R and cam_T disagree about the number of frames")
    rc = lib().srk_similarity_apply(C.c_double(float(s)), _d(Rm), _d(tv), C.c_int64(0 if X is None else X.shape[0]), _d(X),
                                    C.c_int64(0 if cR is None else cR.shape[0]), _d(cR), _d(cT))
    if rc < 0:
        raise ValueError("apply_similarity: s must be finite and > 0")
    return X, cR, cT
