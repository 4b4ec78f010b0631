"""The two-view homography on the device (include/srk_ba.h): p_b ~ G p_a between the 2D-2D matches of pairs of
images, wrong matches among them, by four-point hypotheses from a counter-based sampler, each scored on every match (a wave is
64 hypotheses of one pair), the winner refined by Gauss-Newton rounds on the symmetric transfer error of its inliers, then
decomposed into the plane's two poses (or, without a baseline, the rotation).  The member of the family for planar scenes and
for pure rotation, where relate cannot answer: run both on the same matches and compare the inlier counts and RMS figures."""
import ctypes as C
from collections import namedtuple

import numpy as np

from ._lib import HomographyOptions, lib
from .locate import ransac_hypotheses  # noqa: F401  (sample_size=4 gives the count for an outlier ratio)
from .relate import relate_pair_args

# the bits of `status`
HOMOGRAPHY_FEW_POINTS = 1   # fewer than four matches with q > 0
HOMOGRAPHY_NO_MODEL = 2     # no sample gave a homography
HOMOGRAPHY_STATUS_NAMES = {HOMOGRAPHY_FEW_POINTS: "FEW_POINTS", HOMOGRAPHY_NO_MODEL: "NO_MODEL"}

# G [n][3][3] the pixel homography (norm 1, (G p_a)_3 > 0 for its inliers); H [n][3][3] = K_b^-1 G K_a over its middle singular
# value; n_poses [n] (0, 1 or 2); R [n][2][3][3], T [n][2][3] (= t / d), N [n][2][3], front [n][2] (the inliers with N^T x_a > 0),
# unused entries zero; homog [n][8] (RMS truncated error in pixels, weighted matches, inliers, winning hypothesis, hypotheses with
# a model, rounds accepted, w1 - w3, the inliers' RMS symmetric error); status [n]; inliers [O] uint8 or None
HomographyResult = namedtuple("HomographyResult", "G H n_poses R T N front homog status inliers")
# decompose_homography: H normalised and signed, n_poses, R [2][3][3], T [2][3], N [2][3], front [2], gap = w1 - w3
HomographyPoses = namedtuple("HomographyPoses", "H n_poses R T N front gap")


def homography_status_names(status):
    """the names of the bits set in one status word"""
    return [name for bit, name in HOMOGRAPHY_STATUS_NAMES.items() if int(status) & bit]


def default_homography_options():
    """srk_homography_default_options as a dict"""
    o = HomographyOptions()
    lib().srk_homography_default_options(C.byref(o))
    return dict(hypotheses=o.hypotheses, inlier_pixels=o.inlier_pixels, seed=o.seed, refine_rounds=o.refine_rounds)


def _d(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _options(hypotheses, inlier_pixels, seed, refine_rounds):
    return HomographyOptions(int(hypotheses), float(inlier_pixels), int(seed) & ((1 << 64) - 1), int(refine_rounds))


def _outputs(n, n_obs, want_inliers):
    return (np.zeros((n, 3, 3)), np.zeros((n, 3, 3)), np.zeros(n, np.int32), np.zeros((n, 2, 3, 3)), np.zeros((n, 2, 3)), np.zeros((n, 2, 3)),
            np.zeros((n, 2), np.int32), np.zeros((n, 8)), np.zeros(n, np.uint32), np.zeros(n_obs, np.uint8) if want_inliers else None)


def _call_args(row_ptr, uv_a, uv_b, K_a, K_b, q, opts):
    n, rp, a, b, w, Ka, Kb, shared_k = relate_pair_args(row_ptr, uv_a, uv_b, q, K_a, K_b)
    keep = (rp, a, b, w, Ka, Kb, opts)   # the arrays the pointers below point into
    return n, max(int(rp.max()), 0), [C.c_int32(n), _d(rp), _d(a), _d(b), _d(w), _d(Ka), _d(Kb), C.c_int(int(shared_k)), C.byref(opts)], keep


def relate_homography(ba, f0, row_ptr, uv_a, uv_b, K_a, K_b, q=None, hypotheses=256, inlier_pixels=6.0, seed=1, refine_rounds=4,
                      want_inliers=False):
    """srk_relate_homography: pairs in CSR form (row_ptr [n + 1], uv_a, uv_b [O][2] pixels of the two images, q [O] information or
    None) and the intrinsics of the two cameras ([n][3][3] each, or one 3 x 3 each for all).  `hypotheses` samples per pair
    (1 .. 4096; ransac_hypotheses(share, p, sample_size=4) gives the count for an outlier ratio), inlier_pixels the truncation of
    the score and the inlier test on the symmetric transfer error, seed the sampler's, refine_rounds rounds of local optimisation
    (0 .. 16).  Returns a HomographyResult; with want_inliers its inliers [O] mark the matches within inlier_pixels of the returned
    model.  Both poses of the plane are returned: the library does not choose between the twins.  An uploaded scene of `ba` is left
    untouched."""
    opts = _options(hypotheses, inlier_pixels, seed, refine_rounds)
    n, n_obs, args, _keep = _call_args(row_ptr, uv_a, uv_b, K_a, K_b, q, opts)
    out = _outputs(n, n_obs, want_inliers)
    ba._raise(lib().srk_relate_homography(C.c_void_p(ba._h), C.c_double(f0), *args, *[_d(o) for o in out]))
    return HomographyResult(*out)


def last_kernel_ms(ba):
    """device ms of the kernels of the last relate_homography call on this handle, and of its hypothesis-and-score kernel alone"""
    return float(lib().srk_ba_homography_kernel_ms(C.c_void_p(ba._h))), float(lib().srk_ba_homography_score_ms(C.c_void_p(ba._h)))


def check_pairs(row_ptr, uv_a, uv_b, K_a, K_b, q=None, hypotheses=256, inlier_pixels=6.0, seed=1, refine_rounds=4):
    """srk_homography_check_pairs (host only): None, or the text of the refusal"""
    opts = _options(hypotheses, inlier_pixels, seed, refine_rounds)
    _n, _n_obs, args, _keep = _call_args(row_ptr, uv_a, uv_b, K_a, K_b, q, opts)
    why = C.c_char_p()
    rc = lib().srk_homography_check_pairs(*args, C.byref(why))
    return None if rc == 0 else why.value.decode()


def host_pair(f0, uv_a, uv_b, K_a, K_b, q=None, hypotheses=256, inlier_pixels=6.0, seed=1, refine_rounds=4):
    """srk_homography_host_pair (host only): one pair in the kernels' own order of operations, as a HomographyResult of one pair"""
    a = np.ascontiguousarray(uv_a, dtype=np.float64).reshape(-1, 2)
    b = np.ascontiguousarray(uv_b, dtype=np.float64).reshape(-1, 2)
    w = None if q is None else np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    Ka, Kb = np.ascontiguousarray(K_a, dtype=np.float64).reshape(9), np.ascontiguousarray(K_b, dtype=np.float64).reshape(9)
    if b.shape[0] != a.shape[0] or (w is not None and w.size != a.shape[0]):
        raise ValueError("homography: the match arrays disagree about their length")
    opts = _options(hypotheses, inlier_pixels, seed, refine_rounds)
    out = _outputs(1, a.shape[0], True)
    rc = lib().srk_homography_host_pair(C.c_int64(a.shape[0]), _d(a), _d(b), _d(w), _d(Ka), _d(Kb), C.c_double(f0), C.byref(opts),
                                        *[_d(o) for o in out[:8]], _d(out[9]))
    if rc < 0:
        raise ValueError("homography: the checks refuse the pair")
    out[8][0] = rc
    return HomographyResult(*out)


def apply_homography(G, uv, f0):
    """the pixels uv [n][2] under p_b ~ G p_a with p = (u, v, f0): f0 (G p)_xy / (G p)_3"""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    y = np.column_stack([uv, np.full(len(uv), float(f0))]) @ np.asarray(G, dtype=np.float64).reshape(3, 3).T
    return float(f0) * y[:, :2] / y[:, 2:3]


def decompose_homography(H, x_a, x_b, q=None):
    """srk_homography_decompose (host only): the ray homography H (any scale and sign, x_b ~ H x_a) and the rays x_a, x_b [n][3]
    of its inliers into H = R + (T/d) N^T: both poses of the plane, the one with more inliers in front first, or with
    gap = w1 - w3 <= 1e-10 the rotation alone.  Returns a HomographyPoses."""
    Hm = np.ascontiguousarray(H, dtype=np.float64).reshape(9)
    xa = np.ascontiguousarray(x_a, dtype=np.float64).reshape(-1, 3)
    xb = np.ascontiguousarray(x_b, dtype=np.float64).reshape(-1, 3)
    w = None if q is None else np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    if xb.shape[0] != xa.shape[0] or (w is not None and w.size != xa.shape[0]):
        raise ValueError("homography: the ray arrays disagree about their length")
    Ho, R, T, N, front, gap = np.zeros((3, 3)), np.zeros((2, 3, 3)), np.zeros((2, 3)), np.zeros((2, 3)), np.zeros(2, np.int32), np.zeros(1)
    rc = lib().srk_homography_decompose(_d(Hm), C.c_int64(xa.shape[0]), _d(xa), _d(xb), _d(w), _d(Ho), _d(R), _d(T), _d(N), _d(front), _d(gap))
    if rc < 0:
        raise ValueError("homography: H must be finite and have a middle singular value")
    return HomographyPoses(Ho, rc, R, T, N, front, float(gap[0]))
