"""The two-view fundamental matrix on the device (include/srk_ba.h): p_b^T F p_a = 0 between the 2D-2D matches
of pairs of images, wrong matches among them, without intrinsics: seven-point hypotheses from a counter-based sampler (an eighth
match chooses among the cubic's roots), each scored on every match by the Sampson distance (a wave is 64 hypotheses of one pair),
the winner refined by Levenberg-Marquardt attempts over F = U diag(1, sigma, 0) V^T.  The member of the family for cameras whose K
is a guess: geometric verification of matches that does not depend on K."""
import ctypes as C
from collections import namedtuple

import numpy as np

from ._lib import FundamentalOptions, lib
from .locate import ransac_hypotheses  # noqa: F401  (sample_size=7 gives the count for an outlier ratio)

# the bits of `status`
FUNDAMENTAL_FEW_POINTS = 1   # fewer than eight matches with q > 0
FUNDAMENTAL_NO_MODEL = 2     # no sample gave a fundamental matrix
FUNDAMENTAL_STATUS_NAMES = {FUNDAMENTAL_FEW_POINTS: "FEW_POINTS", FUNDAMENTAL_NO_MODEL: "NO_MODEL"}

# F [n][3][3] (norm 1, rank 2, its largest entry positive); U, V [n][3][3] proper rotations and sigma [n] with
# F = U diag(1, sigma, 0) V^T / sqrt(1 + sigma^2): the epipoles are U[:, :, 2] (in image b) and V[:, :, 2] (in image a), homogeneous
# in (u, v, f0); fund [n][12] (RMS truncated error in pixels, weighted matches, inliers, winning hypothesis, hypotheses with a model,
# the eighth-match error in pixels, attempts accepted, attempts used, the inliers' RMS Sampson distance, sigma, cond_1 of the scaled
# H, the real roots of the winning sample); info [n][7][7] = sum q J^T J over the inliers in the order [a; b; delta]; status [n];
# inliers [O] uint8 or None
FundamentalResult = namedtuple("FundamentalResult", "F U V sigma fund info status inliers")


def fundamental_status_names(status):
    """the names of the bits set in one status word"""
    return [name for bit, name in FUNDAMENTAL_STATUS_NAMES.items() if int(status) & bit]


def default_fundamental_options():
    """srk_fundamental_default_options as a dict"""
    o = FundamentalOptions()
    lib().srk_fundamental_default_options(C.byref(o))
    return dict(hypotheses=o.hypotheses, inlier_pixels=o.inlier_pixels, seed=o.seed, refine_rounds=o.refine_rounds)


def _d(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _options(hypotheses, inlier_pixels, seed, refine_rounds):
    return FundamentalOptions(int(hypotheses), float(inlier_pixels), int(seed) & ((1 << 64) - 1), int(refine_rounds))


def _outputs(n, n_obs, want_inliers):
    return (np.zeros((n, 3, 3)), np.zeros((n, 3, 3)), np.zeros((n, 3, 3)), np.zeros(n), np.zeros((n, 12)), np.zeros((n, 7, 7)),
            np.zeros(n, np.uint32), np.zeros(n_obs, np.uint8) if want_inliers else None)


def _call_args(row_ptr, uv_a, uv_b, q, opts):
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64).reshape(-1)
    a = np.ascontiguousarray(uv_a, dtype=np.float64).reshape(-1, 2)
    b = np.ascontiguousarray(uv_b, dtype=np.float64).reshape(-1, 2)
    w = None if q is None else np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    if rp.size < 1:
        raise ValueError("fundamental: row_ptr needs at least one entry")
    n, n_obs = rp.size - 1, max(int(rp.max()), 0)
    if a.shape[0] < n_obs or b.shape[0] < n_obs or (w is not None and w.size < n_obs):
        raise ValueError("fundamental: the match arrays are shorter than row_ptr says")
    keep = (rp, a, b, w, opts)   # the arrays the pointers below point into
    return n, n_obs, [C.c_int32(n), _d(rp), _d(a), _d(b), _d(w), C.byref(opts)], keep


def relate_uncalibrated(ba, f0, row_ptr, uv_a, uv_b, q=None, hypotheses=256, inlier_pixels=2.0, seed=1, refine_rounds=8, want_inliers=False):
    """srk_relate_uncalibrated: pairs in CSR form (row_ptr [n + 1], uv_a, uv_b [O][2] pixels of the two images, q [O] information or
    None); no intrinsics.  `hypotheses` samples per pair (1 .. 4096; ransac_hypotheses(share, p, sample_size=7) gives the count for
    an outlier ratio), inlier_pixels the truncation of the score and the inlier test on the Sampson distance, seed the sampler's,
    refine_rounds Levenberg-Marquardt attempts (0 .. 16).  Returns a FundamentalResult; with want_inliers its inliers [O] mark the
    matches within inlier_pixels of the returned model.  An uploaded scene of `ba` is left untouched."""
    opts = _options(hypotheses, inlier_pixels, seed, refine_rounds)
    n, n_obs, args, _keep = _call_args(row_ptr, uv_a, uv_b, q, opts)
    out = _outputs(n, n_obs, want_inliers)
    ba._raise(lib().srk_relate_uncalibrated(C.c_void_p(ba._h), C.c_double(f0), *args, *[_d(o) for o in out]))
    return FundamentalResult(*out)


def last_kernel_ms(ba):
    """device ms of the kernels of the last relate_uncalibrated call on this handle, and of its score kernel alone"""
    return float(lib().srk_ba_fundamental_kernel_ms(C.c_void_p(ba._h))), float(lib().srk_ba_fundamental_score_ms(C.c_void_p(ba._h)))


def last_solve_ms(ba):
    """device ms of the solve kernel (the seven-point models) of the last relate_uncalibrated call on this handle"""
    return float(lib().srk_ba_fundamental_solve_ms(C.c_void_p(ba._h)))


def check_pairs(row_ptr, uv_a, uv_b, q=None, hypotheses=256, inlier_pixels=2.0, seed=1, refine_rounds=8):
    """srk_fundamental_check_pairs (host only): None, or the text of the refusal"""
    opts = _options(hypotheses, inlier_pixels, seed, refine_rounds)
    _n, _n_obs, args, _keep = _call_args(row_ptr, uv_a, uv_b, q, opts)
    why = C.c_char_p()
    rc = lib().srk_fundamental_check_pairs(*args, C.byref(why))
    return None if rc == 0 else why.value.decode()


def host_pair(f0, uv_a, uv_b, q=None, hypotheses=256, inlier_pixels=2.0, seed=1, refine_rounds=8):
    """srk_fundamental_host_pair (host only): one pair in the kernels' own order of operations, as a FundamentalResult of one pair"""
    a = np.ascontiguousarray(uv_a, dtype=np.float64).reshape(-1, 2)
    b = np.ascontiguousarray(uv_b, dtype=np.float64).reshape(-1, 2)
    w = None if q is None else np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    if b.shape[0] != a.shape[0] or (w is not None and w.size != a.shape[0]):
        raise ValueError("fundamental: the match arrays disagree about their length")
    opts = _options(hypotheses, inlier_pixels, seed, refine_rounds)
    out = _outputs(1, a.shape[0], True)
    rc = lib().srk_fundamental_host_pair(C.c_int64(a.shape[0]), _d(a), _d(b), _d(w), C.c_double(f0), C.byref(opts), *[_d(o) for o in out[:6]],
                                         _d(out[7]))
    if rc < 0:
        raise ValueError("fundamental: the checks refuse the pair")
    out[6][0] = rc
    return FundamentalResult(*out)


def _homog(uv, f0):
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    return np.column_stack([uv, np.full(len(uv), float(f0))])


def epipolar_lines(F, uv, f0):
    """the epipolar lines [n][3] in image b of the pixels uv [n][2] of image a: l = F p_a with p = (u, v, f0), scaled so that
    (l_0, l_1) is a unit vector and p_b . l is the distance of p_b = (u_b, v_b, f0) from the line in pixels.  With F transposed
    the lines in image a of pixels of image b."""
    l = _homog(uv, f0) @ np.asarray(F, dtype=np.float64).reshape(3, 3).T
    return l / np.linalg.norm(l[:, :2], axis=1, keepdims=True)


def pose_from_fundamental(F, K_a, K_b, uv_a, uv_b, f0, inliers=None):
    """The relative pose of a pair from its fundamental matrix and intrinsics: E ~ K_b^T F K_a is projected onto the essential
    matrices by numpy's SVD (singular values 1, 1, 0); of its four poses (x_b ~ R x_a + T) the one with the most matches (those
    marked by `inliers`, or all) at a positive depth in both cameras is returned as (R, unit T), ready as R0, T0 of refine_pairs."""
    Ka, Kb = np.asarray(K_a, dtype=np.float64).reshape(3, 3), np.asarray(K_b, dtype=np.float64).reshape(3, 3)
    E = Kb.T @ np.asarray(F, dtype=np.float64).reshape(3, 3) @ Ka
    U, _s, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    pa, pb = _homog(uv_a, f0), _homog(uv_b, f0)
    if inliers is not None:
        keep = np.asarray(inliers).reshape(-1).astype(bool)
        pa, pb = pa[keep], pb[keep]
    xa, xb = pa @ np.linalg.inv(Ka).T, pb @ np.linalg.inv(Kb).T
    best, pose = -1, None
    for R in (U @ W @ Vt, U @ W.T @ Vt):
        for T in (U[:, 2], -U[:, 2]):
            ra = xa @ R.T
            # depth_b x_b = depth_a R x_a + T, in the least-squares sense per match
            aa, ab, bb = np.sum(ra * ra, 1), np.sum(ra * xb, 1), np.sum(xb * xb, 1)
            at, bt = ra @ T, xb @ T
            det = aa * bb - ab * ab
            with np.errstate(divide="ignore", invalid="ignore"):
                da, db = (-bb * at + ab * bt) / det, (aa * bt - ab * at) / det
            front = int(np.sum((da > 0) & (db > 0)))
            if front > best:
                best, pose = front, (R, T / np.linalg.norm(T))
    return pose
