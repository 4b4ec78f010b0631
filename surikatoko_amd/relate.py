"""Two-view relative pose on the device (include/srk_ba.h): the rotation and the direction of the
translation between two cameras from their 2D-2D matches, wrong matches among them, by five-point hypotheses from a counter-based
sampler (16 lanes solve one hypothesis), each scored on every match by its Sampson distance (a wave is 64 hypotheses of one pair).
two_view_scene is the bootstrap this exists for: relate, triangulate the inliers, and a scene that Scene / upload take."""
import ctypes as C
from collections import namedtuple

import numpy as np

from ._lib import RelateOptions, lib
from .locate import ransac_hypotheses  # noqa: F401  (sample_size=5 gives the count for an outlier ratio)
from .triangulate import TRI_BEHIND, triangulate_tracks

# the bits of `status`
RELATE_FEW_POINTS = 1   # fewer than six matches with q > 0
RELATE_NO_MODEL = 2     # no sample gave an essential matrix
RELATE_STATUS_NAMES = {RELATE_FEW_POINTS: "FEW_POINTS", RELATE_NO_MODEL: "NO_MODEL"}

# R [n][3][3], T [n][3] (unit): x_b ~ R x_a + T; E [n][3][3] = [T]x R; related [n][8] (RMS truncated Sampson error in pixels,
# weighted matches, inliers, winning hypothesis, hypotheses with a model, the winning sample's sixth-match error in pixels, inliers
# in front of both cameras, their mean parallax in radians); status [n]; inliers [O] uint8 or None.  From relate_frames(..., refine=...)
# R, T, E are the REFINED pose (the C call has one set of pose outputs); the five-point winner itself is what the call without refine returns
RelateResult = namedtuple("RelateResult", "R T E related status inliers")

# cam_R [2][3][3], cam_T [2][3] (frame 0 = (I, 0), |cam_T[1]| = 1), points [N][3], and the observations point-major as Scene takes
# them (row_ptr [N + 1], obs_frame, obs_uv); match [N]: the match each point came from; relate: the RelateResult of the pair
TwoViewScene = namedtuple("TwoViewScene", "cam_R cam_T points row_ptr obs_frame obs_uv match relate")


def relate_status_names(status):
    """the names of the bits set in one status word"""
    return [name for bit, name in RELATE_STATUS_NAMES.items() if int(status) & bit]


def default_relate_options():
    """srk_relate_default_options as a dict: hypotheses, inlier_pixels, seed"""
    o = RelateOptions()
    lib().srk_relate_default_options(C.byref(o))
    return dict(hypotheses=o.hypotheses, inlier_pixels=o.inlier_pixels, seed=o.seed)


def _d(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def relate_pair_args(row_ptr, uv_a, uv_b, q, K_a, K_b):
    """the pair arrays as the C ABI takes them: (n_pairs, row_ptr, uv_a, uv_b, q or None, K_a, K_b, shared_k); the lengths are
    checked here, the values by the library"""
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64).reshape(-1)
    a = np.ascontiguousarray(uv_a, dtype=np.float64).reshape(-1, 2)
    b = np.ascontiguousarray(uv_b, dtype=np.float64).reshape(-1, 2)
    w = None if q is None else np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    if rp.size < 1:
        raise ValueError("relate: row_ptr needs at least one entry")
    n = rp.size - 1
    n_obs = max(int(rp.max()), 0)
    if a.shape[0] < n_obs or b.shape[0] < n_obs or (w is not None and w.size < n_obs):
        raise ValueError("relate: the match arrays are shorter than row_ptr says")
    Ka = np.ascontiguousarray(K_a, dtype=np.float64).reshape(-1, 9)
    Kb = np.ascontiguousarray(K_b, dtype=np.float64).reshape(-1, 9)
    shared_k = Ka.shape[0] == 1 and Kb.shape[0] == 1 and n != 1
    if not shared_k and (Ka.shape[0] != n or Kb.shape[0] != n):
        raise ValueError("relate: row_ptr, K_a and K_b disagree about the number of pairs")
    return n, rp, a, b, w, Ka, Kb, shared_k


def _call_args(row_ptr, uv_a, uv_b, K_a, K_b, q, hypotheses, inlier_pixels, seed):
    n, rp, a, b, w, Ka, Kb, shared_k = relate_pair_args(row_ptr, uv_a, uv_b, q, K_a, K_b)
    lo = RelateOptions(int(hypotheses), float(inlier_pixels), int(seed) & ((1 << 64) - 1))
    keep = (rp, a, b, w, Ka, Kb, lo)   # the arrays the pointers below point into
    return n, max(int(rp.max()), 0), [C.c_int32(n), _d(rp), _d(a), _d(b), _d(w), _d(Ka), _d(Kb), C.c_int(int(shared_k)), C.byref(lo)], keep


def relate_frames(ba, f0, row_ptr, uv_a, uv_b, K_a, K_b, q=None, hypotheses=256, inlier_pixels=2.0, seed=1, want_inliers=False, refine=None):
    """srk_relate_frames: pairs in CSR form (row_ptr [n + 1], uv_a, uv_b [O][2] pixels of the two images, q [O] information or None)
    and the intrinsics of the two cameras ([n][3][3] each, or one 3 x 3 each for all).  `hypotheses` samples per pair (1 .. 4096;
    ransac_hypotheses(share, p, sample_size=5) gives the count for an outlier ratio), inlier_pixels the truncation of the score and the
    inlier test, seed the sampler's.  Returns a RelateResult; with want_inliers its inliers [O] mark the matches within inlier_pixels
    of the winner's epipolar geometry.  An uploaded scene of `ba` is left untouched.
    refine: None, or a dict of the refinement's options (the keywords of pair.pair_options: attempts, rel_change, loss, delta,
    inliers_only; and want_weights): srk_relate_frames_refined, which refines every related pose over all the pair's matches (or,
    with inliers_only, the winner's inliers) without leaving the device, and returns (RelateResult, PairResult).  The RelateResult's
    R, T, E are then the refined ones."""
    n, n_obs, args, _keep = _call_args(row_ptr, uv_a, uv_b, K_a, K_b, q, hypotheses, inlier_pixels, seed)
    if refine is not None:
        from .pair import PairResult, pair_options, pair_outputs
        kw = dict(refine)
        want_weights = bool(kw.pop("want_weights", False))
        opts = pair_options(**kw)
        po = pair_outputs(n, n_obs, want_weights)
        related, status, inl = np.zeros((n, 8)), np.zeros(n, np.uint32), np.zeros(n_obs, np.uint8) if want_inliers else None
        ba._raise(lib().srk_relate_frames_refined(C.c_void_p(ba._h), C.c_double(f0), *args, C.byref(opts), _d(po[0]), _d(po[1]), _d(po[2]), _d(related),
                                                  _d(status), _d(inl), *[_d(a) for a in po[3:]]))
        return RelateResult(po[0], po[1], po[2], related, status, inl), PairResult(*po)
    out = (np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros((n, 3, 3)), np.zeros((n, 8)), np.zeros(n, np.uint32),
           np.zeros(n_obs, np.uint8) if want_inliers else None)
    ba._raise(lib().srk_relate_frames(C.c_void_p(ba._h), C.c_double(f0), *args, *[_d(a) for a in out]))
    return RelateResult(*out)


def last_kernel_ms(ba):
    """device ms of the kernels of the last relate_frames call on this handle, and of its score kernel alone"""
    return float(lib().srk_ba_relate_kernel_ms(C.c_void_p(ba._h))), float(lib().srk_ba_relate_score_ms(C.c_void_p(ba._h)))


def check_pairs(row_ptr, uv_a, uv_b, K_a, K_b, q=None, hypotheses=256, inlier_pixels=2.0, seed=1):
    """srk_relate_check_pairs (host only): None, or the text of the refusal"""
    _n, _n_obs, args, _keep = _call_args(row_ptr, uv_a, uv_b, K_a, K_b, q, hypotheses, inlier_pixels, seed)
    why = C.c_char_p()
    rc = lib().srk_relate_check_pairs(*args, C.byref(why))
    return None if rc == 0 else why.value.decode()


def host_pair(f0, uv_a, uv_b, K_a, K_b, q=None, hypotheses=256, inlier_pixels=2.0, seed=1):
    """srk_relate_host_pair (host only): one pair in the kernels' own order of operations, as a RelateResult of one pair"""
    a = np.ascontiguousarray(uv_a, dtype=np.float64).reshape(-1, 2)
    b = np.ascontiguousarray(uv_b, dtype=np.float64).reshape(-1, 2)
    w = None if q is None else np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    Ka, Kb = np.ascontiguousarray(K_a, dtype=np.float64).reshape(9), np.ascontiguousarray(K_b, dtype=np.float64).reshape(9)
    if b.shape[0] != a.shape[0] or (w is not None and w.size != a.shape[0]):
        raise ValueError("relate: the match arrays disagree about their length")
    lo = RelateOptions(int(hypotheses), float(inlier_pixels), int(seed) & ((1 << 64) - 1))
    out = (np.zeros((1, 3, 3)), np.zeros((1, 3)), np.zeros((1, 3, 3)), np.zeros((1, 8)), np.zeros(a.shape[0], np.uint8))
    rc = lib().srk_relate_host_pair(C.c_int64(a.shape[0]), _d(a), _d(b), _d(w), _d(Ka), _d(Kb), C.c_double(f0), C.byref(lo), *[_d(x) for x in out])
    if rc < 0:
        raise ValueError("relate: the checks refuse the pair")
    return RelateResult(out[0], out[1], out[2], out[3], np.array([rc], np.uint32), out[4])


def two_view_scene(ba, f0, uv_a, uv_b, K_a, K_b, q=None, hypotheses=256, inlier_pixels=2.0, seed=1, refine_attempts=10, refine=None):
    """The two-view bootstrap: relate the pair of images from its matches uv_a, uv_b [M][2], triangulate the inliers from (I, 0)
    and (R, T) (triangulate_tracks, refined), drop the tracks that lie behind a camera, and return a TwoViewScene: poses, points and
    point-major observations as Scene(points, cam_R, cam_T, K, shared_k, row_ptr, obs_frame, obs_uv) takes them, in the scale
    |T| = 1.  Raises ValueError when the pair was not related (TwoViewScene.relate.status would be non-zero).
    refine (None, or the dict relate_frames takes): the pose is refined over the pair's matches before the inliers are triangulated
    from it; TwoViewScene.relate then holds the refined R, T, E.
    To bundle-adjust the result, give Scene the intrinsics as K * f0 (the same cameras, K(2,2) = f0): with K / f0 the adjuster's pose
    derivatives are not those of the error and it moves the scene little or, with two different cameras, not
    at all."""
    a = np.ascontiguousarray(uv_a, dtype=np.float64).reshape(-1, 2)
    b = np.ascontiguousarray(uv_b, dtype=np.float64).reshape(-1, 2)
    rel = relate_frames(ba, f0, [0, a.shape[0]], a, b, np.reshape(K_a, (1, 9)), np.reshape(K_b, (1, 9)), q=q, hypotheses=hypotheses,
                        inlier_pixels=inlier_pixels, seed=seed, want_inliers=True, refine=refine)
    if refine is not None:
        rel = rel[0]
    if rel.status[0]:
        raise ValueError(f"two_view_scene: the pair was not related ({', '.join(relate_status_names(rel.status[0]))})")
    match = np.flatnonzero(rel.inliers)
    cam_R = np.stack([np.eye(3), rel.R[0]])
    cam_T = np.stack([np.zeros(3), rel.T[0]])
    K = np.stack([np.reshape(K_a, (3, 3)), np.reshape(K_b, (3, 3))]).astype(np.float64)
    uv = np.stack([a[match], b[match]], axis=1).reshape(-1, 2)          # track k: its match in frame 0, then in frame 1
    w = None if q is None else np.repeat(np.asarray(q, dtype=np.float64)[match], 2)
    X, _quality, status = triangulate_tracks(ba, f0, 2 * np.arange(len(match) + 1), np.tile(np.array([0, 1], np.int32), len(match)), uv, cam_R, cam_T, K,
                                             q=w, refine_attempts=refine_attempts)
    keep = (status & TRI_BEHIND) == 0
    keep &= np.all(np.isfinite(X), axis=1)
    n = int(keep.sum())
    return TwoViewScene(cam_R, cam_T, X[keep], 2 * np.arange(n + 1, dtype=np.int64), np.tile(np.array([0, 1], np.int32), n),
                        uv.reshape(-1, 2, 2)[keep].reshape(-1, 2), match[keep], rel)
