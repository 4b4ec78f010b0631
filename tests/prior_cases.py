"""The (scene, prior set, keep_gauge) cases of the position-prior tests, shared by tests/test_gpu_priors.py (which runs them
against the yardstick of tests/prior_ref.py) and tests/test_prior_cpu.py (which checks that every one of them gives a
well-conditioned positive definite system).  The scenes are those of tests/constant_cases.py.

The sets sit where the two passes can go wrong: the first and the last landmark of a scene whose N (600) is no multiple of
64, every 7th landmark, every landmark (three blocks of the energy pass), a landmark on a track too long for the run-based
Schur kernels, the gauge frames with both gauge settings, the last frames, frames whose variables straddle the tile and panel
edges of the reduced camera system (constant_cases.py), a full information matrix on a scene uploaded un-normalised with a
rotated frame 0, a rank-1 (height only) information matrix.

Information: E is in (pix / f0)^2 with f0 = 600 and the scenes' 0.3-pixel noise, and the scenes' extent is about one world
unit, so a landmark block (two derivatives of a projection per observation, tracks of 2..30) is of order 10..100 and a frame's
translation block (hundreds of observations) of order 1000.  L = 10 for landmarks and L = 100 for centres put 2 L at the
size of the blocks they are added to: neither term drowns the other in the sums the comparisons look at.  The prior means
are the scene's own positions moved by a seeded offset of up to 5e-3, so that every prior gradient is non-zero."""
import numpy as np

import surikatoko_amd as sa
import constant_cases as cc
import prior_ref as pref

L_POINT = 10.0
L_FRAME = 100.0
OFFSET = 5e-3


def _iso(n, lam):
    return np.broadcast_to(lam * np.eye(3), (n, 3, 3)).copy()


def _full(n, lam, seed):
    """positive definite with off-diagonal entries: lam (A A^T + I / 2), A seeded in [-1, 1]"""
    A = np.random.RandomState(seed).uniform(-1, 1, size=(n, 3, 3))
    return lam * (np.einsum("nab,ncb->nac", A, A) + 0.5 * np.eye(3))


def _height(n, lam):
    L = np.zeros((n, 3, 3))
    L[:, 2, 2] = lam
    return L


def rodrigues(w):
    """rotation matrix of the axis-angle vector w"""
    w = np.asarray(w, dtype=np.float64)
    ang = float(np.linalg.norm(w))
    if ang == 0:
        return np.eye(3)
    k = w / ang
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


INFO = {"iso": _iso, "full": lambda n, lam: _full(n, lam, 11), "height": _height}


def rotated(sc):
    """the same scene in other world coordinates X' = a (Q X + t): frame 0 is rotated and off the origin and the baseline is
    not 1, so the upload's normalisation has R0 != I and s != 1.  R' = R Q^T, T' = a (T - R Q^T t); observations unchanged."""
    Q = rodrigues([0.3, -0.5, 0.4])
    t = np.array([0.7, -1.1, 0.4])
    a = 2.5
    out = sc.copy()
    R = sc.cam_R.reshape(-1, 3, 3)
    Rn = R @ Q.T
    out.cam_R[:] = Rn.reshape(-1, 9)
    out.cam_T[:] = a * (sc.cam_T - Rn @ t)
    out.points[:] = a * (sc.points @ Q.T + t)
    return out


# name -> (scene, landmarks(sc) or None, frames(sc) or None, information kind, keep_gauge, frame variables, rotated world)
CASES = {
    "nf16_first_and_last_landmark": ("nf16_10_tiles", lambda sc: [0, sc.N - 1], None, "iso", 1, 10, False),
    "nf16_every_7th_landmark": ("nf16_10_tiles", lambda sc: cc._every(sc.N, 7), None, "iso", 1, 10, False),
    "nf16_every_landmark": ("nf16_10_tiles", lambda sc: np.arange(sc.N), None, "iso", 1, 10, False),
    "nf16_every_landmark_free_gauge": ("nf16_10_tiles", lambda sc: np.arange(sc.N), None, "iso", 0, 10, False),
    "long_fallback_landmark": ("long_nf30", lambda sc: [0, cc._longest_track(sc), sc.N - 1], None, "iso", 1, 10, False),
    "long_fallback_landmark_fixed_k": ("long_nf30", lambda sc: [0, cc._longest_track(sc), sc.N - 1],
                                       lambda sc: [sc.M - 2, sc.M - 1], "iso", 1, 6, False),
    "nf16_gauge_frames_keep": ("nf16_10_tiles", None, lambda sc: [0, 1], "iso", 1, 10, False),
    "nf16_gauge_frames_free_gauge": ("nf16_10_tiles", lambda sc: cc._every(sc.N, 7), lambda sc: [0, 1], "iso", 0, 10, False),
    "nf16_last_two_frames": ("nf16_10_tiles", None, lambda sc: [sc.M - 2, sc.M - 1], "iso", 1, 10, False),
    "ragged_frames_12_25_tile_and_panel_edges": ("ragged_20", None, lambda sc: [5, 12, 25, 41], "iso", 1, 10, False),
    "ragged_frames_21_42_fixed_k": ("ragged_20", None, lambda sc: [8, 21, 42, 59], "iso", 1, 6, False),
    "ragged_frames_12_25_free_gauge": ("ragged_20", lambda sc: cc._every(sc.N, 7), lambda sc: [12, 25], "iso", 0, 10, False),
    "nf2_full_information_rotated_world": ("nf2_short_runs", lambda sc: cc._every(sc.N, 3), lambda sc: [2, 5], "full", 1, 10, True),
    "nf16_full_information_rotated_world_free_gauge": ("nf16_10_tiles", lambda sc: cc._every(sc.N, 7), lambda sc: [3, 12], "full", 0, 10, True),
    "nf16_height_only": ("nf16_10_tiles", lambda sc: cc._every(sc.N, 7), lambda sc: [3, 12], "height", 1, 10, False),
}
# the case the mode tests run
MODE_CASE = "nf16_frames_and_landmarks"
CASES[MODE_CASE] = ("nf16_10_tiles", lambda sc: cc._every(sc.N, 7), lambda sc: [3, 12], "iso", 1, 10, False)
CASES[MODE_CASE + "_fixed_k"] = ("nf16_10_tiles", lambda sc: cc._every(sc.N, 7), lambda sc: [3, 12], "iso", 1, 6, False)
# end to end: ten iterations with the gauge kept and released
CASES["nf16_ten_iterations_free_gauge"] = ("nf16_10_tiles", lambda sc: cc._every(sc.N, 7), lambda sc: [3, 12], "iso", 0, 10, False)
# a scene of its own for the two-kernel derivative path and the unstaged error kernel: with 60 frames and tracks of 50 no
# workgroup's frame window fits the fused kernel (the scene of hetero_cases.py's "two_kernel_60"); none of the scenes of
# constant_cases.py takes that path
EXTRA_SCENES = {"two_kernel_60": sa.SceneSpec(n_frames=60, grid_nx=12, grid_ny=10, vis_window=50)}
TWO_KERNEL_CASE = "two_kernel_60_frames_and_landmarks"
CASES[TWO_KERNEL_CASE] = ("two_kernel_60", lambda sc: cc._every(sc.N, 7), lambda sc: [3, 12, 59], "iso", 1, 10, False)
# the reordered-frames cases: priors of the unshuffled scene (the test maps the frames through the shuffle, which leaves the
# reduced camera system the same up to a symmetric permutation, so its conditioning is the one checked here)
REORDER_CASES = ("nf16_reordered", "nf16_reordered_free_gauge")
CASES[REORDER_CASES[0]] = ("nf16_10_tiles", lambda sc: cc._every(sc.N, 7), lambda sc: [0, 1, 9, 17], "iso", 1, 10, False)
CASES[REORDER_CASES[1]] = ("nf16_10_tiles", lambda sc: cc._every(sc.N, 7), lambda sc: [0, 1, 9, 17], "iso", 0, 10, False)
FREE_GAUGE_CASES = [n for n, v in CASES.items() if v[4] == 0]


def constant_combination(sc, pri):
    """(frame mask, landmark mask) of the constant blocks the mode case is combined with: a frame and every third landmark
    that carry a prior, and a frame and a landmark that do not"""
    fconst = np.zeros(sc.M, dtype=bool)
    pconst = np.zeros(sc.N, dtype=bool)
    fconst[[int(pri.fidx[0]), 7]] = True
    pconst[pri.pidx[::3]] = True
    pconst[5] = True
    return fconst, pconst
_extra = {}


def priors_for(sc, pts, frames, kind="iso", seed=23, l_point=L_POINT, l_frame=L_FRAME):
    """priors at the scene's own positions moved by a seeded offset, in the scene's coordinates"""
    rs = np.random.RandomState(seed)
    pidx = np.zeros(0, np.int64) if pts is None else np.unique(np.asarray(pts, dtype=np.int64))
    fidx = np.zeros(0, np.int32) if frames is None else np.unique(np.asarray(frames, dtype=np.int32))
    ext = float(np.abs(sc.points - sc.points.mean(axis=0)).max())
    ppos = sc.points[pidx] + ext * rs.uniform(-OFFSET, OFFSET, size=(pidx.size, 3))
    fpos = pref.centres(sc)[fidx] + ext * rs.uniform(-OFFSET, OFFSET, size=(fidx.size, 3))
    # information in units of E per squared world unit: the isotropic values hold for an extent of one
    return pref.Priors(pidx, ppos, INFO[kind](pidx.size, l_point / ext ** 2), fidx, fpos, INFO[kind](fidx.size, l_frame / ext ** 2))


def case(name):
    """(scene copy, f0, priors in the scene's coordinates, keep_gauge, fv)"""
    sname, pf, ff, kind, keep_gauge, fv, rot = CASES[name]
    if sname in EXTRA_SCENES:
        if sname not in _extra:
            _extra[sname] = sa.generate_scene(EXTRA_SCENES[sname])
        sc, f0 = _extra[sname].copy(), EXTRA_SCENES[sname].f0
    else:
        sc, f0 = cc.scene(sname)
    if rot:
        sc = rotated(sc)
    pri = priors_for(sc, None if pf is None else pf(sc), None if ff is None else ff(sc), kind)
    return sc, f0, pri, keep_gauge, fv


L_GEOREF = 0.1


def georeferencing():
    """the noise-free 24-frame scene of constant_cases.sliding_window(k22_f0=True) with its first 8 frames perturbed as well
    (rotations by a seeded axis-angle of up to 1e-3, translations by up to 1e-3), so that every frame and every point is off
    the ground truth by 1e-3, and priors at the ground-truth centres of all 24 frames.  One scalar L = 0.1 (E per squared world
    unit): the centres start several 1e-3 off (a rotation of 1e-3 moves a centre by 1e-3 times its distance from the origin),
    which gives a prior sum of 4.7e-4 at the start beside a reprojection sum of 8.4e-5 (computed by
    tests/test_prior_cpu.py, which asserts that they lie within a factor 100 of each other).
    Returns (spec, scene, priors, pts_gt, R_gt, T_gt)."""
    spec, sc, pts_gt, R_gt, T_gt, _ = cc.sliding_window(k22_f0=True)
    rs = np.random.RandomState(17)
    for j in range(8):
        w = rs.uniform(-1e-3, 1e-3, size=3)
        sc.cam_R[j] = (rodrigues(w) @ R_gt[j].reshape(3, 3)).reshape(9)
        sc.cam_T[j] = T_gt[j] + rs.uniform(-1e-3, 1e-3, size=3)
    assert np.all(np.abs(sc.cam_T - T_gt).max(axis=1) > 1e-4) and np.all(np.abs(sc.cam_R - R_gt).max(axis=1) > 1e-5)
    gt = sa.Scene(pts_gt, R_gt, T_gt, sc.K, sc.shared_k, sc.row_ptr, sc.obs_frame, sc.obs_uv)
    pri = pref.Priors(fidx=np.arange(sc.M), fpos=pref.centres(gt), finfo=_iso(sc.M, L_GEOREF))
    return spec, sc, pri, pts_gt, R_gt, T_gt
