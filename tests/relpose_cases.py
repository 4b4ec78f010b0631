"""The (scene, factor set) cases of the relative-pose factor tests, shared by tests/test_gpu_relpose.py (which runs them
against the yardstick of tests/relpose_ref.py) and tests/test_relpose_cpu.py (which checks that every one of them gives a
well-conditioned positive definite system).  The scenes are those of tests/constant_cases.py.

The pairs sit where the three passes can go wrong: the gauge frames (their fixed variables' rows and columns must stay
identity), a frame with five incident factors (the ordered list walk), pairs whose variables straddle the 128-row tile and
the 256-column panel edges of the reduced camera system (frames 12 | 13 and 25 | 26 with ten variables a frame, 21 | 22 and
42 | 43 with six), a pair of frames that share no landmark (the skyline grows), a pair given as (b, a) with b > a (the
transposed block), the two-kernel derivative path and the long-track Schur path.

Information: E is in (pix / f0)^2 with f0 = 600, and the scenes' extent is about one world unit, so a frame's translation
block (hundreds of observations) is of order 1000 and its rotation block of the same order times the squared distance to the
landmarks.  L_tt = 100 per squared extent and L_rr = 100 put 2 J^T L J at a tenth of the blocks they are added to: neither term
drowns the other in the sums the comparisons look at.  The measurements are the scene's own relative poses moved by a seeded
offset of up to 5e-3 (of the extent, and radians), so that every factor gradient is non-zero.  Those residual rotations sit
between 1e-3 and 9e-3 rad; sweep_case, pi_case and residual_sweep put them at every angle of so3_ref.SWEEP and at pi."""
import numpy as np

import surikatoko_amd as sa
import constant_cases as cc
import prior_cases as pc
import relpose_ref as rr
import so3_ref as so3

L_T = 100.0
L_R = 100.0
OFFSET = 5e-3


def _diag(n, ext):
    L = np.zeros((n, 6, 6))
    L[:, [0, 1, 2], [0, 1, 2]] = L_T / ext ** 2
    L[:, [3, 4, 5], [3, 4, 5]] = L_R
    return L


def _full(n, ext, seed=11):
    """positive definite with every entry non-zero, the translation rows and columns scaled by 1 / extent"""
    A = np.random.RandomState(seed).uniform(-1, 1, size=(n, 6, 6))
    L = 100.0 * (np.einsum("nab,ncb->nac", A, A) / 3.0 + 0.5 * np.eye(6))
    D = np.diag([1 / ext] * 3 + [1.0] * 3)
    return np.einsum("ab,nbc,cd->nad", D, L, D)


def chain(M):
    return [(j, j + 1) for j in range(M - 1)]


def factors_for(sc, pairs, kind="diag", seed=29, offset=OFFSET, angle=None, axes=None):
    """factors on the given pairs (each as given: (a, b) in that direction), sorted by (min, max), measuring the scene's own
    relative poses moved by a seeded offset; in the scene's coordinates.  With angle the rotation is not moved by that offset:
    Z = P Exp(phi)^T with P the scene's own R_a R_b^T and |phi| = angle about a seeded axis per factor (or axes[k]), so the
    rotation residual Log(Z^T P) is phi up to the rounding of the two products, in any world coordinates; the translation
    parts are moved as without angle."""
    pairs = sorted(pairs, key=lambda p: (min(p), max(p)))
    rs = np.random.RandomState(seed)
    n = len(pairs)
    ext = float(np.abs(sc.points - sc.points.mean(axis=0)).max())
    Z, z = np.zeros((n, 3, 3)), np.zeros((n, 3))
    for k, (a, b) in enumerate(pairs):
        Zk, zk = rr.relative_pose(sc, a, b)
        Z[k] = Zk @ pc.rodrigues(rs.uniform(-offset, offset, size=3))
        z[k] = zk + ext * rs.uniform(-offset, offset, size=3)
    if angle is not None:
        ax = so3.axes(n + 1, seed)[1:] if axes is None else np.asarray(axes, dtype=np.float64).reshape(n, 3)
        for k, (a, b) in enumerate(pairs):
            Z[k] = rr.relative_pose(sc, a, b)[0] @ so3.exp(angle * ax[k]).T
    info = _full(n, ext) if kind == "full" else _diag(n, ext)
    return rr.Factors([p[0] for p in pairs], [p[1] for p in pairs], Z, z, info)


# name -> (scene, pairs(sc), information kind, frame variables, rotated world, constant frames or None, keep_gauge)
CASES = {
    "nf2_gauge_frames_full_information_rotated_world": ("nf2_short_runs", lambda sc: [(0, 1), (1, 2), (4, 5)], "full", 10, True, None, 1),
    "nf16_chain_and_five_factors_on_frame_3": ("nf16_10_tiles", lambda sc: chain(sc.M) + [(3, 12), (3, 5), (3, 20)], "diag", 10, False, None, 1),
    "ragged_12_13_25_26_tile_and_panel_edges": ("ragged_20", lambda sc: [(12, 13), (25, 26)], "diag", 10, False, None, 1),
    "ragged_21_22_42_43_fixed_k": ("ragged_20", lambda sc: [(21, 22), (42, 43)], "diag", 6, False, None, 1),
    "ragged_loop_closure_2_59": ("ragged_20", lambda sc: [(2, 59)], "diag", 10, False, None, 1),
    "ragged_pairs_given_backwards": ("ragged_20", lambda sc: [(13, 12), (40, 22), (59, 2)], "full", 10, False, None, 1),
    "long_nf30": ("long_nf30", lambda sc: [(0, 1), (10, 40), (46, 47)], "diag", 10, False, None, 1),
    "nf16_constant_and_free_frame": ("nf16_10_tiles", lambda sc: [(3, 4), (7, 12), (12, 13), (20, 23)], "diag", 10, False, [3, 12], 1),
    "nf16_frame_0_constant_free_gauge": ("nf16_10_tiles", lambda sc: chain(sc.M), "diag", 6, False, [0], 0),
}
# the case the mode tests run
MODE_CASE = "nf16_mode"
CASES[MODE_CASE] = ("nf16_10_tiles", lambda sc: [(3, 4), (3, 12), (11, 12), (20, 23)], "diag", 10, False, None, 1)
CASES[MODE_CASE + "_fixed_k"] = ("nf16_10_tiles", lambda sc: [(3, 4), (3, 12), (11, 12), (20, 23)], "diag", 6, False, None, 1)
TWO_KERNEL_CASE = "two_kernel_60"
CASES[TWO_KERNEL_CASE] = ("two_kernel_60", lambda sc: [(3, 4), (12, 30), (58, 59)], "diag", 10, False, None, 1)
# the reordered-frames case: factors of the unshuffled scene (the test maps the frames through the shuffle)
REORDER_CASE = "nf16_reordered"
CASES[REORDER_CASE] = ("nf16_10_tiles", lambda sc: [(0, 1), (1, 9), (9, 17), (17, 23), (5, 6)], "diag", 10, False, None, 1)

_extra = {}


def case(name):
    """(scene copy, f0, factors in the scene's coordinates, fv, constant-frame mask, keep_gauge)"""
    if name in SWEEP_CASES:
        return pi_case() if name == PI_CASE else sweep_case(SWEEP_CASES[name])
    sname, pf, kind, fv, rot, fc, keep_gauge = CASES[name]
    if sname in pc.EXTRA_SCENES:
        if sname not in _extra:
            _extra[sname] = sa.generate_scene(pc.EXTRA_SCENES[sname])
        sc, f0 = _extra[sname].copy(), pc.EXTRA_SCENES[sname].f0
    else:
        sc, f0 = cc.scene(sname)
    if rot:
        sc = pc.rotated(sc)
    fconst = np.zeros(sc.M, dtype=bool)
    if fc is not None:
        fconst[fc] = True
    return sc, f0, factors_for(sc, pf(sc), kind), fv, fconst, keep_gauge


# ------------------------------------------------------------------ the whole range of residual angles (so3_ref.SWEEP)
# Three factors with full information on the smallest scene: one on the gauge frames, one on (2, 4), one given backwards.
SWEEP = so3.SWEEP
SWEEP_SCENE = "nf2_short_runs"
SWEEP_PAIRS = [(0, 1), (2, 4), (5, 3)]


def sweep_case(angle, fv=10):
    """(scene copy, f0, factors whose rotation residuals all have the given angle, fv, constant-frame mask, keep_gauge)"""
    sc, f0 = cc.scene(SWEEP_SCENE)
    return sc, f0, factors_for(sc, SWEEP_PAIRS, "full", angle=angle), fv, np.zeros(sc.M, dtype=bool), 1


def pi_case(fv=10):
    """two factors whose measurements are half a turn away from the scene's relative rotations: (2, 4) about a coordinate
    axis, Z = P diag(1, -1, -1) exactly, and (5, 3) about a seeded axis.  The rounding of the normalisation and of the two
    products puts the residual on either side of pi, so Log may return +pi a or -pi a: the information matrix is diagonal with
    a multiple of I as its rotation part, for which the energy does not depend on that sign."""
    sc, f0 = cc.scene(SWEEP_SCENE)
    fac = factors_for(sc, SWEEP_PAIRS[1:], "diag", angle=np.pi)
    fac.Z[0] = rr.relative_pose(sc, int(fac.a[0]), int(fac.b[0]))[0] @ np.diag([1.0, -1.0, -1.0])
    return sc, f0, fac, fv, np.zeros(sc.M, dtype=bool), 1


PI_CASE = "sweep_exactly_pi"
# name -> angle: what tests/test_relpose_cpu.py checks for conditioning beside CASES
SWEEP_CASES = {**{f"sweep_{a:.12g}": a for a in SWEEP}, PI_CASE: np.pi}


def residual_sweep(part):
    """factors for the residual getter: all 15 pairs of the six frames, every third one given backwards, factor k at the angle
    SWEEP[15 * part + k] (part 0 or 1: a pair carries one factor, so the sweep takes two settings)"""
    sc, f0 = cc.scene(SWEEP_SCENE)
    angles = SWEEP[15 * part:15 * part + 15]
    pairs = [(a, b) for a in range(sc.M) for b in range(a + 1, sc.M)][:len(angles)]
    pairs = [(b, a) if k % 3 == 2 else (a, b) for k, (a, b) in enumerate(pairs)]
    fac = factors_for(sc, pairs, "diag", angle=0.0)
    ax = so3.axes(len(pairs) + 1, 31 + part)[1:]
    for k in range(fac.n):
        fac.Z[k] = rr.relative_pose(sc, int(fac.a[k]), int(fac.b[k]))[0] @ so3.exp(angles[k] * ax[k]).T
    return sc, f0, fac, np.asarray(angles)


CHUNKED = sa.SceneSpec(n_frames=330, grid_nx=60, grid_ny=40, vis_window=8)  # the smallest scene of test_chunked_solve_equals_single_chain

SCALE = 1.02


def metric_scale():
    """The noise-free 24-frame scene of constant_cases.sliding_window(k22_f0=True) at its ground truth, every centre but frame
    0's and every landmark scaled by 1.02 about C_0 (R unchanged, T_j = -R_j C_j): the projections, and so the reprojection
    sum, do not see that scale.  Factors with the ground-truth relative poses on the consecutive pairs do: their translation
    residuals are 2 % of the baselines.  Frame 0 is constant and the reference's gauge released, so the seven gauge freedoms
    are held by frame 0 (six) and the factors' translation parts (the scale).  L_tt = 1 per squared world unit (of order the
    landmark-driven translation curvature divided by 1000, so the reprojection terms dominate the shape and the factors the
    scale), L_rr = 1.  Returns (spec, scene, factors, fconst, pts_gt, R_gt, T_gt)."""
    spec, sc, pts_gt, R_gt, T_gt, _ = cc.sliding_window(k22_f0=True)
    gt = sa.Scene(pts_gt.copy(), R_gt.copy(), T_gt.copy(), sc.K, sc.shared_k, sc.row_ptr, sc.obs_frame, sc.obs_uv)
    pairs = chain(sc.M)
    Z = np.zeros((len(pairs), 3, 3))
    z = np.zeros((len(pairs), 3))
    for k, (a, b) in enumerate(pairs):
        Z[k], z[k] = rr.relative_pose(gt, a, b)
    L = np.zeros((len(pairs), 6, 6))
    L[:, np.arange(6), np.arange(6)] = 1.0
    fac = rr.Factors([p[0] for p in pairs], [p[1] for p in pairs], Z, z, L)
    R = R_gt.reshape(-1, 3, 3)
    Cn = -np.einsum("jba,jb->ja", R, T_gt)
    C2 = Cn[0] + SCALE * (Cn - Cn[0])
    sc.cam_R[:] = R_gt
    sc.cam_T[:] = -np.einsum("jab,jb->ja", R, C2)
    sc.points[:] = Cn[0] + SCALE * (pts_gt - Cn[0])
    fconst = np.zeros(sc.M, dtype=bool)
    fconst[0] = True
    return spec, sc, fac, fconst, pts_gt, R_gt, T_gt
