"""The (scene, sets) cases of the joint-pose-prior tests, shared by tests/test_gpu_jointprior.py (which runs them against the
yardstick of tests/jointprior_ref.py) and tests/test_jointprior_cpu.py (which checks that every one of them gives a
well-conditioned positive definite system).  The scenes are those of tests/relpose_cases.py (24 frames) and w8_m70.

The sets sit where the passes can go wrong: one frame (no coupling at all), two, sixteen (the limit: a 96 x 96 matrix, 120
coupled pairs, rows reaching back 15 frames), a zero off-diagonal block (a pair that must not enter the plan), two sets on one
frame (the ordered list walk), the gauge frames (their fixed variables' rows and columns must stay identity) with the gauge
kept and released, a mean, a pair that carries a relative-pose factor too, a constant frame.

Information: as in tests/relpose_cases.py, E is in (pix / f0)^2 with f0 = 600 and the scenes' extent is about one world unit,
so L of order 100 (translation rows and columns scaled by 1 / extent) puts 2 J^T L J at a tenth of the blocks it is added to.
The linearisation poses are the scene's own moved by a seeded offset of up to 5e-3 (of the extent, and radians), so that every
gradient term is non-zero; the residual rotations of CASES stay far below 1 rad.  sweep_case, pi_case and residual_sweep put
them at every angle of so3_ref.SWEEP and at pi."""
import numpy as np

import constant_cases as cc
import covariance_cases as vc
import prior_cases as pc
import relpose_cases as rc
import relpose_ref as rr
import jointprior_ref as jr
import so3_ref as so3

OFFSET = 5e-3


def extent(sc):
    return float(np.abs(sc.points - sc.points.mean(axis=0)).max())


def dense_info(k, ext, seed=17, scale=100.0):
    """positive definite 6k x 6k with every entry non-zero, the translation rows and columns scaled by 1 / extent"""
    n = 6 * k
    A = np.random.RandomState(seed).uniform(-1, 1, size=(n, n))
    L = scale * (A @ A.T / n + 0.5 * np.eye(n))
    d = np.tile([1 / ext] * 3 + [1.0] * 3, k)
    return L * d[:, None] * d[None, :]


def chain_info(k, ext, seed=19):
    """positive definite, block tridiagonal: dense blocks on consecutive slots, zero blocks elsewhere"""
    L = np.zeros((6 * k, 6 * k))
    for i in range(k - 1):
        L[6 * i:6 * i + 12, 6 * i:6 * i + 12] += dense_info(2, 1.0, seed + i)
    d = np.tile([1 / ext] * 3 + [1.0] * 3, k)
    return L * d[:, None] * d[None, :]


def set_for(sc, frames, info=None, mean=False, seed=31, offset=OFFSET, angle=None, axes=None):
    """a set over the given frames, linearised at the scene's poses moved by a seeded offset; in the scene's coordinates.
    With angle the rotations are not moved by that offset: Rbar = R Exp(phi) with |phi| = angle about a seeded axis per slot
    (or axes[i]), so the rotation residual Log(R^T Rbar) is phi up to the rounding of the product, in any world coordinates;
    the centres and the mean are as without angle."""
    rs = np.random.RandomState(seed)
    ext = extent(sc)
    fr = np.asarray(sorted(frames), dtype=np.int32)
    k = fr.size
    R, Cn = rr.poses(sc)
    Rb = np.stack([R[j] @ pc.rodrigues(rs.uniform(-offset, offset, size=3)) for j in fr])
    Cb = Cn[fr] + ext * rs.uniform(-offset, offset, size=(k, 3))
    if angle is not None:
        ax = so3.axes(k + 1, seed)[1:] if axes is None else np.asarray(axes, dtype=np.float64).reshape(k, 3)
        Rb = np.stack([R[j] @ so3.exp(angle * ax[i]) for i, j in enumerate(fr)])
    m = None
    if mean:
        m = rs.uniform(-offset, offset, size=6 * k) * np.tile([ext] * 3 + [1.0] * 3, k)
    return dict(frames=fr, R=Rb, C=Cb, mean=m, info=dense_info(k, ext) if info is None else info)


def _three_zero_block(sc):
    return [set_for(sc, [8, 10, 12], chain_info(3, extent(sc)))]


# name -> (scene, sets(sc), frame variables, constant frames or None, keep_gauge, relative-pose pairs or None)
CASES = {
    "one_frame_full_pose_prior": ("nf16_10_tiles", lambda sc: [set_for(sc, [7])], 10, None, 1, None),
    "two_frames": ("nf16_10_tiles", lambda sc: [set_for(sc, [5, 6])], 10, None, 1, None),
    "sixteen_frames_the_limit": ("nf16_10_tiles", lambda sc: [set_for(sc, range(4, 20))], 10, None, 1, None),
    "sixteen_frames_fixed_k": ("nf16_10_tiles", lambda sc: [set_for(sc, range(4, 20))], 6, None, 1, None),
    "three_frames_one_zero_block": ("nf16_10_tiles", _three_zero_block, 10, None, 1, None),
    "two_sets_sharing_frame_5": ("nf16_10_tiles", lambda sc: [set_for(sc, [3, 4, 5]), set_for(sc, [5, 9, 10], seed=37)], 10, None, 1, None),
    "gauge_frames_gauge_kept": ("nf16_10_tiles", lambda sc: [set_for(sc, [0, 1, 2])], 10, None, 1, None),
    "gauge_frames_gauge_released": ("nf16_10_tiles", lambda sc: [set_for(sc, [0, 1, 2])], 6, None, 0, None),
    "non_zero_mean": ("nf16_10_tiles", lambda sc: [set_for(sc, [6, 11], mean=True)], 10, None, 1, None),
    "pair_with_relative_pose_factor": ("nf16_10_tiles", lambda sc: [set_for(sc, [11, 12])], 10, None, 1, [(3, 4), (11, 12)]),
    "constant_frame_in_the_set": ("nf16_10_tiles", lambda sc: [set_for(sc, [3, 12, 13])], 10, [12], 1, None),
}
# the case the mode tests run
MODE_CASE = "mode"
CASES[MODE_CASE] = ("nf16_10_tiles", lambda sc: [set_for(sc, [3, 4, 12]), set_for(sc, [12, 20, 23], seed=41), set_for(sc, [8], seed=43)], 10, None, 1, None)
CASES[MODE_CASE + "_fixed_k"] = CASES[MODE_CASE][:2] + (6,) + CASES[MODE_CASE][3:]
# the reordered-frames case: sets of the unshuffled scene (the test maps the frames through the shuffle)
REORDER_CASE = "reordered"
CASES[REORDER_CASE] = ("nf16_10_tiles", lambda sc: [set_for(sc, [0, 1, 9]), set_for(sc, [9, 17, 23], seed=47), set_for(sc, [5, 6], seed=53)], 10, None, 1, None)


def case(name):
    """(scene copy, f0, Sets in the scene's coordinates, fv, constant-frame mask, keep_gauge, relative-pose Factors or None)"""
    if name in SWEEP_CASES:
        return pi_case() if name == PI_CASE else sweep_case(SWEEP_CASES[name])
    sname, sf, fv, fc, keep_gauge, pairs = CASES[name]
    sc, f0 = cc.scene(sname)
    fconst = np.zeros(sc.M, dtype=bool)
    if fc is not None:
        fconst[fc] = True
    fac = None if pairs is None else rc.factors_for(sc, pairs)
    return sc, f0, jr.Sets(sf(sc)), fv, fconst, keep_gauge, fac


# ------------------------------------------------------------------ the whole range of residual angles (so3_ref.SWEEP)
# One set of three frames on the smallest scene: dense 18 x 18 information, a non-zero mean, every slot at the same angle.
SWEEP = so3.SWEEP
SWEEP_SCENE = rc.SWEEP_SCENE
SWEEP_FRAMES = [1, 2, 4]


def sweep_case(angle, fv=10):
    """(scene copy, f0, Sets, fv, constant-frame mask, keep_gauge, None)"""
    sc, f0 = cc.scene(SWEEP_SCENE)
    return sc, f0, jr.Sets([set_for(sc, SWEEP_FRAMES, mean=True, angle=angle)]), fv, np.zeros(sc.M, dtype=bool), 1, None


def pi_info(k, ext):
    """dense_info over the translation variables of the k slots, 100 I on every slot's rotation variables and zeros between
    the two kinds and between the rotations of different slots: positive definite, and (r - m)^T L (r - m) does not change
    when a rotation residual changes its sign (with a zero mean on the rotation rows)"""
    L = dense_info(k, ext)
    rot = (np.arange(6 * k) % 6) >= 3
    L[rot, :] = 0.0
    L[:, rot] = 0.0
    L[rot, rot] = 100.0
    return L


def pi_case(fv=10):
    """one set of three frames whose linearisation rotations are half a turn away from the scene's: slot 0 about a coordinate
    axis, Rbar = R diag(1, -1, -1) exactly, slot 1 about a seeded axis, slot 2 at 0.05 rad.  Log may return either sign at the
    first two (see relpose_cases.pi_case): the information matrix is pi_info and the mean zero."""
    sc, f0 = cc.scene(SWEEP_SCENE)
    s = set_for(sc, SWEEP_FRAMES, pi_info(3, extent(sc)), angle=np.pi)
    R, _ = rr.poses(sc)
    s["R"][0] = R[SWEEP_FRAMES[0]] @ np.diag([1.0, -1.0, -1.0])
    s["R"][2] = R[SWEEP_FRAMES[2]] @ so3.exp(0.05 * so3.axes(2, 3)[1])
    return sc, f0, jr.Sets([s]), fv, np.zeros(sc.M, dtype=bool), 1, None


PI_CASE = rc.PI_CASE
# name -> angle: what tests/test_jointprior_cpu.py checks for conditioning beside CASES
SWEEP_CASES = {**{f"sweep_{a:.12g}": a for a in SWEEP}, PI_CASE: np.pi}

# frame lists of which no two share more than one frame (the setter's rule), 24 slots on six frames
SLOT_SETS = [[0, 1, 2], [0, 3, 4], [1, 3, 5], [2, 4, 5], [0, 5], [1, 4], [2, 3], [0], [1], [2], [3], [4], [5]]


def sets_for_slots(sc, rotvecs, seed=31):
    """sets over SLOT_SETS, as many as len(rotvecs) slots need (the last one cut short), each with a mean; slot q has the
    rotation residual rotvecs[q]: Rbar = R Exp(rotvecs[q])"""
    R, _ = rr.poses(sc)
    sets, at = [], 0
    for frames in SLOT_SETS:
        fr = frames[:len(rotvecs) - at]
        if not fr:
            break
        s = set_for(sc, fr, mean=True, seed=seed + at, angle=0.0)
        s["R"] = np.stack([R[j] @ so3.exp(rotvecs[at + i]) for i, j in enumerate(fr)])
        sets.append(s)
        at += len(fr)
    assert at == len(rotvecs)
    return jr.Sets(sets)


def residual_sweep():
    """sets for the residual getter: slot q at the angle SWEEP[q] about a seeded axis"""
    sc, f0 = cc.scene(SWEEP_SCENE)
    ax = so3.axes(len(SWEEP) + 1, 61)[1:]
    return sc, f0, sets_for_slots(sc, [a * x for a, x in zip(SWEEP, ax)]), np.asarray(SWEEP)


def w8_m70():
    return vc.scene("w8_m70")


CHUNKED = rc.CHUNKED
