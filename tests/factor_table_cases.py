"""The (scene, options, factor settings) cases of the factor-table tests, shared by tests/test_factor_tables_cpu.py (the tables
of surikatoko_amd/csrc/srk_factors.cpp against the parent commit's, without a GPU) and tests/test_gpu_factor_tables.py (results
against the parent commit's).  The scenes and settings are those of the families' own case files (constant_cases.py,
prior_cases.py, relpose_cases.py, jointprior_cases.py), taken where a table builder branches: fixed intrinsics (6-wide
targets), a renumbered scene (frame_int, obs_rank), a rotated world (the normaliser), pairs given backwards, a zero block, two
sets on one frame, a pair that a factor and a set share, the two-kernel derivative path (the frame-major information), entries
with an all-zero information matrix among live ones, and settings that are stored but switch nothing on.

A case is a dict: scene, f0, fv, reorder (set_frame_reordering mode), and per family None or its setting: info (q [O]),
const (frame mask, landmark mask, keep_gauge), pri (prior_ref.Priors, keep_gauge), fac (relpose_ref.Factors), sets
(jointprior_ref.Sets, keep_gauge)."""
import numpy as np

import surikatoko_amd as sa
from surikatoko_amd.ba import _joint_pose_prior_arrays
import constant_cases as cc
import jointprior_cases as jc
import jointprior_ref as jr
import prior_cases as pc
import prior_ref as pref
import relpose_cases as rc
import relpose_ref as rr
import so3_ref as so3


def _case(sc, f0, fv=10, reorder=-1, info=None, const=None, pri=None, fac=None, sets=None):
    return dict(scene=sc, f0=f0, fv=fv, reorder=reorder, info=info, const=const, pri=pri, fac=fac, sets=sets)


def _shuffle(sc):
    """the scene with every frame but the gauge frames renumbered, as the families' reordered-frames tests shuffle it"""
    perm = np.concatenate([[0, 1], 2 + np.random.RandomState(0).permutation(sc.M - 2)])
    return sa.renumber_frames(sc, perm), perm


def _zero_info(a, which):
    a = a.copy()
    a[which] = 0.0
    return a


def _constant(name, reordered=False):
    sc, f0, fmask, pmask, keep, fv = cc.case(name)
    if not reordered:
        return _case(sc, f0, fv, const=(fmask, pmask, keep))
    sh, perm = _shuffle(sc)
    fm = np.zeros_like(fmask)
    fm[perm[np.flatnonzero(fmask)]] = True
    return _case(sh, f0, fv, reorder=1, const=(fm, pmask, keep))


def _priors(name, reordered=False, zero=None):
    sc, f0, pri, keep, fv = pc.case(name)
    if zero is not None:  # an all-zero prior among live ones, of either kind
        pri.pinfo, pri.finfo = _zero_info(pri.pinfo, zero), _zero_info(pri.finfo, zero)
    if not reordered:
        return _case(sc, f0, fv, pri=(pri, keep))
    sh, perm = _shuffle(sc)
    order = np.argsort(perm[pri.fidx])
    psh = pref.Priors(pri.pidx, pri.ppos, pri.pinfo, perm[pri.fidx][order], pri.fpos[order], pri.finfo[order])
    return _case(sh, f0, fv, reorder=1, pri=(psh, keep))


def _relpose(name, reordered=False, zero=None):
    sc, f0, fac, fv, fconst, keep = rc.case(name)
    if zero is not None:
        fac.info = _zero_info(fac.info, zero)
    if not reordered:
        return _case(sc, f0, fv, fac=fac)
    sh, perm = _shuffle(sc)
    return _case(sh, f0, fv, reorder=1, fac=rr.Factors(perm[fac.a], perm[fac.b], fac.Z, fac.z, fac.info).sorted())


def _shuffled_sets(sets, perm):
    out = []
    for s in sets.sets:
        fr = perm[s["frames"]]
        o = np.argsort(fr)
        idx = (6 * o[:, None] + np.arange(6)).ravel()
        out.append(dict(frames=fr[o], R=s["R"][o], C=s["C"][o], mean=s["mean"][idx], info=s["info"][np.ix_(idx, idx)]))
    return jr.Sets(out)


def _jprior(name, reordered=False, zero=None):
    sc, f0, sets, fv, fconst, keep, fac = jc.case(name)
    if zero is not None:
        sets.sets[zero]["info"][:] = 0.0
    if not reordered:
        return _case(sc, f0, fv, fac=fac, sets=(sets, keep))
    sh, perm = _shuffle(sc)
    return _case(sh, f0, fv, reorder=1, sets=(_shuffled_sets(sets, perm), keep))


def _information(sname):
    if sname in pc.EXTRA_SCENES:
        sc, f0 = sa.generate_scene(pc.EXTRA_SCENES[sname]), pc.EXTRA_SCENES[sname].f0
    else:
        sc, f0 = cc.scene(sname)
    return _case(sc, f0, info=cc.information(sc))


def _all_five():
    sc, f0, pri, keep, fv = pc.case(pc.MODE_CASE)
    fconst, pconst = pc.constant_combination(sc, pri)
    fac = rc.case(rc.MODE_CASE)[2]
    sets = jc.case(jc.MODE_CASE)[2]
    return _case(sc, f0, info=cc.information(sc), const=(fconst, pconst, 1), pri=(pri, 1), fac=fac, sets=(sets, 1))


def _rotated_by(R, angle, axis=(0.6, -0.48, 0.64)):
    return R @ pc.rodrigues(angle * np.asarray(axis))


def _residual_angles():
    """factors and a set whose residual rotations sit in the series branch of the logarithm (1e-5), near pi / 2, and between"""
    sc, f0 = cc.scene("nf2_short_runs")
    sc = pc.rotated(sc)
    fac = rc.factors_for(sc, [(0, 1), (1, 2), (4, 5), (5, 3)], "full")
    R, Cn = rr.poses(sc)
    for k, ang in enumerate((1e-5, np.pi / 2 - 1e-3, 0.3, 0.0)):
        fac.Z[k] = _rotated_by(rr.relative_pose(sc, int(fac.a[k]), int(fac.b[k]))[0], ang)
    s = jc.set_for(sc, [1, 2, 4, 5], mean=True)
    for i, ang in enumerate((1e-5, np.pi / 2 + 1e-3, 0.3, 0.0)):
        s["R"][i] = _rotated_by(R[s["frames"][i]], ang)
    pri = pc.priors_for(sc, cc._every(sc.N, 3), [2, 5], "full")
    return _case(sc, f0, pri=(pri, 1), fac=fac, sets=(jr.Sets([s]), 1))


def _off(family):
    """a setting of the family that is stored but switches nothing on"""
    sc, f0 = cc.scene("nf16_10_tiles")
    if family == "constant":
        return _case(sc, f0, const=(np.zeros(sc.M, bool), np.zeros(sc.N, bool), 1))
    if family == "priors":
        pri = pc.priors_for(sc, cc._every(sc.N, 7), [3, 12])
        pri.pinfo[:], pri.finfo[:] = 0.0, 0.0
        return _case(sc, f0, pri=(pri, 1))
    if family == "relpose":
        fac = rc.factors_for(sc, [(3, 4), (11, 12)])
        fac.info[:] = 0.0
        return _case(sc, f0, fac=fac)
    s = jc.set_for(sc, [3, 4, 12])
    s["info"][:] = 0.0
    return _case(sc, f0, sets=(jr.Sets([s]), 1))


BUILDERS = {
    "c_nf16_frames_and_landmarks_fixed_k": lambda: _constant("nf16_frames_and_landmarks_fixed_k"),
    "c_nf16_reordered": lambda: _constant("nf16_reordered", True),
    "p_nf2_full_information_rotated_world": lambda: _priors("nf2_full_information_rotated_world"),
    "p_nf16_reordered": lambda: _priors("nf16_reordered", True),
    "p_nf16_height_only": lambda: _priors("nf16_height_only"),
    "p_nf16_zero_prior_among_live": lambda: _priors(pc.MODE_CASE, zero=1),
    "r_nf2_gauge_frames_full_information_rotated_world": lambda: _relpose("nf2_gauge_frames_full_information_rotated_world"),
    "r_ragged_pairs_given_backwards": lambda: _relpose("ragged_pairs_given_backwards"),
    "r_ragged_21_22_42_43_fixed_k": lambda: _relpose("ragged_21_22_42_43_fixed_k"),
    "r_nf16_reordered": lambda: _relpose("nf16_reordered", True),
    "r_nf16_zero_factor_among_live": lambda: _relpose(rc.MODE_CASE, zero=1),
    "j_sixteen_frames_the_limit": lambda: _jprior("sixteen_frames_the_limit"),
    "j_sixteen_frames_fixed_k": lambda: _jprior("sixteen_frames_fixed_k"),
    "j_three_frames_one_zero_block": lambda: _jprior("three_frames_one_zero_block"),
    "j_two_sets_sharing_frame_5": lambda: _jprior("two_sets_sharing_frame_5"),
    "j_pair_with_relative_pose_factor": lambda: _jprior("pair_with_relative_pose_factor"),
    "j_reordered": lambda: _jprior("reordered", True),
    "j_mode_one_all_zero_set": lambda: _jprior(jc.MODE_CASE, zero=1),
    "i_ragged_20": lambda: _information("ragged_20"),
    "i_two_kernel_60": lambda: _information("two_kernel_60"),
    "all_five_nf16_10_tiles": _all_five,
    "off_constant": lambda: _off("constant"),
    "off_priors": lambda: _off("priors"),
    "off_relpose": lambda: _off("relpose"),
    "off_jprior": lambda: _off("jprior"),
    "nothing_set": lambda: _case(*cc.scene("nf16_10_tiles")),
    "residual_angles": _residual_angles,
}
NAMES = list(BUILDERS)
_cache = {}

# The residual functions over the whole range of rotation angles (tests/test_so3_cpu.py): every angle of so3_ref.SWEEP about
# eight axes, 15 (angle, axis) combinations a case -- one factor on each of the 15 pairs of the six frames of nf2_short_runs in
# a rotated world, every third pair given backwards, and one slot each in the sets of jointprior_cases.sets_for_slots, with a
# mean.  These cases have no entry in the parent commit's golden tables and are not in NAMES.
SO3_AXES = 8
SO3_PER_CASE = 15


def so3_combinations():
    """[(angle, axis)]: so3_ref.SWEEP x so3_ref.axes(SO3_AXES), angle-major"""
    return [(ang, ax) for ang in so3.SWEEP for ax in so3.axes(SO3_AXES)]


def _so3_sweep(part):
    combos = so3_combinations()[SO3_PER_CASE * part:SO3_PER_CASE * (part + 1)]
    sc, f0 = cc.scene(rc.SWEEP_SCENE)
    sc = pc.rotated(sc)
    n = len(combos)
    pairs = [(a, b) for a in range(sc.M) for b in range(a + 1, sc.M)][:n]
    pairs = [(b, a) if k % 3 == 2 else (a, b) for k, (a, b) in enumerate(pairs)]
    fac = rc.factors_for(sc, pairs, "diag", angle=0.0)
    for k, (ang, ax) in enumerate(combos):  # (the pairs above are already in the order factors_for sorts them into)
        fac.Z[k] = rr.relative_pose(sc, int(fac.a[k]), int(fac.b[k]))[0] @ so3.exp(ang * ax).T
    return _case(sc, f0, fac=fac, sets=(jc.sets_for_slots(sc, [ang * ax for ang, ax in combos]), 1))


SO3_NAMES = [f"so3_sweep_{part:02d}" for part in range(-(-len(so3.SWEEP) * SO3_AXES // SO3_PER_CASE))]
SO3_BUILDERS = {name: (lambda part=part: _so3_sweep(part)) for part, name in enumerate(SO3_NAMES)}


def case(name):
    """built once, not to be changed by the caller"""
    if name not in _cache:
        _cache[name] = (BUILDERS[name] if name in BUILDERS else SO3_BUILDERS[name])()
    return _cache[name]


def apply(ba, c):
    """the case's options and settings on a surikatoko_amd.BundleAdjustmentKanatani, before its upload"""
    ba.set_fixed_intrinsics(c["fv"] == 6)
    ba.set_frame_reordering(c["reorder"])
    if c["info"] is not None:
        ba.set_observation_information(c["info"])
    if c["const"] is not None:
        fm, pm, keep = c["const"]
        ba.set_constant_blocks(frames=fm, points=pm, keep_gauge=bool(keep))
    if c["pri"] is not None:
        c["pri"][0].set_on(ba, c["pri"][1])
    if c["fac"] is not None:
        c["fac"].set_on(ba)
    if c["sets"] is not None:
        c["sets"][0].set_on(ba, c["sets"][1])


# five 6 x 6 matrices for srk_info_psd: zero, positive definite, rank 3, indefinite by -1e-9 of the largest entry, and positive
# semi-definite with a negative rounding pivot of 1e-13 of the largest entry
def psd_matrices():
    A = np.random.RandomState(61).uniform(-1, 1, size=(6, 6))
    pd = A @ A.T + 0.5 * np.eye(6)
    B = np.random.RandomState(67).uniform(-1, 1, size=(6, 3))
    rank3 = B @ B.T
    Q = np.linalg.qr(np.random.RandomState(71).uniform(-1, 1, size=(6, 6)))[0]
    spec = np.array([1.0, 0.7, 0.4, 0.2, 0.1, 0.0])

    def with_last(v):
        M = (Q * np.concatenate([spec[:5], [v]])) @ Q.T
        M = 0.5 * (M + M.T)
        return M, float(np.abs(M).max())
    ind = with_last(0.0)
    ind = with_last(-1e-9 * ind[1])[0]
    rnd = with_last(0.0)
    rnd = with_last(-1e-13 * rnd[1])[0]
    return np.stack([np.zeros((6, 6)), pd, rank3, ind, rnd])


def write_case(path, name, nrm):
    """The case as the raw binary file tests/cpp/test_factor_tables.cpp reads: 20 int64 of header, the scene, the normaliser of
    its upload (R0, T0, s), then per family the arrays as the setters of the C ABI store them."""
    c = case(name)
    sc = c["scene"]
    K = np.ascontiguousarray(np.broadcast_to(np.asarray(sc.K, np.float64).reshape(-1, 9), (sc.M, 9)))
    q = np.zeros(0) if c["info"] is None else np.asarray(c["info"], np.float64)
    fm, pm, ckeep = (np.zeros(0, np.uint8), np.zeros(0, np.uint8), 1) if c["const"] is None else c["const"]
    pri, pkeep = (pref.Priors(), 1) if c["pri"] is None else c["pri"]
    fac = rr.Factors() if c["fac"] is None else c["fac"]
    sets, jkeep = (jr.Sets(), 1) if c["sets"] is None else c["sets"]
    if sets.n:
        jptr, jfr, jR, jC, jm, jL = _joint_pose_prior_arrays(sets.sets)
        at = 0
        for g in range(sets.n):  # stored symmetrised
            n = 6 * int(jptr[g + 1] - jptr[g])
            L = jL[at:at + n * n].reshape(n, n)
            L[:] = np.triu(0.5 * (L + L.T)) + np.triu(0.5 * (L + L.T), 1).T
            at += n * n
    else:
        jptr, jfr, jR, jC, jm, jL = np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0)
    head = np.array([sc.N, sc.M, sc.O, 1 if c["fv"] == 6 else 0, c["reorder"], q.size, 0 if c["const"] is None else 1, ckeep,
                     np.asarray(fm).size, np.asarray(pm).size, 0 if c["pri"] is None else 1, pkeep, pri.pidx.size, pri.fidx.size,
                     fac.n, sets.n, jkeep, jfr.size, jL.size, 0], np.int64)
    nrm_a = np.concatenate([np.array(list(nrm.R0)), np.array(list(nrm.T0)), [float(nrm.world_scale)]])
    with open(path, "wb") as f:
        for a, t in ((head, np.int64), (sc.row_ptr, np.int64), (sc.obs_frame, np.int32), (sc.obs_uv, np.float64),
                     (sc.points, np.float64), (sc.cam_R, np.float64), (sc.cam_T, np.float64), (K, np.float64), (nrm_a, np.float64),
                     (q, np.float64), (fm, np.uint8), (pm, np.uint8),
                     (pri.pidx, np.int64), (pri.ppos, np.float64), (pref.six(pri.pinfo), np.float64),
                     (pri.fidx, np.int32), (pri.fpos, np.float64), (pref.six(pri.finfo), np.float64),
                     (fac.a, np.int32), (fac.b, np.int32), (fac.Z, np.float64), (fac.z, np.float64), (rr.tri21(fac.info), np.float64),
                     (jptr, np.int32), (jfr, np.int32), (jR, np.float64), (jC, np.float64), (jm, np.float64), (jL, np.float64)):
            f.write(np.ascontiguousarray(a, dtype=t).tobytes())
