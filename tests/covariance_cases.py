"""The cases of the covariance tests, shared by tests/test_gpu_covariance.py (which runs them against the reference of
tests/covariance_ref.py) and tests/test_covariance_cpu.py (which checks that every one of them is positive definite and that
the reference's own rounding noise is far below the bound the GPU comparison uses).

Scenes are those of tests/constant_cases.py plus w8_m70: 70 frames with tracks of 8, so that the band of the reduced camera
system is narrower than a 64-row tile -- with six variables n = 420 (seven tile rows, two outer steps of the factorisation),
with ten n = 700 (three outer steps).

The selections sit where the three kernels can go wrong: every frame (a column count that is no multiple of the block
width); the gauge frames 0 and 1 (frame 0 all zeros, frame 1 one zero row and column); frames whose variables straddle a
tile and a panel boundary (10, 21 and 42 with six variables: 60..65, 126..131, 252..257; 6, 12 and 25 with ten: 60..69,
120..129, 250..259); the last frame; the first, the last and the longest-track landmark; a landmark seen from frames in
different tiles; a batch cap of 96 columns (three or more batches); constant frames and landmarks; a landmark with an
observation switched off by q = 0; position priors and relative-pose factors (prior_cases / relpose_cases); a frame-shuffled
scene that the library renumbers internally."""
import numpy as np

import surikatoko_amd as sa
import constant_cases as cc
import covariance_ref as vref
import prior_cases as pc
import prior_ref as pref
import relpose_cases as rc
import relpose_ref as rref
import weighted_ref as wr

W8_M70 = sa.SceneSpec(n_frames=70, grid_nx=24, grid_ny=16, vis_window=8, noise_uv_pix=0.3)

_scenes = {}


def scene(name):
    if name == "w8_m70":
        if name not in _scenes:
            _scenes[name] = sa.generate_scene(W8_M70)
        return _scenes[name].copy(), W8_M70.f0
    return cc.scene(name)


def _straddling_landmark(sc, fv):
    """a landmark whose observing frames' variables lie in different 64-row tiles of the reduced camera system"""
    rp, fr = np.asarray(sc.row_ptr), np.asarray(sc.obs_frame)
    for i in range(sc.N):
        f = fr[rp[i]:rp[i + 1]]
        if f.size and (fv * int(f.min())) // 64 != (fv * int(f.max()) + fv - 1) // 64:
            return i
    raise AssertionError("no landmark straddles a tile")


def _edge_frames(sc, fv):
    return [0, 1] + [f for f in ((10, 21, 42) if fv == 6 else (6, 12, 25)) if f < sc.M] + [sc.M - 1]


def _landmarks(sc, fv):
    return [0, sc.N - 1, cc._longest_track(sc), _straddling_landmark(sc, fv)]


def _all_frames(sc, fv):
    return list(range(sc.M))


# name -> dict(scene, fv, frames(sc, fv), points(sc, fv), and optionally: const = a constant_cases case, prior / relpose = a case
# of prior_cases / relpose_cases, q0 = True, shuffle = True, batch = columns)
CASES = {
    "nf2_all_fv6": dict(scene="nf2_short_runs", fv=6, frames=_all_frames, points=lambda sc, fv: list(range(sc.N))),
    "nf2_all_fv10": dict(scene="nf2_short_runs", fv=10, frames=_all_frames, points=lambda sc, fv: list(range(sc.N))),
    "nf16_edges_fv6": dict(scene="nf16_10_tiles", fv=6, frames=_edge_frames, points=_landmarks),
    "nf16_edges_fv10": dict(scene="nf16_10_tiles", fv=10, frames=_edge_frames, points=_landmarks),
    "ragged_every_frame_fv6": dict(scene="ragged_20", fv=6, frames=_all_frames, points=_landmarks),
    "ragged_every_frame_three_batches_fv6": dict(scene="ragged_20", fv=6, frames=_all_frames, points=_landmarks, batch=96),
    "ragged_edges_repeats_any_order_fv10": dict(scene="ragged_20", fv=10, frames=lambda sc, fv: _edge_frames(sc, fv)[::-1] + [12, 12],
                                                points=lambda sc, fv: _landmarks(sc, fv)[::-1] + [0]),
    "w8_every_frame_fv6": dict(scene="w8_m70", fv=6, frames=_all_frames, points=_landmarks),
    "w8_edges_fv10": dict(scene="w8_m70", fv=10, frames=lambda sc, fv: _edge_frames(sc, fv) + [40], points=_landmarks),
    "long_nf30_fv6": dict(scene="long_nf30", fv=6, frames=_edge_frames, points=_landmarks),
    "nf16_constant_frames_and_landmarks_fv6": dict(scene="nf16_10_tiles", fv=6, const="nf16_frames_and_landmarks_fixed_k",
                                                   frames=_all_frames, points=lambda sc, fv: [0, 1, 7, 14, sc.N - 1]),
    "ragged_constant_free_gauge_fv10": dict(scene="ragged_20", fv=10, const="ragged_frames_12_25_free_gauge",
                                            frames=lambda sc, fv: [0, 1, 12, 13, 25, 59], points=lambda sc, fv: [0, 5, 7, sc.N - 1]),
    "nf16_q0_fv6": dict(scene="nf16_10_tiles", fv=6, q0=True, frames=_edge_frames, points=None),
    "nf16_priors_fv6": dict(scene="nf16_10_tiles", fv=6, prior=pc.MODE_CASE + "_fixed_k", frames=lambda sc, fv: [0, 1, 3, 12, 23],
                            points=lambda sc, fv: [0, 1, 7, sc.N - 1]),
    "nf16_factors_fv6": dict(scene="nf16_10_tiles", fv=6, relpose=rc.MODE_CASE + "_fixed_k", frames=lambda sc, fv: [0, 3, 4, 12, 20, 23],
                             points=_landmarks),
    "nf16_shuffled_fv6": dict(scene="nf16_10_tiles", fv=6, shuffle=True, frames=_all_frames, points=_landmarks),
}
DENSE_CASES = ("nf2_all_fv6", "nf2_all_fv10")  # small enough for the full-Hessian route


class Case:
    pass


def case(name):
    """the case as an object: sc (the scene handed to the library), f0, fv, fconst, pconst, keep_gauge, pri, fac (in sc's
    coordinates, or None), q (or None), frames, points (selections, caller's numbering), batch, shuffle"""
    spec = CASES[name]
    k = Case()
    k.name, k.fv = name, spec["fv"]
    k.sc, k.f0 = scene(spec["scene"])
    k.fconst, k.pconst, k.keep_gauge = np.zeros(k.sc.M, dtype=bool), np.zeros(k.sc.N, dtype=bool), 1
    k.pri = k.fac = k.q = None
    if "const" in spec:
        sc, f0, k.fconst, k.pconst, k.keep_gauge, fv = cc.case(spec["const"])
        assert fv == k.fv and sc.M == k.sc.M
    if "prior" in spec:
        sc, f0, k.pri, k.keep_gauge, fv = pc.case(spec["prior"])
        assert fv == k.fv and sc.M == k.sc.M
    if "relpose" in spec:
        sc, f0, k.fac, fv, k.fconst, k.keep_gauge = rc.case(spec["relpose"])
        assert fv == k.fv and sc.M == k.sc.M
    if spec.get("q0"):
        k.q = wr.make_information(k.sc, 5, zero_frac=0.05)
        assert np.any(k.q == 0)
    k.shuffle = bool(spec.get("shuffle"))
    if k.shuffle:  # the gauge frames stay 0 and 1
        perm = np.concatenate([[0, 1], 2 + np.random.RandomState(0).permutation(k.sc.M - 2)])
        k.sc = sa.renumber_frames(k.sc, perm)
    k.frames = np.asarray(spec["frames"](k.sc, k.fv), dtype=np.int32)
    if spec["points"] is None:  # q = 0: a landmark with a switched-off observation, and its neighbours
        off = np.flatnonzero(k.q == 0)
        i = int(np.searchsorted(np.asarray(k.sc.row_ptr), off[0], side="right") - 1)
        k.points = np.asarray([i, max(i - 1, 0), min(i + 1, k.sc.N - 1)], dtype=np.int64)
    else:
        k.points = np.asarray(spec["points"](k.sc, k.fv), dtype=np.int64)
    k.batch = int(spec.get("batch", 0))
    return k


def configure(gpu, k):
    """the case's settings on a handle (before the upload)"""
    if k.fconst.any() or k.pconst.any() or not k.keep_gauge:
        gpu.set_constant_blocks(k.fconst if k.fconst.any() else None, k.pconst if k.pconst.any() else None, bool(k.keep_gauge))
    if k.pri is not None:
        k.pri.set_on(gpu, k.keep_gauge)
    if k.fac is not None:
        k.fac.set_on(gpu)
    if k.q is not None:
        gpu.set_observation_information(k.q)
    if k.shuffle:
        gpu.set_frame_reordering(1)
    gpu.set_covariance_batch(k.batch)


_refs = {}


def reference(orc, name, c, reverse=False, dense=False):
    """dict(FB [M][fv][fv], PB [N][3][3], cond, nrm, so) of the case at damping c in the normalised scene, computed once"""
    key = (name, float(c), bool(reverse), bool(dense))
    if key in _refs:
        return _refs[key]
    k = case(name)
    so = orc.Scene(k.sc.points, k.sc.cam_R, k.sc.cam_T, k.sc.K, k.sc.shared_k, k.sc.row_ptr, k.sc.obs_frame, k.sc.obs_uv)
    ok, nrm = orc.normalize(so)
    assert ok
    pri = None if k.pri is None else pref.normalised(k.pri, nrm)
    fac = None if k.fac is None else rref.normalised(k.fac, nrm)
    der = None if k.q is None else (lambda s: wr.derivatives(k.f0, s, k.q))
    restricted = vref.blocks_of(orc, k.f0, so, k.fv, k.fconst, k.pconst, pri, fac, der)
    if dense:
        FB, PB = vref.dense_blocks(so, restricted, c, k.fv, k.fconst, k.pconst, k.keep_gauge, fac)
        out = dict(FB=FB, PB=PB, cond=None, nrm=nrm, so=so)
    else:
        FB, PB, cond = vref.covariance_blocks(so, restricted, c, k.fv, k.fconst, k.pconst, k.keep_gauge, fac, reverse)
        out = dict(FB=FB, PB=PB, cond=cond, nrm=nrm, so=so)
    _refs[key] = out
    return out


def bound(cond):
    """64 eps cond_scaled(S_free): a backward-stable factorisation is off by a few eps cond of the diagonally scaled system"""
    return 64.0 * vref.EPS * cond


def dampings(name):
    """what is compared: six variables at c = 1e-4 and c = 0, ten variables at c = 1e-4 only (at c = 0 their scaled condition
    number is 1e14 and beyond).  nf2_short_runs has tracks of two frames: the scale between consecutive pairs of frames is
    free, the undamped system singular, so it is compared at c = 1e-4 only."""
    return (1e-4, 0.0) if CASES[name]["fv"] == 6 and CASES[name]["scene"] != "nf2_short_runs" else (1e-4,)
