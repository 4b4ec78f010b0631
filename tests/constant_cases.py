"""The (scene, constant set, keep_gauge) cases of the constant-block tests, shared by tests/test_gpu_constant.py (which runs
them against the yardstick of tests/constant_ref.py) and tests/test_constant_cpu.py (which checks that every one of them
gives a well-conditioned positive definite system, so that no GPU comparison hides behind a degenerate input).

The sets sit where the masking passes can go wrong: the gauge frames with both gauge settings, the last frames, frames whose
variables straddle the 128-row tile and the 256-column panel boundaries of the reduced camera system (frames 12 and 25 with
ten variables a frame: 120..129 and 250..259; frames 21 and 42 with six: 126..131 and 252..257), landmarks spread over the
runs, the first and the last landmark, a landmark with a track too long for the run-based Schur kernels."""
import numpy as np

import surikatoko_amd as sa

SCENES = {
    "nf2_short_runs": (sa.SceneSpec(n_frames=6, grid_nx=9, grid_ny=7, vis_window=2), 0.0),
    "nf16_10_tiles": (sa.SceneSpec(n_frames=24, grid_nx=30, grid_ny=20, vis_window=16), 0.0),
    "ragged_20": (sa.SceneSpec(n_frames=60, grid_nx=40, grid_ny=30, vis_window=20, noise_uv_pix=0.3), 0.15),
    "long_nf30": (sa.SceneSpec(n_frames=48, grid_nx=12, grid_ny=10, vis_window=30), 0.0),
}

_cache = {}


def scene(name):
    """(scene, f0) of SCENES[name]; generated once, callers get a copy"""
    if name not in _cache:
        spec, frac = SCENES[name]
        sc = sa.generate_scene(spec)
        if frac > 0:
            sc = sa.drop_observations(sc, frac, seed=7)
        _cache[name] = (sc, spec.f0)
    sc, f0 = _cache[name]
    return sc.copy(), f0


def _every(n, k):
    return np.arange(0, n, k)


def _longest_track(sc):
    return int(np.argmax(np.diff(sc.row_ptr)))


# name -> (scene, frames(sc) or None, points(sc) or None, keep_gauge, frame variables)
CASES = {
    "nf2_gauge_frames_keep": ("nf2_short_runs", lambda sc: [0, 1], None, 1, 10),
    "nf2_gauge_frames_free_gauge": ("nf2_short_runs", lambda sc: [0, 1], None, 0, 10),
    "nf16_gauge_frames_keep": ("nf16_10_tiles", lambda sc: [0, 1], None, 1, 10),
    "nf16_gauge_frames_free_gauge": ("nf16_10_tiles", lambda sc: [0, 1], None, 0, 10),
    "nf16_last_two_frames": ("nf16_10_tiles", lambda sc: [sc.M - 2, sc.M - 1], None, 1, 10),
    "nf16_every_7th_landmark": ("nf16_10_tiles", None, lambda sc: _every(sc.N, 7), 1, 10),
    "nf16_first_and_last_landmark": ("nf16_10_tiles", None, lambda sc: [0, sc.N - 1], 1, 10),
    "nf16_frames_and_landmarks_fixed_k": ("nf16_10_tiles", lambda sc: [3, 12], lambda sc: _every(sc.N, 7), 1, 6),
    "ragged_frames_12_25_tile_and_panel_edges": ("ragged_20", lambda sc: [5, 12, 25, 41], None, 1, 10),
    "ragged_frames_12_25_free_gauge": ("ragged_20", lambda sc: [12, 25], lambda sc: _every(sc.N, 7), 0, 10),
    "ragged_frames_21_42_fixed_k": ("ragged_20", lambda sc: [8, 21, 42, 59], None, 1, 6),
    "long_fallback_landmark": ("long_nf30", None, lambda sc: [0, _longest_track(sc), sc.N - 1], 1, 10),
    "long_fallback_landmark_fixed_k": ("long_nf30", lambda sc: [sc.M - 2, sc.M - 1],
                                       lambda sc: [0, _longest_track(sc), sc.N - 1], 1, 6),
    "nf16_all_frames_structure_only": ("nf16_10_tiles", lambda sc: np.arange(sc.M), None, 1, 10),
    "nf16_all_landmarks_motion_only": ("nf16_10_tiles", None, lambda sc: np.arange(sc.N), 0, 10),
}

# the case the mode tests run (deterministic, f32 storage, loss + information, rcs modes, fusion, speculation)
MODE_CASE = "nf16_frames_and_landmarks"
CASES[MODE_CASE] = ("nf16_10_tiles", lambda sc: [3, 12], lambda sc: _every(sc.N, 7), 1, 10)
# the reordered-frames cases: frames and landmarks of the unshuffled scene (the test maps the frames through the shuffle)
REORDER_CASES = ("nf16_reordered", "nf16_reordered_free_gauge")
CASES[REORDER_CASES[0]] = ("nf16_10_tiles", lambda sc: [0, 1, 9, 17], lambda sc: _every(sc.N, 7), 1, 10)
CASES[REORDER_CASES[1]] = ("nf16_10_tiles", lambda sc: [0, 1, 9, 17], lambda sc: _every(sc.N, 7), 0, 10)
# end to end
CASES["c1_to_convergence"] = ("C1", lambda sc: [0, 1, 17, 30], lambda sc: _every(sc.N, 7), 1, 10)
CASES["nf16_ten_iterations"] = ("nf16_10_tiles", lambda sc: [3, 12], lambda sc: _every(sc.N, 7), 0, 10)


def case(name):
    """(scene copy, f0, frame mask, landmark mask, keep_gauge, fv)"""
    sname, ff, pf, keep_gauge, fv = CASES[name]
    if sname == "C1":
        if "C1" not in _cache:
            _cache["C1"] = (sa.config_scene("C1_dino_standin"), 600.0)
        sc, f0 = _cache["C1"][0].copy(), 600.0
    else:
        sc, f0 = scene(sname)
    fmask = np.zeros(sc.M, dtype=bool)
    pmask = np.zeros(sc.N, dtype=bool)
    if ff is not None:
        fmask[np.asarray(ff(sc), dtype=np.int64)] = True
    if pf is not None:
        pmask[np.asarray(pf(sc), dtype=np.int64)] = True
    return sc, f0, fmask, pmask, keep_gauge, fv


def sliding_window(k22_f0=False):
    """a noise-free scene (exact projections of the ground truth), the first 8 of 24 frames at their ground truth, the other
    frames and all points perturbed by 1e-3 (the scene generator's recipe for points and rotations, a seeded shift of the
    translations on top).  k22_f0: K scaled to K(2,2) = f0, the same projections in the convention the closed-form frame
    derivatives assume."""
    spec = sa.SceneSpec(n_frames=24, grid_nx=12, grid_ny=10, vis_window=16, noise_x3d_hi=1e-3, noise_r_hi=1e-3)
    sc, pts_gt, R_gt, T_gt = sa.generate_scene(spec, with_gt=True)
    R_gt, T_gt = R_gt.reshape(-1, 9), T_gt.reshape(-1, 3)
    sc.cam_R[:8], sc.cam_T[:8] = R_gt[:8], T_gt[:8]
    if k22_f0:
        sc.K[:] = sc.K * (spec.f0 / sc.K[:, 8:9])
        sc.cam_T[8:] += np.random.RandomState(3).uniform(-1e-3, 1e-3, size=(sc.M - 8, 3))
        assert np.abs(sc.cam_T[8:] - T_gt[8:]).max() > 5e-4
    assert np.abs(sc.cam_R[8:] - R_gt[8:]).max() > 1e-4 and np.abs(sc.points - pts_gt).max() > 1e-4
    fconst = np.zeros(sc.M, dtype=bool)
    fconst[:8] = True
    return spec, sc, pts_gt, R_gt, T_gt, fconst


def information(sc, seed=5):
    """seeded per-observation information with some q = 0 (as weighted_ref.make_information)"""
    import weighted_ref as wr
    return wr.make_information(sc, seed)
