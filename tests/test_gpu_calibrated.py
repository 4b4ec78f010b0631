"""Calibrated bundle adjustment on the GPU (srk_ba_set_fixed_intrinsics: six pose variables per frame, the intrinsics
constants) against the yardstick of tests/calibrated_ref.py -- the oracle's 10-variable damped system restricted to the pose
and point variables, and the LM loop of bundle-adj-kanatani.cpp:720-893 around it.

Tolerances as the 10-variable parity tests: blocks rel 1e-12 per variable class, reduced camera system 1e-10
class-scaled, corrections 1e-8; gauge corrections exactly 0, K never changed.
"""
import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import ba as B
from surikatoko_amd import _lib
from conftest import load_golden, rel_err, sym_scaled_err, class_rel_err
import calibrated_ref as cref
import lm_trajectory as lt
from gpu_common import orc_scene as _orc_scene, run_lm as _run, compare_runs as _compare_runs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cal():
    h = sa.BundleAdjustmentKanatani(0)
    h.set_fixed_intrinsics(True)
    yield h
    h.close()


def _gauge_zero(corr_frames, M):
    fr = corr_frames.reshape(M, 6)
    return np.all(fr[0] == 0) and fr[1, 1] == 0


def _phases(orc, gpu, sc, f0, c):
    """derivatives -> schur -> solve -> backsub on both sides, checked"""
    so = _orc_scene(orc, sc)
    assert orc.normalize(so)[0]
    K0 = sc.K.copy()
    assert gpu.upload(f0, sc) and gpu.frame_vars() == 6
    N, M = sc.N, sc.M
    eo, _ = orc.reproj_error(f0, so)
    ref = cref.step(orc, f0, so, c, want_system=True)
    gpu.phase_derivatives()
    for which, n in ((B.BUF_GRAD, 3 * N + 6 * M), (B.BUF_FRAME_BLOCKS, 36 * M), (B.BUF_POINT_FRAME, 18 * sc.O),
                     (B.BUF_CORRECTIONS, 3 * N + 6 * M)):
        assert gpu._lib.srk_ba_buffer_size(gpu._h, which) == n
    Vg = gpu.buffer(B.BUF_POINT_BLOCKS).reshape(-1, 3, 3)
    Ug = gpu.buffer(B.BUF_FRAME_BLOCKS).reshape(M, 6, 6)
    Wg = gpu.buffer(B.BUF_POINT_FRAME).reshape(-1, 3, 6)
    gg = gpu.buffer(B.BUF_GRAD)
    dV = np.sqrt(np.abs(np.einsum("nii->ni", ref["V"])))
    dU = np.sqrt(np.abs(np.einsum("mii->mi", ref["U"])))
    assert sym_scaled_err(Vg, ref["V"], dV) < 1e-12
    assert sym_scaled_err(Ug, ref["U"], dU) < 1e-12
    assert class_rel_err(Wg, ref["W"], (1, 2)) < 1e-12
    gs = 2.0 * np.sqrt(max(eo, 1e-300))
    dg = np.concatenate([dV.reshape(-1), dU.reshape(-1)]) * gs
    okg = dg > 0
    assert float((np.abs(gg - ref["grad"])[okg] / dg[okg]).max()) < 1e-10
    gpu.phase_schur(c)
    Sg = gpu.buffer(B.BUF_RCS).reshape(6 * M, 6 * M)
    rg = gpu.buffer(B.BUF_RCS_RHS)
    keep = cref.compact_to_reduced(M) >= 0
    dk = dU.reshape(-1)[keep]
    assert sym_scaled_err(Sg[np.ix_(keep, keep)], ref["S"][np.ix_(keep, keep)], dk) < 1e-10
    assert float((np.abs(rg[keep] - ref["rhs"][keep]) / (dk * gs)).max()) < 1e-10
    for f in np.where(~keep)[0]:  # gauge rows: identity, zero rhs
        row = Sg[f].copy()
        assert row[f] == 1.0
        row[f] = 0
        assert np.all(row == 0) and rg[f] == 0
    assert gpu.phase_solve() and ref["ok"]
    gpu.phase_backsub(c)
    corr = gpu.buffer(B.BUF_CORRECTIONS)
    assert _gauge_zero(corr[3 * N:], M)
    assert rel_err(corr, ref["corr"]) < 1e-8
    orc.apply_corrections(so, ref["corr10"])
    gpu.phase_accept()
    scale = max(1.0, float(np.abs(so.points).max()))
    assert np.abs(gpu.buffer(B.BUF_POINTS).reshape(-1, 3) - so.points).max() < 1e-8 * scale
    assert np.abs(gpu.buffer(B.BUF_CAM_R).reshape(-1, 9) - so.cam_R).max() < 1e-8
    assert np.abs(gpu.buffer(B.BUF_CAM_T).reshape(-1, 3) - so.cam_T).max() < 1e-8 * scale
    e2o, _ = orc.reproj_error(f0, so)
    e2g, _ = gpu.phase_error()
    assert e2g == pytest.approx(e2o, rel=1e-6)
    assert np.array_equal(sc.K, K0)


SCENES = {
    "nf16_10_tiles": (sa.SceneSpec(n_frames=24, grid_nx=30, grid_ny=20, vis_window=16), 0.0),
    "nf20_split_runs": (sa.SceneSpec(n_frames=23, grid_nx=33, grid_ny=31, vis_window=20), 0.0),
    "nf2_short_runs": (sa.SceneSpec(n_frames=6, grid_nx=9, grid_ny=7, vis_window=2), 0.0),
    "ragged_20": (sa.SceneSpec(n_frames=60, grid_nx=40, grid_ny=30, vis_window=20, noise_uv_pix=0.3), 0.15),
    "long_nf30": (sa.SceneSpec(n_frames=48, grid_nx=12, grid_ny=10, vis_window=30), 0.0),
}


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("c", [1e-4, 1e-1])
def test_calibrated_phases_vs_yardstick(orc, cal, name, c):
    spec, frac = SCENES[name]
    sc = sa.generate_scene(spec)
    if frac > 0:
        sc = sa.drop_observations(sc, frac, seed=7)
    if name.startswith("long"):
        assert np.diff(sc.row_ptr).max() > 24
    _phases(orc, cal, sc, spec.f0, c)
    # uniform runs of <= 20 frames go through the 6-wide MFMA Schur kernel; longer tracks take the per-landmark kernel
    if np.diff(sc.row_ptr).max() > 20:
        assert cal.schur_fallback_landmarks() > 0
    elif frac == 0:
        assert cal.schur_fallback_landmarks() == 0


@pytest.mark.parametrize("c", [1e-4, 1e-1])
def test_calibrated_phases_shared_k_mvf_shape(orc, cal, c):
    sc = sa.generate_scene(sa.SceneSpec(n_frames=7, grid_nx=6, grid_ny=4, vis_window=4, f0=1.0))
    sc1 = sa.Scene(sc.points, sc.cam_R, sc.cam_T, sc.K[0:1], 1, sc.row_ptr, sc.obs_frame, sc.obs_uv)
    _phases(orc, cal, sc1, 1.0, c)


@pytest.mark.parametrize("c", [1e-4, 1e-1])
def test_calibrated_phases_c2_full_size(orc, cal, c):
    spec = sa.CONFIGS["C2_200cam_20kpt"]
    _phases(orc, cal, sa.config_scene("C2_200cam_20kpt"), spec.f0, c)
    assert cal.schur_fallback_landmarks() == 0


@pytest.mark.parametrize("c", [1e-4, 1e-1])
def test_calibrated_c3_sampled_rows_and_corrections_vs_skyline_yardstick(orc, cal, c):
    spec = sa.CONFIGS["C3_1kcam_100kpt"]
    sc = sa.config_scene("C3_1kcam_100kpt")
    so = _orc_scene(orc, sc)
    assert orc.normalize(so)[0]
    M, N = sc.M, sc.N
    keep = np.where(cref.compact_to_reduced(M) >= 0)[0]
    rows = keep[np.linspace(0, len(keep) - 1, 40).astype(np.int64)]
    ref = cref.step(orc, spec.f0, so, c, skyline=True, sel_rows=rows)
    assert ref["ok"] and cal.upload(spec.f0, sc)
    assert cal.schur_fallback_landmarks() == 0  # every run of the bench scene on the 6-wide MFMA kernel
    cal.phase_derivatives()
    cal.phase_schur(c)
    Rg = cal.rcs_rows(rows)
    assert Rg.shape == (len(rows), 6 * M)
    idx = cref.compact_to_reduced(M)
    Ro = np.zeros_like(Rg)
    for k in range(len(rows)):
        Ro[k, keep] = ref["rows"][k, idx[keep]]
    Ro[:, ~np.isin(np.arange(6 * M), keep)] = 0
    for k, r in enumerate(rows):
        Ro[k, r + 1:] = 0
    dU = np.sqrt(np.abs(np.einsum("mii->mi", ref["U"]))).reshape(-1)
    d = np.where(dU > 0, dU, 1.0)
    assert float((np.abs(Rg - Ro) / (d[rows][:, None] * d[None, :])).max()) < 1e-10
    assert cal.phase_solve()
    cal.phase_backsub(c)
    corr = cal.buffer(B.BUF_CORRECTIONS)
    assert _gauge_zero(corr[3 * N:], M)
    assert rel_err(corr, ref["corr"]) < 1e-8
    cal.upload(1.0, sa.generate_scene(sa.SceneSpec(n_frames=5, grid_nx=4, grid_ny=3, vis_window=3)))  # release


# ------------------------------------------------------------------ end to end

def _same_as_yardstick(orc, gpu, sc, f0, skyline=False, **kw):
    so = _orc_scene(orc, sc)
    rc_o, rep_o = cref.compute_inplace(orc, f0, so, kw.get("allowed"), kw.get("max_factor"), kw.get("max_iterations", 0),
                                       skyline=skyline)
    ok, rep, sg, log = _run(gpu, sc, f0, **kw)
    assert ok == (rc_o == 0)
    assert rep.status == rep_o.status
    assert (rep.iterations, rep.attempts) == (rep_o.iterations, rep_o.attempts)
    assert list(log["attempts"]) == rep_o.attempts_per_iteration[:rep.iterations]
    assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-8, abs=1e-18)
    lt.assert_same_trajectory(log, rep_o.log, 1e-8, gpu_attempts=rep.attempts, err_abs=1e-18)
    assert np.abs(sg.points - so.points).max() < 1e-8
    assert np.abs(sg.cam_R - so.cam_R).max() < 1e-8
    assert np.abs(sg.cam_T - so.cam_T).max() < 1e-8
    assert np.array_equal(sg.K, sc.K)
    return ok, rep, sg


def test_calibrated_c1_to_convergence_vs_python_lm_loop(orc, cal):
    sc = sa.config_scene("C1_dino_standin")
    _, rep, _ = _same_as_yardstick(orc, cal, sc, 600.0, allowed=1e-12, max_factor=1e6)
    assert rep.err_final < rep.err_initial


def test_calibrated_c2_ten_iterations_vs_python_lm_loop(orc, cal):
    spec = sa.CONFIGS["C2_200cam_20kpt"]
    threads = orc.get_threads()
    orc.set_threads(8)
    try:
        _, rep, _ = _same_as_yardstick(orc, cal, sa.config_scene("C2_200cam_20kpt"), spec.f0, skyline=True, max_iterations=10)
    finally:
        orc.set_threads(threads)
    assert rep.iterations == 10


BAND = sa.SceneSpec(n_frames=120, grid_nx=30, grid_ny=20, vis_window=8)


def test_calibrated_shuffled_frames_take_the_reordering_and_agree(cal):
    sc = sa.generate_scene(BAND)
    perm = np.concatenate([[0, 1], 2 + np.random.RandomState(0).permutation(sc.M - 2)])  # the gauge frames stay 0 and 1
    sh = sa.renumber_frames(sc, perm)
    base = _run(cal, sc, BAND.f0, 1e-10, 1e6, 8)
    got = _run(cal, sh, BAND.f0, 1e-10, 1e6, 8)
    assert cal.frame_order() is not None  # renumbered internally
    ok, rep, sg, log = got
    sg_back = sa.Scene(sg.points, sg.cam_R[perm], sg.cam_T[perm], sc.K, sc.shared_k, sc.row_ptr, sc.obs_frame, sc.obs_uv)
    _compare_runs(base, (ok, rep, sg_back, log))
    # explicit order: the identity on the caller's order gives the unshuffled run's result up to summation order as well
    cal.set_frame_order(np.argsort(perm).astype(np.int32))
    try:
        got2 = _run(cal, sh, BAND.f0, 1e-10, 1e6, 8)
    finally:
        cal.set_frame_order(None)
    ok, rep, sg, log = got2
    _compare_runs(base, (ok, rep, sa.Scene(sg.points, sg.cam_R[perm], sg.cam_T[perm], sc.K, sc.shared_k, sc.row_ptr,
                                           sc.obs_frame, sc.obs_uv), log))


def test_calibrated_loop_scene_reordered_vs_callers_order(cal):
    sc = sa.loop_scene(sa.SceneSpec(n_frames=90, grid_nx=20, grid_ny=15, vis_window=0), window=6)
    a = _run(cal, sc, 600.0, 1e-10, 1e6, 8)
    assert cal.frame_order() is not None
    cal.set_frame_reordering(0)
    try:
        b = _run(cal, sc, 600.0, 1e-10, 1e6, 8)
    finally:
        cal.set_frame_reordering(-1)
    _compare_runs(a, b)


def test_calibrated_solver_modes_fusion_and_speculation_agree(cal):
    sc = sa.generate_scene(sa.SceneSpec(n_frames=120, grid_nx=40, grid_ny=30, vis_window=10))
    base = _run(cal, sc, 600.0, 1e-10, 1e6, 8)
    try:
        for mode in (0, 1, 2):
            for fused in (True, False):
                for spec_on in (True, False):
                    cal.set_rcs_mode(mode)
                    cal.set_solver_fusion(fused)
                    cal.set_speculation(spec_on)
                    _compare_runs(base, _run(cal, sc, 600.0, 1e-10, 1e6, 8), tol=1e-7)
    finally:
        cal.set_rcs_mode(2)
        cal.set_solver_fusion(True)
        cal.set_speculation(True)


# ------------------------------------------------------------------ the default stays as it is

@pytest.mark.parametrize("name", ["C1_dino_standin", "nf20_runs"])
def test_default_is_bitwise_unchanged_after_toggling(name):
    """The default path computes what it computed before fixed intrinsics existed, bit for bit: a handle that had fixed
    intrinsics switched on and off again before the upload, and a fresh handle, against the outputs the commit before them
    wrote (tests/golden/default_det_before_fixed_intrinsics.npz, tools/gen_default_golden.py).  The default mode's fp64
    atomics differ in the last bits from run to run, so all three run the ordered sums of deterministic mode
    (srk_ba_set_deterministic), which share every kernel but the sums' order with the default."""
    g = load_golden("default_det_before_fixed_intrinsics")
    if name == "C1_dino_standin":
        sc, f0 = sa.config_scene(name), 600.0
    else:
        spec = sa.SceneSpec(n_frames=30, grid_nx=33, grid_ny=31, vis_window=20)
        sc, f0 = sa.generate_scene(spec), spec.f0
    fresh = sa.BundleAdjustmentKanatani(0)
    toggled = sa.BundleAdjustmentKanatani(0)
    try:
        assert fresh.frame_vars() == 10
        toggled.set_fixed_intrinsics(True)
        assert toggled.frame_vars() == 6
        toggled.set_fixed_intrinsics(False)
        for h in (fresh, toggled):
            h.set_deterministic(True)
        runs = [_run(h, sc, f0, None, None, 20) for h in (fresh, toggled)]
        assert fresh.deterministic() and toggled.deterministic() and bool(g[f"{name}__det"])
        assert fresh.frame_vars() == toggled.frame_vars() == 10
        assert fresh.VarsCount() == 3 * sc.N + 10 * sc.M
        for ok, rep, sg, log in runs:
            assert [rep.iterations, rep.attempts, rep.status] == g[f"{name}__counts"].tolist()
            assert [rep.err_initial, rep.err_final] == g[f"{name}__err"].tolist()
            assert np.array_equal(log["attempts"], g[f"{name}__attempts"]) and np.array_equal(log["err"], g[f"{name}__log_err"])
            for x in ("points", "cam_R", "cam_T"):
                assert np.array_equal(getattr(sg, x), g[f"{name}__{x}"]), x
    finally:
        fresh.close()
        toggled.close()


# ------------------------------------------------------------------ refusals

def test_unsupported_combinations_are_refused_and_the_handle_stays_usable():
    sc = sa.generate_scene(sa.SceneSpec(n_frames=6, grid_nx=5, grid_ny=4, vis_window=3))
    setters = [("set_deterministic", True), ("set_storage_precision", True), ("set_schur_precision", True)]
    for name, val in setters:
        # the combination made by the second call, in both orders
        h = sa.BundleAdjustmentKanatani(0)
        try:
            h.set_fixed_intrinsics(True)
            with pytest.raises(ValueError):
                getattr(h, name)(val)
            assert "fixed intrinsics" in h.last_error()
            h2 = sa.BundleAdjustmentKanatani(0)
            getattr(h2, name)(val)
            with pytest.raises(ValueError):
                h2.set_fixed_intrinsics(True)
            assert h2.frame_vars() == 10
            h2.close()
            ok, rep, _, _ = _run(h, sc, 600.0, 1e-10, 1e6, 3)  # still calibrated, still usable
            assert h.frame_vars() == 6 and rep.iterations > 0
        finally:
            h.close()
    # more than one rank
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_fixed_intrinsics(True)
        with pytest.raises(ValueError):
            h.set_allreduce(_lib.ALLREDUCE_FN(lambda *a: 0), 0, 2)
        ok, rep, _, _ = _run(h, sc, 600.0, 1e-10, 1e6, 3)
        assert h.frame_vars() == 6 and rep.iterations > 0
    finally:
        h.close()
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_allreduce(_lib.ALLREDUCE_FN(lambda *a: 0), 0, 2)
        with pytest.raises(ValueError):
            h.set_fixed_intrinsics(True)
        assert h.frame_vars() == 10 and "more than one rank" in h.last_error()
    finally:
        h.close()
