"""Shared intrinsics on the GPU (srk_ba_set_intrinsic_groups: one [fx fy u0 v0] per camera group, solved with the poses
and points) against the yardstick of tests/shared_k_ref.py -- the oracle's damped reduced system folded by P, a numpy solve,
the oracle's blocks for the point back-substitution, and the LM loop of bundle-adj-kanatani.cpp:720-893 around it.

Tolerances: the folded system 1e-10 class-scaled (as the parity tests), corrections rel 1e-8, the trial scene and K 1e-10
(relative to their scale); gauge entries exactly 0.
"""
import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import ba as B
from surikatoko_amd import _lib
from conftest import load_golden, rel_err
import shared_k_ref as kref
import lm_trajectory as lt
import robust_ref as rref
import dataclasses
from gpu_common import run_lm as _run

pytestmark = pytest.mark.gpu


def _groups(M, kind):
    if kind == 1:
        return np.zeros(M, dtype=np.int32)
    if kind == 2:
        return (np.arange(M) % 2).astype(np.int32)
    return (np.arange(M) * 32 // M).astype(np.int32)  # 32 groups of consecutive frames


def _to_f0(K, f0):
    """downloaded K (the caller's convention) -> the yardstick's, K(2,2) = f0"""
    K = np.asarray(K, dtype=np.float64).reshape(-1, 9)
    return K * (f0 / K[:, 8:9])


def _phases(orc, gpu, sc, f0, groups, c, loss=None, delta=None):
    """derivatives -> schur -> solve -> backsub on both sides, checked"""
    so = kref.per_frame_scene(orc, sc, f0)
    assert orc.normalize(so)[0]
    N, M = sc.N, sc.M
    G = int(groups.max()) + 1
    n = 6 * M + 4 * G
    gpu.set_intrinsic_groups(groups)
    assert gpu.upload(f0, sc) and gpu.frame_vars() == 6 and gpu.intrinsic_groups() == G
    assert gpu.rcs_chunks() == 0
    kind = rref.KINDS[loss]
    ref = kref.step(orc, f0, so, groups, c, kind=kind if loss else None, delta=delta)
    gpu.set_robust_loss(loss, delta if loss else 1.0)
    gpu.phase_derivatives()
    for which, size in ((B.BUF_GRAD, 3 * N + n), (B.BUF_CORRECTIONS, 3 * N + n), (B.BUF_RCS_RHS, n), (B.BUF_RCS, n * n),
                        (B.BUF_FRAME_BLOCKS, 100 * M), (B.BUF_POINT_FRAME, 30 * sc.O)):
        assert gpu._lib.srk_ba_buffer_size(gpu._h, which) == size
    gg = gpu.buffer(B.BUF_GRAD)
    gref = kref.folded_gradient(ref["gradE"], N, M, groups)
    assert rel_err(gg, gref) < 1e-10
    gpu.phase_schur(c)
    Sg = gpu.buffer(B.BUF_RCS).reshape(n, n)
    rg = gpu.buffer(B.BUF_RCS_RHS)
    gauge = kref.gauge_mask(M, groups)
    keep = ~gauge
    d = np.sqrt(np.abs(np.diag(ref["S"])))
    d = np.where(d > 0, d, 1.0)
    Ss = (Sg - ref["S"]) / np.outer(d, d)
    assert float(np.abs(Ss[np.ix_(keep, keep)]).max()) < 1e-10
    assert float((np.abs(rg - ref["rhs"])[keep] / d[keep]).max()) < 1e-10 * max(1.0, float((np.abs(ref["rhs"]) / d).max()))
    for f in np.where(gauge)[0]:  # gauge rows: identity, zero rhs; the border is exactly 0 at gauge columns
        row = Sg[f].copy()
        assert row[f] == 1.0
        row[f] = 0
        assert np.all(row == 0) and rg[f] == 0
    assert gpu.phase_solve()
    gpu.phase_backsub(c)
    corr = gpu.buffer(B.BUF_CORRECTIONS)
    assert np.all(corr[3 * N:][gauge] == 0)
    assert rel_err(corr, ref["corr"]) < 1e-8
    orc.apply_corrections(so, ref["corr10"])
    so.K[:] = kref.apply_k(so.K, ref["dc"], M, groups)
    gpu.phase_accept()
    scale = max(1.0, float(np.abs(so.points).max()))
    assert np.abs(gpu.buffer(B.BUF_POINTS).reshape(-1, 3) - so.points).max() < 1e-10 * scale
    assert np.abs(gpu.buffer(B.BUF_CAM_R).reshape(-1, 9) - so.cam_R).max() < 1e-10
    assert np.abs(gpu.buffer(B.BUF_CAM_T).reshape(-1, 3) - so.cam_T).max() < 1e-10 * scale
    Kg = _to_f0(gpu.download_intrinsics(), f0)
    first = np.array([np.where(groups == g)[0][0] for g in range(G)])
    kscale = np.abs(so.K).max()
    assert np.abs(Kg - so.K[first]).max() < 1e-10 * kscale
    e2o = rref.energy(f0, so, kind, delta) if loss else orc.reproj_error(f0, so)[0]
    e2g, _ = gpu.phase_error()
    gpu.set_robust_loss(None)
    assert e2g == pytest.approx(e2o, rel=1e-6)


SCENES = {
    "nf16_10_tiles": (sa.SceneSpec(n_frames=24, grid_nx=30, grid_ny=20, vis_window=16), 0.0),
    "nf20_split_runs": (sa.SceneSpec(n_frames=23, grid_nx=33, grid_ny=31, vis_window=20), 0.0),
    "nf2_short_runs": (sa.SceneSpec(n_frames=6, grid_nx=9, grid_ny=7, vis_window=2), 0.0),
    "ragged_20": (sa.SceneSpec(n_frames=60, grid_nx=40, grid_ny=30, vis_window=20, noise_uv_pix=0.3), 0.15),
    "long_nf30": (sa.SceneSpec(n_frames=48, grid_nx=12, grid_ny=10, vis_window=30), 0.0),
}


@pytest.fixture(scope="module")
def shk():
    h = sa.BundleAdjustmentKanatani(0)
    yield h
    h.close()


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("kind", [1, 2, 32])
@pytest.mark.parametrize("c", [1e-4, 1e-1])
def test_shared_k_phases_vs_yardstick(orc, shk, name, kind, c):
    spec, frac = SCENES[name]
    sc = sa.generate_scene(spec)
    if frac > 0:
        sc = sa.drop_observations(sc, frac, seed=7)
    if kind == 32 and sc.M < 32:
        pytest.skip("32 groups need at least 32 frames")
    _phases(orc, shk, sc, spec.f0, _groups(sc.M, kind), c)


@pytest.mark.parametrize("kind", [1, 2, 32])
def test_shared_k_phases_c1(orc, shk, kind):
    _phases(orc, shk, sa.config_scene("C1_dino_standin"), 600.0, _groups(36, kind), 1e-4)


@pytest.mark.parametrize("c", [1e-4, 1e-1])
def test_shared_k_phases_with_huber_vs_yardstick(orc, shk, c):
    """a robust loss acts inside the derivative kernels: the folded system is that of robust_ref's weighted blocks"""
    sc = sa.generate_scene(sa.SceneSpec(n_frames=24, grid_nx=20, grid_ny=15, vis_window=8, noise_uv_pix=0.5))
    rref.inject_outliers(sc, 0.05, 20.0, 60.0, seed=3)
    _phases(orc, shk, sc, 600.0, _groups(sc.M, 2), c, loss="huber", delta=2.0)


def test_shared_k_phases_c2_full_size(orc, shk):
    spec = sa.CONFIGS["C2_200cam_20kpt"]
    threads = orc.get_threads()
    orc.set_threads(8)
    try:
        _phases(orc, shk, sa.config_scene("C2_200cam_20kpt"), spec.f0, _groups(200, 1), 1e-4)
    finally:
        orc.set_threads(threads)


# ------------------------------------------------------------------ staged steps, modes

def _staged(h, sc, f0, groups, c, steps=3):
    """`steps` accepted shared-intrinsics steps through the staged calls; returns the scene and K after them"""
    h.set_intrinsic_groups(groups)
    assert h.upload(f0, sc)
    for _ in range(steps):
        h.phase_derivatives()
        h.phase_schur(c)
        assert h.phase_solve()
        h.phase_backsub(c)
        h.phase_accept()
    return [h.buffer(w) for w in (B.BUF_POINTS, B.BUF_CAM_R, B.BUF_CAM_T, B.BUF_CORRECTIONS)], h.download_intrinsics()


def test_shared_k_staged_steps_are_bitwise_repeatable_in_deterministic_mode():
    sc = sa.config_scene("C1_dino_standin")
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_deterministic(True)
        a, Ka = _staged(h, sc, 600.0, _groups(sc.M, 2), 1e-3)
        assert h.deterministic()
        b, Kb = _staged(h, sc, 600.0, _groups(sc.M, 2), 1e-3)
        assert np.array_equal(Ka, Kb)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    finally:
        h.close()


def test_shared_k_rcs_modes_and_frame_reordering_agree(shk):
    spec = sa.SceneSpec(n_frames=120, grid_nx=30, grid_ny=20, vis_window=8, noise_uv_pix=0.5)
    sc = sa.generate_scene(spec)
    groups = _groups(sc.M, 2)
    base, Kb = _staged(shk, sc, spec.f0, groups, 1e-3)
    try:
        for mode in (0, 1, 2):
            shk.set_rcs_mode(mode)
            got, K = _staged(shk, sc, spec.f0, groups, 1e-3)
            assert rel_err(K, Kb) < 1e-10
            for x, y in zip(got, base):
                assert rel_err(x, y) < 1e-10
    finally:
        shk.set_rcs_mode(2)
    # the same frames shuffled: renumbered internally, groups and downloads in the caller's numbering
    perm = np.concatenate([[0, 1], 2 + np.random.RandomState(0).permutation(sc.M - 2)])
    sh = sa.renumber_frames(sc, perm)  # frame perm[i] of sh is frame i of sc
    gsh = np.empty_like(groups)
    gsh[perm] = groups
    got, K = _staged(shk, sh, spec.f0, gsh, 1e-3)
    assert shk.frame_order() is not None
    N, M = sc.N, sc.M
    assert rel_err(K, Kb) < 1e-8
    assert rel_err(got[0], base[0]) < 1e-8  # points keep their numbering
    assert rel_err(got[1].reshape(-1, 9)[perm], base[1].reshape(-1, 9)) < 1e-8
    assert rel_err(got[2].reshape(-1, 3)[perm], base[2].reshape(-1, 3)) < 1e-8
    cg, cb = got[3], base[3]  # corrections: points, the poses in the caller's frame numbering, the groups' intrinsics
    assert rel_err(cg[:3 * N], cb[:3 * N]) < 1e-8
    assert rel_err(cg[3 * N:3 * N + 6 * M].reshape(M, 6)[perm], cb[3 * N:3 * N + 6 * M].reshape(M, 6)) < 1e-8
    assert rel_err(cg[3 * N + 6 * M:], cb[3 * N + 6 * M:]) < 1e-8
    shk.set_intrinsic_groups(None)


def _same_as_yardstick(orc, gpu, sc, f0, groups, **kw):
    so = kref.per_frame_scene(orc, sc, f0)
    rc_o, rep_o = kref.compute_inplace(orc, f0, so, groups, kw.get("allowed"), kw.get("max_factor"), kw.get("max_iterations", 0))
    gpu.set_intrinsic_groups(groups)
    try:
        ok, rep, sg, log = _run(gpu, sc, f0, **kw)
        G = int(np.max(groups)) + 1
        Kg = _to_f0(gpu.download_intrinsics(), f0)
    finally:
        gpu.set_intrinsic_groups(None)
    assert ok == (rc_o == 0)
    assert rep.status == rep_o.status
    assert (rep.iterations, rep.attempts) == (rep_o.iterations, rep_o.attempts)
    assert list(log["attempts"]) == rep_o.attempts_per_iteration[:rep.iterations]
    assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-6, abs=1e-18)
    lt.assert_same_trajectory(log, rep_o.log, 1e-6, gpu_attempts=rep.attempts, err_abs=1e-18)
    assert np.abs(sg.points - so.points).max() < 1e-6
    assert np.abs(sg.cam_R - so.cam_R).max() < 1e-6
    assert np.abs(sg.cam_T - so.cam_T).max() < 1e-6
    first = np.array([np.where(np.asarray(groups) == g)[0][0] for g in range(G)])
    assert rel_err(Kg, so.K[first]) < 1e-8
    return ok, rep, sg


def test_shared_k_c1_to_convergence_vs_python_lm_loop(orc, shk):
    sc = sa.config_scene("C1_dino_standin")
    _, rep, _ = _same_as_yardstick(orc, shk, sc, 600.0, np.zeros(sc.M, dtype=np.int32), allowed=1e-12, max_factor=1e6)
    assert rep.err_final < rep.err_initial


def test_shared_k_two_groups_ten_iterations_vs_python_lm_loop(orc, shk):
    sc = sa.generate_scene(sa.SceneSpec(n_frames=40, grid_nx=20, grid_ny=15, vis_window=8, noise_uv_pix=0.5))
    _, rep, _ = _same_as_yardstick(orc, shk, sc, 600.0, _groups(sc.M, 2), max_iterations=10)
    assert rep.iterations == 10


SELFCAL = {
    "synthetic_f0_1": sa.SceneSpec(n_frames=24, grid_nx=12, grid_ny=9, vis_window=12, f0=1.0, noise_uv_pix=0.0),
    "C1_dino_standin": dataclasses.replace(sa.CONFIGS["C1_dino_standin"], noise_uv_pix=0.0),
    "demo_circle_grid": dataclasses.replace(sa.CONFIGS["demo_circle_grid"], noise_uv_pix=0.0),
}


def _perturbed_k(K, f0):
    """fx, fy + 3 %, u0, v0 + 5 px (K in the caller's units: pixels / f0 times K(2,2))"""
    K = np.asarray(K, dtype=np.float64).reshape(-1, 9).copy()
    K[:, 0] *= 1.03
    K[:, 4] *= 1.03
    K[:, 2] += 5.0 * K[:, 8] / f0
    K[:, 5] += 5.0 * K[:, 8] / f0
    return K


def _lm_final(h, sc, f0, groups=None, fixed=False):
    h.set_intrinsic_groups(groups)
    h.set_fixed_intrinsics(fixed)
    try:
        _, rep, _, _ = _run(h, sc, f0, 1e-30, 1e10, 200)
        K = h.download_intrinsics() if groups is not None else None
    finally:
        h.set_intrinsic_groups(None)
        h.set_fixed_intrinsics(False)
    return rep, K


@pytest.mark.parametrize("name", list(SELFCAL))
def test_self_calibration_lm_one_camera_recovers_k_where_other_modes_cannot(shk, name):
    """noise-free observations, K perturbed by 3 % and 5 px: the LM loop with one group reaches the convergence floor and
    the true K; the default mode (K corrections thrown away) and the calibrated mode from the same start end at least 100x
    higher.  The f0 = 600 scenes carry K divided by f0, the project's convention."""
    spec = SELFCAL[name]
    sc = sa.generate_scene(spec)
    Ktrue = sc.K.reshape(-1, 9)[0].copy()
    start = sa.Scene(sc.points, sc.cam_R, sc.cam_T, _perturbed_k(sc.K, spec.f0), False, sc.row_ptr, sc.obs_frame, sc.obs_uv)
    rep, Kg = _lm_final(shk, start, spec.f0, np.zeros(sc.M, dtype=np.int32))
    assert rel_err(Kg.reshape(-1), Ktrue) < 1e-6
    rep_d, _ = _lm_final(shk, start, spec.f0)
    rep_c, _ = _lm_final(shk, start, spec.f0, fixed=True)
    assert rep_d.err_final >= 100 * rep.err_final and rep_c.err_final >= 100 * rep.err_final


def test_shared_k_deterministic_lm_runs_are_bitwise_repeatable():
    sc = sa.config_scene("C1_dino_standin")
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_deterministic(True)
        h.set_intrinsic_groups(_groups(sc.M, 2))
        runs = []
        for _ in range(2):
            ok, rep, sg, log = _run(h, sc, 600.0, 1e-12, 1e6, 10)
            runs.append((ok, rep.status, rep.iterations, rep.attempts, rep.err_final, list(log["err"]), sg, h.download_intrinsics()))
        assert h.deterministic()
        a, b = runs
        assert a[:6] == b[:6]
        for x in ("points", "cam_R", "cam_T"):
            assert np.array_equal(getattr(a[6], x), getattr(b[6], x))
        assert np.array_equal(a[7], b[7])
    finally:
        h.close()


def test_shared_k_speculation_takes_the_same_decisions(shk):
    sc = sa.generate_scene(sa.SceneSpec(n_frames=120, grid_nx=40, grid_ny=30, vis_window=10, noise_uv_pix=0.5))
    shk.set_intrinsic_groups(_groups(sc.M, 2))
    try:
        runs = []
        for spec_on in (True, False):
            shk.set_speculation(spec_on)
            ok, rep, sg, log = _run(shk, sc, 600.0, 1e-10, 1e6, 8)
            runs.append((ok, rep.status, rep.iterations, rep.attempts, list(log["attempts"]), rep.err_final, sg.cam_T.copy(),
                         shk.download_intrinsics()))
        a, b = runs
        assert a[:5] == b[:5]
        assert a[5] == pytest.approx(b[5], rel=1e-10)
        assert np.abs(a[6] - b[6]).max() < 1e-10 and rel_err(a[7], b[7]) < 1e-10
    finally:
        shk.set_speculation(True)
        shk.set_intrinsic_groups(None)


# ------------------------------------------------------------------ the default stays as it is

@pytest.mark.parametrize("name", ["C1_dino_standin", "nf20_runs"])
def test_default_is_bitwise_unchanged_after_toggling_groups(name):
    g = load_golden("default_det_before_fixed_intrinsics")
    if name == "C1_dino_standin":
        sc, f0 = sa.config_scene(name), 600.0
    else:
        spec = sa.SceneSpec(n_frames=30, grid_nx=33, grid_ny=31, vis_window=20)
        sc, f0 = sa.generate_scene(spec), spec.f0
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_intrinsic_groups(np.zeros(sc.M, dtype=np.int32))
        assert h.frame_vars() == 6 and h.intrinsic_groups() == 1
        h.set_intrinsic_groups(None)
        h.set_deterministic(True)
        ok, rep, sg, log = _run(h, sc, f0, None, None, 20)
        assert h.deterministic() and h.frame_vars() == 10 and h.intrinsic_groups() == 0
        assert [rep.iterations, rep.attempts, rep.status] == g[f"{name}__counts"].tolist()
        assert [rep.err_initial, rep.err_final] == g[f"{name}__err"].tolist()
        assert np.array_equal(log["attempts"], g[f"{name}__attempts"]) and np.array_equal(log["err"], g[f"{name}__log_err"])
        for x in ("points", "cam_R", "cam_T"):
            assert np.array_equal(getattr(sg, x), g[f"{name}__{x}"]), x
    finally:
        h.close()


# ------------------------------------------------------------------ refusals

def _usable(h, sc, groups=True):
    if groups:
        _staged(h, sc, 600.0, np.zeros(sc.M, dtype=np.int32), 1e-3, steps=1)
    else:
        h.set_intrinsic_groups(None)
        ok, rep, _, _ = _run(h, sc, 600.0, 1e-10, 1e6, 3)
        assert rep.iterations > 0


def test_unsupported_combinations_are_refused_and_the_handle_stays_usable():
    sc = sa.generate_scene(sa.SceneSpec(n_frames=6, grid_nx=5, grid_ny=4, vis_window=3))
    g0 = np.zeros(sc.M, dtype=np.int32)
    for name, val in [("set_fixed_intrinsics", True), ("set_storage_precision", True), ("set_schur_precision", True)]:
        h = sa.BundleAdjustmentKanatani(0)
        try:
            h.set_intrinsic_groups(g0)
            with pytest.raises(ValueError):
                getattr(h, name)(val)
            assert "intrinsic groups" in h.last_error()
            _usable(h, sc)
            h2 = sa.BundleAdjustmentKanatani(0)
            getattr(h2, name)(val)
            with pytest.raises(ValueError):
                h2.set_intrinsic_groups(g0)
            assert h2.intrinsic_groups() == 0
            h2.close()
        finally:
            h.close()
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_intrinsic_groups(g0)
        with pytest.raises(ValueError):
            h.set_allreduce(_lib.ALLREDUCE_FN(lambda *a: 0), 0, 2)
        _usable(h, sc)
    finally:
        h.close()


def test_bad_groups_are_refused_and_the_handle_stays_usable(shk):
    sc = sa.generate_scene(sa.SceneSpec(n_frames=40, grid_nx=12, grid_ny=9, vis_window=6))
    M = sc.M
    with pytest.raises(ValueError):
        shk.set_intrinsic_groups(np.arange(M) % 33)  # 33 groups
    with pytest.raises(ValueError):
        shk.set_intrinsic_groups(np.full(M, -1))
    with pytest.raises(ValueError):
        shk.set_intrinsic_groups(np.where(np.arange(M) < 5, 0, 2))  # group 1 empty
    _usable(shk, sc)
    # K differing inside a group: refused at upload
    K = np.repeat(sc.K.reshape(-1, 9)[:1], M, axis=0)
    K[3, 0] = np.nextafter(K[3, 0], 2 * K[3, 0])
    bad = sa.Scene(sc.points, sc.cam_R, sc.cam_T, K, 0, sc.row_ptr, sc.obs_frame, sc.obs_uv)
    shk.set_intrinsic_groups(np.zeros(M, dtype=np.int32))
    with pytest.raises(ValueError):
        shk.upload(600.0, bad)
    assert "different intrinsics" in shk.last_error()
    # groups for another number of frames
    shk.set_intrinsic_groups(np.zeros(M + 1, dtype=np.int32))
    with pytest.raises(ValueError):
        shk.upload(600.0, sc)
    _usable(shk, sc)
    # download_intrinsics without groups
    _usable(shk, sc, groups=False)
    with pytest.raises(ValueError):
        shk.download_intrinsics()
    _usable(shk, sc)
    shk.set_intrinsic_groups(None)
