"""Per-observation information on the GPU (srk_ba_set_observation_information) and the residual
download (srk_ba_observation_residuals), against the yardstick of tests/weighted_ref.py -- robust_ref's residuals and
Jacobians weighted by q rho'(q s), the oracle's own two-phase step on those blocks, the LM loop of
bundle-adj-kanatani.cpp:720-893 on E = sum rho(q s).

Tolerances are those of tests/test_gpu_robust.py: blocks 1e-12 per variable class, gradient, reduced camera system and its
right-hand side 1e-10 class-scaled, E 1e-13 relative; corrections 1e-8 with six frame variables and 1e-7 with ten; end to
end E per iteration 1e-10 and the scene 1e-8 with six frame variables, 1e-8 and 1e-7 with ten.

Information: weighted_ref.make_information -- seeded, log-uniform in [0.25, 4], then about 3 % of the observations set to 0,
at most one per landmark and only in landmarks with at least four observations.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import ba as B
from conftest import load_golden, rel_err, sym_scaled_err, class_rel_err
import calibrated_ref as cref
import lm_trajectory as lt
import robust_ref as rr
import shared_k_ref as kref
import weighted_ref as wr
from gpu_common import orc_scene as _orc_scene

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = {rr.NONE: None, rr.HUBER: "huber", rr.CAUCHY: "cauchy"}


@pytest.fixture(scope="module")
def handles():
    h = {10: sa.BundleAdjustmentKanatani(0), 6: sa.BundleAdjustmentKanatani(0)}
    h[6].set_fixed_intrinsics(True)
    yield h
    for x in h.values():
        x.close()


def _with_outliers(sc, frac=0.05, seed=7):
    sc = sc.copy()
    rr.inject_outliers(sc, frac, 20, 60, seed)
    return sc


def _information(sc, seed=21):
    q = wr.make_information(sc, seed)
    pos = np.add.reduceat((q > 0).astype(np.int64), np.asarray(sc.row_ptr[:-1]))
    assert pos.min() >= 2  # every landmark keeps two or more positive observations
    assert np.any(q == 0) and q[q > 0].min() >= 0.25 and q.max() <= 4.0
    return q


def _pixel_residuals(f0, so):
    ex, ey = rr.residuals(f0, so)
    return f0 * np.stack([ex, ey], axis=1)


def _phases(orc, gpu, sc, q, f0, kind, delta, fv, c, jac_mode):
    """derivatives -> schur -> solve -> backsub -> accept on both sides, checked; returns the derivative kernel used"""
    so = _orc_scene(orc, sc)
    assert orc.normalize(so)[0]
    gpu.set_jacobian_mode(jac_mode)
    gpu.set_robust_loss(NAMES[kind], delta)
    try:
        # (the shared handle may hold a scene of another size, for which these values would be refused: the scene first,
        # then the information, which takes effect at the next phase call)
        assert gpu.upload(f0, sc) and gpu.frame_vars() == fv
        gpu.set_observation_information(q)
        assert np.array_equal(gpu.observation_information(), q)
        N, M = sc.N, sc.M
        ref = wr.step(orc, f0, so, c, q, kind, delta, fv=fv, want_system=True)
        wts = ref["weights"]
        if kind == rr.HUBER:
            assert np.any(wts[q > 0] == 1.0) and np.any(wts < 0.5)  # both branches of Huber
        E0 = wr.energy(f0, so, q, kind, delta)
        e0g, _ = gpu.phase_error()
        assert e0g == pytest.approx(E0, rel=1e-13)
        gpu.phase_derivatives()
        kernel = gpu.jacobian_kernel()
        Vg = gpu.buffer(B.BUF_POINT_BLOCKS).reshape(-1, 3, 3)
        Ug = gpu.buffer(B.BUF_FRAME_BLOCKS).reshape(M, fv, fv)
        Wg = gpu.buffer(B.BUF_POINT_FRAME).reshape(-1, 3, fv)
        gg = gpu.buffer(B.BUF_GRAD)
        off = 10 - fv
        Uo, Wo = ref["U"][:, off:, off:], ref["W"][:, :, off:]
        go = np.concatenate([ref["gradE"][:3 * N], ref["gradE"][3 * N:].reshape(M, 10)[:, off:].reshape(-1)])
        dV = np.sqrt(np.abs(np.einsum("nii->ni", ref["V"])))
        dU = np.sqrt(np.abs(np.einsum("mii->mi", Uo)))
        assert sym_scaled_err(Vg, ref["V"], dV) < 1e-12
        assert sym_scaled_err(Ug, Uo, dU) < 1e-12
        assert class_rel_err(Wg, Wo, (1, 2)) < 1e-12
        assert np.all(Wg[q == 0] == 0)  # switched off: exact zeros in the stored factors
        assert np.all(np.isfinite(Vg)) and np.all(np.isfinite(Ug)) and np.all(np.isfinite(Wg)) and np.all(np.isfinite(gg))
        gs = 2.0 * np.sqrt(max(E0, 1e-300))
        dg = np.concatenate([dV.reshape(-1), dU.reshape(-1)]) * gs
        okg = dg > 0
        assert float((np.abs(gg - go)[okg] / dg[okg]).max()) < 1e-10
        # what the caller sees, in the caller's order: the loss's factor rho'(q s) and the raw residuals
        assert np.abs(gpu.observation_weights() - wts).max() < 1e-12
        pix = _pixel_residuals(f0, so)
        assert np.abs(gpu.observation_residuals() - pix).max() < 1e-12 * max(1.0, float(np.abs(pix).max()))
        gpu.phase_schur(c)
        rg = gpu.buffer(B.BUF_RCS_RHS)
        Sg = gpu.buffer(B.BUF_RCS).reshape(fv * M, fv * M)
        if fv == 10:  # the oracle's 10M - 7 numbering -> full frame-variable indexing
            idx = cref.reduced_full_index(M)
            keep = idx >= 0
            So = np.zeros_like(Sg)
            So[np.ix_(keep, keep)] = ref["S"][np.ix_(idx[keep], idx[keep])]
            ro = np.zeros_like(rg)
            ro[keep] = ref["rhs"][idx[keep]]
        else:
            keep = cref.compact_to_reduced(M) >= 0
            So, ro = ref["S"], ref["rhs"]
        dk = dU.reshape(-1)[keep]
        dk = np.where(dk > 0, dk, 1.0)
        assert sym_scaled_err(Sg[np.ix_(keep, keep)], So[np.ix_(keep, keep)], dk) < 1e-10
        assert float((np.abs(rg[keep] - ro[keep]) / (dk * gs)).max()) < 1e-10
        assert gpu.phase_solve() and ref["ok"]
        gpu.phase_backsub(c)
        corr = gpu.buffer(B.BUF_CORRECTIONS)
        corr_tol = 1e-8 if fv == 6 else 1e-7
        assert rel_err(corr, ref["corr"]) < corr_tol
        orc.apply_corrections(so, ref["corr10"])
        gpu.phase_accept()
        e1g, _ = gpu.phase_error()
        assert e1g == pytest.approx(wr.energy(f0, so, q, kind, delta), rel=corr_tol)  # after a step: the corrections' tolerance
    finally:
        gpu.set_observation_information(None)
        gpu.set_robust_loss(None)
        gpu.set_jacobian_mode(-1)
    return kernel


# the four small scenes of tests/test_gpu_robust.py::SCENES: the smallest shapes that reach each derivative kernel
SCENES = {
    # name: (scene, jacobian mode, derivative kernel expected)
    "tile_edge_nf16_runs": (lambda: sa.generate_scene(sa.SceneSpec(n_frames=24, grid_nx=30, grid_ny=20, vis_window=16)), 1, 2),
    "ragged_20_unions": (lambda: sa.drop_observations(sa.generate_scene(sa.SceneSpec(n_frames=60, grid_nx=40, grid_ny=30,
                                                                                      vis_window=20)), 0.15, seed=5), 2, 3),
    "long_nf40_per_observation": (lambda: sa.generate_scene(sa.SceneSpec(n_frames=60, grid_nx=12, grid_ny=10, vis_window=50)), 0, 0),
    "small_fused": (lambda: sa.generate_scene(sa.SceneSpec(n_frames=12, grid_nx=10, grid_ny=10, vis_window=5)), 0, 1),
}


@pytest.mark.parametrize("fv", [10, 6])
@pytest.mark.parametrize("kind", [rr.NONE, rr.HUBER, rr.CAUCHY])
@pytest.mark.parametrize("name", list(SCENES))
def test_information_phases_vs_yardstick(orc, handles, name, kind, fv):
    make, mode, kernel = SCENES[name]
    sc = _with_outliers(make())
    if name.startswith("long"):
        assert np.diff(sc.row_ptr).max() > 32
    got = _phases(orc, handles[fv], sc, _information(sc), 600.0, kind, 2.0, fv, 1e-4, mode)
    assert got == kernel


def test_information_with_one_intrinsic_group_vs_yardstick(orc):
    """one group of shared intrinsics: the folded system is that of the weighted blocks (shared_k_ref's fold and solve)"""
    sc = _with_outliers(sa.generate_scene(sa.SceneSpec(n_frames=24, grid_nx=20, grid_ny=15, vis_window=8, noise_uv_pix=0.5)), seed=3)
    q = _information(sc)
    f0, c = 600.0, 1e-4
    groups = np.zeros(sc.M, dtype=np.int32)
    so = kref.per_frame_scene(orc, sc, f0)
    assert orc.normalize(so)[0]
    N, M = sc.N, sc.M
    n = 6 * M + 4
    gradE, V, U, W, _ = wr.derivatives(f0, so, q, rr.HUBER, 2.0)
    ok, _, S10, rhs10 = orc.two_phase(so, gradE, V, U, W, c, want_system=True)
    S, rhs = kref.fold(S10, rhs10, M, groups)
    free = ~kref.gauge_mask(M, groups)
    dc = np.zeros(n)
    dc[free] = np.linalg.solve(S[np.ix_(free, free)], rhs[free])
    dx = kref.backsub(gradE, V, W, so.row_ptr, so.obs_frame, kref.expand(dc, M, groups), c)
    gpu = sa.BundleAdjustmentKanatani(0)
    try:
        gpu.set_intrinsic_groups(groups)
        gpu.set_robust_loss("huber", 2.0)
        gpu.set_observation_information(q)
        assert gpu.upload(f0, sc) and gpu.intrinsic_groups() == 1
        gpu.phase_derivatives()
        assert rel_err(gpu.buffer(B.BUF_GRAD), kref.folded_gradient(gradE, N, M, groups)) < 1e-10
        gpu.phase_schur(c)
        Sg, rg = gpu.buffer(B.BUF_RCS).reshape(n, n), gpu.buffer(B.BUF_RCS_RHS)
        d = np.sqrt(np.abs(np.diag(S)))
        d = np.where(d > 0, d, 1.0)
        assert float(np.abs(((Sg - S) / np.outer(d, d))[np.ix_(free, free)]).max()) < 1e-10
        assert float((np.abs(rg - rhs)[free] / d[free]).max()) < 1e-10 * max(1.0, float((np.abs(rhs) / d).max()))
        assert gpu.phase_solve() and ok
        gpu.phase_backsub(c)
        assert rel_err(gpu.buffer(B.BUF_CORRECTIONS), np.concatenate([dx, dc])) < 1e-8
    finally:
        gpu.close()


# ------------------------------------------------------------------ residuals

def test_residuals_before_and_after_optimise_on_a_reordered_loop_closure(orc):
    sc = _with_outliers(sa.loop_scene(sa.SceneSpec(n_frames=90, grid_nx=20, grid_ny=15, vis_window=0, noise_uv_pix=0.5), window=6))
    q = _information(sc)
    crit = sa.BundleAdjustmentKanataniTermCriteria()
    crit.AllowedReprojErrRelativeChange(1e-10)
    crit.MaxHessianFactor(1e6)
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_frame_reordering(1)
        assert h.upload(600.0, sc) and h.frame_order() is not None
        so = _orc_scene(orc, sc)
        assert orc.normalize(so)[0]
        pix = _pixel_residuals(600.0, so)
        tol = 1e-12 * max(1.0, float(np.abs(pix).max()))
        e0 = h.observation_residuals()
        assert e0.shape == (int(sc.row_ptr[-1]), 2) and np.abs(e0 - pix).max() < tol
        # neither information nor a loss changes them
        h.set_observation_information(q)
        h.set_robust_loss("huber", 2.0)
        assert np.array_equal(h.observation_residuals(), e0)
        h.optimize(crit, 4)
        out = sc.copy()
        h.download(out, revert_normalization=False)
        e1 = h.observation_residuals()
        pix1 = _pixel_residuals(600.0, _orc_scene(orc, out))
        assert np.abs(e1 - pix1).max() < 1e-12 * max(1.0, float(np.abs(pix1).max()))
        assert np.abs(e1).max() > 10 and np.sqrt(np.mean(e1 ** 2)) < np.sqrt(np.mean(e0 ** 2))
        h.set_observation_information(None)
        h.set_robust_loss(None)
        assert np.array_equal(h.observation_residuals(), e1)
    finally:
        h.close()


# ------------------------------------------------------------------ end to end

def _run(gpu, sc, f0, q=None, kind=None, delta=2.0, allowed=None, max_factor=None, max_iterations=0):
    crit = sa.BundleAdjustmentKanataniTermCriteria()
    crit.AllowedReprojErrRelativeChange(allowed)
    crit.MaxHessianFactor(max_factor)
    gpu.set_robust_loss(kind, delta)
    sg = sc.copy()
    try:
        if q is not None:  # a handle that holds a scene of another size refuses the values: this scene first
            assert gpu.upload(f0, sg)
        gpu.set_observation_information(q)
        ok = gpu.ComputeInplace(f0, sg, crit, max_iterations)  # uploads again: the upload applies the information
    finally:
        w = gpu.observation_weights()
        gpu.set_robust_loss(None)
        gpu.set_observation_information(None)
    return ok, gpu.report, sg, gpu.iteration_log(), w


def _same(a, b):
    assert (a[1].iterations, a[1].attempts, a[1].status) == (b[1].iterations, b[1].attempts, b[1].status)
    assert (a[1].err_initial, a[1].err_final) == (b[1].err_initial, b[1].err_final)
    assert np.array_equal(a[3]["attempts"], b[3]["attempts"]) and np.array_equal(a[3]["err"], b[3]["err"])
    assert np.array_equal(a[4], b[4])
    for x in ("points", "cam_R", "cam_T"):
        assert np.array_equal(getattr(a[2], x), getattr(b[2], x)), x


E2E = {
    "C1": lambda: (sa.config_scene("C1_dino_standin"), 600.0),
    "ragged": lambda: (sa.drop_observations(sa.generate_scene(sa.SceneSpec(n_frames=30, grid_nx=23, grid_ny=17, vis_window=7,
                                                                          noise_uv_pix=0.5)), 0.25, seed=3), 600.0),
}


# Seeds (outliers 11, information 21): the yardstick's own ten-iteration runs on them were checked on the CPU to have no
# decision with a margin below lm_trajectory.TIE_MARGIN; the test asserts it again.
@pytest.mark.parametrize("fv", [10, 6])
@pytest.mark.parametrize("kind", [rr.NONE, rr.HUBER])
@pytest.mark.parametrize("name", list(E2E))
def test_information_ten_iterations_vs_python_lm_loop(orc, handles, name, kind, fv):
    sc, f0 = E2E[name]()
    sc = _with_outliers(sc, 0.05, seed=11)
    q = _information(sc)
    so = _orc_scene(orc, sc)
    rc_o, rep_o = wr.compute_inplace(orc, f0, so, q, kind, 2.0, None, None, 10, fv=fv)
    assert np.abs(lt.margins(rep_o.log)).min() >= lt.TIE_MARGIN
    gpu = handles[fv]
    ok, rep, sg, log, w = _run(gpu, sc, f0, q, NAMES[kind], 2.0, max_iterations=10)
    assert ok == (rc_o == 0) and rep.status == rep_o.status
    assert (rep.iterations, rep.attempts) == (rep_o.iterations, rep_o.attempts)
    assert list(log["attempts"]) == rep_o.attempts_per_iteration[:rep.iterations]
    err_tol, scene_tol = (1e-10, 1e-8) if fv == 6 else (1e-8, 1e-7)
    assert np.allclose(log["err"], rep_o.errors, rtol=err_tol, atol=0)
    lt.assert_same_trajectory(log, rep_o.log, err_tol, gpu_attempts=rep.attempts)
    assert rep.err_initial == pytest.approx(rep_o.err_initial, rel=1e-12)
    assert rep.err_final == pytest.approx(rep_o.err_final, rel=err_tol)
    scale = max(1.0, float(np.abs(so.points).max()))
    assert np.abs(sg.points - so.points).max() < scene_tol * scale
    assert np.abs(sg.cam_R - so.cam_R).max() < scene_tol
    assert np.abs(sg.cam_T - so.cam_T).max() < scene_tol * scale
    assert rep.iterations == 10 and rep.err_final < rep.err_initial


# ------------------------------------------------------------------ no re-upload

def test_information_set_on_a_resident_scene_equals_a_fresh_upload_bitwise():
    sc = _with_outliers(sa.config_scene("C1_dino_standin"))
    f0 = 600.0
    crit = sa.BundleAdjustmentKanataniTermCriteria()
    a, b = sa.BundleAdjustmentKanatani(0), sa.BundleAdjustmentKanatani(0)
    try:
        for h in (a, b):
            h.set_deterministic(True)
        assert a.upload(f0, sc) and a.deterministic()
        a.optimize(crit, 4)
        e = a.observation_residuals()
        # the k worst residuals switched off, at most one per landmark, only where four or more observations remain
        worst = np.argsort(-np.hypot(e[:, 0], e[:, 1]))
        lm = np.repeat(np.arange(sc.N), np.diff(sc.row_ptr))
        cnt = np.diff(sc.row_ptr)
        q = np.ones(len(e))
        used = set()
        for o in worst:
            if len(used) == 40:
                break
            if cnt[lm[o]] >= 4 and lm[o] not in used:
                used.add(lm[o])
                q[o] = 0.0
        assert len(used) == 40
        a.reset()
        before = (a.rcs_chunks(), a.jacobian_kernel(), a.frame_order())
        a.set_observation_information(q)
        after = (a.rcs_chunks(), a.jacobian_kernel(), a.frame_order())
        assert before[:2] == after[:2] and (before[2] is None) == (after[2] is None)
        if before[2] is not None:
            assert np.array_equal(before[2], after[2])
        ok_a = a.optimize(crit, 6)
        b.set_observation_information(q)
        assert b.upload(f0, sc)
        ok_b = b.optimize(crit, 6)
        assert ok_a == ok_b
        ra, rb = a.report, b.report
        assert (ra.iterations, ra.attempts, ra.err_initial, ra.err_final) == (rb.iterations, rb.attempts, rb.err_initial, rb.err_final)
        assert np.array_equal(a.iteration_log()["err"], b.iteration_log()["err"])
        for which in (B.BUF_POINTS, B.BUF_CAM_R, B.BUF_CAM_T):
            assert np.array_equal(a.buffer(which), b.buffer(which))
        # reset_scene leaves the information alone
        a.reset()
        assert np.array_equal(a.observation_information(), q)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ unit information is bitwise nothing

def _det_scene(name):
    if name == "C1_dino_standin":
        return sa.config_scene(name), 600.0
    spec = sa.SceneSpec(n_frames=30, grid_nx=33, grid_ny=31, vis_window=20)
    return sa.generate_scene(spec), spec.f0


def _staged_rows(h, sc, f0, q, kind):
    h.set_robust_loss(kind, 2.0)
    h.set_observation_information(q)
    assert h.upload(f0, sc)
    h.phase_derivatives()
    h.phase_schur(1e-4)
    out = h.buffer(B.BUF_GRAD), h.buffer(B.BUF_RCS), h.phase_error()[0]
    h.set_robust_loss(None)
    h.set_observation_information(None)
    return out


@pytest.mark.parametrize("kind", [None, "huber"])
@pytest.mark.parametrize("name", ["C1_dino_standin", "nf20_runs"])
def test_unit_information_is_bitwise_the_run_without(name, kind):
    sc, f0 = _det_scene(name)
    if kind:
        sc = _with_outliers(sc)
    ones = np.ones(int(sc.row_ptr[-1]))
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_deterministic(True)
        a = _run(h, sc, f0, None, kind, 2.0, None, None, 20)
        assert h.deterministic()
        b = _run(h, sc, f0, ones, kind, 2.0, None, None, 20)
        _same(a, b)
        for x, y in zip(_staged_rows(h, sc, f0, None, kind), _staged_rows(h, sc, f0, ones, kind)):
            assert np.array_equal(x, y)
    finally:
        h.close()


@pytest.mark.parametrize("name", ["C1_dino_standin", "nf20_runs"])
def test_default_is_bitwise_unchanged_after_information_toggling(name):
    """information set and cleared: deterministic C1 and the 30-frame run scene give the outputs the commit before fixed
    intrinsics wrote (tests/golden/default_det_before_fixed_intrinsics.npz), bit for bit."""
    g = load_golden("default_det_before_fixed_intrinsics")
    sc, f0 = _det_scene(name)
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_deterministic(True)
        _run(h, sc, f0, _information(sc), None, 2.0, None, None, 2)
        h.set_observation_information(None)
        ok, rep, sg, log, w = _run(h, sc, f0, None, None, 2.0, None, None, 20)
        assert h.deterministic() and bool(g[f"{name}__det"])
        assert np.all(w == 1.0) and np.all(h.observation_information() == 1.0)
        assert [rep.iterations, rep.attempts, rep.status] == g[f"{name}__counts"].tolist()
        assert [rep.err_initial, rep.err_final] == g[f"{name}__err"].tolist()
        assert np.array_equal(log["attempts"], g[f"{name}__attempts"]) and np.array_equal(log["err"], g[f"{name}__log_err"])
        for x in ("points", "cam_R", "cam_T"):
            assert np.array_equal(getattr(sg, x), g[f"{name}__{x}"]), x
    finally:
        h.close()


# ------------------------------------------------------------------ zero equals removed

@pytest.mark.parametrize("fv", [10, 6])
@pytest.mark.parametrize("name", ["tile_edge_nf16_runs", "ragged_20_unions"])
def test_zero_information_equals_the_scene_without_the_observations(handles, name, fv):
    make, mode, _ = SCENES[name]
    sc = _with_outliers(make())
    q = np.ones(int(sc.row_ptr[-1]))
    rng = np.random.RandomState(5)
    cnt = np.diff(sc.row_ptr)
    for i in rng.choice(np.flatnonzero(cnt >= 4), size=sc.N // 10, replace=False):
        q[sc.row_ptr[i] + rng.randint(cnt[i])] = 0.0
    drop = q == 0
    gpu = handles[fv]
    M, c = sc.M, 1e-4

    def staged(scene, info):
        gpu.set_jacobian_mode(mode)
        gpu.set_robust_loss("huber", 2.0)
        try:
            assert gpu.upload(600.0, scene)
            gpu.set_observation_information(info)
            gpu.phase_derivatives()
            out = dict(V=gpu.buffer(B.BUF_POINT_BLOCKS).reshape(-1, 3, 3), U=gpu.buffer(B.BUF_FRAME_BLOCKS).reshape(M, fv, fv),
                       g=gpu.buffer(B.BUF_GRAD), E=gpu.phase_error()[0])
            gpu.phase_schur(c)
            out.update(S=gpu.buffer(B.BUF_RCS).reshape(fv * M, fv * M), rhs=gpu.buffer(B.BUF_RCS_RHS))
            assert gpu.phase_solve()
            gpu.phase_backsub(c)
            out["corr"] = gpu.buffer(B.BUF_CORRECTIONS)
        finally:
            gpu.set_observation_information(None)
            gpu.set_robust_loss(None)
            gpu.set_jacobian_mode(-1)
        return out

    a = staged(sc, q)
    b = staged(wr.remove_observations(sc, drop), None)
    dV = np.sqrt(np.abs(np.einsum("nii->ni", b["V"])))
    dU = np.sqrt(np.abs(np.einsum("mii->mi", b["U"])))
    assert a["E"] == pytest.approx(b["E"], rel=1e-13)
    assert sym_scaled_err(a["V"], b["V"], dV) < 1e-12
    assert sym_scaled_err(a["U"], b["U"], dU) < 1e-12
    gs = 2.0 * np.sqrt(b["E"])
    dg = np.concatenate([dV.reshape(-1), dU.reshape(-1)]) * gs
    okg = dg > 0
    assert float((np.abs(a["g"] - b["g"])[okg] / dg[okg]).max()) < 1e-10
    dk = np.where(dU.reshape(-1) > 0, dU.reshape(-1), 1.0)
    assert sym_scaled_err(a["S"], b["S"], dk) < 1e-10
    assert float((np.abs(a["rhs"] - b["rhs"]) / (dk * gs)).max()) < 1e-10
    assert rel_err(a["corr"], b["corr"]) < (1e-8 if fv == 6 else 1e-7)


# ------------------------------------------------------------------ the feature's purpose

def test_information_improves_the_points_under_mixed_noise():
    """40 frames, 20 x 20 landmarks, vis window 10: half of the observations carry 0.5 px noise, half 4 px; information
    (0.5 / sigma)^2.  Only the ordering is asserted; the RMS values are printed for DESIGN.md section 12."""
    spec = sa.SceneSpec(n_frames=40, grid_nx=20, grid_ny=20, vis_window=10, noise_uv_pix=0.0)
    clean, truth, _, _ = sa.generate_scene(spec, with_gt=True)
    rng = np.random.RandomState(9)
    O = int(clean.row_ptr[-1])
    sigma = np.where(rng.rand(O) < 0.5, 0.5, 4.0)
    sc = clean.copy()
    sc.obs_uv = (np.asarray(clean.obs_uv).reshape(-1, 2) + rng.randn(O, 2) * sigma[:, None]).reshape(np.asarray(clean.obs_uv).shape)
    q = (0.5 / sigma) ** 2
    h = sa.BundleAdjustmentKanatani(0)
    rms = {}
    try:
        for key, info in (("without", None), ("with", q)):
            ok, rep, sg, log, w = _run(h, sc, spec.f0, info, None, 2.0, 1e-14, 1e6, 30)
            rms[key] = _aligned_rms(sg.points.reshape(-1, 3), truth)
    finally:
        h.close()
    print(f"point RMS against ground truth: without information {rms['without']:.6e}, with {rms['with']:.6e}")
    assert rms["with"] < rms["without"]


def _aligned_rms(P, Q):
    """RMS distance after the best similarity transform of P onto Q (the gauge is free)"""
    mp, mq = P.mean(0), Q.mean(0)
    A, Bq = P - mp, Q - mq
    U, S, Vt = np.linalg.svd(A.T @ Bq)
    d = np.sign(np.linalg.det(U @ Vt))
    D = np.diag([1.0, 1.0, d])
    R = U @ D @ Vt
    s = (S * np.diag(D)).sum() / (A * A).sum()
    return float(np.sqrt(np.mean(np.sum((s * A @ R - Bq) ** 2, axis=1))))


# ------------------------------------------------------------------ modes

def test_deterministic_runs_with_information_are_bitwise_reproducible():
    sc = _with_outliers(sa.config_scene("C1_dino_standin"))
    q = _information(sc)
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_deterministic(True)
        runs = [_run(h, sc, 600.0, q, k, 2.0, None, None, 10) for k in (None, None, "huber", "huber")]
        assert h.deterministic()
    finally:
        h.close()
    _same(runs[0], runs[1])
    _same(runs[2], runs[3])


@pytest.mark.parametrize("mode", ["f32_storage", "fp32_schur"])
def test_reduced_precision_modes_with_information_stay_close_to_fp64(mode):
    spec = sa.SceneSpec(n_frames=40, grid_nx=20, grid_ny=20, vis_window=10, noise_uv_pix=0.5)
    sc = _with_outliers(sa.generate_scene(spec))
    q = _information(sc)
    h64, hlo = sa.BundleAdjustmentKanatani(0), sa.BundleAdjustmentKanatani(0)
    try:
        getattr(hlo, "set_storage_precision" if mode == "f32_storage" else "set_schur_precision")(True)
        a = _run(h64, sc, spec.f0, q, "huber", 2.0, None, None, 6)
        b = _run(hlo, sc, spec.f0, q, "huber", 2.0, None, None, 6)
    finally:
        h64.close()
        hlo.close()
    d_err = abs(b[1].err_final - a[1].err_final) / a[1].err_final
    scale = max(1.0, float(np.abs(a[2].points).max()))
    d_scene = max(float(np.abs(a[2].points - b[2].points).max()) / scale, float(np.abs(a[2].cam_T - b[2].cam_T).max()) / scale,
                  float(np.abs(a[2].cam_R - b[2].cam_R).max()))
    print(f"{mode} with information under Huber: d_err {d_err:.2e} d_scene {d_scene:.2e}")
    assert (a[1].iterations, a[1].attempts) == (b[1].iterations, b[1].attempts)
    assert d_err < 1e-5 and d_scene < 1e-5, (d_err, d_scene)


def test_frame_reordering_with_information_matches_the_callers_order():
    sc = _with_outliers(sa.loop_scene(sa.SceneSpec(n_frames=90, grid_nx=20, grid_ny=15, vis_window=0, noise_uv_pix=0.5), window=6))
    q = _information(sc)
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_frame_reordering(1)
        a = _run(h, sc, 600.0, q, "huber", 2.0, 1e-10, 1e6, 8)
        assert h.frame_order() is not None
        h.set_frame_reordering(0)
        b = _run(h, sc, 600.0, q, "huber", 2.0, 1e-10, 1e6, 8)
        assert h.frame_order() is None
    finally:
        h.close()
    assert (a[1].iterations, a[1].attempts) == (b[1].iterations, b[1].attempts)
    assert a[1].err_final == pytest.approx(b[1].err_final, rel=1e-8)
    for x in ("points", "cam_R", "cam_T"):
        assert np.abs(getattr(a[2], x) - getattr(b[2], x)).max() < 1e-8, x
    assert np.abs(a[4] - b[4]).max() < 1e-8  # weights in the caller's order either way


def test_speculation_on_and_off_give_the_same_trajectory():
    sc = _with_outliers(sa.config_scene("C1_dino_standin"))
    q = _information(sc)
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_deterministic(True)
        h.set_speculation(True)
        a = _run(h, sc, 600.0, q, "huber", 2.0, None, None, 10)
        h.set_speculation(False)
        b = _run(h, sc, 600.0, q, "huber", 2.0, None, None, 10)
    finally:
        h.close()
    assert (a[1].iterations, a[1].attempts, a[1].status) == (b[1].iterations, b[1].attempts, b[1].status)
    assert np.array_equal(a[3]["attempts"], b[3]["attempts"])
    assert np.allclose(a[3]["err"], b[3]["err"], rtol=1e-10, atol=0)
    for x in ("points", "cam_R", "cam_T"):
        assert np.abs(getattr(a[2], x) - getattr(b[2], x)).max() < 1e-8, x


def test_two_ranks_on_one_gpu_match_world_size_one(tmp_path):
    import torch.multiprocessing as mp
    import _information_dist_worker
    spec_kwargs = dict(n_frames=30, grid_nx=23, grid_ny=17, vis_window=7, noise_uv_pix=0.5)
    iters = 3
    ref, q = _information_dist_worker.scene(spec_kwargs)
    h = sa.BundleAdjustmentKanatani(0)
    try:
        ok_ref, rep, sg, log, w = _run(h, ref, 600.0, q, "huber", 2.0, 1e-7, None, iters)
    finally:
        h.close()
    world = 2
    mp.spawn(_information_dist_worker.run, args=(world, str(tmp_path), spec_kwargs, iters), nprocs=world, join=True)
    res = [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(world)]
    for r in range(world):
        z = res[r]
        assert bool(z["ok"]) == ok_ref
        assert (int(z["iterations"]), int(z["attempts"])) == (rep.iterations, rep.attempts)
        assert float(z["err_initial"]) == pytest.approx(rep.err_initial, rel=1e-12)
        assert float(z["err_final"]) == pytest.approx(rep.err_final, rel=1e-8)
        assert np.abs(z["cam_T"] - sg.cam_T).max() < 1e-7 and np.abs(z["cam_R"] - sg.cam_R).max() < 1e-7
        lo, hi = int(z["lo"]), int(z["hi"])
        assert np.abs(z["points"] - sg.points[lo:hi]).max() < 1e-7
        o0, o1 = int(ref.row_ptr[lo]), int(ref.row_ptr[hi])
        assert np.abs(z["weights"] - w[o0:o1]).max() < 1e-9  # local: this rank's observations
        assert z["residuals"].shape == (o1 - o0, 2)


# ------------------------------------------------------------------ ABI

def test_information_setter_refusals_and_round_trip():
    sc = sa.generate_scene(sa.SceneSpec(n_frames=12, grid_nx=10, grid_ny=10, vis_window=5))
    other = sa.generate_scene(sa.SceneSpec(n_frames=12, grid_nx=9, grid_ny=10, vis_window=5))
    O = int(sc.row_ptr[-1])
    assert int(other.row_ptr[-1]) != O
    q = _information(sc)
    h = sa.BundleAdjustmentKanatani(0)
    try:
        with pytest.raises(RuntimeError):
            h.observation_residuals()  # no scene yet
        assert h.upload(600.0, sc)
        assert np.array_equal(h.observation_information(), np.ones(O))  # none set: all 1
        h.set_observation_information(q)
        assert np.array_equal(h.observation_information(), q)
        one_left = q.copy()
        one_left[sc.row_ptr[3]:sc.row_ptr[4]] = 0.0
        one_left[sc.row_ptr[3]] = 1.0
        for bad, word in ((-1.0, "negative"), (float("nan"), "finite"), (float("inf"), "finite")):
            b = q.copy()
            b[5] = bad
            with pytest.raises(ValueError):
                h.set_observation_information(b)
            assert word in h.last_error()
            assert np.array_equal(h.observation_information(), q)  # the previous setting stays in force
        with pytest.raises(ValueError):
            h.set_observation_information(q[:-1])
        assert "observations" in h.last_error()
        with pytest.raises(ValueError):
            h.set_observation_information(one_left)
        assert "landmark 3" in h.last_error() and "fewer than two" in h.last_error()
        assert np.array_equal(h.observation_information(), q)
        # ... on the device as well: the energy is still that of q
        so_e = float(np.sum(q * np.sum((h.observation_residuals() / 600.0) ** 2, axis=1)))
        assert h.phase_error()[0] == pytest.approx(so_e, rel=1e-12)
        # another number of observations: the upload is refused while the information is set, fine once it is cleared
        with pytest.raises(ValueError):
            h.upload(600.0, other)
        assert "observations" in h.last_error()
        h.set_observation_information(None)
        assert h.upload(600.0, other)
        assert np.all(h.observation_information() == 1.0)
    finally:
        h.close()


def test_cpp_adapter_set_observation_information(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "information_adapter"
    r = subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "demos"),
                        os.path.join(HERE, "cpp", "test_information_adapter.cpp"), "-o", str(exe),
                        "-L", os.path.join(ROOT, "surikatoko_amd"), "-lsrk_ba",
                        "-Wl,-rpath," + os.path.join(ROOT, "surikatoko_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "information adapter ok" in r.stdout
