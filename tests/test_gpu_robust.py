"""Robust bundle adjustment on the GPU (srk_ba_set_robust_loss: Huber / Cauchy, IRLS weights in every derivative pass)
against the yardstick of tests/robust_ref.py -- numpy residuals and Jacobians weighted per observation, the oracle's own
two-phase step on those blocks, and the LM loop of bundle-adj-kanatani.cpp:720-893 on E = sum rho(s).

Tolerances as the parity tests: blocks 1e-12 per variable class, reduced camera system 1e-10 class-scaled, E 1e-13
relative; corrections 1e-8 with six frame variables and 1e-7 with ten, whose intrinsic columns make the system far worse
conditioned (the parity tests' corr_tol for the same kernels).  End to end the same accept / reject sequence; E per
iteration 1e-10 and the scene 1e-8 with six frame variables, 1e-8 and 1e-7 with ten.
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import ba as B
from conftest import load_golden, rel_err, sym_scaled_err, class_rel_err
import calibrated_ref as cref
import lm_trajectory as lt
import robust_ref as rr
from gpu_common import orc_scene as _orc_scene

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = {rr.HUBER: "huber", rr.CAUCHY: "cauchy"}


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


def _phases(orc, gpu, sc, f0, kind, delta, fv, c, jac_mode):
    """derivatives -> schur -> solve -> backsub -> accept on both sides, checked; returns the derivative kernel used"""
    so = _orc_scene(orc, sc)
    assert orc.normalize(so)[0]
    gpu.set_jacobian_mode(jac_mode)
    gpu.set_robust_loss(NAMES[kind], delta)
    assert gpu.upload(f0, sc) and gpu.frame_vars() == fv
    N, M = sc.N, sc.M
    ref = rr.step(orc, f0, so, c, kind, delta, fv=fv, want_system=True)
    wts = ref["weights"]
    if kind == rr.HUBER:
        assert np.any(wts == 1.0) and np.any(wts < 0.5)  # both branches of Huber
    E0 = rr.energy(f0, so, kind, delta)
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
    gs = 2.0 * np.sqrt(max(E0, 1e-300))
    dg = np.concatenate([dV.reshape(-1), dU.reshape(-1)]) * gs
    okg = dg > 0
    assert float((np.abs(gg - go)[okg] / dg[okg]).max()) < 1e-10
    # the weights the caller sees: the yardstick's, in the caller's order
    assert np.abs(gpu.observation_weights() - wts).max() < 1e-12
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
    assert e1g == pytest.approx(rr.energy(f0, so, kind, delta), rel=corr_tol)  # after a step: the corrections' tolerance
    gpu.set_robust_loss(None)
    gpu.set_jacobian_mode(-1)
    return kernel


SCENES = {
    # name: (scene, jacobian mode, derivative kernel expected)
    "tile_edge_nf16_runs": (lambda: sa.generate_scene(sa.SceneSpec(n_frames=24, grid_nx=30, grid_ny=20, vis_window=16)), 1, 2),
    "ragged_20_unions": (lambda: sa.drop_observations(sa.generate_scene(sa.SceneSpec(n_frames=60, grid_nx=40, grid_ny=30,
                                                                                      vis_window=20)), 0.15, seed=5), 2, 3),
    "long_nf40_per_observation": (lambda: sa.generate_scene(sa.SceneSpec(n_frames=60, grid_nx=12, grid_ny=10, vis_window=50)), 0, 0),
    "small_fused": (lambda: sa.generate_scene(sa.SceneSpec(n_frames=12, grid_nx=10, grid_ny=10, vis_window=5)), 0, 1),
}


@pytest.mark.parametrize("fv", [10, 6])
@pytest.mark.parametrize("kind", [rr.HUBER, rr.CAUCHY])
@pytest.mark.parametrize("name", list(SCENES))
def test_robust_phases_vs_yardstick(orc, handles, name, kind, fv):
    make, mode, kernel = SCENES[name]
    sc = _with_outliers(make())
    if name.startswith("long"):
        assert np.diff(sc.row_ptr).max() > 32
    got = _phases(orc, handles[fv], sc, 600.0, kind, 2.0, fv, 1e-4, mode)
    assert got == kernel


@pytest.mark.parametrize("fv", [10, 6])
def test_robust_phases_c2(orc, handles, fv):
    spec = sa.CONFIGS["C2_200cam_20kpt"]
    sc = _with_outliers(sa.config_scene("C2_200cam_20kpt"))
    _phases(orc, handles[fv], sc, spec.f0, rr.HUBER, 2.0, fv, 1e-4, -1)


# ------------------------------------------------------------------ end to end

def _run(gpu, sc, f0, kind=None, delta=2.0, allowed=None, max_factor=None, max_iterations=0):
    crit = sa.BundleAdjustmentKanataniTermCriteria()
    crit.AllowedReprojErrRelativeChange(allowed)
    crit.MaxHessianFactor(max_factor)
    gpu.set_robust_loss(kind, delta)
    sg = sc.copy()
    try:
        ok = gpu.ComputeInplace(f0, sg, crit, max_iterations)
    finally:
        w = gpu.observation_weights()
        gpu.set_robust_loss(None)
    return ok, gpu.report, sg, gpu.iteration_log(), w


def _same_as_yardstick(orc, gpu, sc, f0, kind, delta=2.0, skyline=False, fv=10, **kw):
    so = _orc_scene(orc, sc)
    rc_o, rep_o = rr.compute_inplace(orc, f0, so, kind, delta, kw.get("allowed"), kw.get("max_factor"),
                                     kw.get("max_iterations", 0), fv=fv, skyline=skyline)
    ok, rep, sg, log, w = _run(gpu, sc, f0, NAMES.get(kind), delta, **kw)
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
    assert np.abs(w - rr.weights(f0, so, kind, delta)).max() < 10 * scene_tol  # weights at scenes that agree to scene_tol
    return rep


E2E = {
    "C1": lambda: (sa.config_scene("C1_dino_standin"), 600.0),
    "ragged": lambda: (sa.drop_observations(sa.generate_scene(sa.SceneSpec(n_frames=30, grid_nx=23, grid_ny=17, vis_window=7,
                                                                          noise_uv_pix=0.5)), 0.25, seed=3), 600.0),
}


@pytest.mark.parametrize("fv", [10, 6])
@pytest.mark.parametrize("kind", [rr.HUBER, rr.CAUCHY])
@pytest.mark.parametrize("name", list(E2E))
def test_robust_ten_iterations_vs_python_lm_loop(orc, handles, name, kind, fv):
    sc, f0 = E2E[name]()
    sc = _with_outliers(sc, 0.05, seed=11)
    rep = _same_as_yardstick(orc, handles[fv], sc, f0, kind, fv=fv, max_iterations=10)
    assert rep.iterations == 10 and rep.err_final < rep.err_initial


def test_robust_c3_three_iterations_vs_skyline_yardstick(orc, handles):
    spec = sa.CONFIGS["C3_1kcam_100kpt"]
    sc = _with_outliers(sa.config_scene("C3_1kcam_100kpt"), 0.02, seed=3)
    threads = orc.get_threads()
    orc.set_threads(8)
    try:
        rep = _same_as_yardstick(orc, handles[10], sc, spec.f0, rr.HUBER, skyline=True, max_iterations=3)
    finally:
        orc.set_threads(threads)
    assert rep.iterations == 3


# ------------------------------------------------------------------ the default stays as it is

@pytest.mark.parametrize("name", ["C1_dino_standin", "nf20_runs"])
def test_default_is_bitwise_unchanged_after_robust_toggling(name):
    """Huber set and then cleared before the upload: deterministic C1 and the 30-frame run scene give the outputs the commit
    before fixed intrinsics wrote (tests/golden/default_det_before_fixed_intrinsics.npz), bit for bit."""
    g = load_golden("default_det_before_fixed_intrinsics")
    if name == "C1_dino_standin":
        sc, f0 = sa.config_scene(name), 600.0
    else:
        spec = sa.SceneSpec(n_frames=30, grid_nx=33, grid_ny=31, vis_window=20)
        sc, f0 = sa.generate_scene(spec), spec.f0
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_robust_loss("huber", 2.0)
        assert h.robust_loss() == ("huber", 2.0)
        h.set_robust_loss(None)
        assert h.robust_loss() == (None, 0.0)
        h.set_deterministic(True)
        ok, rep, sg, log, w = _run(h, sc, f0, None, 2.0, None, None, 20)
        assert h.deterministic() and bool(g[f"{name}__det"])
        assert np.all(w == 1.0)
        assert [rep.iterations, rep.attempts, rep.status] == g[f"{name}__counts"].tolist()
        assert [rep.err_initial, rep.err_final] == g[f"{name}__err"].tolist()
        assert np.array_equal(log["attempts"], g[f"{name}__attempts"]) and np.array_equal(log["err"], g[f"{name}__log_err"])
        for x in ("points", "cam_R", "cam_T"):
            assert np.array_equal(getattr(sg, x), g[f"{name}__{x}"]), x
    finally:
        h.close()


@pytest.mark.parametrize("name", ["C1_dino_standin", "nf20_runs"])
def test_huber_above_every_residual_is_bitwise_plain_least_squares(name):
    """Below Huber's threshold w is exactly 1 and rho(s) is s itself; the robust kernels fold w and sqrt(w) into scale
    factors they multiply anyway (a multiply by 1.0 is exact) and sum rho(s) where the plain kernels sum s, so a threshold
    above every residual reproduces the plain run bit for bit (deterministic mode: ordered sums)."""
    if name == "C1_dino_standin":
        sc, f0 = sa.config_scene(name), 600.0
    else:
        spec = sa.SceneSpec(n_frames=30, grid_nx=33, grid_ny=31, vis_window=20)
        sc, f0 = sa.generate_scene(spec), spec.f0
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_deterministic(True)
        a = _run(h, sc, f0, None, 2.0, None, None, 20)
        b = _run(h, sc, f0, "huber", 1e9, None, None, 20)
    finally:
        h.close()
    assert np.all(b[4] == 1.0)
    assert (a[1].iterations, a[1].attempts, a[1].status) == (b[1].iterations, b[1].attempts, b[1].status)
    assert (a[1].err_initial, a[1].err_final) == (b[1].err_initial, b[1].err_final)
    assert np.array_equal(a[3]["attempts"], b[3]["attempts"]) and np.array_equal(a[3]["err"], b[3]["err"])
    for x in ("points", "cam_R", "cam_T"):
        assert np.array_equal(getattr(a[2], x), getattr(b[2], x)), x


# ------------------------------------------------------------------ modes

def test_deterministic_robust_runs_are_bitwise_reproducible():
    sc = _with_outliers(sa.config_scene("C1_dino_standin"))
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_deterministic(True)
        runs = [_run(h, sc, 600.0, k, 2.0, None, None, 10) for k in ("huber", "huber", "cauchy", "cauchy")]
    finally:
        h.close()
    for a, b in ((runs[0], runs[1]), (runs[2], runs[3])):
        assert (a[1].iterations, a[1].attempts, a[1].err_final) == (b[1].iterations, b[1].attempts, b[1].err_final)
        assert np.array_equal(a[3]["err"], b[3]["err"]) and np.array_equal(a[4], b[4])
        for x in ("points", "cam_R", "cam_T"):
            assert np.array_equal(getattr(a[2], x), getattr(b[2], x)), x


@pytest.mark.parametrize("mode", ["f32_storage", "fp32_schur"])
def test_reduced_precision_modes_under_huber_stay_close_to_fp64(mode):
    spec = sa.SceneSpec(n_frames=40, grid_nx=20, grid_ny=20, vis_window=10, noise_uv_pix=0.5)
    sc = _with_outliers(sa.generate_scene(spec))
    h64, hlo = sa.BundleAdjustmentKanatani(0), sa.BundleAdjustmentKanatani(0)
    try:
        getattr(hlo, "set_storage_precision" if mode == "f32_storage" else "set_schur_precision")(True)
        a = _run(h64, sc, spec.f0, "huber", 2.0, None, None, 6)
        b = _run(hlo, sc, spec.f0, "huber", 2.0, None, None, 6)
    finally:
        h64.close()
        hlo.close()
    d_err = abs(b[1].err_final - a[1].err_final) / a[1].err_final
    scale = max(1.0, float(np.abs(a[2].points).max()))
    d_scene = max(float(np.abs(a[2].points - b[2].points).max()) / scale, float(np.abs(a[2].cam_T - b[2].cam_T).max()) / scale,
                  float(np.abs(a[2].cam_R - b[2].cam_R).max()))
    print(f"{mode} under Huber: d_err {d_err:.2e} d_scene {d_scene:.2e}")
    assert (a[1].iterations, a[1].attempts) == (b[1].iterations, b[1].attempts)
    assert d_err < 1e-5 and d_scene < 1e-5, (d_err, d_scene)


def test_frame_reordering_on_a_loop_closure_scene_matches_the_callers_order():
    sc = _with_outliers(sa.loop_scene(sa.SceneSpec(n_frames=90, grid_nx=20, grid_ny=15, vis_window=0, noise_uv_pix=0.5),
                                      window=6))
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_frame_reordering(1)
        a = _run(h, sc, 600.0, "huber", 2.0, 1e-10, 1e6, 8)
        assert h.frame_order() is not None
        h.set_frame_reordering(0)
        b = _run(h, sc, 600.0, "huber", 2.0, 1e-10, 1e6, 8)
        assert h.frame_order() is None
    finally:
        h.close()
    assert (a[1].iterations, a[1].attempts) == (b[1].iterations, b[1].attempts)
    assert a[1].err_final == pytest.approx(b[1].err_final, rel=1e-8)
    for x in ("points", "cam_R", "cam_T"):
        assert np.abs(getattr(a[2], x) - getattr(b[2], x)).max() < 1e-8, x
    assert np.abs(a[4] - b[4]).max() < 1e-8  # weights in the caller's order either way


def test_two_ranks_on_one_gpu_match_world_size_one(tmp_path):
    import torch.multiprocessing as mp
    import _robust_dist_worker
    spec_kwargs = dict(n_frames=30, grid_nx=23, grid_ny=17, vis_window=7, noise_uv_pix=0.5)
    iters = 3
    ref = _robust_dist_worker.scene(spec_kwargs)
    h = sa.BundleAdjustmentKanatani(0)
    try:
        ok_ref, rep, sg, log, w = _run(h, ref, 600.0, "huber", 2.0, 1e-7, None, iters)
    finally:
        h.close()
    world = 2
    mp.spawn(_robust_dist_worker.run, args=(world, str(tmp_path), spec_kwargs, iters), nprocs=world, join=True)
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
        # the weights are local: this rank's observations
        o0, o1 = int(ref.row_ptr[lo]), int(ref.row_ptr[hi])
        assert np.abs(z["weights"] - w[o0:o1]).max() < 1e-9


# ------------------------------------------------------------------ the feature's purpose: outliers

def test_huber_rejects_injected_outliers():
    """40 frames, 20 x 20 landmarks, vis window 10, 0.5 px noise; 5 % of the observations moved by 20 - 60 px.  The CPU
    yardstick (tests/robust_ref.py, 30 iterations) gave: plain least squares leaves the inliers at 3.33 px RMS; Huber
    (delta 2 px) brings them to 0.75 px (the noise itself: 0.71 px); every outlier has w <= 0.10 and 99.7 % of the inliers
    w = 1.  Thresholds: plain > 2 px, Huber < 1 px, outliers w < 0.2, inliers w = 1 for >= 95 %."""
    spec = sa.SceneSpec(n_frames=40, grid_nx=20, grid_ny=20, vis_window=10, noise_uv_pix=0.5)
    sc = sa.generate_scene(spec)
    # frame numbers shuffled (the gauge frames stay 0 and 1): the library renumbers them internally
    perm = np.concatenate([[0, 1], 2 + np.random.RandomState(0).permutation(sc.M - 2)])
    sc = sa.renumber_frames(sc, perm)
    idx = rr.inject_outliers(sc, 0.05, 20, 60, seed=7)
    inl = np.ones(int(sc.row_ptr[-1]), bool)
    inl[idx] = False
    h = sa.BundleAdjustmentKanatani(0)
    try:
        # the weights must come back in the caller's order through the internal renumbering
        res = {}
        for kind in (None, "huber"):
            ok, rep, sg, log, w = _run(h, sc, spec.f0, kind, 2.0, 1e-12, 1e6, 30)
            assert h.frame_order() is not None
            so = _orc_scene_np(sg)
            ex, ey = rr.residuals(spec.f0, so)
            pix = spec.f0 * np.sqrt(ex * ex + ey * ey)
            res[kind] = (float(np.sqrt(np.mean(pix[inl] ** 2))), w)
    finally:
        h.close()
    print(f"inlier RMS: plain {res[None][0]:.3f} px, Huber {res['huber'][0]:.3f} px")
    assert res[None][0] > 2.0
    assert res["huber"][0] < 1.0
    w = res["huber"][1]
    assert np.all(w[idx] < 0.2)
    assert np.mean(w[inl] == 1.0) >= 0.95
    assert np.all(res[None][1] == 1.0)


def _orc_scene_np(sc):
    class _S:
        pass
    s = _S()
    s.points, s.cam_R, s.cam_T, s.K = sc.points.reshape(-1, 3), sc.cam_R.reshape(-1, 9), sc.cam_T.reshape(-1, 3), sc.K
    s.shared_k, s.row_ptr, s.obs_frame, s.obs_uv = sc.shared_k, sc.row_ptr, sc.obs_frame, sc.obs_uv.reshape(-1, 2)
    s.N, s.M, s.O = s.points.shape[0], s.cam_R.shape[0], int(sc.row_ptr[-1])
    return s


# ------------------------------------------------------------------ ABI

def test_robust_loss_setter_refusals_and_round_trip():
    h = sa.BundleAdjustmentKanatani(0)
    try:
        assert h.robust_loss() == (None, 0.0)
        for kind, delta in (("huber", 0.0), ("huber", -1.0), ("cauchy", float("nan")), ("huber", float("inf"))):
            with pytest.raises(ValueError):
                h.set_robust_loss(kind, delta)
            assert "delta" in h.last_error()
        with pytest.raises(ValueError):
            h.set_robust_loss("tukey", 1.0)
        L = h._lib
        import ctypes as C
        assert L.srk_ba_set_robust_loss(C.c_void_p(h._h), 3, 1.0) == -1 and "kind" in h.last_error()
        assert L.srk_ba_set_robust_loss(C.c_void_p(h._h), -1, 1.0) == -1
        assert h.robust_loss() == (None, 0.0)  # refusals leave the loss as it was
        h.set_robust_loss("cauchy", 3.5)
        assert h.robust_loss() == ("cauchy", 3.5)
        h.set_robust_loss("huber", 1.25)
        assert h.robust_loss() == ("huber", 1.25)
        with pytest.raises(RuntimeError):
            h.observation_weights()  # no scene yet
        h.set_robust_loss(None)
        assert h.robust_loss() == (None, 0.0)
    finally:
        h.close()


def test_cpp_adapter_set_robust_loss(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "robust_adapter"
    r = subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "demos"),
                        os.path.join(HERE, "cpp", "test_robust_adapter.cpp"), "-o", str(exe),
                        "-L", os.path.join(ROOT, "surikatoko_amd"), "-lsrk_ba",
                        "-Wl,-rpath," + os.path.join(ROOT, "surikatoko_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "robust adapter ok" in r.stdout
