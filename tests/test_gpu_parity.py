"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same inputs.

Tolerances (fp64): per-element blocks rel 1e-12 of the block scale; reduced camera system and rhs
rel 1e-10 (reordered sums, fp64 atomics); one-step corrections rel 1e-8 (Cholesky vs Householder QR);
end-to-end: same accept/reject sequence, final error rel 1e-6, scene abs 1e-6 in normalised units.
"""
import os
import sys

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import ba as B
from conftest import load_golden, rel_err, sym_scaled_err, class_rel_err
import lm_trajectory as lt
from gpu_common import orc_scene as _orc_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    h = sa.BundleAdjustmentKanatani(0)
    yield h
    h.close()


def _golden_scene(name):
    g = load_golden(name)
    return sa.Scene(g["in_points"], g["in_cam_R"], g["in_cam_T"], g["in_K"], 0, g["in_row_ptr"], g["in_obs_frame"],
                    g["in_obs_uv"]), float(g["f0"]), g


def _reduced_index(M, comp=1):
    """full frame variable -> reduced index (or -1), bundle-adj-kanatani.cpp:539-563."""
    red = np.full(10 * M, -1, dtype=np.int64)
    r = 0
    for fi in range(10 * M):
        if 4 <= fi <= 9 or fi == 14 + comp:
            continue
        red[fi] = r
        r += 1
    return red


SCENES = {
    "tiny": sa.SceneSpec(n_frames=5, grid_nx=4, grid_ny=3, vis_window=3),
    "all_visible": sa.SceneSpec(n_frames=8, grid_nx=5, grid_ny=5, vis_window=0),       # the demo's visibility
    "ragged_wave": sa.SceneSpec(n_frames=30, grid_nx=23, grid_ny=17, vis_window=7),    # segments straddle waves
    "long_tracks": sa.SceneSpec(n_frames=90, grid_nx=6, grid_ny=5, vis_window=80),     # > one LDS chunk per landmark
    "pixel_noise": sa.SceneSpec(n_frames=12, grid_nx=10, grid_ny=10, vis_window=5, noise_uv_pix=0.5),
}


def _phases(orc, gpu, sc, f0, c, already_normalized=False):
    """Run derivatives -> schur -> solve -> backsub on both sides; return both sets of intermediates."""
    so = _orc_scene(orc, sc)
    if not already_normalized:
        ok, _ = orc.normalize(so)
        assert ok
    assert gpu.upload(f0, sc, already_normalized=already_normalized)
    out = {}
    out["err_o"], out["seen_o"] = orc.reproj_error(f0, so)
    out["err_g"], out["seen_g"] = gpu.phase_error()
    gradE, V, U, W = orc.derivatives(f0, so)
    gpu.phase_derivatives()
    out.update(gradE_o=gradE, V_o=V, U_o=U, W_o=W, gradE_g=gpu.buffer(B.BUF_GRAD),
               V_g=gpu.buffer(B.BUF_POINT_BLOCKS).reshape(-1, 3, 3), U_g=gpu.buffer(B.BUF_FRAME_BLOCKS).reshape(-1, 10, 10),
               W_g=gpu.buffer(B.BUF_POINT_FRAME).reshape(-1, 3, 10))
    ok, corr, S, rhs = orc.two_phase(so, gradE, V, U, W, c, want_system=True)
    gpu.phase_schur(c)
    M = sc.M
    Sg = gpu.buffer(B.BUF_RCS).reshape(10 * M, 10 * M)
    rg = gpu.buffer(B.BUF_RCS_RHS)
    out.update(ok_o=ok, corr_o=corr, S_o=S, rhs_o=rhs, S_g=Sg, rhs_g=rg)
    out["ok_g"] = gpu.phase_solve()
    gpu.phase_backsub(c)
    out["corr_g"] = gpu.buffer(B.BUF_CORRECTIONS)
    orc.apply_corrections(so, corr)
    gpu.phase_accept()
    out.update(pts_o=so.points, R_o=so.cam_R, T_o=so.cam_T, pts_g=gpu.buffer(B.BUF_POINTS).reshape(-1, 3),
               R_g=gpu.buffer(B.BUF_CAM_R).reshape(-1, 9), T_g=gpu.buffer(B.BUF_CAM_T).reshape(-1, 3))
    out["err2_o"], _ = orc.reproj_error(f0, so)
    out["err2_g"], _ = gpu.phase_error()
    return out


def _check_blocks_by_class(V_g, V_o, U_g, U_o, W_g, W_o, gradE_g, gradE_o, err):
    """Derivative blocks on the scale of each variable class (conftest: per-variable-class metrics): point and frame
    blocks with rows / columns scaled by 1 / sqrt(diag) of the oracle's block (1e-12: the u0 / v0 and the intrinsics x
    intrinsics entries are pinned to 1e-12 of THEIR scale, not of the pose entries'), point-frame blocks per (point
    coordinate, frame variable) class (1e-12), gradient entries on their Cauchy-Schwarz scale 2 sqrt(E B_aa) (1e-10)."""
    N, M = V_o.shape[0], U_o.shape[0]
    dV = np.sqrt(np.abs(np.einsum("nii->ni", V_o)))
    dU = np.sqrt(np.abs(np.einsum("mii->mi", U_o)))
    assert sym_scaled_err(V_g, V_o, dV) < 1e-12
    assert sym_scaled_err(U_g, U_o, dU) < 1e-12
    assert class_rel_err(W_g, W_o, (1, 2)) < 1e-12
    gs = 2.0 * np.sqrt(max(err, 1e-300))
    dg = np.concatenate([dV.reshape(-1), dU.reshape(-1)]) * gs
    ok = dg > 0
    assert float((np.abs(gradE_g - gradE_o)[ok] / dg[ok]).max()) < 1e-10
    return dU.reshape(-1)


def _check_system_by_class(S_g, S_o, rhs_g, rhs_o, dU_keep, err, tol=1e-10):
    """Reduced camera system and right-hand side with every row / column on the scale of its variable: divided by
    sqrt(diag) of the oracle's (undamped) frame blocks -- the magnitude of the terms the Schur sums add up."""
    assert sym_scaled_err(S_g, S_o, dU_keep) < tol
    gs = 2.0 * np.sqrt(max(err, 1e-300))
    ok = dU_keep > 0
    assert float((np.abs(rhs_g - rhs_o)[ok] / (dU_keep[ok] * gs)).max()) < tol


def _check(out, M, corr_tol=1e-8):
    assert out["seen_g"] == out["seen_o"]
    assert out["err_g"] == pytest.approx(out["err_o"], rel=1e-12)
    assert rel_err(out["V_g"], out["V_o"]) < 1e-12
    assert rel_err(out["W_g"], out["W_o"]) < 1e-12
    assert rel_err(out["U_g"], out["U_o"]) < 1e-12
    assert rel_err(out["gradE_g"], out["gradE_o"]) < 1e-10  # sums with cancellation
    red = _reduced_index(M)
    keep = red >= 0
    Sg = out["S_g"][np.ix_(keep, keep)]
    assert rel_err(Sg, out["S_o"]) < 1e-10
    assert rel_err(out["rhs_g"][keep], out["rhs_o"]) < 1e-10
    # the same, every entry on the scale of its own variable class
    dU = _check_blocks_by_class(out["V_g"], out["V_o"], out["U_g"], out["U_o"], out["W_g"], out["W_o"], out["gradE_g"],
                                out["gradE_o"], out["err_o"])
    _check_system_by_class(Sg, out["S_o"], out["rhs_g"][keep], out["rhs_o"], dU[keep], out["err_o"])
    # gauge-fixed variables: identity rows, zero rhs
    fixed = np.where(~keep)[0]
    for f in fixed:
        row = out["S_g"][f].copy()
        assert row[f] == 1.0
        row[f] = 0
        assert np.all(row == 0) and out["rhs_g"][f] == 0
    assert out["ok_o"], "oracle solve failed"
    assert out["ok_g"], "GPU solve failed"
    # Cholesky (GPU) vs Householder QR (oracle, as in the reference) on the same system.  QR on the unscaled system
    # loses digits when intrinsics and pose variables live on very different scales (cond ~1e14 on some scenes),
    # so the yardstick is the exact solution of the ORACLE's system (iterative refinement in long double):
    # the GPU must be at least as close to it as the reference's own solver, and within corr_tol when both are good.
    So, ro = out["S_o"], out["rhs_o"]
    x = np.linalg.solve(So, ro)
    Sl, rl = So.astype(np.longdouble), ro.astype(np.longdouble)
    for _ in range(6):
        x = x + np.linalg.solve(So, (rl - Sl @ x.astype(np.longdouble)).astype(np.float64))
    N3 = len(out["corr_g"]) - 10 * M
    d_qr = rel_err(out["corr_o"][N3:][keep], x)
    d_gpu = rel_err(out["corr_g"][N3:][keep], x)
    dsc = 1.0 / np.sqrt(np.abs(np.diag(So)))
    cond_scaled = float(np.linalg.cond(So * dsc[:, None] * dsc[None, :]))
    assert d_gpu < max(1e-9, 100 * np.finfo(np.float64).eps * cond_scaled), (d_gpu, d_qr, cond_scaled)
    tol = max(corr_tol, 4 * d_qr)
    assert tol < 1e-3, f"reference solver itself is off by {d_qr:.2e} on this scene"
    assert rel_err(out["corr_g"], out["corr_o"]) < tol
    N3 = len(out["corr_g"]) - 10 * M
    fr = out["corr_g"][N3:]
    assert np.all(fr[4:10] == 0) and fr[15] == 0  # exact zero gaps (:1618-1654)
    scale = max(1.0, float(np.abs(out["pts_o"]).max()))
    assert np.abs(out["pts_g"] - out["pts_o"]).max() < max(1e-8, tol) * scale
    assert np.abs(out["R_g"] - out["R_o"]).max() < max(1e-8, tol)
    assert np.abs(out["T_g"] - out["T_o"]).max() < max(1e-8, tol) * scale
    assert out["err2_g"] == pytest.approx(out["err2_o"], rel=max(1e-6, 10 * tol))


# ------------------------------------------------------------------ kernels one by one

def test_dense_spd_solve_mfma(gpu):
    """blocked Cholesky with the fp64 MFMA trailing update vs numpy; checks the f64 16x16x4 accumulator map."""
    rng = np.random.RandomState(3)
    for n in (1, 7, 64, 65, 130, 200, 513):
        A = rng.randn(n, n)
        A = A @ A.T + n * np.eye(n)
        A += np.diag(np.arange(n) * 0.37)  # asymmetric-looking spectrum: a transposed tile map would show
        b = rng.randn(n)
        ok, x, _ = gpu.dense_spd_solve(A, b)
        assert ok
        assert np.abs(x - np.linalg.solve(A, b)).max() < 1e-10 * max(1.0, np.abs(x).max())


def test_dense_spd_solve_rejects_indefinite(gpu):
    A = np.eye(70)
    A[40, 40] = -1.0
    ok, _, _ = gpu.dense_spd_solve(A, np.ones(70))
    assert not ok


@pytest.mark.parametrize("case", ["pyproto_case_a", "pyproto_case_b"])
@pytest.mark.parametrize("c", [1e-4, 1e-1])
def test_phases_on_golden_inputs(orc, gpu, case, c):
    sc, f0, g = _golden_scene(case)
    out = _phases(orc, gpu, sc, f0, c)
    _check(out, sc.M, corr_tol=1e-6 if c < 1e-3 else 1e-8)
    # and against the Python prototype's own numbers (committed golden fixtures)
    N, M = sc.N, sc.M
    assert rel_err(out["V_g"].reshape(3 * N, 3), g["deriv_second_point"]) < 1e-12
    assert rel_err(out["U_g"].reshape(10 * M, 10), g["deriv_second_frame"]) < 1e-12
    assert rel_err(out["gradE_g"], g["gradE"]) < 1e-10
    tag = {1e-4: "c1e-4", 1e-1: "c1e-1"}[c]
    assert rel_err(out["corr_g"], g["corrections_" + tag]) < (1e-6 if c < 1e-3 else 1e-8)


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("c", [1e-4, 10.0])
def test_phases_on_synthetic_scenes(orc, gpu, name, c):
    sc = sa.generate_scene(SCENES[name])
    out = _phases(orc, gpu, sc, SCENES[name].f0, c)
    _check(out, sc.M, corr_tol=1e-7)


def test_tracks_over_more_than_256_frames_take_the_mfma_long_track_kernel(orc, gpu):
    """An all-visible scene of 270 frames (every track in every frame, as the reference's demos build their scenes): tracks
    over more than 256 frames used to fall back to the per-landmark global-atomics kernel; k_schur_long now takes any frame
    set.  Blocks, reduced camera system (2693^2) and right-hand side against the oracle (its QR of that system is skipped: the
    Schur sum is what is under test), then one iteration of the LM loop must decrease the error."""
    spec = sa.SceneSpec(n_frames=270, grid_nx=8, grid_ny=6, vis_window=0)
    sc = sa.generate_scene(spec)
    so = _orc_scene(orc, sc)
    ok, _ = orc.normalize(so)
    assert ok and gpu.upload(spec.f0, sc)
    e0, _ = gpu.phase_error()
    eo, _ = orc.reproj_error(spec.f0, so)
    assert e0 == pytest.approx(eo, rel=1e-12)
    gradE, V, U, W = orc.derivatives(spec.f0, so)
    gpu.phase_derivatives()
    dU = _check_blocks_by_class(gpu.buffer(B.BUF_POINT_BLOCKS).reshape(-1, 3, 3), V, gpu.buffer(B.BUF_FRAME_BLOCKS).reshape(-1, 10, 10), U,
                                gpu.buffer(B.BUF_POINT_FRAME).reshape(-1, 3, 10), W, gpu.buffer(B.BUF_GRAD), gradE, eo)
    orc.set_skip_solve(True)
    try:
        _, _, S, rhs = orc.two_phase(so, gradE, V, U, W, 1e-3, want_system=True)
    finally:
        orc.set_skip_solve(False)
    gpu.phase_schur(1e-3)
    keep = _reduced_index(sc.M) >= 0
    Sg = gpu.buffer(B.BUF_RCS).reshape(10 * sc.M, 10 * sc.M)[np.ix_(keep, keep)]
    rg = gpu.buffer(B.BUF_RCS_RHS)[keep]
    assert rel_err(Sg, S) < 1e-10 and rel_err(rg, rhs) < 1e-10
    _check_system_by_class(Sg, S, rg, rhs, dU[keep], eo)
    assert gpu.phase_solve()
    # and one accepted iteration of the library's own loop (whatever damping factor it needs) decreases the error
    assert gpu.upload(spec.f0, sc)
    gpu.optimize(None, max_iterations=1)
    assert gpu.report.iterations == 1 and gpu.report.err_final < gpu.report.err_initial


# ------------------------------------------------------------------ the run-based derivative kernel (k_jac_runs)

JAC_RUN_SCENES = {
    # one wave per task of <= 36 landmarks with identical frame lists; 64 // nf landmarks per iteration
    "nf20": sa.SceneSpec(n_frames=30, grid_nx=33, grid_ny=31, vis_window=20),       # 3 landmarks / iteration, 60 active lanes
    "nf16": sa.SceneSpec(n_frames=24, grid_nx=30, grid_ny=20, vis_window=16),       # 4 / iteration, every lane active
    "nf13": sa.SceneSpec(n_frames=15, grid_nx=17, grid_ny=13, vis_window=13),       # 4 / iteration, 52 lanes
    "nf3_many_per_iteration": sa.SceneSpec(n_frames=12, grid_nx=25, grid_ny=20, vis_window=3),  # 21 / iteration: 189 sums in 3 passes
    "nf2": sa.SceneSpec(n_frames=6, grid_nx=9, grid_ny=7, vis_window=2),            # 32 / iteration
    "nf40_one_per_iteration": sa.SceneSpec(n_frames=44, grid_nx=12, grid_ny=10, vis_window=40),
    "all_visible_nf8": sa.SceneSpec(n_frames=8, grid_nx=9, grid_ny=9, vis_window=0),  # one run of 81 landmarks
    "pixel_noise": sa.SceneSpec(n_frames=12, grid_nx=10, grid_ny=10, vis_window=5, noise_uv_pix=0.5),
}


@pytest.mark.parametrize("name", list(JAC_RUN_SCENES))
def test_run_based_derivative_kernel_vs_oracle(orc, gpu, name):
    """k_jac_runs (a lane keeps one frame's 65 sums in registers over a task; landmark sums in a fixed order through a
    per-wave scratch) forced on small scenes: blocks rel 1e-12, gradient rel 1e-10 against the oracle, and the whole
    chain behind it (bundle-adj-kanatani.cpp:1140-1448)."""
    spec = JAC_RUN_SCENES[name]
    sc = sa.generate_scene(spec)
    gpu.set_jacobian_mode(1)
    try:
        out = _phases(orc, gpu, sc, spec.f0, 1e-4)
        assert gpu.jacobian_kernel() == 2
        _check(out, sc.M, corr_tol=1e-7)
    finally:
        gpu.set_jacobian_mode(-1)


def test_run_based_derivative_kernel_on_golden_inputs_and_ragged_tracks(orc, gpu):
    """The prototype's golden blocks through k_jac_runs; and ragged tracks (every landmark a run of its own: tasks of
    one landmark) still give the oracle's blocks."""
    gpu.set_jacobian_mode(1)
    try:
        for case in ("pyproto_case_a", "pyproto_case_b"):
            sc, f0, g = _golden_scene(case)
            out = _phases(orc, gpu, sc, f0, 1e-1)
            assert gpu.jacobian_kernel() == 2
            _check(out, sc.M, corr_tol=1e-8)
            N, M = sc.N, sc.M
            assert rel_err(out["V_g"].reshape(3 * N, 3), g["deriv_second_point"]) < 1e-12
            assert rel_err(out["U_g"].reshape(10 * M, 10), g["deriv_second_frame"]) < 1e-12
            assert rel_err(out["gradE_g"], g["gradE"]) < 1e-10
        spec = sa.SceneSpec(n_frames=30, grid_nx=23, grid_ny=17, vis_window=7)
        sc = sa.drop_observations(sa.generate_scene(spec), 0.25, seed=3)
        out = _phases(orc, gpu, sc, spec.f0, 1e-4)
        assert gpu.jacobian_kernel() == 2
        _check(out, sc.M, corr_tol=1e-7)
    finally:
        gpu.set_jacobian_mode(-1)


UNION_RUN_SCENES = {
    # tasks = pieces of the Schur kernel's runs over the UNION of their landmarks' frame lists; a lane per (landmark, slot) cell
    "ragged_7": lambda: sa.drop_observations(sa.generate_scene(sa.SceneSpec(n_frames=30, grid_nx=23, grid_ny=17, vis_window=7)), 0.25, seed=3),
    "ragged_20": lambda: sa.drop_observations(sa.generate_scene(sa.SceneSpec(n_frames=60, grid_nx=40, grid_ny=30, vis_window=20)), 0.15, seed=5),
    "ragged_13_noise": lambda: sa.drop_observations(sa.generate_scene(sa.SceneSpec(n_frames=40, grid_nx=30, grid_ny=20, vis_window=13, noise_uv_pix=0.4)), 0.4, seed=7),
    "uniform_nf16": lambda: sa.generate_scene(JAC_RUN_SCENES["nf16"]),             # full masks: the uniform case of the same code
    "uniform_nf3": lambda: sa.generate_scene(JAC_RUN_SCENES["nf3_many_per_iteration"]),
    "two_observations_each": lambda: sa.drop_observations(sa.generate_scene(sa.SceneSpec(n_frames=20, grid_nx=15, grid_ny=12, vis_window=9)), 0.9, seed=1),
    # tracks over 25 .. 32 frames (round 4): the Schur sums take k_schur_long's runs, which do not cover the shorter tracks --
    # the derivative kernel forms runs of its own over unions of <= 32 frames (one mask word)
    "ragged_28_own_runs": lambda: sa.drop_observations(sa.generate_scene(sa.SceneSpec(n_frames=48, grid_nx=40, grid_ny=30, vis_window=28, noise_uv_pix=0.3)), 0.15, seed=9),
    "mixed_12_to_30_own_runs": lambda: sa.drop_observations(sa.generate_scene(sa.SceneSpec(n_frames=48, grid_nx=40, grid_ny=30, vis_window=30)), 0.35, seed=11),
    "uniform_nf32_own_runs": lambda: sa.generate_scene(sa.SceneSpec(n_frames=40, grid_nx=30, grid_ny=20, vis_window=32)),
}


@pytest.mark.parametrize("name", list(UNION_RUN_SCENES))
@pytest.mark.parametrize("c", [1e-4, 10.0])
def test_run_based_derivative_kernel_over_frame_unions_vs_oracle(orc, gpu, name, c):
    """Ragged tracks through k_jac_runs<MASKED>: blocks rel 1e-12, gradient rel 1e-10 against the oracle and the whole chain
    behind it (bundle-adj-kanatani.cpp:1140-1448); automatic mode picks this form when uniform runs are too short to pay."""
    sc = UNION_RUN_SCENES[name]()
    gpu.set_jacobian_mode(2)
    try:
        out = _phases(orc, gpu, sc, 600.0, c)
        assert gpu.jacobian_kernel() == 3
        if name.endswith("own_runs"):
            assert np.diff(sc.row_ptr).max() > 24        # some tracks are beyond the Schur kernels' runs
        _check(out, sc.M, corr_tol=1e-7)
    finally:
        gpu.set_jacobian_mode(-1)


def test_automatic_mode_takes_the_union_form_on_ragged_tracks_of_bench_density(gpu):
    """200 frames, 20 000 landmarks, 20-frame tracks with 10 % of the observations dropped: hardly two landmarks see the same
    frames (uniform tasks of one or two landmarks), the union tasks hold ~100.  The two derivative kernels agree."""
    sc = sa.drop_observations(sa.config_scene("C2_200cam_20kpt"), 0.1, seed=0)
    f0 = sa.CONFIGS["C2_200cam_20kpt"].f0
    res = {}
    for mode in (-1, 0):
        gpu.set_jacobian_mode(mode)
        assert gpu.upload(f0, sc)
        res[mode] = gpu.jacobian_kernel()
        gpu.phase_error()
        gpu.phase_derivatives()
        res[mode, "V"] = gpu.buffer(B.BUF_POINT_BLOCKS)
        res[mode, "U"] = gpu.buffer(B.BUF_FRAME_BLOCKS)
        res[mode, "W"] = gpu.buffer(B.BUF_POINT_FRAME)
        res[mode, "g"] = gpu.buffer(B.BUF_GRAD)
    gpu.set_jacobian_mode(-1)
    assert res[-1] == 3 and res[0] in (0, 1)
    assert rel_err(res[-1, "W"], res[0, "W"]) < 1e-13
    assert rel_err(res[-1, "V"], res[0, "V"]) < 1e-13 and rel_err(res[-1, "U"], res[0, "U"]) < 1e-12
    assert rel_err(res[-1, "g"], res[0, "g"]) < 1e-10


def test_derivative_kernels_agree_at_bench_size(gpu):
    """BASELINE config 3 (the bench workload): the run-based kernel (picked automatically there) and the per-observation
    fused kernel give the same blocks to rounding (different summation orders), landmark by landmark."""
    spec = sa.CONFIGS["C3_1kcam_100kpt"]
    sc = sa.config_scene("C3_1kcam_100kpt")
    res = {}
    try:
        for mode in (-1, 0):
            gpu.set_jacobian_mode(mode)
            assert gpu.upload(spec.f0, sc)
            assert gpu.jacobian_kernel() == (2 if mode == -1 else 1)
            gpu.phase_derivatives()
            res[mode] = (gpu.buffer(B.BUF_GRAD).copy(), gpu.buffer(B.BUF_POINT_BLOCKS).copy(),
                         gpu.buffer(B.BUF_FRAME_BLOCKS).copy(), gpu.buffer(B.BUF_POINT_FRAME)[::97].copy())
    finally:
        gpu.set_jacobian_mode(-1)
    for a, b, tol in zip(res[-1], res[0], (1e-10, 1e-12, 1e-11, 1e-12)):
        assert rel_err(a, b) < tol


MFMA_EDGES = {
    # k_schur_mm sums a run as a (10 nf) x (10 nf) x (3 np) fp64 MFMA product over 16x16 tiles and rounds of four
    # landmarks: frame counts whose 10 nf is / is not a multiple of 16, runs that are not a multiple of four landmarks
    # long, groups split into several runs (> 128 landmarks), one- and two-frame runs
    "nf16_10_tiles": sa.SceneSpec(n_frames=24, grid_nx=30, grid_ny=20, vis_window=16),   # 160 = 10 tiles exactly; runs of 64..68
    "nf20_split_runs": sa.SceneSpec(n_frames=23, grid_nx=33, grid_ny=31, vis_window=20), # 200 -> 13 tiles; groups of 255 / 256
    "nf13": sa.SceneSpec(n_frames=15, grid_nx=17, grid_ny=13, vis_window=13),            # 130 -> 9 tiles; runs of 73 / 74
    "nf2_short_runs": sa.SceneSpec(n_frames=6, grid_nx=9, grid_ny=7, vis_window=2),      # one tile row; runs of 10..15
}


@pytest.mark.parametrize("name", list(MFMA_EDGES))
@pytest.mark.parametrize("c", [1e-4, 10.0])
def test_phases_on_mfma_tile_edges(orc, gpu, name, c):
    sc = sa.generate_scene(MFMA_EDGES[name])
    out = _phases(orc, gpu, sc, MFMA_EDGES[name].f0, c)
    _check(out, sc.M, corr_tol=1e-7)


RAGGED = {
    # ragged feature tracks: observations dropped at random, so that hardly two landmarks see the same frames and the
    # grouped Schur kernel works on unions of frame lists (zero blocks where a landmark misses a frame of its run)
    "ragged_short": (sa.SceneSpec(n_frames=30, grid_nx=23, grid_ny=17, vis_window=7), 0.25),
    "ragged_20": (sa.SceneSpec(n_frames=60, grid_nx=40, grid_ny=30, vis_window=20, noise_uv_pix=0.3), 0.15),  # unions reach 21
    "ragged_wide": (sa.SceneSpec(n_frames=50, grid_nx=24, grid_ny=20, vis_window=23), 0.10),            # 22..24 frames: two half blocks per thread
    "ragged_long": (sa.SceneSpec(n_frames=60, grid_nx=12, grid_ny=10, vis_window=40), 0.30),              # > 24 frames: per-landmark kernel
}


@pytest.mark.parametrize("name", list(RAGGED))
@pytest.mark.parametrize("c", [1e-4, 10.0])
def test_phases_on_ragged_tracks(orc, gpu, name, c):
    spec, frac = RAGGED[name]
    sc = sa.drop_observations(sa.generate_scene(spec), frac, seed=7)
    lists = {sc.obs_frame[sc.row_ptr[i]:sc.row_ptr[i + 1]].tobytes() for i in range(sc.N)}
    assert len(lists) > sc.N // 4  # really ragged
    out = _phases(orc, gpu, sc, spec.f0, c)
    _check(out, sc.M, corr_tol=1e-7)


LONG_TRACKS = {
    # k_schur_long: tracks over more than 24 frames, summed per pair of 8-frame blocks as fp64 MFMA products.  Frame sets
    # that are / are not a whole number of blocks, the shortest long track, the longest a run holds (256 frames), a track beyond that
    # (per-landmark kernel), runs that are not a multiple of eight landmarks, several runs, ragged unions
    "demo_circle_grid_36": (sa.SceneSpec(n_frames=36, grid_nx=9, grid_ny=9, vis_window=0), 0.0),     # the demo's 81 x 36, all visible
    "mvf_60_two_runs": (sa.SceneSpec(n_frames=60, grid_nx=15, grid_ny=13, vis_window=0), 0.0),       # 195 landmarks: runs of 128 + 67
    "nf25": (sa.SceneSpec(n_frames=27, grid_nx=7, grid_ny=5, vis_window=25), 0.0),
    "nf64_whole_blocks": (sa.SceneSpec(n_frames=64, grid_nx=5, grid_ny=4, vis_window=0), 0.0),
    "nf128_many_pairs": (sa.SceneSpec(n_frames=128, grid_nx=4, grid_ny=3, vis_window=0), 0.0),
    "nf256_full_run": (sa.SceneSpec(n_frames=256, grid_nx=3, grid_ny=3, vis_window=0), 0.0),
    "nf260_beyond_a_run": (sa.SceneSpec(n_frames=260, grid_nx=3, grid_ny=2, vis_window=0), 0.0),
    "ragged_40": (sa.SceneSpec(n_frames=70, grid_nx=14, grid_ny=12, vis_window=40, noise_uv_pix=0.3), 0.25),
    "mixed_short_and_long": (sa.SceneSpec(n_frames=48, grid_nx=12, grid_ny=10, vis_window=30), 0.35),  # tracks of 12..30 frames
}


@pytest.mark.parametrize("name", list(LONG_TRACKS))
@pytest.mark.parametrize("c", [1e-4, 10.0])
def test_phases_on_long_tracks(orc, gpu, name, c):
    spec, frac = LONG_TRACKS[name]
    sc = sa.generate_scene(spec)
    if frac > 0:
        sc = sa.drop_observations(sc, frac, seed=11)
    nf = np.diff(sc.row_ptr)
    assert nf.max() > 24
    out = _phases(orc, gpu, sc, spec.f0, c)
    _check(out, sc.M, corr_tol=1e-7)


def test_ragged_tracks_end_to_end(orc, gpu):
    spec, frac = RAGGED["ragged_20"]
    sc = sa.drop_observations(sa.generate_scene(spec), frac, seed=3)
    rc_o, rep_o, so, ok, rep, sg = _end_to_end(orc, gpu, sc, spec.f0, allowed=1e-7, max_factor=1e6, max_iterations=5)
    assert ok == (rc_o == 0)
    assert (rep.iterations, rep.attempts) == (rep_o.iterations, rep_o.attempts)
    lt.assert_same_trajectory(gpu.iteration_log(), rep_o.log, 1e-6, gpu_attempts=rep.attempts)
    assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-6)
    assert np.abs(sg.points - so.points).max() < 1e-6


def test_singular_point_blocks_are_skipped(orc, gpu):
    """A landmark whose damped 3x3 block has |det| <= 1e-12 is skipped in the Schur sum and gets a zero correction
    (bundle-adj-kanatani.cpp:1876-1881, 1939-1943).  Far-away landmarks have tiny derivatives (det ~ depth^-6).
    Landmarks seen once are NOT singular under the multiplicative damping and must still agree with the oracle."""
    sc = sa.generate_scene(sa.SceneSpec(n_frames=6, grid_nx=5, grid_ny=4, vis_window=3))
    keep = np.ones(sc.O, dtype=bool)
    for i in (0, 7, 19):   # three landmarks cut down to a single observation
        keep[sc.row_ptr[i] + 1:sc.row_ptr[i + 1]] = False
    counts = np.array([keep[sc.row_ptr[i]:sc.row_ptr[i + 1]].sum() for i in range(sc.N)])
    pts = sc.points.copy()
    far = (3, 11)
    for i in far:          # two landmarks pushed ~1e4 scene units away
        pts[i] = pts[i] * 3e3 + np.array([2e4, -1e4, 3e4])
    sc2 = sa.Scene(pts, sc.cam_R, sc.cam_T, sc.K, 0, np.concatenate([[0], np.cumsum(counts)]),
                   sc.obs_frame[keep], sc.obs_uv[keep])
    out = _phases(orc, gpu, sc2, 600.0, 1e-4)
    _check(out, sc2.M, corr_tol=1e-7)
    for i in far:
        assert abs(np.linalg.det(out["V_o"][i])) < 1e-12
        assert np.all(out["corr_g"][3 * i:3 * i + 3] == 0)
        assert np.all(out["corr_o"][3 * i:3 * i + 3] == 0)
    for i in (0, 7, 19):
        assert np.any(out["corr_o"][3 * i:3 * i + 3] != 0)


def _without_frame(sc, frame):
    keep = sc.obs_frame != frame
    counts = np.add.reduceat(keep.astype(np.int64), sc.row_ptr[:-1])
    return sa.Scene(sc.points, sc.cam_R, sc.cam_T, sc.K, sc.shared_k, np.concatenate([[0], np.cumsum(counts)]),
                    sc.obs_frame[keep], sc.obs_uv[keep])


def test_failed_solve_is_hessian_overflow_as_in_the_reference_and_leaves_no_residue(orc, gpu):
    """When does the Cholesky that replaces the reference's Householder QR (bundle-adj-kanatani.cpp:1911) fail, and what
    happens then?  The damping is multiplicative on both diagonals (:1818-1819, :1830-1831), so the reduced system is
    >= c diag(G): scaled to a unit diagonal its smallest eigenvalue is >= c >= 1e-4 and a pivot cannot turn
    non-positive through rounding.  A pivot fails only where diag(G) holds an exact zero -- e.g. a frame that observes
    nothing -- and there the reference's QR divides by a zero diagonal entry of R, its solution is not finite
    (:1912-1913) and ComputeInplace ends with "hessian overflow" after that one attempt.  Chosen behaviour = the same:
    status, result, iteration and attempt counts of the oracle's QR restatement.
    The failed factorisation leaves NaNs in the slot's matrices (also outside the parts a later attempt rewrites): the
    next run on the same handle -- after a reset and after a fresh upload -- must be clean."""
    spec = sa.SceneSpec(n_frames=7, grid_nx=6, grid_ny=5, vis_window=4)
    good = sa.generate_scene(spec)
    bad = _without_frame(good, 4)
    assert np.diff(bad.row_ptr).min() >= 2
    rc_o, rep_o, so, ok, rep, sg = _end_to_end(orc, gpu, bad, spec.f0, allowed=1e-12, max_factor=1e6, max_iterations=30)
    assert rc_o == 1 and orc.status_string(rep_o.status) == "hessian overflow"
    assert not ok and sa.status_string(rep.status) == "hessian overflow"
    assert (rep.iterations, rep.attempts) == (rep_o.iterations, rep_o.attempts) == (0, 1)
    lt.assert_same_trajectory(gpu.iteration_log(), rep_o.log, 1e-6, gpu_attempts=rep.attempts)
    assert rep.err_final == rep.err_initial == pytest.approx(rep_o.err_initial, rel=1e-12)
    # the scene is handed back unchanged (up to the normalise / revert round trip), as the reference restores its backup
    assert np.abs(sg.points - bad.points).max() < 1e-9 and np.abs(sg.cam_T - bad.cam_T).max() < 1e-9
    # same handle, same (failing) scene again after a reset: still the same answer, no crash
    gpu.reset()
    assert not gpu.optimize(None, max_iterations=5) and gpu.OptimizationStatusString() == "hessian overflow"
    # and a good scene afterwards runs exactly as on a fresh handle: nothing of the failed solve survives
    rc_o, rep_o, so, ok, rep, sg = _end_to_end(orc, gpu, good, spec.f0, allowed=1e-12, max_factor=1e6, max_iterations=30)
    assert ok == (rc_o == 0) and sa.status_string(rep.status) == orc.status_string(rep_o.status)
    assert (rep.iterations, rep.attempts) == (rep_o.iterations, rep_o.attempts)
    lt.assert_same_trajectory(gpu.iteration_log(), rep_o.log, 1e-6, gpu_attempts=rep.attempts, err_abs=1e-18)
    assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-6, abs=1e-18)
    assert np.abs(sg.points - so.points).max() < 1e-6


def test_failed_solve_on_a_loop_closure_scene_then_reset(orc, gpu):
    """a non-monotone skyline (the last frames see the landmarks of the first ones: a loop closure) makes
    k_panel sweep rows whose own skyline starts further right; after a failed factorisation those rows hold NaNs outside
    what the next attempt rewrites.  Staged calls: fail a solve, then repair the scene on the same handle (upload keeps
    the allocations) and compare a full run with the oracle."""
    spec = sa.SceneSpec(n_frames=40, grid_nx=12, grid_ny=10, vis_window=6)
    sc = sa.generate_scene(spec)
    # loop closure: the landmarks of the first window are also seen by the last two frames
    rp, fr, uv = sc.row_ptr, sc.obs_frame, sc.obs_uv
    sc_gt, pts_gt, Rg, Tg = sa.generate_scene(spec, with_gt=True)
    f_new, uv_new, cnt = [], [], []
    for i in range(sc.N):
        o = slice(rp[i], rp[i + 1])
        f_i, uv_i = list(fr[o]), [tuple(x) for x in uv[o]]
        if fr[rp[i]] == 0:
            for j in (38, 39):
                if j not in f_i:
                    X = Rg[j].reshape(3, 3) @ pts_gt[i] + Tg[j]
                    Kj = sc.K[j].reshape(3, 3)
                    p = Kj @ X
                    f_i.append(j)
                    uv_i.append((spec.f0 * p[0] / p[2], spec.f0 * p[1] / p[2]))
        order = np.argsort(f_i)
        f_new += [f_i[k] for k in order]
        uv_new += [uv_i[k] for k in order]
        cnt.append(len(f_i))
    loop = sa.Scene(sc.points, sc.cam_R, sc.cam_T, sc.K, 0, np.concatenate([[0], np.cumsum(cnt)]),
                    np.array(f_new, dtype=np.int32), np.array(uv_new))
    bad = _without_frame(loop, 20)
    assert gpu.upload(spec.f0, bad)
    gpu.phase_derivatives()
    gpu.phase_schur(1e-4)
    assert not gpu.phase_solve()          # zero pivot in frame 20's block
    rc_o, rep_o, so, ok, rep, sg = _end_to_end(orc, gpu, loop, spec.f0, allowed=1e-10, max_factor=1e6, max_iterations=6)
    assert ok == (rc_o == 0) and sa.status_string(rep.status) == orc.status_string(rep_o.status)
    assert (rep.iterations, rep.attempts) == (rep_o.iterations, rep_o.attempts) and rep.iterations >= 1
    lt.assert_same_trajectory(gpu.iteration_log(), rep_o.log, 1e-6, gpu_attempts=rep.attempts, err_abs=1e-18)
    assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-6, abs=1e-18)
    assert np.abs(sg.points - so.points).max() < 1e-6


def test_indefinite_matrix_is_reported_by_the_solver(gpu):
    """The solver itself: a symmetric matrix with one slightly negative eigenvalue is reported (info), never 'solved'."""
    rng = np.random.RandomState(5)
    n = 200
    Q, _ = np.linalg.qr(rng.randn(n, n))
    ev = np.linspace(1.0, 3.0, n)
    ev[17] = -1e-6
    A = (Q * ev) @ Q.T
    A = 0.5 * (A + A.T)
    ok, x, _ = gpu.dense_spd_solve(A, rng.randn(n))
    assert not ok
    ev[17] = 1e-6                          # barely positive definite: solved, to the accuracy its conditioning allows
    A = (Q * ev) @ Q.T
    A = 0.5 * (A + A.T)
    b = rng.randn(n)
    ok, x, _ = gpu.dense_spd_solve(A, b)
    assert ok and np.abs(A @ x - b).max() < 1e-8 * np.abs(x).max()


def test_shared_k_mode(orc, gpu):
    """multi-view-factorization call contract: shared K, f0 = 1 (multi-view-factorization.cpp:387-391)."""
    sc = sa.generate_scene(sa.SceneSpec(n_frames=7, grid_nx=6, grid_ny=4, vis_window=4, f0=1.0))
    sc1 = sa.Scene(sc.points, sc.cam_R, sc.cam_T, sc.K[0:1], 1, sc.row_ptr, sc.obs_frame, sc.obs_uv)
    out = _phases(orc, gpu, sc1, 1.0, 1e-4)
    _check(out, sc1.M, corr_tol=1e-7)


# ------------------------------------------------------------------ end to end

def _end_to_end(orc, gpu, sc, f0, allowed=None, max_factor=None, max_iterations=0):
    so = _orc_scene(orc, sc)
    rc_o, rep_o, rep_o.log = orc.compute_inplace(f0, so, allowed, max_factor, max_iterations, want_log=True)
    crit = sa.BundleAdjustmentKanataniTermCriteria()
    crit.AllowedReprojErrRelativeChange(allowed)
    crit.MaxHessianFactor(max_factor)
    sg = sc.copy()
    ok = gpu.ComputeInplace(f0, sg, crit, max_iterations)
    return rc_o, rep_o, so, ok, gpu.report, sg


@pytest.mark.parametrize("name,allowed,max_it", [("tiny", 1e-12, 0), ("all_visible", 1e-12, 0),
                                                  ("ragged_wave", 1e-7, 40), ("pixel_noise", 1e-12, 0)])
def test_compute_inplace_matches_oracle(orc, gpu, name, allowed, max_it):
    spec = SCENES[name]
    sc = sa.generate_scene(spec)
    rc_o, rep_o, so, ok, rep, sg = _end_to_end(orc, gpu, sc, spec.f0, allowed=allowed, max_factor=1e6,
                                               max_iterations=max_it)
    assert ok == (rc_o == 0)
    assert sa.status_string(rep.status) == orc.status_string(rep_o.status)
    assert rep.seen == rep_o.seen
    assert rep.err_initial == pytest.approx(rep_o.err_initial, rel=1e-12)
    # identical accept / reject sequence (a fork on a near tie would show here)
    assert (rep.iterations, rep.attempts) == (rep_o.iterations, rep_o.attempts)
    lt.assert_same_trajectory(gpu.iteration_log(), rep_o.log, 1e-6, gpu_attempts=rep.attempts, err_abs=1e-18)
    assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-6, abs=1e-18)
    assert np.abs(sg.points - so.points).max() < 1e-6
    assert np.abs(sg.cam_R - so.cam_R).max() < 1e-6
    assert np.abs(sg.cam_T - so.cam_T).max() < 1e-6
    assert rep.err_final < rep.err_initial


def test_compute_inplace_iteration_cap_and_report(orc, gpu):
    spec = SCENES["ragged_wave"]
    sc = sa.generate_scene(spec)
    gpu.set_profile(1)  # phase events fill report.ms_* (and serialise the attempts)
    try:
        rc_o, rep_o, so, ok, rep, sg = _end_to_end(orc, gpu, sc, spec.f0, max_iterations=2)
    finally:
        gpu.set_profile(0)
    assert not ok and rc_o == 1
    assert sa.status_string(rep.status) == "max iterations" == orc.status_string(rep_o.status)
    assert rep.iterations == 2 == rep_o.iterations and rep.attempts == rep_o.attempts
    lt.assert_same_trajectory(gpu.iteration_log(), rep_o.log, 1e-6, gpu_attempts=rep.attempts)
    assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-6)
    assert rep.ms_jacobian > 0 and rep.ms_schur > 0 and rep.ms_solve > 0
    assert np.abs(sg.points - so.points).max() < 1e-6


def test_abs_err_threshold_early_out(orc, gpu):
    """err_initial < threshold -> true, 'abs err threshold', scene untouched up to the normalise/revert round trip
    (bundle-adj-kanatani.cpp:749-753)."""
    spec = sa.SceneSpec(n_frames=5, grid_nx=3, grid_ny=3, vis_window=3, noise_x3d_hi=0.0, noise_r_hi=0.0)
    sc = sa.generate_scene(spec)
    crit = sa.BundleAdjustmentKanataniTermCriteria()
    crit.AllowedReprojErrRelativeChange(1e-5)
    sg = sc.copy()
    assert gpu.ComputeInplace(spec.f0, sg, crit)
    assert gpu.OptimizationStatusString() == "abs err threshold"
    assert gpu.report.iterations == 0
    assert np.abs(sg.points - sc.points).max() < 1e-12


def test_normalisation_failure_returns_false(gpu):
    """cam0 and cam1 at the same height along y: T01[y] ~ 0 -> ComputeInplace returns false, status string empty
    (bundle-adj-kanatani.cpp:215-217, 681-682)."""
    spec = sa.SceneSpec(n_frames=4, grid_nx=3, grid_ny=3, vis_window=0)
    sc = sa.generate_scene(spec)
    sc.cam_R[1] = sc.cam_R[0]
    sc.cam_T[1] = sc.cam_T[0] + np.array([0.3, 0.0, 0.0])
    before = sc.copy()
    assert gpu.ComputeInplace(spec.f0, sc) is False
    assert gpu.OptimizationStatusString() == ""
    assert np.array_equal(sc.points, before.points)


def test_argument_errors(gpu):
    spec = SCENES["tiny"]
    sc = sa.generate_scene(spec)
    with pytest.raises(ValueError):       # CHECK(!IsClose(0, f0)) :420
        gpu.ComputeInplace(0.0, sc.copy())
    bad = sc.copy()
    bad.obs_frame[1], bad.obs_frame[0] = bad.obs_frame[0], bad.obs_frame[1]
    with pytest.raises(ValueError):
        gpu.ComputeInplace(600.0, bad)
    one = sa.Scene(sc.points, sc.cam_R[:1], sc.cam_T[:1], sc.K[:1], 0, sc.row_ptr, np.zeros_like(sc.obs_frame), sc.obs_uv)
    with pytest.raises(ValueError):       # needs M >= 2
        gpu.ReprojError(600.0, one)


def test_reproj_error_api(orc, gpu):
    spec = SCENES["ragged_wave"]
    sc = sa.generate_scene(spec)
    e, seen = gpu.ReprojError(spec.f0, sc)
    eo, so = orc.reproj_error(spec.f0, _orc_scene(orc, sc))
    assert seen == so == sc.O
    assert e == pytest.approx(eo, rel=1e-12)
    assert gpu.ReprojErrorPixPerPoint(e, seen) == pytest.approx(spec.f0 * np.sqrt(eo / so), rel=1e-12)


# ------------------------------------------------------------------ BASELINE configs 1 and 2 at full size vs the oracle

@pytest.mark.parametrize("dense_literal", [False, True])
def test_c1_dino_standin_end_to_end_vs_oracle(orc, gpu, dense_literal):
    """BASELINE config 1 (demo-dino: 36 cams / 4983 pts / 16432 obs; the labelled synthetic stand-in, the oxfvisgeom
    files are not in the reference tree) end to end with the dino flagfile's criteria (--f0=600
    --allowed_repr_err=4.56e-8, cpp_impl/flagfile-demo-dino.txt:6-11; call at demo-bundle-adj-dinosaur.cpp:232-238)
    against the oracle, once with its block-sparse storage and once with the reference's literal dense storage and
    per-point n x n product (bundle-adj-kanatani.cpp:581,1891; n = 353): same result, status, iteration / attempt
    counts, error rel 1e-6, scene abs 1e-6."""
    sc = sa.config_scene("C1_dino_standin")
    assert (sc.M, sc.N, sc.O) == (36, 4983, 16432)
    so = _orc_scene(orc, sc)
    rc_o, rep_o, rep_o.log = orc.compute_inplace(600.0, so, 4.56e-8, None, 0, dense_literal=dense_literal, want_log=True)
    crit = sa.BundleAdjustmentKanataniTermCriteria()
    crit.AllowedReprojErrRelativeChange(4.56e-8)
    sg = sc.copy()
    ok = gpu.ComputeInplace(600.0, sg, crit)
    rep = gpu.report
    assert ok == (rc_o == 0)
    assert sa.status_string(rep.status) == orc.status_string(rep_o.status) == "small relative err change"
    assert rep.seen == rep_o.seen == 16432
    assert rep.err_initial == pytest.approx(rep_o.err_initial, rel=1e-12)
    assert (rep.iterations, rep.attempts) == (rep_o.iterations, rep_o.attempts)
    lt.assert_same_trajectory(gpu.iteration_log(), rep_o.log, 1e-6, gpu_attempts=rep.attempts)
    assert rep.iterations >= 10
    assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-6)
    assert np.abs(sg.points - so.points).max() < 1e-6
    assert np.abs(sg.cam_R - so.cam_R).max() < 1e-6
    assert np.abs(sg.cam_T - so.cam_T).max() < 1e-6


def test_c2_full_size_blocks_system_and_one_iteration_vs_oracle(orc, gpu):
    """BASELINE config 2 (200 cams / 20k pts / 400k obs) at full size against the oracle: derivative blocks rel 1e-12,
    reduced camera system (n = 1993) and rhs rel 1e-10, corrections against the exact solution of the oracle's system,
    the updated scene and its error; then one accepted LM iteration through the library's own loop with the same
    attempt count and error as the oracle's loop."""
    spec = sa.CONFIGS["C2_200cam_20kpt"]
    sc = sa.config_scene("C2_200cam_20kpt")
    assert (sc.M, sc.N, sc.O) == (200, 20000, 400000)
    out = _phases(orc, gpu, sc, spec.f0, 1e-4)
    _check(out, sc.M)
    rc_o, rep_o, so, ok, rep, sg = _end_to_end(orc, gpu, sc, spec.f0, max_iterations=1)
    assert not ok and rc_o == 1 and sa.status_string(rep.status) == "max iterations"
    assert (rep.iterations, rep.attempts) == (rep_o.iterations, rep_o.attempts) and rep.iterations == 1
    lt.assert_same_trajectory(gpu.iteration_log(), rep_o.log, 1e-6, gpu_attempts=rep.attempts)
    assert rep.err_initial == pytest.approx(rep_o.err_initial, rel=1e-12)
    assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-6)
    assert np.abs(sg.points - so.points).max() < 1e-6
    assert np.abs(sg.cam_R - so.cam_R).max() < 1e-6
    assert np.abs(sg.cam_T - so.cam_T).max() < 1e-6


def test_c2_ten_iterations_end_to_end_vs_the_oracle_loop(orc, gpu):
    """BASELINE config 2 at full size END TO END (SURVEY 8d asks for the same accept / reject sequence on configs 1 and 2):
    ten accepted LM iterations through the library's loop against the oracle's restatement of
    ComputeOnNormalizedWorld (bundle-adj-kanatani.cpp:720-893) with its skyline Cholesky (orc.set_solver(1): the same Schur
    arithmetic term by term, pinned against the literal QR path by tests/test_oracle_skyline.py; the 1993^2 Householder QR
    would take a minute an attempt): same iterations, attempts and status, error rel 1e-6, scene abs 1e-6."""
    spec = sa.CONFIGS["C2_200cam_20kpt"]
    sc = sa.config_scene("C2_200cam_20kpt")
    orc.set_solver(1)
    threads = orc.get_threads()
    orc.set_threads(8)
    try:
        rc_o, rep_o, so, ok, rep, sg = _end_to_end(orc, gpu, sc, spec.f0, max_iterations=10)
    finally:
        orc.set_solver(0)
        orc.set_threads(threads)
    assert not ok and rc_o == 1 and sa.status_string(rep.status) == orc.status_string(rep_o.status) == "max iterations"
    assert rep.iterations == rep_o.iterations == 10
    assert rep.attempts == rep_o.attempts and rep.attempts > rep.iterations      # some attempts were rejected on the way
    lt.assert_same_trajectory(gpu.iteration_log(), rep_o.log, 1e-6, gpu_attempts=rep.attempts)
    assert rep.err_initial == pytest.approx(rep_o.err_initial, rel=1e-12)
    assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-6)
    assert np.abs(sg.points - so.points).max() < 1e-6
    assert np.abs(sg.cam_R - so.cam_R).max() < 1e-6
    assert np.abs(sg.cam_T - so.cam_T).max() < 1e-6
    log = gpu.iteration_log()
    assert len(log["attempts"]) == 10 and int(log["attempts"].sum()) == rep.attempts
    assert np.all(np.diff(log["err"]) < 0) and log["err"][-1] == rep.err_final


def test_c2_all_visible_full_size_blocks_system_and_corrections_vs_oracle(orc, gpu):
    """Config 2 in the shape the reference's own demo produces (demo-bundle-adj-circle-grid.cpp:196-207 projects every
    point into every frame; SURVEY 8d: "one run with full visibility O = 4e6"): 200 frames x 20 000 points, every track 200
    frames long (k_schur_long: the MFMA kernel over pairs of 8-frame blocks), a DENSE reduced camera system of 1993
    variables.  At full size against the oracle: error, gradient, all blocks (rel 1e-12 / 1e-10 and per variable class), the
    WHOLE reduced system and right-hand side (rel 1e-10, class-scaled 1e-10) and the corrections of the step against the
    oracle's Cholesky on the same system (rel 1e-8); then one LM iteration through both loops."""
    import os
    spec = sa.CONFIGS["C2_all_visible"]
    sc = sa.generate_scene(spec)
    assert (sc.M, sc.N, sc.O) == (200, 20000, 4000000)
    so = _orc_scene(orc, sc)
    ok, _ = orc.normalize(so)
    assert ok and gpu.upload(spec.f0, sc)
    M, c = sc.M, 1e-4
    threads = orc.get_threads()
    orc.set_threads(max(1, min(32, (os.cpu_count() or 2) // 2)))
    try:
        eo, seen_o = orc.reproj_error(spec.f0, so)
        eg, seen_g = gpu.phase_error()
        assert seen_g == seen_o == sc.O and eg == pytest.approx(eo, rel=1e-12)
        gradE, V, U, W = orc.derivatives(spec.f0, so)
        gpu.phase_derivatives()
        Vg_, Ug_, gg_ = (gpu.buffer(B.BUF_POINT_BLOCKS).reshape(-1, 3, 3), gpu.buffer(B.BUF_FRAME_BLOCKS).reshape(-1, 10, 10),
                         gpu.buffer(B.BUF_GRAD))
        assert rel_err(Vg_, V) < 1e-12 and rel_err(Ug_, U) < 1e-12 and rel_err(gg_, gradE) < 1e-10
        Wg = gpu.buffer(B.BUF_POINT_FRAME).reshape(-1, 3, 10)
        assert rel_err(Wg, W) < 1e-12
        dU = _check_blocks_by_class(Vg_, V, Ug_, U, Wg, W, gg_, gradE, eo)
        del Wg, Vg_
        red = _reduced_index(M)
        keep = red >= 0
        n = int(keep.sum())
        ok_o, corr_o, S_o, rhs_o = orc.two_phase_skyline(so, gradE, V, U, W, c, sel_rows=np.arange(n), want_rhs=True)
        assert ok_o
        del W
        gpu.phase_schur(c)
        rg = gpu.buffer(B.BUF_RCS_RHS)
        assert rel_err(rg[keep], rhs_o) < 1e-10
        Sg = np.tril(gpu.buffer(B.BUF_RCS).reshape(10 * M, 10 * M)[np.ix_(keep, keep)])
        assert np.count_nonzero(S_o) > 0.49 * n * n          # the system really is dense (lower triangle filled)
        assert float(np.abs(Sg - S_o).max()) < 1e-10 * float(np.abs(S_o).max())
        dk = dU[keep]
        assert float((np.abs(Sg - S_o) / (dk[:, None] * dk[None, :])).max()) < 1e-10
        assert float((np.abs(rg[keep] - rhs_o) / (dk * 2.0 * np.sqrt(eo))).max()) < 1e-10
        assert gpu.phase_solve()
        gpu.phase_backsub(c)
        corr_g = gpu.buffer(B.BUF_CORRECTIONS)
        assert rel_err(corr_g[3 * sc.N:], corr_o[3 * sc.N:]) < 1e-8
        assert rel_err(corr_g[:3 * sc.N], corr_o[:3 * sc.N]) < 1e-8
        orc.set_solver(1)
        rc_o, rep_o, so2, ok2, rep, sg = _end_to_end(orc, gpu, sc, spec.f0, max_iterations=1)
        assert (rep.iterations, rep.attempts) == (rep_o.iterations, rep_o.attempts) and rep.iterations == 1
        lt.assert_same_trajectory(gpu.iteration_log(), rep_o.log, 1e-6, gpu_attempts=rep.attempts)
        assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-6)
        assert np.abs(sg.points - so2.points).max() < 1e-6 and np.abs(sg.cam_T - so2.cam_T).max() < 1e-6
    finally:
        orc.set_solver(0)
        orc.set_threads(threads)
    gpu.upload(SCENES["tiny"].f0, sa.generate_scene(SCENES["tiny"]))


def test_c3_full_size_blocks_and_reduced_system_vs_oracle(orc, gpu):
    """BASELINE config 3 (the bench workload: 1000 cams / 100k pts / 2M obs) against the oracle for everything but the
    dense solve (the oracle's Householder QR of the 9993^2 system would take hours): reprojection error, gradient,
    point / frame / point-frame blocks (rel 1e-12, gradient 1e-10), and the whole reduced camera system and right-hand
    side (rel 1e-10) -- 800 MB each side; the solve itself is covered at this size by
    test_c3_solver_modes_agree_at_bench_size (three factorisations of the same system agree), and the corrections of the
    step against the oracle's skyline Cholesky of the same system (point and frame parts rel 1e-8, as for C5)."""
    spec = sa.CONFIGS["C3_1kcam_100kpt"]
    sc = sa.config_scene("C3_1kcam_100kpt")
    so = _orc_scene(orc, sc)
    ok, _ = orc.normalize(so)
    assert ok and gpu.upload(spec.f0, sc)
    eo, seen_o = orc.reproj_error(spec.f0, so)
    eg, seen_g = gpu.phase_error()
    assert seen_g == seen_o == 2000000 and eg == pytest.approx(eo, rel=1e-12)
    gradE, V, U, W = orc.derivatives(spec.f0, so)
    gpu.phase_derivatives()
    Vg_, Ug_, gg_ = gpu.buffer(B.BUF_POINT_BLOCKS).reshape(-1, 3, 3), gpu.buffer(B.BUF_FRAME_BLOCKS).reshape(-1, 10, 10), gpu.buffer(B.BUF_GRAD)
    assert rel_err(Vg_, V) < 1e-12
    assert rel_err(Ug_, U) < 1e-12
    assert rel_err(gg_, gradE) < 1e-10
    Wg = gpu.buffer(B.BUF_POINT_FRAME).reshape(-1, 3, 10)
    assert rel_err(Wg, W) < 1e-12
    dU = _check_blocks_by_class(Vg_, V, Ug_, U, Wg, W, gg_, gradE, eo)  # every entry on the scale of its variable class
    del Wg
    orc.set_skip_solve(True)   # the system is formed, the QR is not run
    threads = orc.get_threads()
    try:
        _, _, S, rhs = orc.two_phase(so, gradE, V, U, W, 1e-4, want_system=True)
    finally:
        orc.set_skip_solve(False)
    try:  # the step itself: the oracle's skyline Cholesky of the same system
        orc.set_threads(min(16, os.cpu_count() or 1))
        ok_o, corr_o = orc.two_phase_skyline(so, gradE, V, U, W, 1e-4)
        assert ok_o
    finally:
        orc.set_threads(threads)
    del W
    gpu.phase_schur(1e-4)
    M = sc.M
    keep = _reduced_index(M) >= 0
    rg = gpu.buffer(B.BUF_RCS_RHS)
    assert rel_err(rg[keep], rhs) < 1e-10
    Sg = gpu.buffer(B.BUF_RCS).reshape(10 * M, 10 * M)
    idx = np.where(keep)[0]
    scale = float(np.abs(S).max())
    dk = dU[keep]
    worst = worst_scaled = 0.0
    for r0 in range(0, len(idx), 1000):          # row blocks: no second 800 MB copy
        rows = idx[r0:r0 + 1000]
        diff = np.abs(Sg[np.ix_(rows, idx)] - S[r0:r0 + 1000])
        worst = max(worst, float(diff.max()))
        worst_scaled = max(worst_scaled, float((diff / (dk[r0:r0 + 1000, None] * dk[None, :])).max()))
    assert worst < 1e-10 * scale
    assert worst_scaled < 1e-10                   # rows / columns on the scale of their variable (1 / sqrt(diag U))
    gs = 2.0 * np.sqrt(eo)
    assert float((np.abs(rg[keep] - rhs) / (dk * gs)).max()) < 1e-10
    del S, Sg
    assert gpu.phase_solve()
    gpu.phase_backsub(1e-4)
    corr_g = gpu.buffer(B.BUF_CORRECTIONS)
    assert rel_err(corr_g[3 * sc.N:], corr_o[3 * sc.N:]) < 1e-8
    assert rel_err(corr_g[:3 * sc.N], corr_o[:3 * sc.N]) < 1e-8
    gpu.upload(SCENES["tiny"].f0, sa.generate_scene(SCENES["tiny"]))  # release the large buffers


# ------------------------------------------------------------------ full-size properties (no oracle at this size)

def test_c2_size_properties(gpu):
    """BASELINE config 2 (200 cams / 20k pts / 400k obs): size-independent properties --
    the error decreases monotonically over accepted iterations (slowly: the reference solves for intrinsics
    corrections but never applies them, bundle-adj-kanatani.cpp:2027-2034), the result is still gauge-normalised
    before the revert, and the reverted scene reproduces the final error."""
    spec = sa.CONFIGS["C2_200cam_20kpt"]
    sc, pts_gt, Rg, Tg = sa.generate_scene(spec, with_gt=True)
    assert gpu.upload(spec.f0, sc)
    e0, seen = gpu.phase_error()
    assert seen == 400000
    errs = [e0]
    for _ in range(3):
        ok = gpu.optimize(None, max_iterations=1)
        assert not ok and gpu.OptimizationStatusString() == "max iterations"
        errs.append(gpu.report.err_final)
    assert all(b < a for a, b in zip(errs[:-1], errs[1:]))
    nrm_scene = sc.copy()
    gpu.download(nrm_scene, revert_normalization=False)
    assert sa.check_world_is_normalized(nrm_scene)
    out = sc.copy()
    gpu.download(out, revert_normalization=True)
    # the gauge leaves a similarity free, so compare through the reprojection error only
    e_final, _ = gpu.ReprojError(spec.f0, out)
    assert e_final == pytest.approx(errs[-1], rel=1e-6)


def test_c3_solver_modes_agree_at_bench_size(gpu):
    """The bench workload (BASELINE config 3: 1000 cams / 100k pts / 2M obs): one LM iteration through the nested
    dissection (4 levels), the single skyline chain and the dense factorisation must be the same step -- same error,
    same corrections; and a second iteration still decreases the error."""
    spec = sa.CONFIGS["C3_1kcam_100kpt"]
    sc = sa.generate_scene(spec)
    res = {}
    try:
        for mode in (2, 1, 0):
            gpu.set_rcs_mode(mode)
            assert gpu.upload(spec.f0, sc)
            if mode == 2:
                assert gpu.rcs_chunks() >= 8 and gpu.rcs_fill() < 0.15
            ok = gpu.optimize(None, max_iterations=1)
            assert not ok and gpu.report.iterations == 1 and gpu.report.attempts == 1
            res[mode] = (gpu.report.err_initial, gpu.report.err_final, gpu.buffer(B.BUF_CORRECTIONS).copy())
    finally:
        gpu.set_rcs_mode(2)
    e0, e1, corr = res[1]
    assert e1 < e0
    for mode in (2, 0):
        assert res[mode][0] == e0
        assert res[mode][1] == pytest.approx(e1, rel=1e-9)
        assert rel_err(res[mode][2], corr) < 1e-8
    assert gpu.upload(spec.f0, sc)
    gpu.optimize(None, max_iterations=2)
    assert gpu.report.iterations == 2 and gpu.report.err_final < e1


def test_c5_nested_dissection_agrees_with_single_chain(gpu):
    """BASELINE config 5 (4000 cams / 1M pts / 20M obs): two LM iterations through the nested dissection (32 chunks; its
    batched panel launches carry more workgroups than the chip holds at once, so workgroups of one launch do not all
    start together) and through the single skyline chain must agree."""
    spec = sa.CONFIGS["C5_4kcam_1Mpt"]
    sc = sa.generate_scene(spec)
    res = {}
    try:
        for mode in (2, 1):
            gpu.set_rcs_mode(mode)
            assert gpu.upload(spec.f0, sc)
            if mode == 2:
                assert gpu.rcs_chunks() >= 16
            gpu.optimize(None, max_iterations=2)
            r = gpu.report
            res[mode] = (r.iterations, r.attempts, r.err_initial, r.err_final, gpu.buffer(B.BUF_CORRECTIONS).copy())
    finally:
        gpu.set_rcs_mode(2)
        gpu.upload(SCENES["tiny"].f0, sa.generate_scene(SCENES["tiny"]))  # release the 13 GB system
    assert res[2][:3] == res[1][:3] and res[1][0] == 2
    assert res[2][3] < res[2][2]
    assert res[2][3] == pytest.approx(res[1][3], rel=1e-9)
    assert rel_err(res[2][4], res[1][4]) < 1e-8


def test_c5_full_size_blocks_sampled_system_rows_and_corrections_vs_oracle(orc, gpu):
    """BASELINE config 5 (4000 cams / 1M pts / 20M obs, n = 39993) at full size against the oracle: reprojection error,
    gradient and every point / frame / point-frame block (rel 1e-12, gradient 1e-10, and on the scale of each variable
    class), the right-hand side of the reduced camera system, its rows for 25 frames spread over the sequence (250 rows
    of 39993 entries: the oracle's skyline variant returns selected rows, so neither side needs the 12.8 GB dense
    matrix), and the corrections of the whole step against the oracle's skyline Cholesky (rel 1e-8).  The oracle runs its
    OpenMP variant (bit-identical to one thread, tests/test_oracle_skyline.py)."""
    import os
    spec = sa.CONFIGS["C5_4kcam_1Mpt"]
    sc = sa.config_scene("C5_4kcam_1Mpt")
    assert (sc.M, sc.N, sc.O) == (4000, 1000000, 20000000)
    so = _orc_scene(orc, sc)
    ok, _ = orc.normalize(so)
    assert ok and gpu.upload(spec.f0, sc)
    M, c = sc.M, 1e-4
    orc.set_threads(max(1, min(32, (os.cpu_count() or 2) // 2)))
    try:
        eo, seen_o = orc.reproj_error(spec.f0, so)
        eg, seen_g = gpu.phase_error()
        assert seen_g == seen_o == sc.O and eg == pytest.approx(eo, rel=1e-12)
        gradE, V, U, W = orc.derivatives(spec.f0, so)
        gpu.phase_derivatives()
        Vg_, Ug_, gg_ = (gpu.buffer(B.BUF_POINT_BLOCKS).reshape(-1, 3, 3), gpu.buffer(B.BUF_FRAME_BLOCKS).reshape(-1, 10, 10),
                         gpu.buffer(B.BUF_GRAD))
        assert rel_err(Vg_, V) < 1e-12 and rel_err(Ug_, U) < 1e-12 and rel_err(gg_, gradE) < 1e-10
        Wg = gpu.buffer(B.BUF_POINT_FRAME).reshape(-1, 3, 10)
        assert rel_err(Wg, W) < 1e-12
        dU = _check_blocks_by_class(Vg_, V, Ug_, U, Wg, W, gg_, gradE, eo)
        del Wg, Vg_
        red = _reduced_index(M)
        keep = red >= 0
        frames = np.unique(np.linspace(2, M - 1, 25).astype(np.int64))
        full_rows = (10 * frames[:, None] + np.arange(10)[None, :]).reshape(-1)
        ok_o, corr_o, rows_o, rhs_o = orc.two_phase_skyline(so, gradE, V, U, W, c, sel_rows=red[full_rows], want_rhs=True)
        assert ok_o
    finally:
        orc.set_threads(1)
    del W
    gpu.phase_schur(c)
    rg = gpu.buffer(B.BUF_RCS_RHS)
    assert rel_err(rg[keep], rhs_o) < 1e-10
    rows_g = gpu.rcs_rows(full_rows)[:, keep]
    scale = float(np.abs(rows_o).max())     # (the sampled rows hold pose-variable diagonals: the system's largest entries)
    assert float(np.abs(rows_g - rows_o).max()) < 1e-10 * scale
    dk = dU[keep]
    assert float((np.abs(rows_g - rows_o) / (dU[full_rows][:, None] * dk[None, :])).max()) < 1e-10
    gs = 2.0 * np.sqrt(eo)
    assert float((np.abs(rg[keep] - rhs_o) / (dk * gs)).max()) < 1e-10
    assert gpu.phase_solve()
    gpu.phase_backsub(c)
    corr_g = gpu.buffer(B.BUF_CORRECTIONS)
    assert rel_err(corr_g[3 * sc.N:], corr_o[3 * sc.N:]) < 1e-8
    assert rel_err(corr_g[:3 * sc.N], corr_o[:3 * sc.N]) < 1e-8
    gpu.upload(SCENES["tiny"].f0, sa.generate_scene(SCENES["tiny"]))  # release the 13 GB system


# ------------------------------------------------------------------ sharded path, world size 1 on the GPU

def test_native_rccl_exchange_world_size_1(orc):
    """The library's own RCCL path (srk_ba_rccl_get_unique_id / srk_ba_rccl_init, librccl.so opened on first use,
    ncclAllReduce on the attempt's stream, no host synchronisation) at world size 1 -- all one GPU can run: the packed
    band, the right-hand side and the {error, status} words go through ncclAllReduce and come back unchanged, so the
    run must equal the oracle's like any single-GPU run."""
    spec = SCENES["ragged_wave"]
    sc = sa.generate_scene(spec)
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        ba.rccl_init(ba.rccl_unique_id(), 0, 1)
        so = _orc_scene(orc, sc)
        rc_o, rep_o, rep_o.log = orc.compute_inplace(spec.f0, so, 1e-7, 1e6, 40, want_log=True)
        crit = sa.BundleAdjustmentKanataniTermCriteria()
        crit.AllowedReprojErrRelativeChange(1e-7)
        crit.MaxHessianFactor(1e6)
        sg = sc.copy()
        ok = ba.ComputeInplace(spec.f0, sg, crit, 40)
        rep = ba.report
        assert ok == (rc_o == 0) and sa.status_string(rep.status) == orc.status_string(rep_o.status)
        assert (rep.iterations, rep.attempts) == (rep_o.iterations, rep_o.attempts)
        lt.assert_same_trajectory(ba.iteration_log(), rep_o.log, 1e-6, gpu_attempts=rep.attempts, err_abs=1e-18)
        assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-6, abs=1e-18)
        assert np.abs(sg.points - so.points).max() < 1e-6
    finally:
        ba.close()


def test_native_rccl_two_communicators_keep_the_attempt_pairs_world_size_1(orc):
    """srk_ba_rccl_init_second: the second attempt slot's own communicator, so that the speculative attempt pairs stay on
    with the native exchange -- two communicators on one device, all-reduces of both slots in flight on two streams, at
    world size 1 (all one GPU can run).  Same accept / reject sequence and numbers as the oracle's sequential loop."""
    spec = SCENES["ragged_wave"]
    sc = sa.generate_scene(spec)
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        ba.rccl_init(ba.rccl_unique_id(), 0, 1)
        ba.rccl_init_second(ba.rccl_unique_id())
        so = _orc_scene(orc, sc)
        rc_o, rep_o, rep_o.log = orc.compute_inplace(spec.f0, so, 1e-7, 1e6, 40, want_log=True)
        crit = sa.BundleAdjustmentKanataniTermCriteria()
        crit.AllowedReprojErrRelativeChange(1e-7)
        crit.MaxHessianFactor(1e6)
        sg = sc.copy()
        ok = ba.ComputeInplace(spec.f0, sg, crit, 40)
        rep = ba.report
        assert ok == (rc_o == 0) and sa.status_string(rep.status) == orc.status_string(rep_o.status)
        assert (rep.iterations, rep.attempts) == (rep_o.iterations, rep_o.attempts)
        lt.assert_same_trajectory(ba.iteration_log(), rep_o.log, 1e-6, gpu_attempts=rep.attempts, err_abs=1e-18)
        assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-6, abs=1e-18)
        assert np.abs(sg.points - so.points).max() < 1e-6
        assert ba.solver_sync_timeouts() == 0
    finally:
        ba.close()


@pytest.mark.parametrize("native", [True, False])
def test_damping_parallel_schedule_world_size_1(orc, native, monkeypatch):
    """The multi-rank schedule of DESIGN 6 (three damping factors a round, band k reduced to rank k, corrections broadcast,
    one all-reduce of all status words) forced at world size 1 (srk_ba_set_multi_schedule(h, 2)) -- all one GPU can run of it:
    natively every ncclReduce / ncclBroadcast / ncclAllReduce goes through the handle's communicator on its collective
    stream inside ncclGroups with the event hand-offs to the three slot streams; with the callback the same program order
    runs through host-blocking sums.  Same accept / reject sequence and numbers as the oracle's sequential loop."""
    spec = SCENES["ragged_wave"]
    sc = sa.generate_scene(spec)
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        ba.set_multi_schedule("dp_force")
        assert ba.multi_schedule() == "dp"
        calls = []
        if native:
            ba.rccl_init(ba.rccl_unique_id(), 0, 1)
        else:
            from surikatoko_amd._lib import ALLREDUCE_FN
            hook = ALLREDUCE_FN(lambda ctx, ptr, n: calls.append(n) or 0)
            ba.set_allreduce(hook, 0, 1)
        so = _orc_scene(orc, sc)
        rc_o, rep_o, rep_o.log = orc.compute_inplace(spec.f0, so, 1e-7, 1e6, 40, want_log=True)
        crit = sa.BundleAdjustmentKanataniTermCriteria()
        crit.AllowedReprojErrRelativeChange(1e-7)
        crit.MaxHessianFactor(1e6)
        sg = sc.copy()
        ok = ba.ComputeInplace(spec.f0, sg, crit, 40)
        rep = ba.report
        assert ok == (rc_o == 0) and sa.status_string(rep.status) == orc.status_string(rep_o.status)
        assert (rep.iterations, rep.attempts) == (rep_o.iterations, rep_o.attempts)
        lt.assert_same_trajectory(ba.iteration_log(), rep_o.log, 1e-6, gpu_attempts=rep.attempts, err_abs=1e-18)
        assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-6, abs=1e-18)
        assert np.abs(sg.points - so.points).max() < 1e-6
        assert np.abs(sg.cam_T - so.cam_T).max() < 1e-6
        assert ba.solver_sync_timeouts() == 0
        # natively the first round checked itself (checksums of the bands and of the corrections through plain all-reduces)
        assert ba.multi_schedule() == ("dp (self-check passed)" if native else "dp")
        if not native:
            assert 24 in calls, "the three slots' status words travel in one sum"
    finally:
        ba.close()


def test_native_rccl_handles_release_both_communicators():
    """srk_ba_destroy / srk_ba_set_allreduce release the second slot's communicator as well as the first (it used to leak
    with every handle that had used the two-communicator path): create / init both / close in a loop at world size 1, and
    a callback set after the communicators replaces them."""
    spec = SCENES["tiny"]
    sc = sa.generate_scene(spec)
    for k in range(6):
        ba = sa.BundleAdjustmentKanatani(0)
        try:
            ba.rccl_init(ba.rccl_unique_id(), 0, 1)
            ba.rccl_init_second(ba.rccl_unique_id())
            if k % 2:
                calls = []
                from surikatoko_amd._lib import ALLREDUCE_FN
                hook = ALLREDUCE_FN(lambda ctx, ptr, n: calls.append(n) or 0)
                ba.set_allreduce(hook, 0, 1)  # detaches (and destroys) both communicators
            crit = sa.BundleAdjustmentKanataniTermCriteria()
            crit.AllowedReprojErrRelativeChange(1e-7)
            ba.ComputeInplace(spec.f0, sc.copy(), crit, 3)
            assert ba.report.iterations >= 1
            if k % 2:
                assert calls, "the callback set after srk_ba_rccl_init must be the exchange that runs"
        finally:
            ba.close()


def test_allreduce_hook_with_device_pointers(orc, gpu):
    """The RCCL path end to end at world size 1: the library packs the skyline, calls the torch.distributed hook with
    DEVICE pointers (zero-copy __cuda_array_interface__ views) and must give the same iterations as without it."""
    import os
    import socket
    import torch
    import torch.distributed as dist
    from surikatoko_amd.ba import covisibility
    from surikatoko_amd.dist import make_allreduce_hook
    spec = SCENES["ragged_wave"]
    sc = sa.generate_scene(spec)
    ref = sc.copy()
    crit = sa.BundleAdjustmentKanataniTermCriteria()
    crit.AllowedReprojErrRelativeChange(1e-7)
    ok_ref = gpu.ComputeInplace(spec.f0, ref, crit, 6)
    rep_ref = (gpu.report.iterations, gpu.report.attempts, gpu.report.err_final)

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        h = sa.BundleAdjustmentKanatani(0)
        calls = []
        inner = make_allreduce_hook(None, "cuda:0")

        from surikatoko_amd._lib import ALLREDUCE_FN

        def counting(ctx, ptr, count):
            calls.append(int(count))
            return inner(ctx, ptr, count)

        h.set_allreduce(ALLREDUCE_FN(counting), 0, 1)
        full = sc.copy()
        ok, nrm = sa.normalize_scene_inplace(full)
        assert ok
        shard, _ = full.shard(0, 1)
        assert h.upload(spec.f0, shard, already_normalized=True)
        assert h.rcs_fill() == pytest.approx(1.0, abs=0.35)   # no covisibility given yet: (padded) full triangle
        h.set_covisibility(covisibility(full))
        assert 0 < h.rcs_fill() <= 1.0
        ok_h = h.optimize(crit, 6)
        out = shard.copy()
        h.download(out, revert_normalization=False)
        from surikatoko_amd.ba import revert_normalization
        revert_normalization(out, nrm)
        assert ok_h == ok_ref
        assert (h.report.iterations, h.report.attempts) == rep_ref[:2]
        assert h.report.err_final == pytest.approx(rep_ref[2], rel=1e-9)
        assert np.abs(out.points - ref.points).max() < 1e-8
        # exchanges: seen count and initial error (1 value each), then per attempt the packed skyline with the rhs
        # behind it (one call) and {error, solver status, point-update status}; the frame blocks need none
        assert 1 in calls and 3 in calls and 65 * sc.M not in calls
        big = [c for c in calls if c > 3]
        assert len(big) == h.report.attempts and len(set(big)) == 1
        assert calls.count(3) == h.report.attempts
        h.close()
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------ chunked (bordered block-diagonal) solve

@pytest.mark.parametrize("n_frames,window", [(330, 8), (500, 12), (500, 30), (700, 70), (800, 95)])
def test_chunked_solve_equals_single_chain(gpu, n_frames, window):
    """Banded reduced camera system cut into independent chunks + separator system (srk_chol_solve_chunked) against
    the single-chain skyline Cholesky and against numpy on the downloaded system.  window 30 needs 512-wide
    separators, 70 needs 768, 95 needs 1024 (the widest the chunked solve takes on)."""
    spec = sa.SceneSpec(n_frames=n_frames, grid_nx=60, grid_ny=40, vis_window=window)  # every frame well observed
    sc = sa.generate_scene(spec)
    c = 1e-3
    sols = {}
    for mode in (2, 1):
        gpu.set_rcs_mode(mode)
        assert gpu.upload(spec.f0, sc)
        if mode == 2:
            assert gpu.rcs_chunks() >= 2
        else:
            assert gpu.rcs_chunks() == 0
        gpu.phase_derivatives()
        gpu.phase_schur(c)
        if mode == 2:
            S = gpu.buffer(B.BUF_RCS).reshape(10 * n_frames, 10 * n_frames)
            rhs = gpu.buffer(B.BUF_RCS_RHS)
        assert gpu.phase_solve()
        gpu.phase_backsub(c)
        sols[mode] = gpu.buffer(B.BUF_CORRECTIONS)
    gpu.set_rcs_mode(2)
    x = np.linalg.solve(S, rhs)
    for _ in range(3):
        x = x + np.linalg.solve(S, rhs - S @ x)
    dc2 = sols[2][3 * sc.N:]
    assert rel_err(dc2, x) < 1e-9
    assert rel_err(sols[2], sols[1]) < 1e-9
    assert np.all(dc2[4:10] == 0) and dc2[15] == 0


@pytest.mark.parametrize("n_frames", [26, 52, 77, 103, 128, 129, 154, 180, 205, 256, 257])
def test_nested_plan_edge_sizes(gpu, n_frames):
    """System sizes around every multiple of the 256-column outer panel (ld = 512 ... 2816): whatever plan the cost
    model picks (none, one level, nested; chunks of one or two panels), the corrections must equal numpy's."""
    spec = sa.SceneSpec(n_frames=n_frames, grid_nx=60, grid_ny=40, vis_window=8)  # every frame sees >= 7 landmarks
    sc = sa.generate_scene(spec)
    c = 1e-3
    assert gpu.upload(spec.f0, sc)
    gpu.phase_derivatives()
    gpu.phase_schur(c)
    S = gpu.buffer(B.BUF_RCS).reshape(10 * n_frames, 10 * n_frames)
    rhs = gpu.buffer(B.BUF_RCS_RHS)
    assert gpu.phase_solve()
    gpu.phase_backsub(c)
    dc = gpu.buffer(B.BUF_CORRECTIONS)[3 * sc.N:]
    x = np.linalg.solve(S, rhs)
    for _ in range(3):
        x = x + np.linalg.solve(S, rhs - S @ x)
    assert rel_err(dc, x) < 1e-9, (n_frames, gpu.rcs_chunks())


def test_fused_outer_step_is_reproducible_and_agrees_with_the_panel_sequence_dense(gpu):
    """k_step256 (an outer step of the blocked Cholesky as ONE launch: a diagonal-block workgroup that owns the 256 x 256
    block for all four sub-steps and hands L and X tiles one way to row workgroups) against the k_panel / k_upd64 launch
    sequence it replaces.  Same factorisation, but the block's own rows are eliminated in potrf64's unscaled form (round 4), so
    the two agree to rounding; the fused solve must be IDENTICAL from run to run (no atomics, fixed summation order; repeated,
    so that a stale read of a handed-off tile would have several chances to show).  Dense systems of one to five outer steps;
    the last step's chain ends at the last tile with real columns (1, 2, 3 or 4 sub-steps: 300, 360, 420, 200 / 256)."""
    rng = np.random.RandomState(5)
    try:
        for n in (200, 256, 300, 360, 420, 777, 1280):
            A = rng.randn(n, n)
            A = A @ A.T + n * np.eye(n) + np.diag(np.arange(n) * 0.37)
            b = rng.randn(n)
            sols = {}
            for fused in (1, 0, 1, 1, 1):
                gpu.set_solver_fusion(fused)
                ok, x, _ = gpu.dense_spd_solve(A, b)
                assert ok
                if fused in sols:
                    assert np.array_equal(x, sols[fused]), n
                sols[fused] = x
            ref = np.linalg.solve(A, b)
            assert np.abs(sols[1] - sols[0]).max() < 1e-13 * max(1.0, np.abs(ref).max()), n
            assert np.abs(sols[1] - ref).max() < 1e-10 * max(1.0, np.abs(ref).max())
        assert gpu.solver_sync_timeouts() == 0
    finally:
        gpu.set_solver_fusion(1)


@pytest.mark.parametrize("cond", [1e6, 1e10, 1e13])
def test_solver_is_backward_stable_on_ill_conditioned_systems(gpu, cond):
    """potrf64's pivot reciprocals take ONE Newton step on the v_rcp_f64 seed (2e-15 relative) and, since round 4, the second
    pivot of a pair as a quotient of determinants: neither may cost backward stability.  Dense SPD systems with a prescribed
    spectrum (condition 1e6 .. 1e13, eigenvalues geometrically spaced, random orthogonal basis), 640 variables = three outer
    steps, fused and unfused: the normwise backward error ||A x - b|| / (||A|| ||x|| + ||b||) stays at n eps, the forward
    error within cond x that (a Cholesky that lost digits in its pivots would show in the first; LAPACK's own solve is the
    yardstick for the second)."""
    rng = np.random.RandomState(11)
    n = 640
    Q, _ = np.linalg.qr(rng.randn(n, n))
    lam = np.geomspace(1.0, 1.0 / cond, n)
    A = (Q * lam) @ Q.T
    A = 0.5 * (A + A.T)
    x_true = rng.randn(n)
    b = A @ x_true
    try:
        for fused in (1, 0):
            gpu.set_solver_fusion(fused)
            ok, x, _ = gpu.dense_spd_solve(A, b)
            assert ok
            berr = np.linalg.norm(A @ x - b) / (np.linalg.norm(A, 2) * np.linalg.norm(x) + np.linalg.norm(b))
            assert berr < 50 * n * np.finfo(np.float64).eps / 8, (fused, berr)     # ~ 9e-13 / 8: a few n eps
            x_lapack = np.linalg.solve(A, b)
            ferr, ferr_lapack = np.linalg.norm(x - x_true) / np.linalg.norm(x_true), np.linalg.norm(x_lapack - x_true) / np.linalg.norm(x_true)
            assert ferr < max(20 * ferr_lapack, 1e-13), (fused, ferr, ferr_lapack)
    finally:
        gpu.set_solver_fusion(1)


@pytest.mark.parametrize("n_frames,window", [(103, 8), (330, 8), (500, 30), (800, 95)])
def test_fused_outer_step_is_reproducible_and_agrees_with_the_panel_sequence_chunked(gpu, n_frames, window):
    """The same on nested chunks with 256- to 1024-wide separators (batched items, border rows, structurally zero border
    rows skipped per step): the chunked solve works on copies, so the SAME reduced camera system is solved both ways; both
    must be as close to the exact solution of that system as a backward-stable factorisation gets."""
    spec = sa.SceneSpec(n_frames=n_frames, grid_nx=60, grid_ny=40, vis_window=window)
    sc = sa.generate_scene(spec)
    try:
        assert gpu.upload(spec.f0, sc)
        assert gpu.rcs_chunks() >= 2
        gpu.phase_derivatives()
        gpu.phase_schur(1e-3)
        S = gpu.buffer(B.BUF_RCS).reshape(10 * n_frames, 10 * n_frames)
        rhs = gpu.buffer(B.BUF_RCS_RHS)
        sols = {}
        for fused in (1, 0, 1, 1, 1):
            gpu.set_solver_fusion(fused)
            assert gpu.phase_solve()
            x = gpu.buffer(B.BUF_CORRECTIONS)[3 * sc.N:]
            assert np.all(np.isfinite(x))
            if fused in sols:
                assert np.array_equal(x, sols[fused])
            sols[fused] = x
        ref = np.linalg.solve(S, rhs)
        for _ in range(3):
            ref = ref + np.linalg.solve(S, rhs - S @ ref)
        assert rel_err(sols[1], ref) < 1e-9 and rel_err(sols[0], ref) < 1e-9
        assert rel_err(sols[1], sols[0]) < 1e-9
        assert gpu.solver_sync_timeouts() == 0
    finally:
        gpu.set_solver_fusion(1)


def test_fused_solve_hand_offs_stay_exact_beside_a_streaming_load():
    """tools/stress_fused.py in small: the bench scene's reduced camera system solved 60 times with the fused outer
    step while another stream keeps HBM busy (uneven load, consumer caches warm from the previous solve); every solution
    must equal the first one bit for bit (a stale read of a handed-off tile would differ), agree with the unfused sequence's
    to rounding, and no hand-off may time out."""
    import torch
    spec = sa.CONFIGS["C3_1kcam_100kpt"]
    sc = sa.generate_scene(spec)
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_speculation(False)
        assert h.upload(spec.f0, sc)
        h.phase_derivatives()
        h.phase_schur(1e-3)
        h.set_solver_fusion(0)
        assert h.phase_solve()
        unfused = h.buffer(B.BUF_CORRECTIONS)[3 * sc.N:].copy()
        h.set_solver_fusion(1)
        assert h.phase_solve()
        ref = h.buffer(B.BUF_CORRECTIONS)[3 * sc.N:].copy()
        assert rel_err(ref, unfused) < 1e-9
        side = torch.cuda.Stream()
        x = torch.empty(32 * 1024 * 1024, device="cuda", dtype=torch.float64)
        y = torch.empty_like(x)
        for it in range(60):
            with torch.cuda.stream(side):
                y.copy_(x)
                x.add_(1.0)
            assert h.phase_solve()
            assert np.array_equal(h.buffer(B.BUF_CORRECTIONS)[3 * sc.N:], ref), it
        torch.cuda.synchronize()
        assert h.solver_sync_timeouts() == 0
    finally:
        h.close()


def _run_dev_worker(which):
    """The development build (surikatoko_amd/libsrk_ba_dev.so: make dev, -DSRK_DEV) carries the fault-injection hooks the
    product library does not export; a subprocess loads it through SRK_BA_LIBRARY and runs tests/_dev_worker.py <which>."""
    import subprocess
    lib = os.path.join(os.path.dirname(os.path.abspath(sa.__file__)), "libsrk_ba_dev.so")
    if not os.path.exists(lib):
        pytest.fail("surikatoko_amd/libsrk_ba_dev.so is not built (__graft_entry__.build() / make -C surikatoko_amd/csrc dev)")
    env = dict(os.environ, SRK_BA_LIBRARY=lib)
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "_dev_worker.py"), which],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]


def test_product_library_exports_no_development_hooks():
    import ctypes as C
    L = sa.lib()
    for name in ("srk_dbg_step_fault", "srk_dbg_dp_corrupt", "srk_dbg_step_stamps", "srk_dbg_mm_stamps", "srk_dbg_panel_stamps"):
        assert not hasattr(L, name), name


def test_a_lost_hand_off_times_out_and_the_attempt_is_repeated_with_the_panel_sequence():
    """Every wait inside k_step256 is bounded.  Test hook (development build): one launch's diagonal-block workgroup
    publishes nothing; its consumers give up, the solve reports bit 8, the LM loop repeats that attempt with the unfused
    kernels (and stays there) -- same iterations, attempts and numbers as an undisturbed run."""
    _run_dev_worker("lost_hand_off_lm_loop")


def test_a_lost_hand_off_in_the_staged_solve_calls_is_repeated_unfused():
    """The same scheduling event through the step-wise entry points: srk_ba_phase_solve (nested plan: the system is intact,
    the solve runs again with the panel sequence and reports success) and srk_ba_dense_spd_solve (inputs staged again from
    the host copies) -- a hand-off timeout is not reported as a numerical failure."""
    _run_dev_worker("lost_hand_off_staged")


@pytest.mark.parametrize("stage", ["reduce", "broadcast"])
def test_failed_self_check_of_the_first_native_dp_round_falls_back_to_the_allreduce_schedule(stage):
    """The native damping-parallel round checks itself on its first run (checksums beside the rooted collectives).  Test hook
    (development build): the check finds a mismatch at the reduce / the broadcast stage -- the handle switches to the
    all-reduce schedule, repeats the round that way and the run gives the oracle's sequence and numbers; the handle says so."""
    _run_dev_worker("dp_selfcheck_" + stage)


def test_chunked_end_to_end_matches_single_chain(gpu):
    spec = sa.SceneSpec(n_frames=400, grid_nx=60, grid_ny=40, vis_window=10, noise_uv_pix=0.2)
    sc = sa.generate_scene(spec)
    res = {}
    for mode in (2, 1):
        gpu.set_rcs_mode(mode)
        s2 = sc.copy()
        gpu.ComputeInplace(spec.f0, s2, None, 4)
        res[mode] = (gpu.report.iterations, gpu.report.attempts, gpu.report.err_final, s2)
    gpu.set_rcs_mode(2)
    assert res[1][:2] == res[2][:2]
    assert res[2][2] == pytest.approx(res[1][2], rel=1e-8)
    assert np.abs(res[2][3].points - res[1][3].points).max() < 1e-8
    assert np.abs(res[2][3].cam_T - res[1][3].cam_T).max() < 1e-8


def test_nested_plan_counts_its_mfma_flops(gpu):
    """srk_ba_solve_mfma_flops (dry walk of the launch sequence) == the flops the profiled solve reports, in every
    reduced-camera-system mode; nested dissection executes more trailing-update flops than the single chain."""
    spec = sa.SceneSpec(n_frames=400, grid_nx=60, grid_ny=40, vis_window=10, noise_uv_pix=0.2)
    sc = sa.generate_scene(spec)
    gpu.set_profile(True)
    flops = {}
    try:
        for mode in (0, 1, 2):
            gpu.set_rcs_mode(mode)
            s2 = sc.copy()
            gpu.ComputeInplace(spec.f0, s2, None, 1)
            r = gpu.report
            assert r.attempts >= 1
            assert r.solve_mfma_flops / r.attempts == pytest.approx(gpu.solve_mfma_flops(), rel=1e-12)
            assert r.ms_solve_syrk > 0
            flops[mode] = gpu.solve_mfma_flops()
    finally:
        gpu.set_profile(0)
        gpu.set_rcs_mode(2)
    assert gpu.rcs_chunks() >= 2
    assert flops[0] > flops[1] > 0


# ------------------------------------------------------------------ standalone scoring

def test_reproj_error_does_not_disturb_an_uploaded_scene(orc, gpu):
    spec = SCENES["ragged_wave"]
    sc = sa.generate_scene(spec)
    assert gpu.upload(spec.f0, sc)
    e_before, _ = gpu.phase_error()
    other = sa.generate_scene(SCENES["tiny"])
    e, seen = gpu.ReprojError(spec.f0, other)
    eo, so = orc.reproj_error(spec.f0, _orc_scene(orc, other))
    assert seen == so and e == pytest.approx(eo, rel=1e-12)
    assert gpu.phase_error()[0] == e_before  # the resident BA scene is untouched


def test_mvf_scorer_matches_oracle_and_skips_points_at_infinity(orc, gpu):
    """MultiViewIterativeFactorizer::ReprojError (multi-view-factorization.cpp:415-475): shared K, f0 = 1, |z| <= 1e-5
    skipped, false when nothing is summed."""
    spec = sa.SceneSpec(n_frames=9, grid_nx=7, grid_ny=6, vis_window=4, f0=1.0)
    sc = sa.generate_scene(spec)
    ok, e, n = gpu.ReprojErrorMvf(1.0, sc)
    oko, eo, no = orc.reproj_error_mvf(1.0, _orc_scene(orc, sc))
    assert ok and oko and n == no == sc.O
    assert e == pytest.approx(eo, rel=1e-12)
    # move three landmarks into the focal plane of one of the cameras that sees them: z_cam = 0 -> skipped there only
    s2 = sc.copy()
    moved = 0
    for i in (0, 5, 11):
        j = int(s2.obs_frame[s2.row_ptr[i]])
        R, T = s2.cam_R[j].reshape(3, 3), s2.cam_T[j]
        xc = R @ s2.points[i] + T
        xc[2] = 0.0
        s2.points[i] = R.T @ (xc - T)
        moved += 1
    ok2, e2, n2 = gpu.ReprojErrorMvf(1.0, s2)
    oko2, eo2, no2 = orc.reproj_error_mvf(1.0, _orc_scene(orc, s2))
    assert ok2 and oko2 and n2 == no2 and sc.O - n2 >= moved
    assert e2 == pytest.approx(eo2, rel=1e-12)
    # a single frame is a legal MVF call; nothing to sum -> False
    one = sa.Scene(sc.points[:2], sc.cam_R[:1], sc.cam_T[:1], sc.K[:1], 1, np.array([0, 0, 0], dtype=np.int64),
                   np.zeros(0, dtype=np.int32), np.zeros((0, 2)))
    ok3, _, n3 = gpu.ReprojErrorMvf(1.0, one)
    assert not ok3 and n3 == 0
    with pytest.raises(ValueError):
        gpu.ReprojErrorMvf(0.0, sc)


# ------------------------------------------------------------------ f32 boundary (reference built with Scalar = float)

def test_f32_boundary_matches_f64_run_on_the_same_rounded_inputs(gpu):
    """srk_ba_compute_inplace_f32 = widen -> fp64 pipeline -> round: its result must be the float rounding of the f64
    call on the float-rounded inputs, with the same accept / reject sequence."""
    spec = SCENES["pixel_noise"]
    sc = sa.generate_scene(spec)
    f32 = {k: np.ascontiguousarray(getattr(sc, k), dtype=np.float32) for k in ("points", "cam_R", "cam_T", "K", "obs_uv")}
    sc64 = sa.Scene(f32["points"].astype(np.float64), f32["cam_R"].astype(np.float64), f32["cam_T"].astype(np.float64),
                    f32["K"].astype(np.float64), sc.shared_k, sc.row_ptr, sc.obs_frame, f32["obs_uv"].astype(np.float64))
    crit = sa.BundleAdjustmentKanataniTermCriteria()
    crit.AllowedReprojErrRelativeChange(float(np.float32(1e-6)))
    ok64 = gpu.ComputeInplace(float(np.float32(spec.f0)), sc64, crit, 6)
    rep64 = (gpu.report.iterations, gpu.report.attempts, gpu.report.status)
    ok32 = gpu.ComputeInplaceF32(spec.f0, f32["points"], f32["cam_R"], f32["cam_T"], f32["K"], sc.shared_k, sc.row_ptr,
                                 sc.obs_frame, f32["obs_uv"], crit, 6)
    assert ok32 == ok64 and (gpu.report.iterations, gpu.report.attempts, gpu.report.status) == rep64
    for k in ("points", "cam_R", "cam_T"):
        want = getattr(sc64, k).astype(np.float32).reshape(f32[k].shape)
        # fp64 atomics reorder sums run to run: allow one float ulp
        assert np.abs(f32[k] - want).max() <= 2 * np.finfo(np.float32).eps * max(1.0, float(np.abs(want).max()))
    with pytest.raises(ValueError):
        gpu.ComputeInplaceF32(spec.f0, sc.points, f32["cam_R"], f32["cam_T"], f32["K"], sc.shared_k, sc.row_ptr,
                              sc.obs_frame, f32["obs_uv"])


# ------------------------------------------------------------------ opt-in mixed precision

@pytest.mark.parametrize("name", ["ragged_wave", "pixel_noise", "ragged_20"])
def test_fp32_schur_run_sums_stay_close_to_fp64(orc, gpu, name):
    """srk_ba_set_schur_precision(1): W and E^-1 W rounded to fp32, packed fp32 FMAs over a run, fp64 everywhere else.
    Tolerance table of this mode (against the fp64 path on the same inputs): reduced camera system 2e-6 of its largest
    entry, one-step corrections 2e-3, the LM loop must take the same accept / reject decisions over the first
    iterations and land within 1e-4 of the fp64 error."""
    if name in SCENES:
        spec, sc = SCENES[name], sa.generate_scene(SCENES[name])
    else:
        spec, frac = RAGGED[name]
        sc = sa.drop_observations(sa.generate_scene(spec), frac, seed=7)
    res = {}
    try:
        for fp32 in (False, True):
            gpu.set_schur_precision(fp32)
            assert gpu.upload(spec.f0, sc)
            gpu.phase_derivatives()
            gpu.phase_schur(1e-3)
            S = gpu.buffer(B.BUF_RCS).copy()
            assert gpu.phase_solve()
            gpu.phase_backsub(1e-3)
            corr = gpu.buffer(B.BUF_CORRECTIONS).copy()
            s2 = sc.copy()
            gpu.ComputeInplace(spec.f0, s2, None, 4)
            res[fp32] = (S, corr, gpu.report.iterations, gpu.report.attempts, gpu.report.err_final)
    finally:
        gpu.set_schur_precision(False)
    S64, c64, it64, at64, e64 = res[False]
    S32, c32, it32, at32, e32 = res[True]
    assert np.abs(S32 - S64).max() < 2e-6 * np.abs(S64).max()
    assert np.abs(S32 - S64).max() > 0  # the switch really changes the arithmetic
    assert rel_err(c32, c64) < 2e-3
    assert (it32, at32) == (it64, at64)
    assert e32 == pytest.approx(e64, rel=1e-4)


# ------------------------------------------------------------------ f32 storage mode

F32_SCENES = {
    "ragged_wave": SCENES["ragged_wave"],                                                # per-observation derivative kernel
    "nf20_runs": sa.SceneSpec(n_frames=30, grid_nx=33, grid_ny=31, vis_window=20),      # k_jac_runs + k_schur_mm
    "nf22_grouped": sa.SceneSpec(n_frames=26, grid_nx=12, grid_ny=10, vis_window=22),   # k_schur_grouped
    "long_tracks": SCENES["long_tracks"],                                               # per-landmark Schur kernel
}


@pytest.mark.parametrize("name", list(F32_SCENES))
def test_f32_storage_mode_tolerance_table(orc, name):
    """srk_ba_set_storage_precision(1): the rank-2 factors of the point-frame blocks W are stored as float (half the bytes of
    what the derivative pass writes and the Schur and back-substitution passes read), widened on load; sums, reduced camera
    system and solve stay fp64.  Tolerance table:
      against the ORACLE WITH THE SAME FACTORS ROUNDED TO FLOAT (orc.set_w_storage_f32(2), round 4: formula 9 regrouped as
        Ap Af + Bp Bf, the four factors rounded, the products formed in double -- exactly what the library stores): W equal to
        1e-12 of the block scale in all but a handful of entries (a factor whose double value sits within an ulp of a float
        rounding boundary can round the other way on the two sides: at most two flipped factors an entry, 1.3e-7), reduced
        system 1e-9, the LM loop with the same accept / reject sequence and error rel 1e-6 -- i.e. the mode IS the fp64
        algorithm on identically rounded W;
      against the fp64 path: W 2.5e-7, reduced system 1.5e-6 of its largest entry, one-step corrections 1e-3, error rel 1e-4."""
    spec = F32_SCENES[name]
    sc = sa.generate_scene(spec)
    gpu = sa.BundleAdjustmentKanatani(0)
    res = {}
    try:
        for f32 in (False, True):
            gpu.set_storage_precision(f32)
            orc.set_w_storage_f32(2 if f32 else 0)
            out = _phases(orc, gpu, sc, spec.f0, 1e-4)
            # blocks: V, U, gradient are never rounded
            assert rel_err(out["V_g"], out["V_o"]) < 1e-12 and rel_err(out["U_g"], out["U_o"]) < 1e-12
            dW = np.abs(out["W_g"] - out["W_o"]) / np.abs(out["W_o"]).max()
            assert dW.max() < (1.3e-7 if f32 else 1e-12)
            assert np.quantile(dW, 0.999) < 1e-12         # identically rounded factors but for rare boundary cases
            red = _reduced_index(sc.M)
            keep = red >= 0
            assert rel_err(out["S_g"][np.ix_(keep, keep)], out["S_o"]) < (1e-9 if f32 else 1e-10)
            rc_o, rep_o, so, ok, rep, sg = _end_to_end(orc, gpu, sc, spec.f0, allowed=1e-9, max_factor=1e6, max_iterations=6)
            assert (rep.iterations, rep.attempts) == (rep_o.iterations, rep_o.attempts)
            lt.assert_same_trajectory(gpu.iteration_log(), rep_o.log, 1e-6, gpu_attempts=rep.attempts)
            assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-6)
            res[f32] = (out["S_g"].copy(), out["corr_g"].copy(), rep.err_final, out["W_g"].copy())
    finally:
        orc.set_w_storage_f32(0)
        gpu.close()
    S64, c64, e64, W64 = res[False]
    S32, c32, e32, W32 = res[True]
    assert 0 < np.abs(W32 - W64).max() < 2.5e-7 * np.abs(W64).max()     # the switch really changes the storage
    assert np.abs(S32 - S64).max() < 1.5e-6 * np.abs(S64).max()
    assert rel_err(c32, c64) < 1e-3
    assert e32 == pytest.approx(e64, rel=1e-4)


# ------------------------------------------------------------------ the f32 row against the reference's own float arithmetic

def _scene_distance(a, b):
    """largest absolute difference of two scenes' points and camera translations / rotations (normalised-world units)"""
    return max(float(np.abs(np.asarray(a.points, dtype=np.float64) - np.asarray(b.points, dtype=np.float64)).max()),
               float(np.abs(np.asarray(a.cam_T, dtype=np.float64) - np.asarray(b.cam_T, dtype=np.float64)).max()),
               float(np.abs(np.asarray(a.cam_R, dtype=np.float64) - np.asarray(b.cam_R, dtype=np.float64)).max()))


@pytest.mark.parametrize("name", list(F32_SCENES) + ["C1_dino_standin"])
def test_f32_modes_against_the_reference_float_build(orc, name):
    """SURVEY 8(f) row 4, pinned (round 4).  oracle/libba_oracle_f32.so is the CPU restatement compiled with the reference's
    `Scalar = float` (rt-config.h:41-48, suriko-engine/CMakeLists.txt:14-15,76-82): every operation rounded to float, as the
    reference's f32 build computes.  Its result after a fixed number of LM iterations lies at some distance d_ref from the
    fp64 restatement's (float arithmetic on a 1e-4-damped Gauss-Newton system loses a few digits per iteration) -- that
    distance is the tolerance the reference itself sets for "f32 mode".  The product's two f32 entry points
      (a) srk_ba_compute_inplace_f32: float arrays in and out, fp64 pipeline in between,
      (b) srk_ba_set_storage_precision(1): the point-frame factors stored as float, everything else fp64,
    must both stay INSIDE it: no further from the fp64 oracle than the reference's float build is (in error and in scene),
    and hence within 2 d_ref of the float build itself.  They are more accurate than the reference's f32 arithmetic by
    construction; the table printed below records by how much."""
    from oracle import oracle_f32 as o32
    if name == "C1_dino_standin":
        spec, sc = sa.CONFIGS[name], sa.config_scene(name)
        iters = 4
    else:
        spec, sc = F32_SCENES[name], sa.generate_scene(F32_SCENES[name])
        iters = 6
    f0 = float(np.float32(spec.f0))
    # float-representable inputs for everybody (what a caller built with Scalar = float hands over)
    f32 = {k: np.ascontiguousarray(getattr(sc, k), dtype=np.float32) for k in ("points", "cam_R", "cam_T", "K", "obs_uv")}
    sc64 = sa.Scene(f32["points"].astype(np.float64), f32["cam_R"].astype(np.float64), f32["cam_T"].astype(np.float64),
                    f32["K"].astype(np.float64), sc.shared_k, sc.row_ptr, sc.obs_frame, f32["obs_uv"].astype(np.float64))
    # fp64 oracle (skyline Cholesky on C1's 353 variables: the QR's own rounding is not the subject here)
    so = _orc_scene(orc, sc64)
    rc_o, rep_o, log_o = orc.compute_inplace(f0, so, None, None, iters, want_log=True)
    # the reference's float build
    s32 = o32.SceneF32(sc64)
    rc_f, rep_f = o32.compute_inplace(f0, s32, None, None, iters)
    assert rep_f.iterations >= 1 and np.isfinite(rep_f.err_final)
    d_err_ref = abs(rep_f.err_final - rep_o.err_final) / rep_o.err_final
    d_scene_ref = _scene_distance(s32, so)
    # a float build that works and is visibly float (measured: 3e-4 .. 0.3 in the error, 3e-4 .. 0.09 in the scene after
    # 4 - 6 iterations -- that wide a distance is what "f32 mode" means for the reference itself)
    assert 0 < d_err_ref < 1.0 and 0 < d_scene_ref < 1.0, (d_err_ref, d_scene_ref)
    floor_err, floor_scene = 1e-6, 4 * np.finfo(np.float32).eps * max(1.0, float(np.abs(so.points).max()))
    gpu = sa.BundleAdjustmentKanatani(0)
    try:
        # (a) the f32 boundary
        a = {k: v.copy() for k, v in f32.items()}
        gpu.ComputeInplaceF32(spec.f0, a["points"], a["cam_R"], a["cam_T"], a["K"], sc.shared_k, sc.row_ptr, sc.obs_frame,
                              a["obs_uv"], None, iters)
        rep_a = (gpu.report.iterations, gpu.report.attempts, gpu.report.err_final)
        log_a = gpu.iteration_log()

        class _S:  # (points, cam_T, cam_R holder for _scene_distance)
            pass
        sa_ = _S()
        sa_.points, sa_.cam_T, sa_.cam_R = a["points"], a["cam_T"], a["cam_R"]
        d_err_a = abs(rep_a[2] - rep_o.err_final) / rep_o.err_final
        d_scene_a = _scene_distance(sa_, so)
        # (b) f32 storage of the point-frame factors
        gpu.set_storage_precision(True)
        sb = sc64.copy()
        gpu.ComputeInplace(f0, sb, None, iters)
        rep_b = (gpu.report.iterations, gpu.report.attempts, gpu.report.err_final)
        d_err_b = abs(rep_b[2] - rep_o.err_final) / rep_o.err_final
        d_scene_b = _scene_distance(sb, so)
    finally:
        gpu.set_storage_precision(False)
        gpu.close()
    print(f"f32 row {name}: float build of the reference d_err {d_err_ref:.2e} d_scene {d_scene_ref:.2e} | f32 boundary "
          f"{d_err_a:.2e} {d_scene_a:.2e} | f32 storage {d_err_b:.2e} {d_scene_b:.2e} | iterations/attempts oracle "
          f"{rep_o.iterations}/{rep_o.attempts} float build {rep_f.iterations}/{rep_f.attempts} boundary {rep_a[0]}/{rep_a[1]} "
          f"storage {rep_b[0]}/{rep_b[1]}")
    assert d_err_a <= max(d_err_ref, floor_err) and d_scene_a <= max(d_scene_ref, floor_scene), (d_err_a, d_scene_a)
    assert d_err_b <= max(d_err_ref, floor_err) and d_scene_b <= max(d_scene_ref, floor_scene), (d_err_b, d_scene_b)
    # ... and the LM loop of the fp64 pipeline takes the fp64 oracle's decisions (the float build may fork: it is reported above)
    assert (rep_a[0], rep_a[1]) == (rep_o.iterations, rep_o.attempts)
    lt.assert_same_trajectory(log_a, log_o, max(d_err_ref, floor_err), gpu_attempts=rep_a[1])


# ------------------------------------------------------------------ deterministic mode (srk_ba_set_deterministic)

DET_SCENES = {
    "nf20_runs": (sa.SceneSpec(n_frames=30, grid_nx=33, grid_ny=31, vis_window=20), 0.0),          # uniform runs: k_schur_mm KIND 0
    "nf7_runs": (sa.SceneSpec(n_frames=60, grid_nx=40, grid_ny=30, vis_window=7, noise_uv_pix=0.2), 0.0),
    "ragged_17": (sa.SceneSpec(n_frames=60, grid_nx=40, grid_ny=30, vis_window=17, noise_uv_pix=0.3), 0.15),   # unions of <= 20 frames: KIND 1
}


@pytest.mark.parametrize("name", list(DET_SCENES))
def test_deterministic_mode_blocks_and_system_vs_oracle_and_bitwise_repeatable(orc, name):
    """srk_ba_set_deterministic(h, 1): the derivative kernel's frame sums and the Schur kernel's run sums go through staging
    buffers and an ordered second pass instead of fp64 atomics.  Same numbers as the oracle to the usual tolerances (blocks
    1e-12, system and right-hand side 1e-10, class-scaled), and IDENTICAL bits from two handles (the default mode differs in
    the last bits from run to run)."""
    spec, drop = DET_SCENES[name]
    sc = sa.generate_scene(spec)
    if drop:
        sc = sa.drop_observations(sc, drop, seed=7)
    outs = []
    for rep_ in range(2):
        gpu = sa.BundleAdjustmentKanatani(0)
        try:
            gpu.set_deterministic(True)
            out = _phases(orc, gpu, sc, spec.f0, 1e-4)
            assert gpu.deterministic()
            if rep_ == 0:
                _check(out, sc.M)
            outs.append({k: np.array(out[k], copy=True) for k in ("U_g", "gradE_g", "V_g", "S_g", "rhs_g", "corr_g", "pts_g", "T_g")})
        finally:
            gpu.close()
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


def test_deterministic_mode_lm_runs_are_bitwise_identical_on_the_bench_scene():
    """The bench workload (config 3), K = 20 iterations -- the run whose late iterations are rounding-level ties and whose
    attempt count differs from run to run in the default mode (55 or 56): in deterministic mode two runs from fresh handles
    give the same attempts, the same error bits and the same scene bits; and the run is still the oracle-checked algorithm
    (same iterations, error within 1e-9 of the default mode's after the converging phase)."""
    spec = sa.CONFIGS["C3_1kcam_100kpt"]
    sc = sa.config_scene("C3_1kcam_100kpt")
    res = []
    for rep_ in range(2):
        h = sa.BundleAdjustmentKanatani(0)
        try:
            h.set_deterministic(True)
            s2 = sc.copy()
            h.ComputeInplace(spec.f0, s2, None, 20)
            assert h.deterministic()
            log = h.iteration_log()
            res.append((h.report.iterations, h.report.attempts, h.report.err_final, s2, log["attempts"].copy(), log["err"].copy()))
        finally:
            h.close()
    a, b = res
    assert a[0] == b[0] == 20 and a[1] == b[1]
    assert a[2] == b[2] and np.array_equal(a[5], b[5]) and np.array_equal(a[4], b[4])
    assert np.array_equal(a[3].points, b[3].points) and np.array_equal(a[3].cam_R, b[3].cam_R) and np.array_equal(a[3].cam_T, b[3].cam_T)
    # against the default mode: the same converging phase (first ten iterations) to rounding
    h = sa.BundleAdjustmentKanatani(0)
    try:
        s3 = sc.copy()
        h.ComputeInplace(spec.f0, s3, None, 10)
        assert not h.deterministic()
        d_log = h.iteration_log()
    finally:
        h.close()
    assert np.array_equal(d_log["attempts"], a[4][:10])
    assert np.allclose(d_log["err"], a[5][:10], rtol=1e-9, atol=0)


def test_deterministic_mode_is_declined_for_scenes_it_does_not_cover(gpu):
    """Tracks over more than 20 frames take kernels the mode does not cover: the upload succeeds, the default kernels run and
    srk_ba_deterministic says 0."""
    spec = SCENES["long_tracks"]
    sc = sa.generate_scene(spec)
    try:
        gpu.set_deterministic(True)
        assert gpu.upload(spec.f0, sc)
        assert not gpu.deterministic()
    finally:
        gpu.set_deterministic(False)


# ------------------------------------------------------------------ speculative attempts

@pytest.mark.parametrize("name", ["ragged_wave", "pixel_noise", "ragged_20"])
def test_speculative_attempts_follow_the_sequential_loop(orc, name):
    """Two attempt slots (the next damping factor runs beside the current one) against one slot: the same accept /
    reject sequence, status, errors and scene -- and both equal to the oracle's loop."""
    if name in SCENES:
        spec, sc = SCENES[name], sa.generate_scene(SCENES[name])
    else:
        spec, frac = RAGGED[name]
        sc = sa.drop_observations(sa.generate_scene(spec), frac, seed=7)
    crit = sa.BundleAdjustmentKanataniTermCriteria()
    crit.AllowedReprojErrRelativeChange(1e-9)
    out = {}
    for spec_on in (True, False):
        h = sa.BundleAdjustmentKanatani(0)
        try:
            h.set_speculation(spec_on)
            s2 = sc.copy()
            ok = h.ComputeInplace(spec.f0, s2, crit, 12)
            r = h.report
            out[spec_on] = (ok, r.iterations, r.attempts, r.status, r.err_final, r.hessian_factor, s2, h.iteration_log())
        finally:
            h.close()
    a, b = out[True], out[False]
    assert a[:4] == b[:4] and a[1] >= 3 and a[2] > a[1]   # several iterations, some of them with rejected attempts
    assert a[4] == pytest.approx(b[4], rel=1e-9) and a[5] == pytest.approx(b[5])
    assert np.abs(a[6].points - b[6].points).max() < 1e-8 and np.abs(a[6].cam_T - b[6].cam_T).max() < 1e-8
    so = _orc_scene(orc, sc)
    rc_o, rep_o, log_o = orc.compute_inplace(spec.f0, so, 1e-9, None, 12, want_log=True)
    assert (a[1], a[2]) == (rep_o.iterations, rep_o.attempts) and a[0] == (rc_o == 0)
    for r in (a, b):  # each mode, iteration by iteration: a pair that counts its second slot in the wrong iteration fails here
        lt.assert_same_trajectory(r[7], log_o, 1e-6, gpu_attempts=r[2])


# ------------------------------------------------------------------ frames in another order than time (srk_ba_set_frame_reordering)

def _shuffled(spec, seed, drop=0.0):
    sc = sa.generate_scene(spec)
    if drop:
        sc = sa.drop_observations(sc, drop, seed=seed)
    return sa.renumber_frames(sc, np.random.RandomState(seed).permutation(sc.M))


UNORDERED = {
    # an unordered image set: the band is there, the numbering hides it
    "shuffled_60": lambda: _shuffled(sa.SceneSpec(n_frames=60, grid_nx=20, grid_ny=15, vis_window=6, noise_uv_pix=0.3), 1),
    "shuffled_ragged_45": lambda: _shuffled(sa.SceneSpec(n_frames=45, grid_nx=24, grid_ny=18, vis_window=9), 2, drop=0.3),
    # a sequence that closes a loop: band + corner blocks
    "loop_90": lambda: sa.loop_scene(sa.SceneSpec(n_frames=90, grid_nx=20, grid_ny=15, vis_window=0), window=6),
}


@pytest.mark.parametrize("name", list(UNORDERED))
@pytest.mark.parametrize("c", [1e-4, 10.0])
def test_phases_with_renumbered_frames_vs_oracle(orc, gpu, name, c):
    """The frames are renumbered inside (reverse Cuthill-McKee), the gauge stays on the caller's frames 0 and 1, every
    download comes back in the caller's order: the same checks as for any other scene, against the oracle run on the
    caller's numbering (the reference's dense system does not care, bundle-adj-kanatani.cpp:1911)."""
    sc = UNORDERED[name]()
    out = _phases(orc, gpu, sc, 600.0, c)
    to_int = gpu.frame_order()
    assert to_int is not None and sorted(to_int.tolist()) == list(range(sc.M))
    _check(out, sc.M)
    # selected rows of the system come back in the caller's numbering too
    rows = np.array([0, 3, 10, 16, 10 * sc.M - 1, 10 * (sc.M // 2) + 7], np.int64)
    gpu.phase_schur(c)
    full = gpu.buffer(B.BUF_RCS).reshape(10 * sc.M, 10 * sc.M)
    assert np.array_equal(gpu.rcs_rows(rows), np.tril(full)[rows])


@pytest.mark.parametrize("name", list(UNORDERED))
def test_compute_inplace_with_renumbered_frames_matches_oracle(orc, gpu, name):
    sc = UNORDERED[name]()
    rc_o, rep_o, so, ok, rep, sg = _end_to_end(orc, gpu, sc, 600.0, allowed=1e-10, max_factor=1e6, max_iterations=12)
    assert gpu.frame_order() is not None
    assert ok == (rc_o == 0) and sa.status_string(rep.status) == orc.status_string(rep_o.status)
    assert (rep.iterations, rep.attempts) == (rep_o.iterations, rep_o.attempts) and rep.iterations >= 1
    lt.assert_same_trajectory(gpu.iteration_log(), rep_o.log, 1e-6, gpu_attempts=rep.attempts, err_abs=1e-18)
    assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-6, abs=1e-18)
    assert np.abs(sg.points - so.points).max() < 1e-6
    assert np.abs(sg.cam_R - so.cam_R).max() < 1e-6
    assert np.abs(sg.cam_T - so.cam_T).max() < 1e-6


def test_renumbering_gives_an_unordered_400_frame_scene_its_chunked_solve_back():
    """400 frames, 20-frame tracks, frame numbers shuffled: in the caller's order the skyline is nearly the full triangle
    and the solve is one chain; renumbered, the system is the band of the time-ordered sequence again and is cut into
    chunks.  Both runs take the same decisions and end in the same scene."""
    spec = sa.SceneSpec(n_frames=400, grid_nx=80, grid_ny=50, vis_window=20, noise_uv_pix=0.2)
    sc = _shuffled(spec, 7)
    res = {}
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        for mode in (0, -1):
            ba.set_frame_reordering(mode)
            s2 = sc.copy()
            ba.ComputeInplace(spec.f0, s2, None, 4)
            res[mode] = (ba.report.iterations, ba.report.attempts, ba.report.err_final, s2, ba.rcs_chunks(), ba.rcs_fill(),
                         ba.frame_order())
        assert res[0][6] is None and res[-1][6] is not None
        assert res[0][4] == 0 and res[-1][4] >= 2
        assert res[-1][5] < 0.3 < res[0][5]
        assert res[0][:2] == res[-1][:2]
        assert res[-1][2] == pytest.approx(res[0][2], rel=1e-8)
        assert np.abs(res[-1][3].points - res[0][3].points).max() < 1e-8
        assert np.abs(res[-1][3].cam_T - res[0][3].cam_T).max() < 1e-8
        # a time-ordered sequence is left alone; forcing the ordering on it changes nothing but the summation order
        tm = sa.generate_scene(spec)
        ba.set_frame_reordering(-1)
        assert ba.upload(spec.f0, tm) and ba.frame_order() is None
        # the exchange cannot be configured on a renumbered scene (every shard would find its own numbering)
        assert ba.upload(spec.f0, sc) and ba.frame_order() is not None
        with pytest.raises(RuntimeError):
            ba.set_covisibility(sa.ba.covisibility(sc))
    finally:
        ba.close()


# ------------------------------------------------------------------ the benchmarked run, attempt by attempt

_C3_ORACLE = {}


def _c3_normalized():
    """the bench's scene: C3, gauge-normalised once on the host (bench.py)"""
    sc = sa.config_scene("C3_1kcam_100kpt")
    ok, _ = sa.normalize_scene_inplace(sc)
    assert ok
    return sc


def _c3_oracle_run(orc):
    """the oracle's loop on the bench's normalised C3 scene, 20 iterations, skyline Cholesky, min(16, cpus) threads (once
    per module): (log, report, final scene, seconds)"""
    if not _C3_ORACLE:
        import time
        so = _orc_scene(orc, _c3_normalized())
        threads = orc.get_threads()
        orc.set_solver(1)
        orc.set_threads(min(16, os.cpu_count() or 1))
        try:
            t0 = time.perf_counter()
            rc, rep, log = orc.compute_inplace(sa.CONFIGS["C3_1kcam_100kpt"].f0, so, None, None, 20, want_log=True)
            sec = time.perf_counter() - t0
        finally:
            orc.set_solver(0)
            orc.set_threads(threads)
        assert rc == 1 and orc.status_string(rep.status) == "max iterations" and rep.iterations == 20
        lt.check_log_consistent(log, rep)
        print(f"C3 oracle loop: {sec:.1f} s at {min(16, os.cpu_count() or 1)} threads, {rep.attempts} attempts, per iteration "
              f"{lt.fold(log)['attempts'].tolist()}")
        _C3_ORACLE.update(log=log, rep=rep, scene=so, sec=sec)
    return _C3_ORACLE


def _bench_shape_run(sc, deterministic, speculation=True, warm_up=5, groups=None, f0=None):
    """bench.py's timed region on a fresh handle: upload(already_normalized=True), optimize(warm_up), reset(), optimize(20);
    warm_up = 0: no warm-up and no reset.  Returns (report, iteration log, downloaded scene (normalised), K of the groups)"""
    f0 = sa.CONFIGS["C3_1kcam_100kpt"].f0 if f0 is None else f0
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_profile(0)
        h.set_deterministic(deterministic)
        h.set_speculation(speculation)
        if groups is not None:
            h.set_intrinsic_groups(groups)
        assert h.upload(f0, sc, already_normalized=True)
        if warm_up:
            h.optimize(None, max_iterations=warm_up)
            assert h.report.iterations == warm_up
            h.reset()
        h.optimize(None, max_iterations=20)
        rep = h.report
        s2 = sc.copy()
        h.download(s2, revert_normalization=False)
        K = h.download_intrinsics() if groups is not None else None
        return rep, h.iteration_log(), s2, K
    finally:
        h.close()


def test_c3_bench_run_vs_the_oracle_loop_attempt_by_attempt(orc):
    """The benchmarked run (bench.py: C3 normalised on the host, upload(already_normalized=True), a 5-iteration warm-up,
    reset(), optimize(20)) in deterministic mode against the oracle's loop on the same normalised scene (skyline Cholesky):
    20 iterations, "max iterations", every accepted iteration with the oracle's attempt count and damping factor, err_final
    rel 1e-6, scene abs 1e-6.  The oracle normalises the scene it is given once more; on an already normalised C3 scene
    that moves the points by 1.2e-14, cam_T by 2e-14 and cam_R by 7e-16 (world scale 1 + 1e-15), so both loops start
    from the same scene to rounding.
    Past the converging phase (iterations 1..11) the run sits at the noise floor: the oracle accepts iterations 12..20 by
    margins of 2e-13 and rejects their first attempts by 3e-13 .. 6e-11.  A fork there is allowed only at a decision on a
    margin below 1e-10 (lm_trajectory.TIE_MARGIN); DESIGN 2 records what the GPU does there."""
    o = _c3_oracle_run(orc)
    rep, log, s2, _ = _bench_shape_run(_c3_normalized(), deterministic=True)
    print(f"C3 deterministic bench run: {rep.attempts} attempts, per iteration {log['attempts'].tolist()}; oracle "
          f"{o['rep'].attempts}")
    assert rep.iterations == 20 and sa.status_string(rep.status) == "max iterations"
    fork = lt.assert_same_trajectory(log, o["log"], 1e-6, gpu_attempts=None, allow_tie_fork=True)
    if fork is None:
        assert rep.attempts == o["rep"].attempts
    else:
        print(f"deterministic run parts from the oracle at a tie in iteration {fork + 1}: margin "
              f"{lt.decisive_margin(log, o['log'], fork):+.3e}")
        assert fork >= 11
    assert rep.err_final == pytest.approx(o["rep"].err_final, rel=1e-6)
    so = o["scene"]
    assert np.abs(s2.points - so.points).max() < 1e-6
    assert np.abs(s2.cam_R - so.cam_R).max() < 1e-6 and np.abs(s2.cam_T - so.cam_T).max() < 1e-6


def test_c3_default_mode_bench_run_vs_the_oracle_loop(orc):
    """The same run in the default mode (speculative pairs, fp64 atomics: what the bench line measures): the converging
    phase (the first 11 iterations, bench.py's converging_phase) matches the oracle iteration by iteration with the error
    rel 1e-9; after it the first place the attempts differ, if any, must be a tie (oracle margin < 1e-10)."""
    o = _c3_oracle_run(orc)
    rep, log, s2, _ = _bench_shape_run(_c3_normalized(), deterministic=False)
    print(f"C3 default-mode bench run: {rep.attempts} attempts, per iteration {log['attempts'].tolist()}")
    assert rep.iterations == 20 and sa.status_string(rep.status) == "max iterations"
    lt.assert_same_trajectory(log, o["log"], 1e-9, n_iter=11)
    fork = lt.assert_same_trajectory(log, o["log"], 1e-6, allow_tie_fork=True)
    if fork is not None:
        print(f"default-mode run parts from the oracle at a tie in iteration {fork + 1}: margin "
              f"{lt.decisive_margin(log, o['log'], fork):+.3e}")


@pytest.mark.parametrize("speculation", [True, False])
def test_reset_after_a_warm_up_reproduces_a_fresh_run(speculation):
    """reset() is the bench's state machine: after a 5-iteration warm-up, reset() and optimize(20) must give, bit for bit in
    deterministic mode, what a fresh handle's first optimize(20) gives -- iteration log, report and scene: the current /
    trial slot swap, the attempt slots and the damping factor start over."""
    sc = _c3_normalized()
    a = _bench_shape_run(sc, deterministic=True, speculation=speculation, warm_up=5)
    b = _bench_shape_run(sc, deterministic=True, speculation=speculation, warm_up=0)
    _assert_same_run(a, b)


def _assert_same_run(a, b):
    (ra, la, sa_, Ka), (rb, lb, sb, Kb) = a, b
    assert (ra.iterations, ra.attempts, ra.status, ra.err_initial, ra.err_final, ra.hessian_factor) == \
        (rb.iterations, rb.attempts, rb.status, rb.err_initial, rb.err_final, rb.hessian_factor)
    for k in ("attempts", "err", "hessian_factor"):
        assert np.array_equal(la[k], lb[k]), k
    for k in ("points", "cam_R", "cam_T"):
        assert np.array_equal(getattr(sa_, k), getattr(sb, k)), k
    if Ka is not None:
        assert np.array_equal(Ka, Kb)


def test_reset_restores_the_uploaded_intrinsics_in_shared_k_mode():
    """Shared intrinsics on C1 (one group, K off by 3 % and 5 px): the warm-up moves K; reset() must restore the uploaded K,
    so that warm-up + reset + 20 iterations equals a fresh handle's 20 iterations, K included (deterministic mode)."""
    f0 = sa.CONFIGS["C1_dino_standin"].f0
    sc = sa.config_scene("C1_dino_standin")
    K = sc.K.reshape(-1, 9).copy()
    K[:, 0] *= 1.03
    K[:, 4] *= 1.03
    K[:, 2] += 5.0 * K[:, 8] / f0
    K[:, 5] += 5.0 * K[:, 8] / f0
    sc = sa.Scene(sc.points, sc.cam_R, sc.cam_T, K, sc.shared_k, sc.row_ptr, sc.obs_frame, sc.obs_uv)
    ok, _ = sa.normalize_scene_inplace(sc)
    assert ok
    groups = np.zeros(sc.M, dtype=np.int32)
    a = _bench_shape_run(sc, deterministic=True, warm_up=5, groups=groups, f0=f0)
    b = _bench_shape_run(sc, deterministic=True, warm_up=0, groups=groups, f0=f0)
    assert not np.array_equal(a[3], K.reshape(-1, 3, 3)[:1])   # K moved
    _assert_same_run(a, b)
