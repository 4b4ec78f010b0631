"""Per-frame and per-group intrinsics through every kernel and host path that reads a camera pack.

srk_scene_generate writes one K into every frame, so on its scenes a kernel, a re-pack or a permutation that took another
frame's (or group's) intrinsics computes the right numbers.  The scenes of tests/hetero_cases.py give every frame its own fx,
fy, u0 and v0 (15 % apart) and leave the rays, and with them the conditioning, as they were; tests/test_hetero_cpu.py
checks on the CPU that the yardsticks alone stay inside the tolerances on them.

Nothing here has a tolerance of its own: the checks are those of tests/test_gpu_parity.py (_phases / _check: blocks 1e-12
per variable class, system 1e-10, corrections max(corr_tol, 4 d_qr) with the call site's corr_tol: 1e-7 as on its synthetic
scenes where this file calls _check, 1e-8 inside its renumbered-frame and deterministic-mode tests), test_gpu_calibrated.py,
test_gpu_information.py, test_gpu_constant.py and test_gpu_shared_k.py, imported and run on these scenes; where an existing
check is a test function over a table of scenes, that function is called with the table pointing at the heterogeneous scene.
tests/test_hetero_cpu.py holds 4 d_qr below the corr_tol of every use, so none of them is widened.

What reads a K, and the test that now runs it with distinct ones (a kernel is asserted where the library tells which one ran:
jacobian_kernel(); the error and Schur kernels follow from it and from the track lengths by the host's selection rules):
  k_jac_points / k_jac_frames, k_jac_fused, k_jac_runs uniform and masked
                                              test_derivative_and_error_kernels, test_derivatives_after_an_accepted_step
  k_error_staged (launched whenever every workgroup's frame window fits, which jacobian_kernel() == 1 asserts for fused_12;
    windows with a first frame > 0)           test_derivative_and_error_kernels[fused_12]
  k_error_staged_robust                       test_huber_and_information[fused_12]
  k_obs_weights, k_obs_residuals              test_huber_and_information
  k_cam_apply (the re-pack after a step)      test_derivatives_after_an_accepted_step, test_ten_lm_iterations_vs_the_oracle_loop
  k_const_cam_keep                            test_constant_blocks
  Kexp under reverse Cuthill-McKee            test_phases_with_renumbered_frames, test_compute_inplace_with_renumbered_frames
  srk_ba_reset_scene                          test_reset_restores_every_frames_pack, test_reset_restores_each_groups_own_k
  landmark shards of two ranks                test_two_ranks_on_one_gpu_match_world_size_one
  srk_ba_compute_inplace_f32                  test_f32_boundary
  srk_ba_reproj_error / _mvf                  test_reproj_error_entry_points
  calibrated mode (set_fixed_intrinsics)      test_calibrated, test_huber_and_information[6]
  group-to-frame expansion, shared intrinsics test_shared_intrinsics_with_distinct_group_k, test_one_group_with_per_frame_k_is_refused
  f32 storage, deterministic mode             test_f32_storage, test_deterministic_mode
  (k_schur_mm, k_schur_grouped, k_schur_long read no K: test_schur_paths gives them W that differs per frame)

A k_cam_apply that re-packs with K instead of K + 9 j is caught by every test here that compares with a yardstick after a step;
before this file only the golden inputs and the shared-intrinsics tests with two or more groups caught it.  A Kexp that is
not permuted with the frames is caught by the renumbered-frame tests here and by no earlier test.
"""
import os

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import ba as B
import constant_cases as cc
import hetero_cases as hc
import lm_trajectory as lt
import robust_ref as rr
import test_gpu_calibrated as tcal
import test_gpu_constant as tcon
import test_gpu_information as tinf
import test_gpu_parity as tp
import test_gpu_shared_k as tshk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    h = sa.BundleAdjustmentKanatani(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def cal():
    h = sa.BundleAdjustmentKanatani(0)
    h.set_fixed_intrinsics(True)
    yield h
    h.close()


def _phases_in_mode(orc, gpu, name, c):
    sc, f0 = hc.case(name)
    _, mode, kernel = hc.CASES[name][:3]
    gpu.set_jacobian_mode(mode)
    try:
        out = tp._phases(orc, gpu, sc, f0, c)
        if kernel is not None:
            assert gpu.jacobian_kernel() == kernel
    finally:
        gpu.set_jacobian_mode(-1)
    return sc, f0, out


# ------------------------------------------------------------------ derivative and error kernels

@pytest.mark.parametrize("c", hc.DAMPINGS)
@pytest.mark.parametrize("name", hc.DERIVATIVE_CASES)
def test_derivative_and_error_kernels(orc, gpu, name, c):
    """k_jac_points / k_jac_frames (0), k_jac_fused (1), k_jac_runs uniform (2) and masked (3), and the error kernel that goes
    with each (k_error_staged with the fused kernel's frame windows).  The fused and the run case have workgroups whose camera
    window in LDS starts at a later frame than 0: a pack indexed by the frame instead of frame - first frame would show."""
    sc, f0, out = _phases_in_mode(orc, gpu, name, c)
    assert gpu.frame_order() is None  # the library's frames are the caller's: block_first_frames() describes its workgroups
    if name in ("fused_12", "runs_nf16"):
        jmin = hc.block_first_frames(sc)
        assert len(jmin) > 1 and jmin[1:].max() > 0
    assert hc.distinct_intrinsics(sc) == (sc.M,) * 4
    tp._check(out, sc.M, corr_tol=hc.CORR_TOL)


@pytest.mark.parametrize("name", hc.DERIVATIVE_CASES)
def test_derivatives_after_an_accepted_step(orc, gpu, name):
    """After phase_accept the camera packs are rebuilt from the stepped poses and every frame's own K (k_cam_apply).  A second
    phase_derivatives against the oracle AT THE LIBRARY'S STEPPED SCENE holds the packs to 1e-12; the error after a step, which
    is all the one-step checks see of them, only to 1e-6."""
    sc, f0 = hc.case(name)
    _, mode, kernel = hc.CASES[name][:3]
    gpu.set_jacobian_mode(mode)
    try:
        out = tp._phases(orc, gpu, sc, f0, 1e-4)
        so = orc.Scene(out["pts_g"], out["R_g"], out["T_g"], sc.K, 0, sc.row_ptr, sc.obs_frame, sc.obs_uv)
        e_o, _ = orc.reproj_error(f0, so)
        assert out["err2_g"] == pytest.approx(e_o, rel=1e-12)
        gradE, V, U, W = orc.derivatives(f0, so)
        gpu.phase_derivatives()
        assert gpu.jacobian_kernel() == kernel
        tp._check_blocks_by_class(gpu.buffer(B.BUF_POINT_BLOCKS).reshape(-1, 3, 3), V, gpu.buffer(B.BUF_FRAME_BLOCKS).reshape(-1, 10, 10),
                                  U, gpu.buffer(B.BUF_POINT_FRAME).reshape(-1, 3, 10), W, gpu.buffer(B.BUF_GRAD), gradE, e_o)
    finally:
        gpu.set_jacobian_mode(-1)


# ------------------------------------------------------------------ Schur kernels

@pytest.mark.parametrize("c", hc.DAMPINGS)
@pytest.mark.parametrize("name", hc.SCHUR_CASES)
def test_schur_paths(orc, gpu, name, c):
    """k_schur_mm on ragged runs, k_schur_grouped on unions of 22 .. 24 frames, k_schur_long beyond: they do not read K, the
    point-frame blocks they sum differ from frame to frame now"""
    sc, f0, out = _phases_in_mode(orc, gpu, name, c)
    nf = np.diff(sc.row_ptr)
    if name == "schur_mm_ragged_7":
        assert nf.max() <= 7 and len({sc.obs_frame[sc.row_ptr[i]:sc.row_ptr[i + 1]].tobytes() for i in range(sc.N)}) > sc.N // 4
    elif name == "schur_grouped_23":
        assert 20 < nf.max() <= 24
    else:
        assert nf.max() > 24
    tp._check(out, sc.M, corr_tol=hc.CORR_TOL)


# ------------------------------------------------------------------ frames renumbered inside

@pytest.mark.parametrize("c", hc.DAMPINGS)
@pytest.mark.parametrize("name", hc.UNORDERED_CASES)
def test_phases_with_renumbered_frames(orc, gpu, monkeypatch, name, c):
    """the intrinsics are drawn BEFORE the frames are shuffled, the library renumbers the frames again (reverse
    Cuthill-McKee) and has to take every K along: tests/test_gpu_parity.py's test on its table of unordered scenes"""
    sc, _ = hc.case(name)
    assert hc.distinct_intrinsics(sc) == (sc.M,) * 4
    monkeypatch.setitem(tp.UNORDERED, name, lambda: sc.copy())
    tp.test_phases_with_renumbered_frames_vs_oracle(orc, gpu, name, c)


@pytest.mark.parametrize("name", hc.UNORDERED_CASES)
def test_compute_inplace_with_renumbered_frames(orc, gpu, monkeypatch, name):
    sc, _ = hc.case(name)
    monkeypatch.setitem(tp.UNORDERED, name, lambda: sc.copy())
    tp.test_compute_inplace_with_renumbered_frames_matches_oracle(orc, gpu, name)


# ------------------------------------------------------------------ modes

@pytest.mark.parametrize("c", [1e-4, 1e-1])
@pytest.mark.parametrize("name", ["runs_nf16", "schur_long_34"])
def test_calibrated(orc, cal, name, c):
    """fixed intrinsics are for cameras with known, different K: six variables a frame against calibrated_ref"""
    sc, f0 = hc.case(name)
    mode, kernel = hc.CASES[name][1:3]
    cal.set_jacobian_mode(mode)
    try:
        tcal._phases(orc, cal, sc, f0, c)
        if kernel is not None:
            assert cal.jacobian_kernel() == kernel
    finally:
        cal.set_jacobian_mode(-1)


@pytest.mark.parametrize("name", ["union_ragged_20", "fused_12"])
@pytest.mark.parametrize("fv", [10, 6])
def test_huber_and_information(orc, gpu, cal, fv, name):
    """Huber's weights and information with some q = 0 on the union case and on the fused case (the robust error kernel with
    staged cameras); observation_weights() and observation_residuals() (k_obs_weights, k_obs_residuals) per observation in the
    caller's order"""
    sc, f0, q = hc.huber_information_case(name)
    mode, kernel = hc.CASES[name][1:3]
    assert tinf._phases(orc, {10: gpu, 6: cal}[fv], sc, q, f0, rr.HUBER, 2.0, fv, 1e-4, mode) == kernel


def test_constant_blocks(orc):
    """constant frames and landmarks (k_const_cam_keep among the masking passes): constant frames keep the bits of R and T"""
    _, _, fconst, pconst, keep_gauge, fv = cc.case(cc.MODE_CASE)
    sc, f0 = hc.case("runs_nf16")
    assert fconst.shape == (sc.M,) and pconst.shape == (sc.N,) and fconst.any() and pconst.any()
    h = tcon._handle(fv)
    try:
        tcon._set(h, fconst, pconst, keep_gauge)
        tcon._phases(orc, h, sc, f0, 1e-4, fconst, pconst, keep_gauge, fv)
    finally:
        h.close()


def _run_on(monkeypatch, sc, spec, test, *args):
    """tests/test_gpu_parity.py's mode tests generate their scene from a table of specs: run `test` with this scene handed to it
    in place of the one generated from `spec` -- exactly once and for exactly that spec, or the test did not run on it"""
    calls = []

    def stand_in(asked, with_gt=False):
        assert asked == spec and not with_gt, asked
        calls.append(asked)
        return sc.copy()

    with monkeypatch.context() as m:
        m.setattr(tp.sa, "generate_scene", stand_in)
        test(*args)
    assert len(calls) == 1


def test_f32_storage(orc, monkeypatch):
    """the float factors of W against orc.set_w_storage_f32(2): test_f32_storage_mode_tolerance_table on the run case"""
    sc, _ = hc.case("runs_nf16")
    spec = sa.SceneSpec(n_frames=24, grid_nx=30, grid_ny=20, vis_window=16)
    monkeypatch.setitem(tp.F32_SCENES, "hetero", spec)
    _run_on(monkeypatch, sc, spec, tp.test_f32_storage_mode_tolerance_table, orc, "hetero")


def test_deterministic_mode(orc, monkeypatch):
    """the ordered sums: against the oracle and bitwise repeatable over two handles"""
    sc, _ = hc.case("runs_nf16")
    spec = sa.SceneSpec(n_frames=24, grid_nx=30, grid_ny=20, vis_window=16)
    monkeypatch.setitem(tp.DET_SCENES, "hetero", (spec, 0.0))
    _run_on(monkeypatch, sc, spec, tp.test_deterministic_mode_blocks_and_system_vs_oracle_and_bitwise_repeatable, orc, "hetero")


def test_reset_restores_every_frames_pack():
    """srk_ba_reset_scene rebuilds the camera packs of the uploaded scene: after three iterations and a reset the derivative
    blocks are those of the fresh upload, bit for bit in deterministic mode"""
    sc, f0 = hc.case("runs_nf16")
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_deterministic(True)
        assert h.upload(f0, sc) and h.deterministic()
        e0 = h.phase_error()[0]
        h.phase_derivatives()
        first = [h.buffer(b).copy() for b in (B.BUF_FRAME_BLOCKS, B.BUF_POINT_BLOCKS, B.BUF_GRAD)]
        h.optimize(None, max_iterations=3)
        assert h.report.iterations == 3 and h.phase_error()[0] < e0
        h.reset()
        assert h.phase_error()[0] == e0
        h.phase_derivatives()
        for a, b in zip(first, (B.BUF_FRAME_BLOCKS, B.BUF_POINT_BLOCKS, B.BUF_GRAD)):
            assert np.array_equal(a, h.buffer(b))
    finally:
        h.close()


# ------------------------------------------------------------------ shared intrinsics, every group its own K

def _grouped(G, seed=5):
    sc, f0 = hc.same_k("groups_48")
    groups = hc.groups_of(sc.M, G)
    het = hc.per_group_intrinsics(sc, f0, groups, hc.SPREAD, seed)
    assert hc.distinct_intrinsics(het) == (G,) * 4
    return het, f0, groups


@pytest.mark.parametrize("c", [1e-4, 1e-1])
@pytest.mark.parametrize("G", [2, 32])
def test_shared_intrinsics_with_distinct_group_k(orc, G, c):
    """every group starts from its own K (so far all groups started from one and differed by a step's corrections): the
    group-to-frame expansion, the folded system and download_intrinsics() group by group against shared_k_ref"""
    sc, f0, groups = _grouped(G)
    h = sa.BundleAdjustmentKanatani(0)
    try:
        tshk._phases(orc, h, sc, f0, groups, c)
    finally:
        h.close()


@pytest.mark.parametrize("G", [2, 32])
def test_reset_restores_each_groups_own_k(G):
    sc, f0, groups = _grouped(G)
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_intrinsic_groups(groups)
        assert h.upload(f0, sc) and h.intrinsic_groups() == G
        K0 = h.download_intrinsics()
        first = np.array([np.flatnonzero(groups == g)[0] for g in range(G)])
        Kup = sc.K.reshape(-1, 3, 3)[first]
        assert np.abs(K0 - Kup).max() <= 4 * np.finfo(np.float64).eps * np.abs(Kup).max()  # each group's own, in the caller's convention
        h.optimize(None, max_iterations=3)
        assert h.report.iterations == 3
        K1 = h.download_intrinsics()
        assert np.all(np.any((K1 != K0).reshape(G, -1), axis=1))  # every group's K moved
        h.reset()
        assert np.array_equal(h.download_intrinsics(), K0)
    finally:
        h.close()


def test_one_group_with_per_frame_k_is_refused():
    sc, f0 = hc.case("groups_48")
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_intrinsic_groups(np.zeros(sc.M, dtype=np.int32))
        with pytest.raises(ValueError):
            h.upload(f0, sc)
        assert "different intrinsics" in h.last_error()
        # two groups fed the K of 32: refused as well
        het32, _, _ = _grouped(32)
        h.set_intrinsic_groups(hc.groups_of(sc.M, 2))
        with pytest.raises(ValueError):
            h.upload(f0, het32)
        assert "different intrinsics" in h.last_error()
    finally:
        h.close()


# ------------------------------------------------------------------ the LM loop

@pytest.mark.parametrize("name", ["runs_nf16", "C1"])
def test_ten_lm_iterations_vs_the_oracle_loop(orc, gpu, name):
    """attempt by attempt (lm_trajectory); tests/test_hetero_cpu.py checks that no decision of the oracle's run is a tie"""
    sc, f0 = hc.c1() if name == "C1" else hc.case(name)
    rc_o, rep_o, so, ok, rep, sg = tp._end_to_end(orc, gpu, sc, f0, max_iterations=10)
    assert not ok and rc_o == 1 and sa.status_string(rep.status) == orc.status_string(rep_o.status) == "max iterations"
    assert rep.iterations == rep_o.iterations == 10 and rep.attempts == rep_o.attempts
    lt.assert_same_trajectory(gpu.iteration_log(), rep_o.log, 1e-6, gpu_attempts=rep.attempts)
    assert rep.err_initial == pytest.approx(rep_o.err_initial, rel=1e-12)
    assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-6)
    assert np.abs(sg.points - so.points).max() < 1e-6
    assert np.abs(sg.cam_R - so.cam_R).max() < 1e-6
    assert np.abs(sg.cam_T - so.cam_T).max() < 1e-6
    assert np.array_equal(sg.K, sc.K)


# ------------------------------------------------------------------ other entry points

def test_reproj_error_entry_points(orc, gpu):
    """srk_ba_reproj_error and srk_ba_reproj_error_mvf pack the cameras of the scene they are given on their own"""
    sc, f0 = hc.case("two_kernel_60")
    e, seen = gpu.ReprojError(f0, sc)
    eo, so = orc.reproj_error(f0, tp._orc_scene(orc, sc))
    assert seen == so == sc.O and e == pytest.approx(eo, rel=1e-12)
    spec = sa.SceneSpec(n_frames=9, grid_nx=7, grid_ny=6, vis_window=4, f0=1.0)
    het = hc.per_frame_intrinsics(sa.generate_scene(spec), 1.0, hc.SPREAD, 2)
    ok, e, n = gpu.ReprojErrorMvf(1.0, het)
    oko, eo, no = orc.reproj_error_mvf(1.0, tp._orc_scene(orc, het))
    assert ok and oko and n == no == het.O and e == pytest.approx(eo, rel=1e-12)


def test_f32_boundary(gpu, monkeypatch):
    """srk_ba_compute_inplace_f32 widens every frame's K: test_f32_boundary_matches_f64_run_on_the_same_rounded_inputs"""
    sc, _ = hc.case("pixel_noise_12")
    assert sc.O == sa.generate_scene(tp.SCENES["pixel_noise"]).O  # the scene of that test, with per-frame intrinsics
    _run_on(monkeypatch, sc, tp.SCENES["pixel_noise"], tp.test_f32_boundary_matches_f64_run_on_the_same_rounded_inputs, gpu)


def test_two_ranks_on_one_gpu_match_world_size_one(tmp_path):
    """landmark shards of two ranks, the cameras (and every K) replicated: tests/test_gpu_multirank.py's comparison"""
    import torch.multiprocessing as mp
    import _dist_gpu_worker
    kw = dict(n_frames=30, grid_nx=23, grid_ny=17, vis_window=7)
    iters, world, seed = 3, 2, 4
    ref = hc.per_frame_intrinsics(sa.generate_scene(sa.SceneSpec(**kw)), 600.0, hc.SPREAD, seed)
    assert hc.distinct_intrinsics(ref) == (ref.M,) * 4
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        crit = sa.BundleAdjustmentKanataniTermCriteria()
        crit.AllowedReprojErrRelativeChange(1e-7)
        ok_ref = ba.ComputeInplace(600.0, ref, crit, iters)
        rep = ba.report
        want = (rep.iterations, rep.attempts, rep.seen, rep.status)
        e_initial, e_final = rep.err_initial, rep.err_final
    finally:
        ba.close()
    mp.spawn(_dist_gpu_worker.run, args=(world, 0, str(tmp_path), dict(kw, _hetero=seed), iters, "dp"), nprocs=world, join=True)
    res = [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(world)]
    assert res[0]["lo"] == 0 and res[-1]["hi"] == ref.N and int(res[1]["lo"]) == int(res[0]["hi"])
    for z in res:
        assert bool(z["ok"]) == ok_ref
        assert (int(z["iterations"]), int(z["attempts"]), int(z["seen"]), int(z["status"])) == want
        assert float(z["err_initial"]) == pytest.approx(e_initial, rel=1e-12)
        assert float(z["err_final"]) == pytest.approx(e_final, rel=1e-8)
        assert np.array_equal(z["cam_R"], res[0]["cam_R"]) and np.array_equal(z["cam_T"], res[0]["cam_T"])
        assert np.abs(z["cam_T"] - ref.cam_T).max() < 1e-7 and np.abs(z["cam_R"] - ref.cam_R).max() < 1e-7
        assert np.abs(z["points"] - ref.points[int(z["lo"]):int(z["hi"])]).max() < 1e-7
