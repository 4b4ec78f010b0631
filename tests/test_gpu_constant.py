"""Constant parameter blocks on the GPU (srk_ba_set_constant_blocks) against the yardstick of tests/constant_ref.py -- the
oracle's blocks restricted to the free blocks, orc.two_phase with the gauge kept and a dense numpy Schur complement without
it -- and the LM loop of bundle-adj-kanatani.cpp:720-893 around it.  The cases are those of tests/constant_cases.py, each
checked for conditioning by tests/test_constant_cpu.py.

Tolerances as the existing parity tests: blocks 1e-12 per variable class, reduced camera system and rhs 1e-10 symmetric-scaled,
corrections and the applied scene 1e-8 relative, widened as tests/test_gpu_parity.py does to four times the distance of the
yardstick's own solver (the oracle's Householder QR on the unscaled system) from the exact solution of its system.  Identity
rows, zero right-hand sides and zero corrections are exact, constant blocks of the resident scene bit-equal.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import ba as B
from surikatoko_amd import _lib
from conftest import rel_err, sym_scaled_err, class_rel_err
import constant_cases as cc
import constant_ref as kref
import lm_trajectory as lt
import weighted_ref as wr
from gpu_common import orc_scene as _orc_scene, handle as _handle, run_lm as _run, compare_runs as _compare_runs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _set(h, fconst, pconst, keep_gauge):
    h.set_constant_blocks(fconst if fconst.any() else None, pconst if pconst.any() else None, bool(keep_gauge))


def _phases(orc, gpu, sc, f0, c, fconst, pconst, keep_gauge, fv, derivatives=None, energy=None, w_tol=1e-12, s_tol=1e-10,
            corr_tol=1e-8):
    """derivatives -> schur -> solve -> backsub -> accept on both sides, checked; gpu has the constant blocks set"""
    so = _orc_scene(orc, sc)
    assert orc.normalize(so)[0]
    assert gpu.upload(f0, sc) and gpu.frame_vars() == fv
    N, M, off = sc.N, sc.M, 10 - fv
    ref = kref.step(orc, f0, so, c, fconst, pconst, keep_gauge, fv, want_system=True, derivatives=derivatives)
    assert ref["ok"]
    gE, Vo, Uo, Wo = ref["blocks"][:4]
    eo = energy(so) if energy else orc.reproj_error(f0, so)[0]
    P0, R0, T0 = (gpu.buffer(b).copy() for b in (B.BUF_POINTS, B.BUF_CAM_R, B.BUF_CAM_T))
    pobs = pconst[kref.obs_points(so)]
    idx = kref.frame_var_index(M, fv)
    fixed = ref["fixed"][idx]  # over the library's fv M frame variables
    cvar = np.repeat(fconst, fv)

    gpu.phase_derivatives()
    Vg = gpu.buffer(B.BUF_POINT_BLOCKS).reshape(-1, 3, 3)
    Ug = gpu.buffer(B.BUF_FRAME_BLOCKS).reshape(M, fv, fv)
    Wg = gpu.buffer(B.BUF_POINT_FRAME).reshape(-1, 3, fv)
    gg = gpu.buffer(B.BUF_GRAD)
    dV = np.sqrt(np.abs(np.einsum("nii->ni", Vo)))
    dU = np.sqrt(np.abs(np.einsum("mii->mi", Uo)))[:, off:]
    assert np.all(Vg[pconst] == np.eye(3))                          # constant landmarks: the identity, exactly
    assert sym_scaled_err(Vg[~pconst], Vo[~pconst], dV[~pconst]) < 1e-12
    assert sym_scaled_err(Ug, Uo[:, off:, off:], dU) < 1e-12        # the frame blocks stay unmasked
    assert np.all(Wg[pobs] == 0)                                    # ... exact zeros
    if np.any(~pobs):
        if w_tol <= 1e-12:
            assert class_rel_err(Wg[~pobs], Wo[~pobs][:, :, off:], (1, 2)) < 1e-12
        else:  # f32 storage: the table of tests/test_gpu_parity.py::test_f32_storage_mode_tolerance_table
            dW = np.abs(Wg[~pobs] - Wo[~pobs][:, :, off:]) / np.abs(Wo[:, :, off:]).max()
            assert dW.max() < w_tol and np.quantile(dW, 0.999) < 1e-12
    gref = kref.to_layout(ref["g"], N, M, fv)
    assert np.all(gg[:3 * N].reshape(-1, 3)[pconst] == 0) and np.all(gg[3 * N:][cvar] == 0)
    gs = 2.0 * np.sqrt(max(eo, 1e-300))
    dg = np.concatenate([dV.reshape(-1), dU.reshape(-1)]) * gs
    cmp_g = (dg > 0) & ~np.concatenate([np.repeat(pconst, 3), cvar])
    assert float((np.abs(gg - gref)[cmp_g] / dg[cmp_g]).max()) < 1e-10

    gpu.phase_schur(c)
    Sg = gpu.buffer(B.BUF_RCS).reshape(fv * M, fv * M)
    rg = gpu.buffer(B.BUF_RCS_RHS)
    free = ~fixed
    cond = 1.0
    if np.any(free):
        dk = dU.reshape(-1)[free]
        So = ref["S"][np.ix_(idx[free], idx[free])]
        dd = 1.0 / np.sqrt(np.abs(np.diag(So)))
        cond = float(np.linalg.cond(So * dd[:, None] * dd[None, :]))
        if s_tol <= 1e-10:
            assert sym_scaled_err(Sg[np.ix_(free, free)], So, dk) < 1e-10
            assert float((np.abs(rg[free] - ref["rhs"][idx[free]]) / (dk * gs)).max()) < 1e-10
        else:  # f32 storage: rel 1e-9 of the largest entry, as the same table
            assert rel_err(Sg[np.ix_(free, free)], So) < s_tol
            # a relative perturbation s_tol of the system moves its solution by at most cond(S) * s_tol
            corr_tol = max(corr_tol, cond * s_tol)
    for f in np.flatnonzero(fixed):  # constant and gauge variables: identity rows (and, S being symmetric here, columns), zero rhs
        row = Sg[f].copy()
        assert row[f] == 1.0
        row[f] = 0
        assert np.all(row == 0) and rg[f] == 0
    some = np.flatnonzero(fixed)[:: max(1, int(fixed.sum()) // 6)]
    if some.size:
        rows = gpu.rcs_rows(some)
        for k, f in enumerate(some):
            assert rows[k, f] == 1.0 and np.count_nonzero(rows[k]) == 1

    assert gpu.phase_solve()
    gpu.phase_backsub(c)
    corr = gpu.buffer(B.BUF_CORRECTIONS)
    assert np.all(corr[:3 * N].reshape(-1, 3)[pconst] == 0) and np.all(corr[3 * N:][fixed] == 0)
    cref_l = kref.to_layout(ref["corr"], N, M, fv)
    tol = max(corr_tol, 4 * ref["d_solver"])
    print(f"\ncond {cond:.3e}; yardstick solver off by {ref['d_solver']:.3e}; corrections differ by {rel_err(corr, cref_l):.3e} "
          f"(tolerance {tol:.3e})")
    assert 4 * ref["d_solver"] < 1e-6, f"the yardstick's solver itself is off by {ref['d_solver']:.2e} on this case"
    assert rel_err(corr, cref_l) < tol
    if np.any(free):  # and against the exact solution of the yardstick's system
        # (as tests/test_gpu_parity.py::_check holds the library to the exact solution of the oracle's system)
        lim = max(1e-9, 100 * np.finfo(np.float64).eps * cond) if corr_tol <= 1e-8 else corr_tol
        assert rel_err(corr[3 * N:][free], ref["dc_exact"][idx[free]]) < lim
    # the current scene before the accept, and the trial scene that becomes current with it: constant blocks keep the
    # uploaded bits
    P1, R1, T1 = (gpu.buffer(b) for b in (B.BUF_POINTS, B.BUF_CAM_R, B.BUF_CAM_T))
    assert np.array_equal(P1, P0) and np.array_equal(R1, R0) and np.array_equal(T1, T0)
    gpu.phase_accept()
    bak = (so.points.copy(), so.cam_R.copy(), so.cam_T.copy())
    orc.apply_corrections(so, ref["corr"])
    so.points[pconst], so.cam_R[fconst], so.cam_T[fconst] = bak[0][pconst], bak[1][fconst], bak[2][fconst]
    P1, R1, T1 = (gpu.buffer(b) for b in (B.BUF_POINTS, B.BUF_CAM_R, B.BUF_CAM_T))
    assert np.array_equal(P1.reshape(-1, 3)[pconst], P0.reshape(-1, 3)[pconst])
    assert np.array_equal(R1.reshape(-1, 9)[fconst], R0.reshape(-1, 9)[fconst])
    assert np.array_equal(T1.reshape(-1, 3)[fconst], T0.reshape(-1, 3)[fconst])
    if np.any(~pconst):
        assert np.any(P1.reshape(-1, 3)[~pconst] != P0.reshape(-1, 3)[~pconst])
    scale = max(1.0, float(np.abs(so.points).max()))
    assert np.abs(P1.reshape(-1, 3) - so.points).max() < tol * scale
    assert np.abs(R1.reshape(-1, 9) - so.cam_R).max() < tol
    assert np.abs(T1.reshape(-1, 3) - so.cam_T).max() < tol * scale
    e2o = energy(so) if energy else orc.reproj_error(f0, so)[0]
    assert gpu.phase_error()[0] == pytest.approx(e2o, rel=1e-6)
    return dict(S=Sg, rhs=rg, corr=corr, ref=ref, points=P1, cam_R=R1, cam_T=T1)


PHASE_CASES = [n for n in cc.CASES if n != "c1_to_convergence" and n not in cc.REORDER_CASES]


@pytest.mark.parametrize("c", [1e-4, 1e-1])
@pytest.mark.parametrize("name", PHASE_CASES)
def test_constant_phases_vs_yardstick(orc, name, c):
    sc, f0, fconst, pconst, keep_gauge, fv = cc.case(name)
    h = _handle(fv)
    try:
        _set(h, fconst, pconst, keep_gauge)
        out = _phases(orc, h, sc, f0, c, fconst, pconst, keep_gauge, fv)
        if name.startswith("long"):
            assert np.diff(sc.row_ptr).max() > 24
            if fv == 6:  # the constant landmark with the longest track takes the per-landmark Schur kernel
                assert h.schur_fallback_landmarks() > 0
        N, M = sc.N, sc.M
        if name == "nf16_all_frames_structure_only":
            # every frame constant: dc all zeros, and each landmark moves by its own damped 3 x 3 step -(V (1 + c))^-1 g
            assert np.all(out["corr"][3 * N:] == 0)
            V, g = out["ref"]["V"].copy(), out["ref"]["g"][:3 * N].reshape(N, 3)
            V[:, np.arange(3), np.arange(3)] *= 1 + c
            own = -np.linalg.solve(V, g[:, :, None])[:, :, 0]
            assert rel_err(out["corr"][:3 * N].reshape(N, 3), own) < 1e-8
        if name == "nf16_all_landmarks_motion_only":
            assert np.all(out["corr"][:3 * N] == 0) and np.all(np.any(out["corr"][3 * N:].reshape(M, 10) != 0, axis=1))
    finally:
        h.close()


MODES = {
    "deterministic": dict(deterministic=True),
    "rcs_dense": dict(rcs_mode=0),
    "rcs_one_chain": dict(rcs_mode=1),
    "rcs_chunks": dict(rcs_mode=2),
    "fusion_off": dict(solver_fusion=False),
    "speculation_off": dict(speculation=False),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_constant_phases_in_every_mode(orc, mode):
    sc, f0, fconst, pconst, keep_gauge, fv = cc.case(cc.MODE_CASE)
    h = _handle(fv, **MODES[mode])
    try:
        _set(h, fconst, pconst, keep_gauge)
        a = _phases(orc, h, sc, f0, 1e-4, fconst, pconst, keep_gauge, fv)
        if mode == "deterministic":  # the masking passes are deterministic by construction: two runs, the same bits
            assert h.deterministic()
            b = _phases(orc, h, sc, f0, 1e-4, fconst, pconst, keep_gauge, fv)
            for k in ("S", "rhs", "corr", "points", "cam_R", "cam_T"):
                assert np.array_equal(a[k], b[k]), k
    finally:
        h.close()


def test_constant_phases_f32_storage(orc):
    """W stored as float: against the oracle with the same factors rounded to float, with the tolerances of
    tests/test_gpu_parity.py::test_f32_storage_mode_tolerance_table (W 1.3e-7 at most with the 0.999 quantile at 1e-12, reduced
    system rel 1e-9).  Corrections: a relative perturbation of 1e-9 of the system moves its solution by at most
    cond(S) * 1e-9, with cond(S) of the yardstick's system after diagonal scaling (_phases computes it; below 1e5 here)."""
    sc, f0, fconst, pconst, keep_gauge, fv = cc.case(cc.MODE_CASE)
    h = _handle(fv, storage_precision=True)
    orc.set_w_storage_f32(2)
    try:
        _set(h, fconst, pconst, keep_gauge)
        _phases(orc, h, sc, f0, 1e-4, fconst, pconst, keep_gauge, fv, w_tol=1.3e-7, s_tol=1e-9)
    finally:
        orc.set_w_storage_f32(0)
        h.close()


def test_constant_phases_huber_loss_and_information(orc):
    sc, f0, fconst, pconst, keep_gauge, fv = cc.case(cc.MODE_CASE)
    q = cc.information(sc)
    assert np.any(q == 0)
    h = _handle(fv)
    try:
        _set(h, fconst, pconst, keep_gauge)
        h.set_robust_loss("huber", 1.0)
        h.set_observation_information(q)
        _phases(orc, h, sc, f0, 1e-4, fconst, pconst, keep_gauge, fv,
                derivatives=lambda so: wr.derivatives(f0, so, q, wr.HUBER, 1.0), energy=lambda so: wr.energy(f0, so, q, wr.HUBER, 1.0))
    finally:
        h.close()


# ------------------------------------------------------------------ reordered frames

@pytest.mark.parametrize("name", cc.REORDER_CASES)
def test_constant_shuffled_frames_take_the_reordering_and_agree(orc, name):
    """a shuffled-frame scene with set_frame_reordering(1): the constant frames go through the renumbering.  Phase by phase
    against the yardstick on the shuffled scene, and the LM run against the caller's-order run of the unshuffled scene, to the
    tolerance tests/test_gpu_calibrated.py uses for the same comparison (1e-7)."""
    sc, f0, fconst, pconst, keep_gauge, fv = cc.case(name)
    perm = np.concatenate([[0, 1], 2 + np.random.RandomState(0).permutation(sc.M - 2)])  # the gauge frames stay 0 and 1
    sh = sa.renumber_frames(sc, perm)
    fsh = np.zeros(sc.M, dtype=bool)
    fsh[perm[np.flatnonzero(fconst)]] = True
    h = _handle(fv)
    try:
        _set(h, fconst, pconst, keep_gauge)
        base = _run(h, sc, f0, 1e-10, 1e6, 8)
        h.set_frame_reordering(1)
        _set(h, fsh, pconst, keep_gauge)
        _phases(orc, h, sh, f0, 1e-4, fsh, pconst, keep_gauge, fv)
        assert h.frame_order() is not None  # renumbered internally
        ok, rep, sg, log = _run(h, sh, f0, 1e-10, 1e6, 8)
        assert h.frame_order() is not None
        assert np.array_equal(sg.cam_T[fsh], sh.cam_T[fsh]) and np.array_equal(sg.cam_R[fsh], sh.cam_R[fsh])
        back = sa.Scene(sg.points, sg.cam_R[perm], sg.cam_T[perm], sc.K, sc.shared_k, sc.row_ptr, sc.obs_frame, sc.obs_uv)
        _compare_runs(base, (ok, rep, back, log))
    finally:
        h.close()


# ------------------------------------------------------------------ end to end

def _same_as_yardstick(orc, gpu, sc, f0, fconst, pconst, keep_gauge, fv, **kw):
    so = _orc_scene(orc, sc)
    skyline = kw.pop("skyline", False)
    rc_o, rep_o = kref.compute_inplace(orc, f0, so, fconst, pconst, keep_gauge, fv, kw.get("allowed"), kw.get("max_factor"),
                                       kw.get("max_iterations", 0), skyline=skyline)
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
    # ComputeInplace does not write constant blocks back: the caller's entries keep their bits
    assert np.array_equal(sg.points[pconst], sc.points[pconst])
    assert np.array_equal(sg.cam_R[fconst], sc.cam_R[fconst]) and np.array_equal(sg.cam_T[fconst], sc.cam_T[fconst])
    assert np.all(np.any(sg.cam_T[~fconst] != sc.cam_T[~fconst], axis=1))
    return ok, rep, sg


def test_constant_c1_to_convergence_vs_python_lm_loop(orc):
    sc, f0, fconst, pconst, keep_gauge, fv = cc.case("c1_to_convergence")
    h = _handle(fv)
    try:
        _set(h, fconst, pconst, keep_gauge)
        # (about 1900 iterations: the Python loop runs the oracle's skyline Cholesky on 8 threads, which gives the bits of one)
        threads = orc.get_threads()
        orc.set_threads(8)
        try:
            _, rep, _ = _same_as_yardstick(orc, h, sc, f0, fconst, pconst, keep_gauge, fv, allowed=1e-12, max_factor=1e6,
                                           skyline=True)
        finally:
            orc.set_threads(threads)
        assert rep.err_final < rep.err_initial
    finally:
        h.close()


def test_constant_24_frames_ten_iterations_vs_python_lm_loop(orc):
    sc, f0, fconst, pconst, keep_gauge, fv = cc.case("nf16_ten_iterations")
    assert sc.M == 24 and keep_gauge == 0
    h = _handle(fv)
    try:
        _set(h, fconst, pconst, keep_gauge)
        _, rep, _ = _same_as_yardstick(orc, h, sc, f0, fconst, pconst, keep_gauge, fv, max_iterations=10)
        assert rep.iterations == 10
    finally:
        h.close()


def test_sliding_window_vs_python_lm_loop(orc):
    """the sliding-window case (first 8 of 24 frames constant, no gauge kept) attempt by attempt against the Python LM loop,
    the constant poses bit-unchanged in the caller's arrays after ComputeInplace"""
    spec, sc, _, _, _, fconst = cc.sliding_window()
    h = _handle(10)
    try:
        h.set_constant_blocks(frames=np.arange(8), keep_gauge=False, n_frames=sc.M)
        got = h.constant_blocks()
        assert got[0].tolist() == [True] * 8 + [False] * 16 and got[1] is None and got[2] is False
        _same_as_yardstick(orc, h, sc, spec.f0, fconst, np.zeros(sc.N, dtype=bool), 0, 10, max_iterations=10)
    finally:
        h.close()


def test_sliding_window_returns_to_ground_truth():
    """a noise-free scene, the first 8 of 24 frames constant at their ground truth, the other frames and all points
    perturbed (1e-3), no gauge kept: the free poses and the points return to the ground truth within 1e-6 and the constant
    poses keep their bits in the caller's arrays.

    The run is a calibrated one (fixed intrinsics) on a scene whose K has K(2,2) = f0, because only there are the steps of the
    reference's LM loop Gauss-Newton steps of the error: the closed-form frame derivatives are those of the error only in that
    convention of K (with the generator's K / f0 the pose entries are off by powers of f0), and the
    ten-variable mode solves for intrinsic corrections that are never applied (bundle-adj-kanatani.cpp:2025-2033).  The Python
    loop around the oracle converges here in four iterations (err 7.6e-05 -> 1.4e-20, poses within 7e-10); with the
    generator's K, or with ten variables a frame, the same loop -- with or without constant blocks -- leaves poses perturbed by
    1e-3 still 9e-4 away after 400 iterations."""
    spec, sc, pts_gt, R_gt, T_gt, fconst = cc.sliding_window(k22_f0=True)
    h = _handle(6)
    try:
        h.set_constant_blocks(frames=np.arange(8), keep_gauge=False, n_frames=sc.M)
        ok, rep, sg, _ = _run(h, sc, spec.f0, 1e-30, 1e12, 12)
        print(f"sliding window: {rep.iterations} iterations, {rep.attempts} attempts, err {rep.err_initial:.3e} -> {rep.err_final:.3e}; "
              f"free poses from the ground truth: T {np.abs(sg.cam_T[8:] - T_gt[8:]).max():.3e} R {np.abs(sg.cam_R[8:] - R_gt[8:]).max():.3e}; "
              f"points {np.abs(sg.points - pts_gt).max():.3e}")
        assert np.array_equal(sg.cam_R[:8], sc.cam_R[:8]) and np.array_equal(sg.cam_T[:8], sc.cam_T[:8])
        assert np.abs(sg.cam_T[8:] - T_gt[8:]).max() < 1e-6
        assert np.abs(sg.cam_R[8:] - R_gt[8:]).max() < 1e-6
        assert np.abs(sg.points - pts_gt).max() < 1e-6
        assert np.array_equal(sg.K, sc.K)
    finally:
        h.close()


def test_all_landmarks_constant_moves_frames_only():
    sc, f0, fconst, pconst, keep_gauge, fv = cc.case("nf16_all_landmarks_motion_only")
    h = _handle(fv)
    try:
        _set(h, fconst, pconst, keep_gauge)
        ok, rep, sg, _ = _run(h, sc, f0, 1e-12, 1e6, 10)
        assert rep.iterations > 0 and rep.err_final < rep.err_initial
        assert np.array_equal(sg.points, sc.points)
        assert np.all(np.any(sg.cam_T != sc.cam_T, axis=1))
    finally:
        h.close()


# ------------------------------------------------------------------ refusals and state

SMALL = sa.SceneSpec(n_frames=6, grid_nx=5, grid_ny=4, vis_window=3)


def test_unsupported_combinations_are_refused_and_the_handle_stays_usable():
    sc = sa.generate_scene(SMALL)
    frames = np.array([2, 4])
    hook = _lib.ALLREDUCE_FN(lambda *a: 0)
    # shared intrinsics, both orders
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_constant_blocks(frames=frames, n_frames=sc.M)
        with pytest.raises(ValueError):
            h.set_intrinsic_groups(np.zeros(sc.M, np.int32))
        assert "constant blocks" in h.last_error() and h.intrinsic_groups() == 0
        ok, rep, sg, _ = _run(h, sc, 600.0, 1e-10, 1e6, 3)
        assert rep.iterations > 0 and np.array_equal(sg.cam_T[frames], sc.cam_T[frames])
    finally:
        h.close()
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_intrinsic_groups(np.zeros(sc.M, np.int32))
        with pytest.raises(ValueError):
            h.set_constant_blocks(frames=frames, n_frames=sc.M)
        assert "intrinsic groups" in h.last_error() and h.constant_blocks() is None and h.intrinsic_groups() == 1
        h.set_intrinsic_groups(None)
        h.set_constant_blocks(frames=frames, n_frames=sc.M)  # fine once the groups are gone
        ok, rep, sg, _ = _run(h, sc, 600.0, 1e-10, 1e6, 3)
        assert rep.iterations > 0 and np.array_equal(sg.cam_T[frames], sc.cam_T[frames])
    finally:
        h.close()
    # more than one rank, both orders
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_constant_blocks(frames=frames, n_frames=sc.M)
        with pytest.raises(ValueError):
            h.set_allreduce(hook, 0, 2)
        assert "more than one rank" in h.last_error()
        ok, rep, sg, _ = _run(h, sc, 600.0, 1e-10, 1e6, 3)
        assert rep.iterations > 0 and np.array_equal(sg.cam_T[frames], sc.cam_T[frames])
    finally:
        h.close()
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_allreduce(hook, 0, 2)
        with pytest.raises(ValueError):
            h.set_constant_blocks(frames=frames, n_frames=sc.M)
        assert "more than one rank" in h.last_error() and h.constant_blocks() is None
    finally:
        h.close()


def test_count_mismatch_everything_constant_and_clearing():
    sc = sa.generate_scene(SMALL)
    other = sa.generate_scene(sa.SceneSpec(n_frames=5, grid_nx=4, grid_ny=3, vis_window=3))
    h = sa.BundleAdjustmentKanatani(0)
    try:
        assert h.constant_blocks() is None
        # everything constant: refused, nothing stored
        with pytest.raises(ValueError):
            h.set_constant_blocks(frames=np.ones(sc.M, bool), points=np.ones(sc.N, bool))
        assert "nothing is left" in h.last_error() and h.constant_blocks() is None
        h.set_constant_blocks(frames=np.ones(sc.M, bool))          # every frame alone is fine
        h.set_constant_blocks(points=np.ones(sc.N, bool), keep_gauge=False)  # and every landmark
        # a stored setting for another scene: the upload is refused; the setting survives reset_scene and is dropped by None
        pm = np.zeros(sc.N, bool)
        pm[::3] = True
        h.set_constant_blocks(frames=[1, 3], points=pm, n_frames=sc.M)
        with pytest.raises(ValueError):
            h.upload(600.0, other)
        assert "constant blocks" in h.last_error()
        with pytest.raises(ValueError):
            _run(h, other, 600.0, 1e-10, 1e6, 3)
        assert h.upload(600.0, sc)
        h.reset()
        fm, pm2, kg = h.constant_blocks()
        assert np.flatnonzero(fm).tolist() == [1, 3] and np.array_equal(pm2, pm) and kg is True
        h.set_constant_blocks(None, None)
        assert h.constant_blocks() is None
        assert h.upload(600.0, other)
        ok, rep, sg, _ = _run(h, sc, 600.0, 1e-10, 1e6, 3)
        assert np.all(np.any(sg.points != sc.points, axis=1))       # the default again: everything moves
    finally:
        h.close()


@pytest.mark.parametrize("name", ["C1_dino_standin", "nf16_10_tiles"])
def test_default_is_bitwise_unchanged_after_toggling(name):
    """Set blocks, run, clear, run again: the second run equals a fresh handle's run bit for bit (nothing of the feature is
    launched or left behind when it is unset).  The default mode's fp64 atomics differ in the last bits from run to run, so
    both handles run the ordered sums of deterministic mode, which share every kernel but the sums' order with the default."""
    if name == "C1_dino_standin":
        sc, f0 = sa.config_scene(name), 600.0
    else:
        sc, f0 = cc.scene(name)
    fresh = sa.BundleAdjustmentKanatani(0)
    toggled = sa.BundleAdjustmentKanatani(0)
    try:
        for h in (fresh, toggled):
            h.set_deterministic(True)
        pm = np.zeros(sc.N, bool)
        pm[::7] = True
        toggled.set_constant_blocks(frames=[2, 5], points=pm, keep_gauge=False, n_frames=sc.M)
        ok, rep, sg, _ = _run(toggled, sc, f0, None, None, 6)
        assert np.array_equal(sg.points[pm], sc.points[pm]) and rep.iterations > 0
        toggled.set_constant_blocks(None, None)
        runs = [_run(h, sc, f0, None, None, 12) for h in (fresh, toggled)]
        assert fresh.deterministic() and toggled.deterministic()
        (ok_a, rep_a, sg_a, log_a), (ok_b, rep_b, sg_b, log_b) = runs
        assert (ok_a, rep_a.iterations, rep_a.attempts, rep_a.status) == (ok_b, rep_b.iterations, rep_b.attempts, rep_b.status)
        assert (rep_a.err_initial, rep_a.err_final) == (rep_b.err_initial, rep_b.err_final)
        assert np.array_equal(log_a["attempts"], log_b["attempts"]) and np.array_equal(log_a["err"], log_b["err"])
        for x in ("points", "cam_R", "cam_T"):
            assert np.array_equal(getattr(sg_a, x), getattr(sg_b, x)), x
    finally:
        fresh.close()
        toggled.close()


def test_cpp_adapter_set_constant_blocks(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "constant_adapter"
    r = subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "demos"),
                        os.path.join(HERE, "cpp", "test_constant_adapter.cpp"), "-o", str(exe),
                        "-L", os.path.join(ROOT, "surikatoko_amd"), "-lsrk_ba",
                        "-Wl,-rpath," + os.path.join(ROOT, "surikatoko_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "constant adapter ok" in r.stdout
