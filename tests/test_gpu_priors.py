"""Gaussian position priors on the GPU (srk_ba_set_position_priors) against the yardstick of tests/prior_ref.py -- the oracle's
blocks plus the prior terms in numpy, orc.two_phase with the gauge kept and the dense numpy Schur complement of
tests/constant_ref.py without it -- and the LM loop of bundle-adj-kanatani.cpp:720-893 around it.  The cases are those of
tests/prior_cases.py, each checked for conditioning by tests/test_prior_cpu.py.

Comparisons and tolerances are those of tests/test_gpu_constant.py::_phases: blocks 1e-12 scaled, gradient, reduced camera
system and rhs 1e-10 scaled, corrections and the applied scene 1e-8 relative (widened to four times the distance of the
yardstick's own solver from the exact solution of its system), the corrections against that exact solution, and phase_error
after the accept at rel 1e-6.
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
import prior_cases as pc
import prior_ref as pref
import weighted_ref as wr
from gpu_common import orc_scene as _orc_scene, handle as _handle, run_lm as _run, compare_runs as _compare_runs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _phases(orc, gpu, sc, f0, c, pri_w, keep_gauge, fv, fconst=None, pconst=None, derivatives=None, energy=None, w_tol=1e-12,
            s_tol=1e-10, corr_tol=1e-8):
    """derivatives -> schur -> solve -> backsub -> accept on both sides, checked (tests/test_gpu_constant.py::_phases with the
    prior terms on the yardstick's side); gpu has the priors pri_w (the coordinates of sc) and any constant blocks set"""
    so = _orc_scene(orc, sc)
    ok, nrm = orc.normalize(so)
    assert ok
    pri = pref.normalised(pri_w, nrm)
    assert gpu.upload(f0, sc) and gpu.frame_vars() == fv
    N, M, off = sc.N, sc.M, 10 - fv
    fconst = np.zeros(M, dtype=bool) if fconst is None else fconst
    pconst = np.zeros(N, dtype=bool) if pconst is None else pconst
    ref = pref.step(orc, f0, so, c, pri, keep_gauge, fv, fconst, pconst, want_system=True, derivatives=derivatives)
    assert ref["ok"]
    gE, Vo, Uo, Wo = ref["blocks"][:4]

    def total(s):
        return (energy(s) if energy else orc.reproj_error(f0, s)[0]) + sum(pref.energy(pri, s))

    eo = total(so)
    assert gpu.phase_error()[0] == pytest.approx(eo, rel=1e-9)
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
    assert np.all(Vg[pconst] == np.eye(3))                          # a constant landmark with a prior: the mask wins
    assert sym_scaled_err(Vg[~pconst], Vo[~pconst], dV[~pconst]) < 1e-12
    assert sym_scaled_err(Ug, Uo[:, off:, off:], dU) < 1e-12
    assert np.all(Wg[pobs] == 0)
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
    # the prior terms are there at all: without them the blocks and the gradient are off by far more than the tolerance
    base = orc.derivatives(f0, so) if derivatives is None else derivatives(so)
    live = np.setdiff1d(pri.pidx, np.flatnonzero(pconst))
    if live.size and np.abs(pri.pinfo[np.isin(pri.pidx, live)]).max() > 0:
        assert sym_scaled_err(Vg[live], base[1][live], dV[live]) > 1e-6
    if pri.fidx.size and np.abs(pri.finfo).max() > 0:
        assert sym_scaled_err(Ug[pri.fidx], base[2][pri.fidx][:, off:, off:], dU[pri.fidx]) > 1e-6

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
    for f in np.flatnonzero(fixed):  # constant and gauge variables: identity rows, zero rhs
        row = Sg[f].copy()
        assert row[f] == 1.0
        row[f] = 0
        assert np.all(row == 0) and rg[f] == 0

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
        lim = max(1e-9, 100 * np.finfo(np.float64).eps * cond) if corr_tol <= 1e-8 else corr_tol
        assert rel_err(corr[3 * N:][free], ref["dc_exact"][idx[free]]) < lim
    P1, R1, T1 = (gpu.buffer(b) for b in (B.BUF_POINTS, B.BUF_CAM_R, B.BUF_CAM_T))
    assert np.array_equal(P1, P0) and np.array_equal(R1, R0) and np.array_equal(T1, T0)
    gpu.phase_accept()
    bak = (so.points.copy(), so.cam_R.copy(), so.cam_T.copy())
    orc.apply_corrections(so, ref["corr"])
    so.points[pconst], so.cam_R[fconst], so.cam_T[fconst] = bak[0][pconst], bak[1][fconst], bak[2][fconst]
    P1, R1, T1 = (gpu.buffer(b) for b in (B.BUF_POINTS, B.BUF_CAM_R, B.BUF_CAM_T))
    assert np.array_equal(P1.reshape(-1, 3)[pconst], P0.reshape(-1, 3)[pconst])
    assert np.array_equal(T1.reshape(-1, 3)[fconst], T0.reshape(-1, 3)[fconst])
    scale = max(1.0, float(np.abs(so.points).max()))
    assert np.abs(P1.reshape(-1, 3) - so.points).max() < tol * scale
    assert np.abs(R1.reshape(-1, 9) - so.cam_R).max() < tol
    assert np.abs(T1.reshape(-1, 3) - so.cam_T).max() < tol * scale
    e2 = gpu.phase_error()[0]
    assert e2 == pytest.approx(total(so), rel=1e-6)
    ep, ef = gpu.prior_error()  # the trial scene that became current: the two prior sums on their own
    want = pref.energy(pri, so)
    assert ep == pytest.approx(want[0], rel=1e-6, abs=1e-18) and ef == pytest.approx(want[1], rel=1e-6, abs=1e-18)
    return dict(S=Sg, rhs=rg, corr=corr, ref=ref, points=P1, cam_R=R1, cam_T=T1, err=e2, V=Vg, U=Ug, g=gg)


PHASE_CASES = [n for n in pc.CASES if not n.startswith("nf16_ten_iterations") and n != pc.TWO_KERNEL_CASE and n not in pc.REORDER_CASES]


@pytest.mark.parametrize("c", [1e-4, 1e-1])
@pytest.mark.parametrize("name", PHASE_CASES)
def test_prior_phases_vs_yardstick(orc, name, c):
    sc, f0, pri, keep_gauge, fv = pc.case(name)
    h = _handle(fv)
    try:
        pri.set_on(h, keep_gauge)
        _phases(orc, h, sc, f0, c, pri, keep_gauge, fv)
        if name == "nf16_every_landmark":
            assert pri.pidx.size == 600 and sc.N % 64 != 0  # three blocks of the energy pass
        if name.startswith("long"):
            assert np.diff(sc.row_ptr).max() > 24
            if fv == 6:  # the landmark with the longest track takes the per-landmark Schur kernel
                assert h.schur_fallback_landmarks() > 0
    finally:
        h.close()


MODES = {
    "deterministic": dict(deterministic=True),
    "rcs_dense": dict(rcs_mode=0),
    "rcs_one_chain": dict(rcs_mode=1),
    "rcs_chunks": dict(rcs_mode=2),
    "fusion_off": dict(solver_fusion=False),
    "speculation_off": dict(speculation=False),
    "jacobian_auto": dict(jacobian_mode=-1),
    "jacobian_per_observation": dict(jacobian_mode=0),
    "jacobian_runs": dict(jacobian_mode=1),
    "jacobian_frame_unions": dict(jacobian_mode=2),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_prior_phases_in_every_mode(orc, mode):
    sc, f0, pri, keep_gauge, fv = pc.case(pc.MODE_CASE)
    h = _handle(fv, **MODES[mode])
    try:
        pri.set_on(h, keep_gauge)
        a = _phases(orc, h, sc, f0, 1e-4, pri, keep_gauge, fv)
        print(f"{mode}: derivative kernel {h.jacobian_kernel()}")
        if mode == "deterministic":  # the passes have one owner per entry and a fixed summation order: two runs, the same bits
            assert h.deterministic()
            b = _phases(orc, h, sc, f0, 1e-4, pri, keep_gauge, fv)
            for k in ("S", "rhs", "corr", "points", "cam_R", "cam_T", "err", "V", "U", "g"):
                assert np.array_equal(a[k], b[k]), k
    finally:
        h.close()


@pytest.mark.parametrize("fv", [10, 6])
def test_prior_phases_two_kernel_derivatives_and_unstaged_error_kernel(orc, fv):
    """k_jac_points + k_jac_frames in front of the prior pass, and the prior partials behind those of the unstaged error
    kernel: a scene whose frame windows do not fit the fused kernel"""
    sc, f0, pri, keep_gauge, _ = pc.case(pc.TWO_KERNEL_CASE)
    h = _handle(fv, jacobian_mode=0)
    try:
        pri.set_on(h, keep_gauge)
        _phases(orc, h, sc, f0, 1e-4, pri, keep_gauge, fv)
        assert h.jacobian_kernel() == 0
    finally:
        h.close()


@pytest.mark.parametrize("mode", [-1, 0])
def test_prior_phases_fixed_intrinsics_both_derivative_modes(orc, mode):
    """six variables a frame: the [Tx Ty Tz] part is variables 0..2 of the frame's block (SRK_UGS(6))"""
    sc, f0, pri, keep_gauge, fv = pc.case(pc.MODE_CASE + "_fixed_k")
    h = _handle(fv, jacobian_mode=mode)
    try:
        pri.set_on(h, keep_gauge)
        _phases(orc, h, sc, f0, 1e-4, pri, keep_gauge, fv)
    finally:
        h.close()


def test_prior_phases_f32_storage(orc):
    """W stored as float: the tolerances of tests/test_gpu_constant.py::test_constant_phases_f32_storage"""
    sc, f0, pri, keep_gauge, fv = pc.case(pc.MODE_CASE)
    h = _handle(fv, storage_precision=True)
    orc.set_w_storage_f32(2)
    try:
        pri.set_on(h, keep_gauge)
        _phases(orc, h, sc, f0, 1e-4, pri, keep_gauge, fv, w_tol=1.3e-7, s_tol=1e-9)
    finally:
        orc.set_w_storage_f32(0)
        h.close()


def test_prior_phases_huber_loss_and_information(orc):
    """no robust loss acts on a prior: the energy is the robust / weighted observation energy plus the plain prior sums"""
    sc, f0, pri, keep_gauge, fv = pc.case(pc.MODE_CASE)
    q = cc.information(sc)
    h = _handle(fv)
    try:
        pri.set_on(h, keep_gauge)
        h.set_robust_loss("huber", 1.0)
        h.set_observation_information(q)
        _phases(orc, h, sc, f0, 1e-4, pri, keep_gauge, fv,
                derivatives=lambda so: wr.derivatives(f0, so, q, wr.HUBER, 1.0), energy=lambda so: wr.energy(f0, so, q, wr.HUBER, 1.0))
    finally:
        h.close()


def test_prior_on_a_constant_block_adds_a_constant_to_the_error_and_nothing_else(orc):
    """together with constant blocks: a constant landmark and a constant frame that also carry priors keep their identity block,
    zero gradient and bits (the masking passes run after the prior pass and win); their prior sums stay in the error"""
    sc, f0, pri, keep_gauge, fv = pc.case(pc.MODE_CASE)
    fconst, pconst = pc.constant_combination(sc, pri)
    h = _handle(fv)
    try:
        pri.set_on(h, keep_gauge)
        h.set_constant_blocks(fconst, pconst, True)
        _phases(orc, h, sc, f0, 1e-4, pri, keep_gauge, fv, fconst=fconst, pconst=pconst)
    finally:
        h.close()


# ------------------------------------------------------------------ LM runs

@pytest.mark.parametrize("name", pc.REORDER_CASES)
def test_prior_shuffled_frames_take_the_reordering_and_agree(orc, name):
    """a shuffled-frame scene with set_frame_reordering(1): the frame priors go through the renumbering.  Phase by phase
    against the yardstick on the shuffled scene, and the LM run against the run of the unshuffled scene (1e-7, as
    tests/test_gpu_constant.py::test_constant_shuffled_frames_take_the_reordering_and_agree)."""
    sc, f0, pri, keep_gauge, fv = pc.case(name)
    perm = np.concatenate([[0, 1], 2 + np.random.RandomState(0).permutation(sc.M - 2)])  # the gauge frames stay 0 and 1
    sh = sa.renumber_frames(sc, perm)
    new = perm[pri.fidx]
    order = np.argsort(new)
    psh = pref.Priors(pri.pidx, pri.ppos, pri.pinfo, new[order], pri.fpos[order], pri.finfo[order])
    assert np.abs(pref.centres(sh)[psh.fidx] - pref.centres(sc)[pri.fidx][order]).max() < 1e-14
    h = _handle(10)
    try:
        pri.set_on(h, keep_gauge)
        base = _run(h, sc, f0, 1e-10, 1e6, 8)
        h.set_frame_reordering(1)
        psh.set_on(h, keep_gauge)
        _phases(orc, h, sh, f0, 1e-4, psh, keep_gauge, 10)
        assert h.frame_order() is not None  # renumbered internally
        ok, rep, sg, log = _run(h, sh, f0, 1e-10, 1e6, 8)
        back = sa.Scene(sg.points, sg.cam_R[perm], sg.cam_T[perm], sc.K, sc.shared_k, sc.row_ptr, sc.obs_frame, sc.obs_uv)
        _compare_runs(base, (ok, rep, back, log))
    finally:
        h.close()


def _same_as_yardstick(orc, gpu, sc, f0, pri, keep_gauge, fv, **kw):
    so = _orc_scene(orc, sc)
    rc_o, rep_o = pref.compute_inplace(orc, f0, so, pri, keep_gauge, fv, kw.get("allowed"), kw.get("max_factor"),
                                       kw.get("max_iterations", 0))
    ok, rep, sg, log = _run(gpu, sc, f0, **kw)
    assert ok == (rc_o == 0)
    assert rep.status == rep_o.status
    assert (rep.iterations, rep.attempts) == (rep_o.iterations, rep_o.attempts)
    assert list(log["attempts"]) == rep_o.attempts_per_iteration[:rep.iterations]
    assert rep.err_initial == pytest.approx(rep_o.err_initial, rel=1e-8, abs=1e-18)
    assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-8, abs=1e-18)
    lt.assert_same_trajectory(log, rep_o.log, 1e-8, gpu_attempts=rep.attempts, err_abs=1e-18)
    assert np.abs(sg.points - so.points).max() < 1e-8
    assert np.abs(sg.cam_R - so.cam_R).max() < 1e-8
    assert np.abs(sg.cam_T - so.cam_T).max() < 1e-8
    return ok, rep, sg, so


@pytest.mark.parametrize("name", [pc.MODE_CASE, "nf16_ten_iterations_free_gauge"])
def test_prior_24_frames_ten_iterations_vs_python_lm_loop(orc, name):
    """the gauge kept, and released: attempt by attempt against the Python loop"""
    sc, f0, pri, keep_gauge, fv = pc.case(name)
    assert sc.M == 24 and keep_gauge == (1 if name == pc.MODE_CASE else 0)
    h = _handle(fv)
    try:
        pri.set_on(h, keep_gauge)
        _, rep, sg, _ = _same_as_yardstick(orc, h, sc, f0, pri, keep_gauge, fv, max_iterations=10)
        assert rep.iterations == 10
        if keep_gauge:
            assert np.abs(sg.cam_T[0] - sc.cam_T[0]).max() < 1e-12  # the gauge frame stays (up to the normalise / revert round trip)
        else:
            assert np.abs(sg.cam_T[0] - sc.cam_T[0]).max() > 1e-9  # nothing is held
    finally:
        h.close()


def _distance(sg, pts_gt, R_gt, T_gt):
    return max(float(np.abs(sg.cam_T - T_gt).max()), float(np.abs(sg.cam_R - R_gt).max()), float(np.abs(sg.points - pts_gt).max()))


def test_georeferencing_returns_to_ground_truth(orc):
    """The noise-free 24-frame scene of prior_cases.georeferencing(): every frame and every point perturbed by 1e-3, priors
    (one scalar L = 0.1; prior sum 4.7e-4 beside a reprojection sum of 8.4e-5 at the start) at the ground-truth centres of all 24
    frames, nothing held (keep_gauge = 0), calibrated for the reason given in
    tests/test_gpu_constant.py::test_sliding_window_returns_to_ground_truth.  Poses and points return to the ground truth;
    the same start without priors and with the gauge kept stays more than 1e-4 from it (the reconstruction is then right only
    up to a similarity), which shows that the test can fail.

    The bound on the GPU run is ten times the distance the Python loop reaches on the CPU, and not below 1e-9.  Measured on
    the CPU: the Python loop reaches 1.6e-8 in 12 iterations (err 5.5e-4 -> 7.2e-19, and no closer in 40: along the seven gauge
    directions only the priors' small curvature acts, and the loop stalls at the rounding floor of the sums), so the bound
    is 1.6e-7.  The same loop without priors, gauge kept, ends 9.9e-2 from the ground truth."""
    spec, sc, pri, pts_gt, R_gt, T_gt = pc.georeferencing()
    so = _orc_scene(orc, sc)
    rc_o, rep_o = pref.compute_inplace(orc, spec.f0, so, pri, 0, 6, 1e-30, 1e12, 12)
    d_cpu = _distance(so, pts_gt, R_gt, T_gt)
    bound = max(10 * d_cpu, 1e-9)
    print(f"python loop: {rep_o.iterations} iterations, err {rep_o.err_initial:.3e} -> {rep_o.err_final:.3e}, distance {d_cpu:.3e}; "
          f"bound {bound:.3e}")
    assert d_cpu < 1e-7, "the yardstick itself does not return to the ground truth"
    h = _handle(6)
    try:
        pri.set_on(h, 0)
        ok, rep, sg, _ = _run(h, sc, spec.f0, 1e-30, 1e12, 12)
        d_gpu = _distance(sg, pts_gt, R_gt, T_gt)
        print(f"gpu: {rep.iterations} iterations, {rep.attempts} attempts, err {rep.err_initial:.3e} -> {rep.err_final:.3e}, "
              f"distance {d_gpu:.3e}")
        assert d_gpu < bound
        assert np.array_equal(sg.K, sc.K)
        dp, df = h.prior_residuals()
        assert dp.shape == (0, 3) and np.abs(df).max() < bound
        h.set_position_priors(None, None)
        ok, rep, sg, _ = _run(h, sc, spec.f0, 1e-30, 1e12, 12)
        d_free = _distance(sg, pts_gt, R_gt, T_gt)
        print(f"without priors, gauge kept: err {rep.err_initial:.3e} -> {rep.err_final:.3e}, distance {d_free:.3e}")
        assert d_free > 1e-4
    finally:
        h.close()


def test_deterministic_mode_gives_identical_bits_with_priors():
    sc, f0, pri, keep_gauge, fv = pc.case("nf16_ten_iterations_free_gauge")
    runs = []
    for _ in range(2):
        h = _handle(fv, deterministic=True)
        try:
            pri.set_on(h, keep_gauge)
            runs.append(_run(h, sc, f0, None, None, 6))
            assert h.deterministic()
        finally:
            h.close()
    (ok_a, rep_a, sg_a, log_a), (ok_b, rep_b, sg_b, log_b) = runs
    assert rep_a.iterations > 0 and (rep_a.iterations, rep_a.attempts) == (rep_b.iterations, rep_b.attempts)
    assert (rep_a.err_initial, rep_a.err_final) == (rep_b.err_initial, rep_b.err_final)
    assert np.array_equal(log_a["err"], log_b["err"])
    for x in ("points", "cam_R", "cam_T"):
        assert np.array_equal(getattr(sg_a, x), getattr(sg_b, x)), x


def test_all_zero_information_gives_the_bits_of_the_run_without_that_prior():
    """an all-zero information matrix is a valid, switched-off prior: the run equals, bit for bit, the run of the setting
    without it (deterministic mode: the default's fp64 atomics differ in the last bits from run to run)"""
    sc, f0, pri, keep_gauge, fv = pc.case(pc.MODE_CASE)
    more = pc.priors_for(sc, np.union1d(pri.pidx, [5, sc.N - 1]), np.union1d(pri.fidx, [7]))
    assert 5 not in pri.pidx and 7 not in pri.fidx
    pinfo, finfo = more.pinfo.copy(), more.finfo.copy()
    ppos, fpos = more.ppos.copy(), more.fpos.copy()
    keep_p, keep_f = np.isin(more.pidx, pri.pidx), np.isin(more.fidx, pri.fidx)
    ppos[keep_p], pinfo[keep_p], fpos[keep_f], finfo[keep_f] = pri.ppos, pri.pinfo, pri.fpos, pri.finfo
    pinfo[~keep_p] = 0
    finfo[~keep_f] = 0
    with_off = pref.Priors(more.pidx, ppos, pinfo, more.fidx, fpos, finfo)
    runs = []
    for p in (pri, with_off):
        h = _handle(fv, deterministic=True)
        try:
            p.set_on(h, keep_gauge)
            runs.append(_run(h, sc, f0, None, None, 4))
            if p is with_off:
                got = h.position_priors()
                assert got["point_index"].size == pri.pidx.size + 2 and got["frame_index"].size == pri.fidx.size + 1
                dp, df = h.prior_residuals()  # the switched-off priors still report their offsets
                assert dp.shape == (pri.pidx.size + 2, 3) and np.all(np.any(dp != 0, axis=1))
        finally:
            h.close()
    (ok_a, rep_a, sg_a, log_a), (ok_b, rep_b, sg_b, log_b) = runs
    assert rep_a.iterations > 0 and (rep_a.iterations, rep_a.attempts) == (rep_b.iterations, rep_b.attempts)
    assert (rep_a.err_initial, rep_a.err_final) == (rep_b.err_initial, rep_b.err_final)
    assert np.array_equal(log_a["err"], log_b["err"])
    for x in ("points", "cam_R", "cam_T"):
        assert np.array_equal(getattr(sg_a, x), getattr(sg_b, x)), x


# ------------------------------------------------------------------ getters

def test_getters_prior_error_phase_error_and_residuals(orc):
    """prior_error() equals the yardstick's two sums (rel 1e-12), phase_error the observation energy plus both, and
    prior_residuals() X - Xbar, C - Cbar computed from download_scene in the caller's coordinates (1e-10 of the extent), on the
    scene uploaded un-normalised with a rotated frame 0, before and after an optimisation"""
    sc, f0, pri, keep_gauge, fv = pc.case("nf16_full_information_rotated_world_free_gauge")
    h = _handle(fv)
    try:
        pri.set_on(h, keep_gauge)
        got = h.position_priors()
        assert np.array_equal(got["point_index"], pri.pidx) and np.array_equal(got["frame_index"], pri.fidx)
        assert np.array_equal(got["point_pos"], pri.ppos) and np.array_equal(got["frame_centre"], pri.fpos)
        assert np.array_equal(got["point_info"], pref.six(pri.pinfo)) and np.array_equal(got["frame_info"], pref.six(pri.finfo))
        assert got["keep_gauge"] is False
        assert h.upload(f0, sc)
        # the yardstick's priors through the library's host map with the normaliser the upload computes (bit for bit what the
        # device holds), its scene the resident one, downloaded normalised: what is compared is the energy arithmetic alone
        nsc = sc.copy()
        ok, nrm = sa.normalize_scene_inplace(nsc)
        assert ok
        pn = pref.Priors(pri.pidx, *(lambda a, b: (a, pref.full(b)))(*B.normalize_position_priors(nrm, pri.ppos, pref.six(pri.pinfo))),
                         pri.fidx, *(lambda a, b: (a, pref.full(b)))(*B.normalize_position_priors(nrm, pri.fpos, pref.six(pri.finfo))))
        so = _orc_scene(orc, nsc)
        extent = float(np.abs(sc.points - sc.points.mean(axis=0)).max())
        for stage in ("uploaded", "optimised"):
            if stage == "optimised":
                crit = sa.BundleAdjustmentKanataniTermCriteria()
                crit.AllowedReprojErrRelativeChange(None)
                crit.MaxHessianFactor(None)
                h.optimize(crit, 3)
            got_sc = sc.copy()
            h.download(got_sc, revert_normalization=False)
            so.points[:], so.cam_R[:], so.cam_T[:] = got_sc.points, got_sc.cam_R, got_sc.cam_T
            want = pref.energy(pn, so)
            ep, ef = h.prior_error()
            print(f"{stage}: prior sums {ep:.17g} {ef:.17g}, yardstick {want[0]:.17g} {want[1]:.17g}")
            assert ep == pytest.approx(want[0], rel=1e-12) and ef == pytest.approx(want[1], rel=1e-12)
            assert h.phase_error()[0] == pytest.approx(orc.reproj_error(f0, so)[0] + want[0] + want[1], rel=1e-10)
            world = sc.copy()
            h.download(world)
            wp, wf = pref.offsets(pri, world)
            dp, df = h.prior_residuals()
            assert np.abs(dp - wp).max() < 1e-10 * extent and np.abs(df - wf).max() < 1e-10 * extent
            assert np.abs(dp).max() > 1e-5 * extent
            # the energy is invariant under the normalisation: the caller's offsets against the caller's information
            assert float(np.einsum("na,nab,nb->", dp, pri.pinfo, dp)) == pytest.approx(ep, rel=1e-8)
    finally:
        h.close()


# ------------------------------------------------------------------ state and refusals

SMALL = sa.SceneSpec(n_frames=6, grid_nx=5, grid_ny=4, vis_window=3)


def _small_priors(sc):
    return pc.priors_for(sc, [1, 4, 9], [2, 4])


def test_unsupported_combinations_are_refused_in_either_order_and_the_handle_stays_usable():
    sc = sa.generate_scene(SMALL)
    pri = _small_priors(sc)
    hook = _lib.ALLREDUCE_FN(lambda *a: 0)
    h = sa.BundleAdjustmentKanatani(0)
    try:
        pri.set_on(h, 1)
        with pytest.raises(ValueError):
            h.set_intrinsic_groups(np.zeros(sc.M, np.int32))
        assert "position priors" in h.last_error() and h.intrinsic_groups() == 0
        ok, rep, sg, _ = _run(h, sc, 600.0, 1e-10, 1e6, 3)
        assert rep.iterations > 0 and h.prior_error()[0] > 0
    finally:
        h.close()
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_intrinsic_groups(np.zeros(sc.M, np.int32))
        with pytest.raises(ValueError):
            pri.set_on(h, 1)
        assert "intrinsic groups" in h.last_error() and h.position_priors() is None and h.intrinsic_groups() == 1
        h.set_intrinsic_groups(None)
        pri.set_on(h, 1)  # fine once the groups are gone
        ok, rep, sg, _ = _run(h, sc, 600.0, 1e-10, 1e6, 3)
        assert rep.iterations > 0 and h.prior_error()[0] > 0
    finally:
        h.close()
    h = sa.BundleAdjustmentKanatani(0)
    try:
        pri.set_on(h, 1)
        with pytest.raises(ValueError):
            h.set_allreduce(hook, 0, 2)
        assert "more than one rank" in h.last_error()
        ok, rep, sg, _ = _run(h, sc, 600.0, 1e-10, 1e6, 3)
        assert rep.iterations > 0 and h.prior_error()[0] > 0
    finally:
        h.close()
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_allreduce(hook, 0, 2)
        with pytest.raises(ValueError):
            pri.set_on(h, 1)
        assert "more than one rank" in h.last_error() and h.position_priors() is None
    finally:
        h.close()


def test_bad_arguments_leave_the_previous_setting_in_force():
    sc = sa.generate_scene(SMALL)
    pri = _small_priors(sc)
    L = sa.lib()
    h = sa.BundleAdjustmentKanatani(0)
    try:
        assert h.position_priors() is None
        pri.set_on(h, 0)

        def raw(pidx, ppos, pinfo, fidx, fpos, finfo, kg):
            a = [np.ascontiguousarray(x) for x in (np.asarray(pidx, np.int64), np.asarray(ppos, np.float64), np.asarray(pinfo, np.float64),
                                                   np.asarray(fidx, np.int32), np.asarray(fpos, np.float64), np.asarray(finfo, np.float64))]
            q = [x.ctypes.data_as(B.C.c_void_p) for x in a]
            return L.srk_ba_set_position_priors(B.C.c_void_p(h._h), B.C.c_int64(a[0].size), q[0], q[1], q[2], B.C.c_int32(a[3].size),
                                                q[3], q[4], q[5], B.C.c_int(kg))

        good = (pri.pidx, pri.ppos, pref.six(pri.pinfo), pri.fidx, pri.fpos, pref.six(pri.finfo))
        nan_pos = pri.ppos.copy()
        nan_pos[1, 2] = np.nan
        inf_info = pref.six(pri.finfo)
        inf_info[0, 0] = np.inf
        indefinite = pref.six(pri.pinfo)
        indefinite[2] = [1.0, 2.0, 0.0, 1.0, 0.0, 1.0]  # eigenvalues 3, 1, -1
        negative = pref.six(pri.pinfo)
        negative[0] = [-1.0, 0, 0, 1.0, 0, 1.0]
        bad = {
            "unsorted landmarks": (pri.pidx[::-1], good[1], good[2], good[3], good[4], good[5], 1),
            "repeated landmark": ([1, 4, 4], good[1], good[2], good[3], good[4], good[5], 1),
            "negative landmark": ([-1, 4, 9], good[1], good[2], good[3], good[4], good[5], 1),
            "repeated frame": (good[0], good[1], good[2], [2, 2], good[4], good[5], 1),
            "nan position": (good[0], nan_pos, good[2], good[3], good[4], good[5], 1),
            "infinite information": (good[0], good[1], good[2], good[3], good[4], inf_info, 1),
            "indefinite information": (good[0], good[1], indefinite, good[3], good[4], good[5], 1),
            "negative information": (good[0], good[1], negative, good[3], good[4], good[5], 1),
            "keep_gauge 2": good + (2,),
        }
        for what, args in bad.items():
            assert raw(*args) == -1, what
            assert "position priors" in h.last_error(), what
            got = h.position_priors()
            assert got is not None and got["keep_gauge"] is False and np.array_equal(got["point_index"], pri.pidx), what
            assert np.array_equal(got["point_info"], pref.six(pri.pinfo)) and np.array_equal(got["frame_centre"], pri.fpos), what
        # valid: an all-zero and a rank-1 information matrix
        semi = pref.six(pri.pinfo)
        semi[0] = 0
        n = np.array([1.0, -2.0, 0.5])
        semi[1] = pref.six(np.outer(n, n)[None])[0]
        assert raw(good[0], good[1], semi, good[3], good[4], good[5], 1) == 0
        ok, rep, sg, _ = _run(h, sc, 600.0, 1e-10, 1e6, 3)
        assert rep.iterations > 0
    finally:
        h.close()


def test_index_beyond_the_scene_fails_the_upload_and_the_setting_survives_reset_and_compute_inplace():
    sc = sa.generate_scene(SMALL)
    other = sa.generate_scene(sa.SceneSpec(n_frames=4, grid_nx=3, grid_ny=3, vis_window=3))
    pri = _small_priors(sc)
    assert pri.pidx.max() >= other.N and pri.fidx.max() >= other.M
    h = sa.BundleAdjustmentKanatani(0)
    try:
        pri.set_on(h, 1)
        with pytest.raises(ValueError):
            h.upload(600.0, other)
        assert "position priors" in h.last_error()
        with pytest.raises(ValueError):
            _run(h, other, 600.0, 1e-10, 1e6, 3)
        only_frames = pref.Priors(fidx=pri.fidx, fpos=pri.fpos, finfo=pri.finfo)
        only_frames.set_on(h, 1)
        with pytest.raises(ValueError):
            h.upload(600.0, other)  # frame 4 of 4
        pri.set_on(h, 1)
        assert h.upload(600.0, sc)
        e0 = h.prior_error()
        assert e0[0] > 0 and e0[1] > 0
        h.reset()
        got = h.position_priors()
        assert np.array_equal(got["point_index"], pri.pidx) and np.array_equal(got["frame_index"], pri.fidx) and got["keep_gauge"] is True
        assert h.prior_error() == e0
        # re-applied by compute_inplace (an upload of its own): the result differs from the run without priors
        with_p = _run(h, sc, 600.0, 1e-10, 1e6, 5)
        assert h.prior_error()[0] > 0
        h.set_position_priors(None, None)
        assert h.position_priors() is None
        without = _run(h, sc, 600.0, 1e-10, 1e6, 5)
        assert h.prior_error() == (0.0, 0.0)
        assert np.abs(with_p[2].points - without[2].points).max() > 1e-6
        assert h.upload(600.0, other)  # and the other scene uploads again
    finally:
        h.close()


@pytest.mark.parametrize("name", ["C1_dino_standin", "nf16_10_tiles"])
def test_default_is_bitwise_unchanged_after_toggling(name):
    """Set priors, run, clear, run again: the second run equals a fresh handle's run bit for bit (nothing of the feature is
    launched or left behind when it is unset).  As tests/test_gpu_constant.py::test_default_is_bitwise_unchanged_after_toggling:
    both handles run the ordered sums of deterministic mode."""
    if name == "C1_dino_standin":
        sc, f0 = sa.config_scene(name), 600.0
    else:
        sc, f0 = cc.scene(name)
    fresh = sa.BundleAdjustmentKanatani(0)
    toggled = sa.BundleAdjustmentKanatani(0)
    try:
        for h in (fresh, toggled):
            h.set_deterministic(True)
        pri = pc.priors_for(sc, cc._every(sc.N, 7), [2, 5])
        if hasattr(toggled, "set_position_priors"):
            pri.set_on(toggled, 0)
            ok, rep, sg, _ = _run(toggled, sc, f0, None, None, 6)
            assert rep.iterations > 0 and toggled.prior_error()[0] > 0
            toggled.set_position_priors(None, None)
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


def test_cpp_adapter_set_position_priors(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "prior_adapter"
    r = subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "demos"),
                        os.path.join(HERE, "cpp", "test_prior_adapter.cpp"), "-o", str(exe),
                        "-L", os.path.join(ROOT, "surikatoko_amd"), "-lsrk_ba",
                        "-Wl,-rpath," + os.path.join(ROOT, "surikatoko_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "prior adapter ok" in r.stdout
