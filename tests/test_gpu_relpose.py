"""Relative-pose factors on the GPU (srk_ba_set_relative_pose_factors) against the yardstick of tests/relpose_ref.py -- the
oracle's blocks plus the factors' terms in numpy, the dense numpy Schur complement of tests/constant_ref.py plus the coupling
blocks, restricted to the free variables -- and lm_ref.loop around it.  The cases are those of tests/relpose_cases.py, each
checked for conditioning by tests/test_relpose_cpu.py.

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
import relpose_cases as rc
import relpose_ref as rr
import so3_ref as so3
import weighted_ref as wr
from gpu_common import orc_scene as _orc_scene, handle as _handle, run_lm as _run, compare_runs as _compare_runs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _phases(orc, gpu, sc, f0, c, fac_w, keep_gauge, fv, fconst=None, pconst=None, derivatives=None, energy=None, pri_w=None,
            w_tol=1e-12, s_tol=1e-10, corr_tol=1e-8):
    """derivatives -> schur -> solve -> backsub -> accept on both sides, checked (tests/test_gpu_constant.py::_phases with the
    factors' terms and couplings on the yardstick's side); gpu has the factors fac_w (the coordinates of sc) and any constant
    blocks / priors set"""
    so = _orc_scene(orc, sc)
    ok, nrm = orc.normalize(so)
    assert ok
    fac = rr.normalised(fac_w, nrm)
    pri = None if pri_w is None else pref.normalised(pri_w, nrm)
    assert gpu.upload(f0, sc) and gpu.frame_vars() == fv
    N, M, off = sc.N, sc.M, 10 - fv
    fconst = np.zeros(M, dtype=bool) if fconst is None else fconst
    pconst = np.zeros(N, dtype=bool) if pconst is None else pconst
    ref = rr.step(orc, f0, so, c, fac, keep_gauge, fv, fconst, pconst, want_system=True, derivatives=derivatives, pri=pri)
    assert ref["ok"]
    gE, Vo, Uo, Wo = ref["blocks"][:4]

    def total(s):
        return (energy(s) if energy else orc.reproj_error(f0, s)[0]) + rr.energy(fac, s) + (sum(pref.energy(pri, s)) if pri else 0.0)

    eo = total(so)
    assert gpu.phase_error()[0] == pytest.approx(eo, rel=1e-9)
    assert gpu.relative_pose_error() == pytest.approx(rr.energy(fac, so), rel=1e-9)
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
    assert np.all(Vg[pconst] == np.eye(3))
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
    # the factors' terms are there at all: without them the frame blocks are off by far more than the tolerance
    base = orc.derivatives(f0, so) if derivatives is None else derivatives(so)
    base = base[:4] if pri is None else pref.add_terms(base[:4], so, pri)
    touched = np.unique(np.concatenate([fac.a, fac.b]))
    assert sym_scaled_err(Ug[touched], base[2][touched][:, off:, off:], dU[touched]) > 1e-6

    gpu.phase_schur(c)
    Sg = gpu.buffer(B.BUF_RCS).reshape(fv * M, fv * M)
    rg = gpu.buffer(B.BUF_RCS_RHS)
    free = ~fixed
    cond = 1.0
    dk = dU.reshape(-1)[free]
    So = ref["S"][np.ix_(idx[free], idx[free])]
    dd = 1.0 / np.sqrt(np.abs(np.diag(So)))
    cond = float(np.linalg.cond(So * dd[:, None] * dd[None, :]))
    if s_tol <= 1e-10:
        assert sym_scaled_err(Sg[np.ix_(free, free)], So, dk) < 1e-10
        assert float((np.abs(rg[free] - ref["rhs"][idx[free]]) / (dk * gs)).max()) < 1e-10
    else:  # f32 storage: rel 1e-9 of the largest entry, as the same table
        assert rel_err(Sg[np.ix_(free, free)], So) < s_tol
        corr_tol = max(corr_tol, cond * s_tol)
    # the coupling blocks on their own, and as download_rcs_rows shows them: block (a, b) of the downloaded system is the
    # yardstick's (Schur complement plus coupling; zero where a variable is fixed)
    Cb = rr.couplings(fac, so)
    ds = dU
    for k in range(fac.n):
        a, b = int(fac.a[k]), int(fac.b[k])
        ra, rb = fv * a + (fv - 6) + np.arange(6), fv * b + (fv - 6) + np.arange(6)
        got = Sg[np.ix_(ra, rb)]
        want = ref["S"][np.ix_(idx[ra], idx[rb])].copy()
        want[fixed[ra], :] = 0
        want[:, fixed[rb]] = 0
        scale = ds[a, fv - 6:, None] * ds[b, None, fv - 6:]
        assert float((np.abs(got - want) / scale).max()) < 1e-10, k
        if not (fixed[ra].all() or fixed[rb].all() or np.abs(fac.info[k]).max() == 0):
            assert float((np.abs(Cb[k]) / scale).max()) > 1e-6  # and it is no rounding-sized block
        hi, lo = (ra, rb) if a > b else (rb, ra)  # download_rcs_rows fills columns <= row: the rows of the later frame
        rows = gpu.rcs_rows(hi[-2:])
        assert np.array_equal(rows[:, lo], Sg[np.ix_(hi[-2:], lo)])
    for f in np.flatnonzero(fixed):  # constant and gauge variables: identity rows and columns, zero rhs
        row, col = Sg[f].copy(), Sg[:, f].copy()
        assert row[f] == 1.0
        row[f] = col[f] = 0
        assert np.all(row == 0) and np.all(col == 0) and rg[f] == 0

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
    lim = max(1e-9, 100 * np.finfo(np.float64).eps * cond) if corr_tol <= 1e-8 else corr_tol
    assert rel_err(corr[3 * N:][free], ref["dc_exact"][idx[free]]) < lim
    # and numpy on the downloaded system
    x = np.linalg.solve(Sg, rg)
    for _ in range(3):
        x = x + np.linalg.solve(Sg, rg - Sg @ x)
    assert rel_err(corr[3 * N:], x) < lim
    P1, R1, T1 = (gpu.buffer(b) for b in (B.BUF_POINTS, B.BUF_CAM_R, B.BUF_CAM_T))
    assert np.array_equal(P1, P0) and np.array_equal(R1, R0) and np.array_equal(T1, T0)
    gpu.phase_accept()
    bak = (so.points.copy(), so.cam_R.copy(), so.cam_T.copy())
    orc.apply_corrections(so, ref["corr"])
    so.points[pconst], so.cam_R[fconst], so.cam_T[fconst] = bak[0][pconst], bak[1][fconst], bak[2][fconst]
    P1, R1, T1 = (gpu.buffer(b) for b in (B.BUF_POINTS, B.BUF_CAM_R, B.BUF_CAM_T))
    assert np.array_equal(T1.reshape(-1, 3)[fconst], T0.reshape(-1, 3)[fconst])
    assert np.array_equal(R1.reshape(-1, 9)[fconst], R0.reshape(-1, 9)[fconst])
    scale = max(1.0, float(np.abs(so.points).max()))
    assert np.abs(P1.reshape(-1, 3) - so.points).max() < tol * scale
    assert np.abs(R1.reshape(-1, 9) - so.cam_R).max() < tol
    assert np.abs(T1.reshape(-1, 3) - so.cam_T).max() < tol * scale
    e2 = gpu.phase_error()[0]
    assert e2 == pytest.approx(total(so), rel=1e-6)
    assert gpu.relative_pose_error() == pytest.approx(rr.energy(fac, so), rel=1e-6, abs=1e-18)
    return dict(S=Sg, rhs=rg, corr=corr, ref=ref, points=P1, cam_R=R1, cam_T=T1, err=e2, V=Vg, U=Ug, g=gg)


def _set_case(h, fac, fconst, keep_gauge):
    fac.set_on(h)
    if fconst.any() or not keep_gauge:
        h.set_constant_blocks(fconst if fconst.any() else None, None, bool(keep_gauge))


PHASE_CASES = [n for n in rc.CASES if n not in (rc.TWO_KERNEL_CASE, rc.REORDER_CASE)]


@pytest.mark.parametrize("c", [1e-4, 1e-1])
@pytest.mark.parametrize("name", PHASE_CASES)
def test_relpose_phases_vs_yardstick(orc, name, c):
    sc, f0, fac, fv, fconst, keep_gauge = rc.case(name)
    # the loop closure in the caller's frame order, where its row reaches back to frame 2 (the automatic renumbering folds the
    # 60 frames into a band of about 40, which the 256-column granularity of the skyline does not show at this size; the case
    # with the pairs given backwards runs it)
    h = _handle(fv, frame_reordering=0) if name == "ragged_loop_closure_2_59" else _handle(fv)
    try:
        assert h.upload(f0, sc)
        fill0, chunks0, order0 = h.rcs_fill(), h.rcs_chunks(), h.frame_order()
        _set_case(h, fac, fconst, keep_gauge)
        _phases(orc, h, sc, f0, c, fac, keep_gauge, fv, fconst=fconst)
        print(f"{name}: rcs_fill {fill0} -> {h.rcs_fill()}, chunks {chunks0} -> {h.rcs_chunks()}")
        if name == "ragged_loop_closure_2_59":
            assert h.rcs_fill() > fill0 and h.frame_order() is None  # (2, 59) shares no landmark: the skyline grows
        elif name == "ragged_pairs_given_backwards":
            assert h.rcs_fill() >= fill0
            print("frames renumbered:", h.frame_order() is not None)
        elif name.startswith("nf16") or name.startswith("ragged") or name.startswith("nf2"):
            assert h.rcs_fill() == fill0 and h.rcs_chunks() == chunks0  # pairs inside the window: the plan of the run without
            assert (h.frame_order() is None) == (order0 is None)
        if name == "nf16_chain_and_five_factors_on_frame_3":
            assert np.count_nonzero((fac.a == 3) | (fac.b == 3)) == 5
        if name == "ragged_pairs_given_backwards":
            assert np.all(fac.a > fac.b)
        if name.startswith("long"):
            assert np.diff(sc.row_ptr).max() > 24
    finally:
        h.close()


def test_loop_closure_pair_shares_no_landmark():
    sc, f0, fac, fv, fconst, keep_gauge = rc.case("ragged_loop_closure_2_59")
    pts = np.repeat(np.arange(sc.N), np.diff(sc.row_ptr))
    assert not np.intersect1d(pts[sc.obs_frame == 2], pts[sc.obs_frame == 59]).size


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
def test_relpose_phases_in_every_mode(orc, mode):
    sc, f0, fac, fv, fconst, keep_gauge = rc.case(rc.MODE_CASE)
    h = _handle(fv, **MODES[mode])
    try:
        fac.set_on(h)
        a = _phases(orc, h, sc, f0, 1e-4, fac, keep_gauge, fv)
        if mode == "deterministic":  # the passes have one owner per entry and a fixed summation order: two runs, the same bits
            assert h.deterministic()
            b = _phases(orc, h, sc, f0, 1e-4, fac, keep_gauge, fv)
            for k in ("S", "rhs", "corr", "points", "cam_R", "cam_T", "err", "V", "U", "g"):
                assert np.array_equal(a[k], b[k]), k
    finally:
        h.close()


# ------------------------------------------------------------------ the whole range of residual angles

def _finite(*arrays):
    return all(np.all(np.isfinite(a)) for a in arrays)


@pytest.mark.parametrize("angle", rc.SWEEP, ids=lambda a: f"{a:.12g}")
def test_relpose_phases_over_the_angle_range(orc, angle):
    """relpose_cases.sweep_case: three factors with full information whose rotation residuals all have the given angle, on the
    gauge frames, on (2, 4) and given backwards on (5, 3), through _phases at c = 1e-4 with its tolerances as they are, ten
    and six variables a frame, and with jacobian_mode 0 (per-observation derivative kernels, of which this six-frame scene
    takes the fused one; the two-kernel path needs the 60 frames of relpose_cases.TWO_KERNEL_CASE, whose own test runs it) at one
    angle on either side of every switch of the three formulas.  The yardstick's Log and Jr^-1 are those of tests/so3_ref.py.  The
    factor sum itself is held to rel 1e-10 here: the residuals are within 1e-13 of the yardstick's and no factor's residual is
    shorter than 2e-3 (the translation offsets see to that)."""
    for fv in (10, 6):
        for kw in [{}] + ([dict(jacobian_mode=0)] if angle in so3.AT_SWITCHES else []):
            sc, f0, fac, fv, fconst, keep_gauge = rc.sweep_case(angle, fv)
            h = _handle(fv, **kw)
            try:
                fac.set_on(h)
                assert h.upload(f0, sc)
                so = _orc_scene(orc, sc)
                ok, nrm = orc.normalize(so)
                assert ok
                fn = rr.normalised(fac, nrm)
                e = rr.residuals(fn, so)
                assert np.linalg.norm(e, axis=1).min() > 2e-3 and np.abs(np.linalg.norm(e[:, 3:], axis=1) - angle).max() < 1e-13
                want, got = rr.energy(fn, so), h.relative_pose_error()
                out = _phases(orc, h, sc, f0, 1e-4, fac, keep_gauge, fv)
                assert h.jacobian_kernel() in ((0, 1) if kw else (1, 2, 3))
                Uo = out["ref"]["blocks"][2][:, 10 - fv:, 10 - fv:]
                dU = np.sqrt(np.abs(np.einsum("mii->mi", Uo)))
                print(f"angle {angle:.12g} fv {fv} {kw}: factor sum off by {abs(got - want) / want:.2e}, frame blocks by "
                      f"{sym_scaled_err(out['U'], Uo, dU):.2e} (scaled)")
                assert got == pytest.approx(want, rel=1e-10)
            finally:
                h.close()


def test_relative_pose_residuals_over_the_angle_range():
    """the host getter at every angle of the sweep: rotation rows within 1e-13 of the reference's on the downloaded scene
    (tests/test_so3_cpu.py derives the bound), translation rows within 1e-10 of the extent.  A pair carries one factor and the
    scene has 15 pairs, so the sweep takes two settings on one handle."""
    h = _handle(10)
    try:
        seen = []
        for part in (0, 1):
            sc, f0, fac, angles = rc.residual_sweep(part)
            fac.set_on(h)
            assert h.upload(f0, sc)
            world = sc.copy()
            h.download(world)
            want, got = rr.residuals(fac, world), h.relative_pose_residuals()
            extent = float(np.abs(sc.points - sc.points.mean(axis=0)).max())
            assert got.shape == want.shape == (angles.size, 6)
            assert np.abs(np.linalg.norm(want[:, 3:], axis=1) - angles).max() < 1e-13
            for k, a in enumerate(angles):
                print(f"angle {a:.12g}: rotation rows off by {np.abs(got[k, 3:] - want[k, 3:]).max():.2e}")
            assert np.abs(got[:, :3] - want[:, :3]).max() < 1e-10 * extent
            assert np.abs(got[:, 3:] - want[:, 3:]).max() < 1e-13
            seen += list(angles)
        assert seen == list(rc.SWEEP)
    finally:
        h.close()


def test_relpose_at_exactly_pi():
    """relpose_cases.pi_case: half a turn about a coordinate axis and about a seeded one.  The rounding of the normalisation
    lands on either side of pi, so only what both signs of the residual share is held: everything downloaded is finite, the
    solve succeeds, the residuals have the length pi, and the factor sum (a rotation information that is a multiple of I) is
    the yardstick's."""
    sc, f0, fac, fv, fconst, keep_gauge = rc.pi_case()
    h = _handle(fv)
    try:
        fac.set_on(h)
        assert h.upload(f0, sc)
        nsc = sc.copy()
        ok, nrm = sa.normalize_scene_inplace(nsc)
        assert ok
        fn = rr.normalised(fac, nrm)
        want, got = rr.energy(fn, nsc), h.relative_pose_error()
        err = h.phase_error()[0]
        h.phase_derivatives()
        V, U, W, g = (h.buffer(b).copy() for b in (B.BUF_POINT_BLOCKS, B.BUF_FRAME_BLOCKS, B.BUF_POINT_FRAME, B.BUF_GRAD))
        h.phase_schur(1e-4)
        S, rhs = h.buffer(B.BUF_RCS).copy(), h.buffer(B.BUF_RCS_RHS).copy()
        assert _finite(V, U, W, g, S, rhs) and np.isfinite(err) and np.isfinite(got)
        assert h.phase_solve()
        h.phase_backsub(1e-4)
        assert _finite(h.buffer(B.BUF_CORRECTIONS))
        res = h.relative_pose_residuals()
        ang = np.linalg.norm(res[:, 3:], axis=1)
        print(f"half a turn: residual angles - pi {ang - np.pi}, factor sum {got:.17g}, yardstick {want:.17g}")
        assert _finite(res) and np.abs(ang - np.pi).max() < 1e-13
        assert np.abs(np.abs(res[0, 3:]) - [np.pi, 0, 0]).max() < 1e-13  # about the first axis of Z^T P = diag(1, -1, -1)
        assert got == pytest.approx(want, rel=1e-10) and err > got
    finally:
        h.close()


@pytest.mark.parametrize("fv", [10, 6])
def test_relpose_phases_two_kernel_derivatives_and_unstaged_error_kernel(orc, fv):
    sc, f0, fac, _, fconst, keep_gauge = rc.case(rc.TWO_KERNEL_CASE)
    h = _handle(fv, jacobian_mode=0)
    try:
        fac.set_on(h)
        _phases(orc, h, sc, f0, 1e-4, fac, keep_gauge, fv)
        assert h.jacobian_kernel() == 0
    finally:
        h.close()


def test_relpose_phases_fixed_intrinsics(orc):
    """six variables a frame: the pose part is the whole block (SRK_UGS(6))"""
    sc, f0, fac, fv, fconst, keep_gauge = rc.case(rc.MODE_CASE + "_fixed_k")
    h = _handle(fv)
    try:
        fac.set_on(h)
        _phases(orc, h, sc, f0, 1e-4, fac, keep_gauge, fv)
    finally:
        h.close()


def test_relpose_phases_f32_storage_and_fp32_schur(orc):
    """W stored as float: the tolerances of tests/test_gpu_constant.py::test_constant_phases_f32_storage; and fp32 Schur sums
    run to the end with the factors (their own arithmetic stays fp64: the factor sum equals the yardstick's to 1e-9)"""
    sc, f0, fac, fv, fconst, keep_gauge = rc.case(rc.MODE_CASE)
    h = _handle(fv, storage_precision=True)
    orc.set_w_storage_f32(2)
    try:
        fac.set_on(h)
        _phases(orc, h, sc, f0, 1e-4, fac, keep_gauge, fv, w_tol=1.3e-7, s_tol=1e-9)
    finally:
        orc.set_w_storage_f32(0)
        h.close()
    h = _handle(fv, schur_precision=True)
    try:
        fac.set_on(h)
        base = _run(h, sc, f0, 1e-10, 1e6, 6)
    finally:
        h.close()
    h = _handle(fv)
    try:
        fac.set_on(h)
        full = _run(h, sc, f0, 1e-10, 1e6, 6)
    finally:
        h.close()
    assert base[1].iterations == full[1].iterations and base[1].err_final == pytest.approx(full[1].err_final, rel=1e-5)


def test_relpose_phases_huber_loss_and_information(orc):
    """no robust loss and no information acts on a factor: the energy is the weighted observation energy plus the plain factor sum"""
    sc, f0, fac, fv, fconst, keep_gauge = rc.case(rc.MODE_CASE)
    q = cc.information(sc)
    h = _handle(fv)
    try:
        fac.set_on(h)
        h.set_robust_loss("huber", 1.0)
        h.set_observation_information(q)
        _phases(orc, h, sc, f0, 1e-4, fac, keep_gauge, fv,
                derivatives=lambda so: wr.derivatives(f0, so, q, wr.HUBER, 1.0), energy=lambda so: wr.energy(f0, so, q, wr.HUBER, 1.0))
    finally:
        h.close()


def test_relpose_phases_with_position_priors(orc):
    sc, f0, fac, fv, fconst, keep_gauge = rc.case(rc.MODE_CASE)
    pri = pc.priors_for(sc, cc._every(sc.N, 7), [3, 12])
    h = _handle(fv)
    try:
        fac.set_on(h)
        pri.set_on(h, 1)
        out = _phases(orc, h, sc, f0, 1e-4, fac, keep_gauge, fv, pri_w=pri)
        ep, ef = h.prior_error()
        assert ep > 0 and ef > 0 and h.relative_pose_error() > 0
        assert out["err"] > ep + ef + h.relative_pose_error()
    finally:
        h.close()


def test_speculation_on_and_off_take_the_same_decisions():
    sc, f0, fac, fv, fconst, keep_gauge = rc.case(rc.MODE_CASE)
    runs = []
    for spec in (True, False):
        h = _handle(fv, speculation=spec)
        try:
            fac.set_on(h)
            runs.append(_run(h, sc, f0, 1e-10, 1e6, 8))
        finally:
            h.close()
    assert runs[0][1].iterations > 0
    _compare_runs(*runs)


# ------------------------------------------------------------------ reordered frames, chunked solve

def test_relpose_shuffled_frames_take_the_reordering_and_agree(orc):
    """a shuffled-frame scene with set_frame_reordering(1): the pairs go through the renumbering, which flips some of them
    (the transposed block).  Phase by phase against the yardstick on the shuffled scene, and the LM run against the run of the
    unshuffled scene (1e-7, as tests/test_gpu_constant.py::test_constant_shuffled_frames_take_the_reordering_and_agree)."""
    sc, f0, fac, fv, fconst, keep_gauge = rc.case(rc.REORDER_CASE)
    perm = np.concatenate([[0, 1], 2 + np.random.RandomState(0).permutation(sc.M - 2)])  # the gauge frames stay 0 and 1
    sh = sa.renumber_frames(sc, perm)
    fsh = rr.Factors(perm[fac.a], perm[fac.b], fac.Z, fac.z, fac.info).sorted()
    assert rr.energy(fsh, sh) == pytest.approx(rr.energy(fac, sc), rel=1e-12)
    h = _handle(fv)
    try:
        fac.set_on(h)
        base = _run(h, sc, f0, 1e-10, 1e6, 8)
        h.set_frame_reordering(1)
        fsh.set_on(h)
        _phases(orc, h, sh, f0, 1e-4, fsh, keep_gauge, fv)
        order = h.frame_order()
        assert order is not None  # renumbered internally
        ia, ib = np.asarray(order)[fsh.a], np.asarray(order)[fsh.b]
        assert np.any((ia > ib) != (fsh.a > fsh.b))  # the internal order flips a pair
        ok, rep, sg, log = _run(h, sh, f0, 1e-10, 1e6, 8)
        back = sa.Scene(sg.points, sg.cam_R[perm], sg.cam_T[perm], sc.K, sc.shared_k, sc.row_ptr, sc.obs_frame, sc.obs_uv)
        _compare_runs(base, (ok, rep, back, log))
    finally:
        h.close()


def test_set_covisibility_on_one_rank_keeps_the_pairs_in_the_skyline():
    """a caller's covisibility (landmarks only) handed to set_covisibility after the upload: the loop-closure pair is put back
    into min_cv, so the coupling block stays inside the skyline and the corrections are those of before"""
    sc, f0, fac, fv, fconst, keep_gauge = rc.case("ragged_loop_closure_2_59")
    h = _handle(fv, frame_reordering=0)
    try:
        fac.set_on(h)
        sols, fills = [], []
        for given in (False, True):
            assert h.upload(f0, sc)
            if given:
                h.set_covisibility(B.covisibility(sc))
            fills.append(h.rcs_fill())
            h.phase_derivatives()
            h.phase_schur(1e-4)
            S = h.buffer(B.BUF_RCS).reshape(fv * sc.M, fv * sc.M)
            assert np.abs(S[10 * 59 + 4:10 * 59 + 10, 10 * 2 + 4:10 * 2 + 10]).max() > 0
            assert h.phase_solve()
            h.phase_backsub(1e-4)
            sols.append(h.buffer(B.BUF_CORRECTIONS))
        assert fills[0] == fills[1] and rel_err(sols[1], sols[0]) < 1e-9
    finally:
        h.close()


@pytest.mark.parametrize("pairs", ["chain", "far", "far_renumbered"])
def test_chunked_scene_with_factors(pairs):
    """330 frames, window 8 (the smallest scene of test_chunked_solve_equals_single_chain).  A consecutive chain leaves the
    chunk plan alone: rcs modes 2, 1 and 0 agree with each other and with numpy on the downloaded system, as that test
    compares.  One pair (5, 300) in the caller's frame order is beyond the 1024-variable band: no chunks, the result still
    right.  With the automatic renumbering the tied sequence becomes a band again (about twice as wide) and whatever plan
    follows gives the same result."""
    spec = rc.CHUNKED
    sc = sa.generate_scene(spec)
    M = sc.M
    fac = rc.factors_for(sc, rc.chain(M) if pairs == "chain" else [(5, 300)])
    c = 1e-3
    h = _handle(10, frame_reordering=0) if pairs == "far" else _handle(10)
    sols = {}
    try:
        fac.set_on(h)
        for mode in (2, 1, 0):
            h.set_rcs_mode(mode)
            assert h.upload(spec.f0, sc)
            if mode == 2:
                print(f"{pairs}: chunks {h.rcs_chunks()}, fill {h.rcs_fill():.4f}, renumbered {h.frame_order() is not None}")
                if pairs != "far_renumbered":
                    assert (h.rcs_chunks() >= 2) if pairs == "chain" else (h.rcs_chunks() == 0)
            h.phase_derivatives()
            h.phase_schur(c)
            if mode == 2:
                S = h.buffer(B.BUF_RCS).reshape(10 * M, 10 * M)
                rhs = h.buffer(B.BUF_RCS_RHS)
            assert h.phase_solve()
            h.phase_backsub(c)
            sols[mode] = h.buffer(B.BUF_CORRECTIONS)
        blk = S[10 * 300 + 4:10 * 300 + 10, 10 * 5 + 4:10 * 5 + 10] if pairs != "chain" else S[10 * 200 + 4:10 * 200 + 10, 10 * 199 + 4:10 * 199 + 10]
        assert np.abs(blk).max() > 0
        x = np.linalg.solve(S, rhs)
        for _ in range(3):
            x = x + np.linalg.solve(S, rhs - S @ x)
        dc2 = sols[2][3 * sc.N:]
        assert rel_err(dc2, x) < 1e-9
        assert rel_err(sols[2], sols[1]) < 1e-9 and rel_err(sols[2], sols[0]) < 1e-9
        assert np.all(dc2[4:10] == 0) and dc2[15] == 0
    finally:
        h.close()


# ------------------------------------------------------------------ LM runs

def _same_as_yardstick(orc, gpu, sc, f0, fac, keep_gauge, fv, fconst, **kw):
    so = _orc_scene(orc, sc)
    rc_o, rep_o = rr.compute_inplace(orc, f0, so, fac, keep_gauge, fv, fconst=fconst, allowed_err_change=kw.get("allowed"),
                                     max_hessian_factor=kw.get("max_factor"), max_iterations=kw.get("max_iterations", 0))
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


@pytest.mark.parametrize("name", [rc.MODE_CASE, "nf16_frame_0_constant_free_gauge"])
def test_relpose_24_frames_ten_iterations_vs_python_lm_loop(orc, name):
    """attempt by attempt against the Python loop, with the reference's gauge and with frame 0 constant instead of it"""
    sc, f0, fac, fv, fconst, keep_gauge = rc.case(name)
    assert sc.M == 24
    h = _handle(fv)
    try:
        _set_case(h, fac, fconst, keep_gauge)
        _, rep, sg, _ = _same_as_yardstick(orc, h, sc, f0, fac, keep_gauge, fv, fconst, max_iterations=10)
        assert rep.iterations == 10
        assert np.array_equal(sg.cam_T[fconst], sc.cam_T[fconst])
    finally:
        h.close()


def _distance(sg, pts_gt, R_gt, T_gt):
    return max(float(np.abs(sg.cam_T - T_gt).max()), float(np.abs(sg.cam_R - R_gt).max()), float(np.abs(sg.points - pts_gt).max()))


def test_metric_scale_comes_from_the_factors(orc):
    """relpose_cases.metric_scale(): the noise-free scene scaled by 1.02 about C_0, frame 0 constant, the reference's gauge
    released, ground-truth relative poses on the consecutive pairs.  The reprojection sum is blind to the scale (it starts at
    rounding level), the factors are not.  The GPU run reproduces the Python loop's iterations, attempts and status and lands
    as close to the ground truth as the Python loop does: the bound is ten times the distance that loop reaches here (the
    factor 10 for summation order), computed in this test and not chosen in advance.  Measured on the CPU
    (tests/test_relpose_cpu.py prints it): 12 iterations, 27 attempts, err 1.8e-2 -> 1.9e-17, distance 4.9e-8 from a start
    0.25 away, so the bound is 4.9e-7.  Without the factors the same run stays at the 2 % scale."""
    import test_relpose_cpu as cpu
    spec, sc, fac, fconst, pts_gt, R_gt, T_gt = rc.metric_scale()
    so = _orc_scene(orc, sc)
    rc_o, rep_o = rr.compute_inplace(orc, spec.f0, so, fac, 0, 6, fconst=fconst, allowed_err_change=1e-30, max_hessian_factor=1e12,
                                     max_iterations=cpu.METRIC_ITERATIONS)
    d_cpu = _distance(so, pts_gt, R_gt, T_gt)
    bound = 10 * d_cpu
    print(f"python loop: {rep_o.iterations} iterations, {rep_o.attempts} attempts, status {rep_o.status}, err {rep_o.err_initial:.3e} -> "
          f"{rep_o.err_final:.3e}, distance {d_cpu:.3e}; bound {bound:.3e}")
    assert d_cpu < 1e-6, "the yardstick itself does not return to the ground truth"
    h = _handle(6)
    try:
        fac.set_on(h)
        h.set_constant_blocks(fconst, None, False)
        assert h.upload(spec.f0, sc)
        e_all, e_fac = h.phase_error()[0], h.relative_pose_error()
        assert e_all - e_fac < 1e-12 * e_fac  # the reprojection sum does not see the scale
        ok, rep, sg, log = _run(h, sc, spec.f0, 1e-30, 1e12, cpu.METRIC_ITERATIONS)
        d_gpu = _distance(sg, pts_gt, R_gt, T_gt)
        print(f"gpu: {rep.iterations} iterations, {rep.attempts} attempts, status {rep.status}, err {rep.err_initial:.3e} -> "
              f"{rep.err_final:.3e}, distance {d_gpu:.3e}")
        assert (rep.iterations, rep.attempts, rep.status) == (rep_o.iterations, rep_o.attempts, rep_o.status)
        assert ok == (rc_o == 0)
        assert d_gpu < bound
        res = h.relative_pose_residuals()
        assert res.shape == (fac.n, 6) and np.abs(res).max() < bound
        h.set_relative_pose_factors(None)
        ok, rep, sg, _ = _run(h, sc, spec.f0, 1e-30, 1e12, cpu.METRIC_ITERATIONS)
        d_free = _distance(sg, pts_gt, R_gt, T_gt)
        print(f"without factors: err {rep.err_initial:.3e} -> {rep.err_final:.3e}, distance {d_free:.3e}")
        assert d_free > 1e-3
    finally:
        h.close()


def test_zero_residual_factors_leave_gradient_and_error_unchanged(orc):
    """factors whose measurements are the current relative poses (relative_pose() of the uploaded scene): no NaN anywhere, the
    error and the gradient are those of the run without factors up to the rounding of R_a R_b^T (e_r of order 1e-16: the
    gradient moves by less than 1e-12 of its scale), the frame blocks grow by 2 J^T L J"""
    sc, f0, fac, fv, fconst, keep_gauge = rc.case(rc.MODE_CASE)
    for k in range(fac.n):
        fac.Z[k], fac.z[k] = B.relative_pose(sc, int(fac.a[k]), int(fac.b[k]))
    h = _handle(fv)
    try:
        assert h.upload(f0, sc)
        e0 = h.phase_error()[0]
        h.phase_derivatives()
        g0, U0 = h.buffer(B.BUF_GRAD).copy(), h.buffer(B.BUF_FRAME_BLOCKS).copy()
        fac.set_on(h)
        assert h.upload(f0, sc)
        e1, ef = h.phase_error()[0], h.relative_pose_error()
        h.phase_derivatives()
        g1, U1 = h.buffer(B.BUF_GRAD), h.buffer(B.BUF_FRAME_BLOCKS)
        h.phase_schur(1e-4)
        S = h.buffer(B.BUF_RCS)
        print(f"factor sum {ef:.3e}, error {e0:.17g} -> {e1:.17g}, gradient moved by {np.abs(g1 - g0).max():.3e} of {np.abs(g0).max():.3e}")
        assert np.all(np.isfinite(g1)) and np.all(np.isfinite(U1)) and np.all(np.isfinite(S))
        assert ef < 1e-24 and e1 == pytest.approx(e0, rel=1e-14)
        assert np.abs(g1 - g0).max() < 1e-12 * np.abs(g0).max()
        assert np.abs(U1 - U0).max() > 1.0
        assert np.abs(h.relative_pose_residuals()).max() < 1e-12
    finally:
        h.close()


def test_deterministic_mode_gives_identical_bits_with_factors():
    sc, f0, fac, fv, fconst, keep_gauge = rc.case("nf16_chain_and_five_factors_on_frame_3")
    runs = []
    for _ in range(2):
        h = _handle(fv, deterministic=True)
        try:
            fac.set_on(h)
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


def test_all_zero_information_gives_the_bits_of_the_run_without_that_factor():
    """an all-zero information matrix is a valid, switched-off factor: plan and run equal, bit for bit, those of the setting
    without it, even where its pair would widen the skyline (deterministic mode)"""
    sc, f0, fac, fv, fconst, keep_gauge = rc.case(rc.MODE_CASE)
    more = rc.factors_for(sc, list(zip(fac.a, fac.b)) + [(2, 22), (15, 16)])
    keep = np.array([(int(a), int(b)) in set(zip(fac.a.tolist(), fac.b.tolist())) for a, b in zip(more.a, more.b)])
    more.Z[keep], more.z[keep], more.info[keep] = fac.Z, fac.z, fac.info
    more.info[~keep] = 0
    runs, fills = [], []
    for f in (fac, more):
        h = _handle(fv, deterministic=True)
        try:
            f.set_on(h)
            runs.append(_run(h, sc, f0, None, None, 4))
            fills.append(h.rcs_fill())
            if f is more:
                assert h.relative_pose_factors()["pairs"].shape == (fac.n + 2, 2)
                res = h.relative_pose_residuals()  # the switched-off factors still report their residuals
                assert res.shape == (fac.n + 2, 6) and np.all(np.any(res != 0, axis=1))
        finally:
            h.close()
    (ok_a, rep_a, sg_a, log_a), (ok_b, rep_b, sg_b, log_b) = runs
    assert fills[0] == fills[1]
    assert rep_a.iterations > 0 and (rep_a.iterations, rep_a.attempts) == (rep_b.iterations, rep_b.attempts)
    assert (rep_a.err_initial, rep_a.err_final) == (rep_b.err_initial, rep_b.err_final)
    assert np.array_equal(log_a["err"], log_b["err"])
    for x in ("points", "cam_R", "cam_T"):
        assert np.array_equal(getattr(sg_a, x), getattr(sg_b, x)), x


# ------------------------------------------------------------------ getters

def test_getters_error_and_residuals_in_the_callers_units(orc):
    """relative_pose_error() equals the yardstick's sum (rel 1e-12) on the library's own normalised factors, phase_error the
    observation energy plus it, and relative_pose_residuals() the yardstick's [e_t; e_r] of the downloaded scene in the
    caller's coordinates (1e-10 of the extent), on the scene uploaded un-normalised with a rotated frame 0 and s = 2.5, before
    and after an optimisation"""
    sc, f0, fac, fv, fconst, keep_gauge = rc.case("nf2_gauge_frames_full_information_rotated_world")
    h = _handle(fv)
    try:
        fac.set_on(h)
        got = h.relative_pose_factors()
        assert np.array_equal(got["pairs"], np.stack([fac.a, fac.b], axis=1)) and np.array_equal(got["rel_R"], fac.Z)
        assert np.array_equal(got["rel_t"], fac.z) and np.array_equal(got["info"], rr.tri21(fac.info))
        assert h.upload(f0, sc)
        nsc = sc.copy()
        ok, nrm = sa.normalize_scene_inplace(nsc)
        assert ok
        zn, ln = B.normalize_relative_pose_factors(nrm, fac.z, rr.tri21(fac.info))
        fn = rr.Factors(fac.a, fac.b, fac.Z, zn, rr.full(ln))
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
            want = rr.energy(fn, so)
            e = h.relative_pose_error()
            print(f"{stage}: factor sum {e:.17g}, yardstick {want:.17g}")
            assert e == pytest.approx(want, rel=1e-12)
            assert h.phase_error()[0] == pytest.approx(orc.reproj_error(f0, so)[0] + want, rel=1e-10)
            world = sc.copy()
            h.download(world)
            wres = rr.residuals(fac, world)
            res = h.relative_pose_residuals()
            assert np.abs(res[:, :3] - wres[:, :3]).max() < 1e-10 * extent and np.abs(res[:, 3:] - wres[:, 3:]).max() < 1e-10
            assert np.abs(res[:, :3]).max() > 1e-5 * extent and np.abs(res[:, 3:]).max() > 1e-5
            # the energy is invariant under the normalisation: the caller's residuals against the caller's information
            assert float(np.einsum("na,nab,nb->", res, fac.info, res)) == pytest.approx(e, rel=1e-8)
        # SRK_E_STATE: the stored setting changed after the upload
        f2 = fac.copy()
        f2.z[0] += 1e-3
        f2.set_on(h)
        with pytest.raises(Exception):
            h.relative_pose_residuals()
        assert "changed after the upload" in h.last_error()
        assert h.relative_pose_error() == pytest.approx(e, rel=1e-12)  # still the resident scene's lists
        assert h.upload(f0, sc)
        assert h.relative_pose_residuals().shape == (fac.n, 6)
        h.set_profile(1)
        h.phase_derivatives(); h.phase_schur(1e-4); h.phase_error()
        ms = h.relative_pose_pass_ms()
        print("pass ms", ms)
        assert all(0 < m < 5 for m in ms)
    finally:
        h.close()


# ------------------------------------------------------------------ state and refusals

SMALL = sa.SceneSpec(n_frames=6, grid_nx=5, grid_ny=4, vis_window=3)


def _small_factors(sc):
    return rc.factors_for(sc, [(0, 1), (2, 4), (5, 3)], "full")


def test_unsupported_combinations_are_refused_in_either_order_and_the_handle_stays_usable():
    sc = sa.generate_scene(SMALL)
    fac = _small_factors(sc)
    hook = _lib.ALLREDUCE_FN(lambda *a: 0)
    h = sa.BundleAdjustmentKanatani(0)
    try:
        fac.set_on(h)
        with pytest.raises(ValueError):
            h.set_intrinsic_groups(np.zeros(sc.M, np.int32))
        assert "relative-pose factors" in h.last_error() and h.intrinsic_groups() == 0
        ok, rep, sg, _ = _run(h, sc, 600.0, 1e-10, 1e6, 3)
        assert rep.iterations > 0 and h.relative_pose_error() > 0
    finally:
        h.close()
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_intrinsic_groups(np.zeros(sc.M, np.int32))
        with pytest.raises(ValueError):
            fac.set_on(h)
        assert "intrinsic groups" in h.last_error() and h.relative_pose_factors() is None and h.intrinsic_groups() == 1
        h.set_intrinsic_groups(None)
        fac.set_on(h)  # fine once the groups are gone
        ok, rep, sg, _ = _run(h, sc, 600.0, 1e-10, 1e6, 3)
        assert rep.iterations > 0 and h.relative_pose_error() > 0
    finally:
        h.close()
    h = sa.BundleAdjustmentKanatani(0)
    try:
        fac.set_on(h)
        with pytest.raises(ValueError):
            h.set_allreduce(hook, 0, 2)
        assert "more than one rank" in h.last_error()
    finally:
        h.close()
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_allreduce(hook, 0, 2)
        with pytest.raises(ValueError):
            fac.set_on(h)
        assert "more than one rank" in h.last_error() and h.relative_pose_factors() is None
    finally:
        h.close()


def test_bad_arguments_leave_the_previous_setting_in_force():
    sc = sa.generate_scene(SMALL)
    fac = _small_factors(sc)
    h = sa.BundleAdjustmentKanatani(0)
    try:
        assert h.relative_pose_factors() is None
        fac.set_on(h)
        bad_Z = fac.Z.copy()
        bad_Z[1] *= 1.0 + 1e-6
        neg = fac.info.copy()
        neg[0] = -np.eye(6)
        nan_z = fac.z.copy()
        nan_z[2, 0] = np.nan
        bad = {
            "a == b": ([(0, 1), (2, 2), (5, 3)], fac.Z, fac.z, fac.info),
            "twice": ([(0, 1), (1, 0), (5, 3)], fac.Z, fac.z, fac.info),
            "unsorted": ([(2, 4), (0, 1), (5, 3)], fac.Z, fac.z, fac.info),
            "negative": ([(-1, 1), (2, 4), (5, 3)], fac.Z, fac.z, fac.info),
            "rotation": (np.stack([fac.a, fac.b], axis=1), bad_Z, fac.z, fac.info),
            "information": (np.stack([fac.a, fac.b], axis=1), fac.Z, fac.z, neg),
            "nan": (np.stack([fac.a, fac.b], axis=1), fac.Z, nan_z, fac.info),
        }
        for what, (pairs, Z, z, info) in bad.items():
            with pytest.raises(ValueError):
                h.set_relative_pose_factors(pairs, Z, z, info=info)
            assert "relative-pose factors" in h.last_error(), what
            got = h.relative_pose_factors()
            assert got is not None and np.array_equal(got["pairs"], np.stack([fac.a, fac.b], axis=1)), what
            assert np.array_equal(got["rel_t"], fac.z) and np.array_equal(got["info"], rr.tri21(fac.info)), what
        ok, rep, sg, _ = _run(h, sc, 600.0, 1e-10, 1e6, 3)
        assert rep.iterations > 0
    finally:
        h.close()


def test_index_beyond_the_scene_fails_the_upload_and_the_setting_survives_reset_and_compute_inplace():
    sc = sa.generate_scene(SMALL)
    other = sa.generate_scene(sa.SceneSpec(n_frames=4, grid_nx=3, grid_ny=3, vis_window=3))
    fac = _small_factors(sc)
    assert max(fac.a.max(), fac.b.max()) >= other.M
    h = sa.BundleAdjustmentKanatani(0)
    try:
        fac.set_on(h)
        with pytest.raises(ValueError):
            h.upload(600.0, other)
        assert "relative-pose factors" in h.last_error()
        with pytest.raises(ValueError):
            _run(h, other, 600.0, 1e-10, 1e6, 3)
        assert h.upload(600.0, sc)
        e0 = h.relative_pose_error()
        assert e0 > 0
        h.reset()
        assert np.array_equal(h.relative_pose_factors()["pairs"], np.stack([fac.a, fac.b], axis=1))
        assert h.relative_pose_error() == e0
        with_f = _run(h, sc, 600.0, 1e-10, 1e6, 5)  # re-applied by compute_inplace (an upload of its own)
        assert h.relative_pose_error() > 0
        h.set_relative_pose_factors(None)
        assert h.relative_pose_factors() is None
        without = _run(h, sc, 600.0, 1e-10, 1e6, 5)
        assert h.relative_pose_error() == 0.0
        assert np.abs(with_f[2].cam_T - without[2].cam_T).max() > 1e-6
        assert h.upload(600.0, other)  # and the other scene uploads again
    finally:
        h.close()


@pytest.mark.parametrize("name", ["C1_dino_standin", "nf16_10_tiles"])
def test_default_is_bitwise_unchanged_after_toggling(name):
    """Set factors (a loop closure among them, so that the skyline and the plans change), run, clear, run again: the second
    run equals a fresh handle's run bit for bit.  As tests/test_gpu_constant.py::test_default_is_bitwise_unchanged_after_toggling:
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
        fac = rc.factors_for(sc, rc.chain(sc.M) + [(0, sc.M - 1)])
        fac.set_on(toggled)
        ok, rep, sg, _ = _run(toggled, sc, f0, None, None, 6)
        assert rep.iterations > 0 and toggled.relative_pose_error() > 0
        toggled.set_relative_pose_factors(None)
        runs = [_run(h, sc, f0, None, None, 12) for h in (fresh, toggled)]
        assert fresh.deterministic() and toggled.deterministic()
        assert fresh.rcs_fill() == toggled.rcs_fill() and fresh.rcs_chunks() == toggled.rcs_chunks()
        (ok_a, rep_a, sg_a, log_a), (ok_b, rep_b, sg_b, log_b) = runs
        assert (ok_a, rep_a.iterations, rep_a.attempts, rep_a.status) == (ok_b, rep_b.iterations, rep_b.attempts, rep_b.status)
        assert (rep_a.err_initial, rep_a.err_final) == (rep_b.err_initial, rep_b.err_final)
        assert np.array_equal(log_a["attempts"], log_b["attempts"]) and np.array_equal(log_a["err"], log_b["err"])
        for x in ("points", "cam_R", "cam_T"):
            assert np.array_equal(getattr(sg_a, x), getattr(sg_b, x)), x
    finally:
        fresh.close()
        toggled.close()


def test_cpp_adapter_set_relative_pose_factors(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "relpose_adapter"
    r = subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "demos"),
                        os.path.join(HERE, "cpp", "test_relpose_adapter.cpp"), "-o", str(exe),
                        "-L", os.path.join(ROOT, "surikatoko_amd"), "-lsrk_ba",
                        "-Wl,-rpath," + os.path.join(ROOT, "surikatoko_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "relpose adapter ok" in r.stdout
