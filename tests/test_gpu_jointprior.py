"""Joint Gaussian pose priors on the GPU (srk_ba_set_joint_pose_priors) against the yardstick of tests/jointprior_ref.py -- the
oracle's blocks plus the sets' terms in numpy, the dense numpy Schur complement of tests/constant_ref.py plus the coupling
blocks, restricted to the free variables -- and lm_ref.loop around it.  The cases are those of tests/jointprior_cases.py, each
checked for conditioning by tests/test_jointprior_cpu.py.

Comparisons and tolerances are those of tests/test_gpu_constant.py::_phases, as tests/test_gpu_relpose.py takes them: blocks
1e-12 scaled, gradient, reduced camera system and rhs 1e-10 scaled, corrections and the applied scene 1e-8 relative (widened
to four times the distance of the yardstick's own solver from the exact solution of its system), the corrections against
that exact solution, and phase_error after the accept at rel 1e-6.
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
import covariance_cases as vc
import lm_trajectory as lt
import prior_cases as pc
import prior_ref as pref
import relpose_ref as rr
import jointprior_cases as jc
import jointprior_ref as jr
import so3_ref as so3
import weighted_ref as wr
from test_jointprior_cpu import DOUBLING_FRAMES, doubling_reference
from gpu_common import orc_scene as _orc_scene, handle as _handle, run_lm as _run, compare_runs as _compare_runs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _phases(orc, gpu, sc, f0, c, sets_w, keep_gauge, fv, fconst=None, fac_w=None, derivatives=None, energy=None, pri_w=None,
            w_tol=1e-12, s_tol=1e-10, corr_tol=1e-8):
    """derivatives -> schur -> solve -> backsub -> accept on both sides, checked (tests/test_gpu_relpose.py::_phases with the
    sets' terms and couplings on the yardstick's side); gpu has the sets sets_w (the coordinates of sc) and any factors,
    constant blocks and position priors set"""
    so = _orc_scene(orc, sc)
    ok, nrm = orc.normalize(so)
    assert ok
    sets = jr.normalised(sets_w, nrm)
    fac = None if fac_w is None else rr.normalised(fac_w, nrm)
    pri = None if pri_w is None else pref.normalised(pri_w, nrm)
    assert gpu.upload(f0, sc) and gpu.frame_vars() == fv
    N, M, off = sc.N, sc.M, 10 - fv
    fconst = np.zeros(M, dtype=bool) if fconst is None else fconst
    pconst = np.zeros(N, dtype=bool)
    ref = jr.step(orc, f0, so, c, sets, keep_gauge, fv, fconst, pconst, want_system=True, derivatives=derivatives, pri=pri, fac=fac)
    assert ref["ok"]
    gE, Vo, Uo, Wo = ref["blocks"][:4]

    def total(s):
        return ((energy(s) if energy else orc.reproj_error(f0, s)[0]) + jr.energy(sets, s) + (rr.energy(fac, s) if fac else 0.0) +
                (sum(pref.energy(pri, s)) if pri else 0.0))

    eo = total(so)
    assert gpu.phase_error()[0] == pytest.approx(eo, rel=1e-9)
    assert gpu.joint_pose_prior_error() == pytest.approx(jr.energy(sets, so), rel=1e-9)
    P0, R0, T0 = (gpu.buffer(b).copy() for b in (B.BUF_POINTS, B.BUF_CAM_R, B.BUF_CAM_T))
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
    assert sym_scaled_err(Vg, Vo, dV) < 1e-12
    assert sym_scaled_err(Ug, Uo[:, off:, off:], dU) < 1e-12
    if w_tol <= 1e-12:
        assert class_rel_err(Wg, Wo[:, :, off:], (1, 2)) < 1e-12
    else:  # f32 storage: the table of tests/test_gpu_parity.py::test_f32_storage_mode_tolerance_table
        dW = np.abs(Wg - Wo[:, :, off:]) / np.abs(Wo[:, :, off:]).max()
        assert dW.max() < w_tol and np.quantile(dW, 0.999) < 1e-12
    gref = kref.to_layout(ref["g"], N, M, fv)
    assert np.all(gg[3 * N:][cvar] == 0)
    gs = 2.0 * np.sqrt(max(eo, 1e-300))
    dg = np.concatenate([dV.reshape(-1), dU.reshape(-1)]) * gs
    cmp_g = (dg > 0) & ~np.concatenate([np.zeros(3 * N, dtype=bool), cvar])
    assert float((np.abs(gg - gref)[cmp_g] / dg[cmp_g]).max()) < 1e-10
    # the sets' terms are there at all: without them the frame blocks are off by far more than the tolerance
    base = orc.derivatives(f0, so) if derivatives is None else derivatives(so)
    base = base[:4] if pri is None else pref.add_terms(base[:4], so, pri)
    if fac is not None:
        base = rr.add_terms(base, so, fac)
    touched = sets.frames()
    assert sym_scaled_err(Ug[touched], base[2][touched][:, off:, off:], dU[touched]) > 1e-6

    gpu.phase_schur(c)
    Sg = gpu.buffer(B.BUF_RCS).reshape(fv * M, fv * M)
    rg = gpu.buffer(B.BUF_RCS_RHS)
    free = ~fixed
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
    # the coupling blocks on their own, and as download_rcs_rows shows them
    for a, b, Cb in jr.couplings(sets, so):
        ra, rb = fv * a + (fv - 6) + np.arange(6), fv * b + (fv - 6) + np.arange(6)
        got = Sg[np.ix_(ra, rb)]
        want = ref["S"][np.ix_(idx[ra], idx[rb])].copy()
        want[fixed[ra], :] = 0
        want[:, fixed[rb]] = 0
        scale = dU[a, fv - 6:, None] * dU[b, None, fv - 6:]
        assert float((np.abs(got - want) / scale).max()) < 1e-10, (a, b)
        if not (fixed[ra].all() or fixed[rb].all()):
            assert float((np.abs(Cb) / scale).max()) > 1e-6  # and it is no rounding-sized block
        hi, lo = (ra, rb) if a > b else (rb, ra)
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
    assert np.all(corr[3 * N:][fixed] == 0)
    cref_l = kref.to_layout(ref["corr"], N, M, fv)
    tol = max(corr_tol, 4 * ref["d_solver"])
    print(f"\ncond {cond:.3e}; yardstick solver off by {ref['d_solver']:.3e}; corrections differ by {rel_err(corr, cref_l):.3e} "
          f"(tolerance {tol:.3e})")
    assert 4 * ref["d_solver"] < 1e-6, f"the yardstick's solver itself is off by {ref['d_solver']:.2e} on this case"
    assert rel_err(corr, cref_l) < tol
    lim = max(1e-9, 100 * np.finfo(np.float64).eps * cond) if corr_tol <= 1e-8 else corr_tol
    assert rel_err(corr[3 * N:][free], ref["dc_exact"][idx[free]]) < lim
    x = np.linalg.solve(Sg, rg)  # and numpy on the downloaded system
    for _ in range(3):
        x = x + np.linalg.solve(Sg, rg - Sg @ x)
    assert rel_err(corr[3 * N:], x) < lim
    P1, R1, T1 = (gpu.buffer(b) for b in (B.BUF_POINTS, B.BUF_CAM_R, B.BUF_CAM_T))
    assert np.array_equal(P1, P0) and np.array_equal(R1, R0) and np.array_equal(T1, T0)
    gpu.phase_accept()
    bak = (so.cam_R.copy(), so.cam_T.copy())
    orc.apply_corrections(so, ref["corr"])
    so.cam_R[fconst], so.cam_T[fconst] = bak[0][fconst], bak[1][fconst]
    P1, R1, T1 = (gpu.buffer(b) for b in (B.BUF_POINTS, B.BUF_CAM_R, B.BUF_CAM_T))
    assert np.array_equal(T1.reshape(-1, 3)[fconst], T0.reshape(-1, 3)[fconst])
    assert np.array_equal(R1.reshape(-1, 9)[fconst], R0.reshape(-1, 9)[fconst])
    scale = max(1.0, float(np.abs(so.points).max()))
    assert np.abs(P1.reshape(-1, 3) - so.points).max() < tol * scale
    assert np.abs(R1.reshape(-1, 9) - so.cam_R).max() < tol
    assert np.abs(T1.reshape(-1, 3) - so.cam_T).max() < tol * scale
    e2 = gpu.phase_error()[0]
    assert e2 == pytest.approx(total(so), rel=1e-6)
    assert gpu.joint_pose_prior_error() == pytest.approx(jr.energy(sets, so), rel=1e-6, abs=1e-18)
    return dict(S=Sg, rhs=rg, corr=corr, ref=ref, points=P1, cam_R=R1, cam_T=T1, err=e2, V=Vg, U=Ug, g=gg)


def _set_case(h, sets, fconst, keep_gauge, fac):
    sets.set_on(h, keep_gauge)
    if fac is not None:
        fac.set_on(h)
    if fconst.any():
        h.set_constant_blocks(fconst, None, True)


PHASE_CASES = [n for n in jc.CASES if n not in (jc.REORDER_CASE, jc.MODE_CASE + "_fixed_k")]


@pytest.mark.parametrize("c", [1e-4, 1.0])
@pytest.mark.parametrize("name", PHASE_CASES)
def test_jointprior_phases_vs_yardstick(orc, name, c):
    sc, f0, sets, fv, fconst, keep_gauge, fac = jc.case(name)
    h = _handle(fv)
    try:
        assert h.upload(f0, sc)
        fill0, chunks0 = h.rcs_fill(), h.rcs_chunks()
        _set_case(h, sets, fconst, keep_gauge, fac)
        _phases(orc, h, sc, f0, c, sets, keep_gauge, fv, fconst=fconst, fac_w=fac)
        print(f"{name}: rcs_fill {fill0} -> {h.rcs_fill()}, chunks {chunks0} -> {h.rcs_chunks()}")
        got, kg = h.joint_pose_priors()
        assert kg == bool(keep_gauge) and len(got) == sets.n
        if name.startswith("sixteen"):
            assert sets.sets[0]["frames"].size == 16 and len(jr.frame_pairs(sets)) == 120
        if name == "three_frames_one_zero_block":
            assert jr.frame_pairs(sets) == [(8, 10), (10, 12)]
            S = h.buffer(B.BUF_RCS).reshape(fv * sc.M, fv * sc.M)
            assert np.abs(S[fv * 12 + 4:fv * 12 + 10, fv * 10 + 4:fv * 10 + 10]).max() > 0
        if name.startswith("one_frame"):
            assert jr.frame_pairs(sets) == [] and h.rcs_fill() == fill0 and h.rcs_chunks() == chunks0
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
def test_jointprior_phases_in_every_mode(orc, mode):
    sc, f0, sets, fv, fconst, keep_gauge, fac = jc.case(jc.MODE_CASE)
    h = _handle(fv, **MODES[mode])
    try:
        sets.set_on(h)
        a = _phases(orc, h, sc, f0, 1e-4, sets, keep_gauge, fv)
        if mode == "deterministic":  # the passes have one owner per entry and a fixed summation order: two runs, the same bits
            assert h.deterministic()
            b = _phases(orc, h, sc, f0, 1e-4, sets, keep_gauge, fv)
            for k in ("S", "rhs", "corr", "points", "cam_R", "cam_T", "err", "V", "U", "g"):
                assert np.array_equal(a[k], b[k]), k
    finally:
        h.close()


# ------------------------------------------------------------------ the whole range of residual angles

def _finite(*arrays):
    return all(np.all(np.isfinite(a)) for a in arrays)


@pytest.mark.parametrize("angle", jc.SWEEP, ids=lambda a: f"{a:.12g}")
def test_jointprior_phases_over_the_angle_range(orc, angle):
    """jointprior_cases.sweep_case: one set of three frames, dense 18 x 18 information, a non-zero mean, every slot's rotation
    residual at the given angle, through _phases at c = 1e-4 with its tolerances as they are, ten and six variables a frame,
    and with jacobian_mode 0 (per-observation derivative kernels) at one angle on either side of every switch of the three
    formulas.  The yardstick's Log and
    Jl^-1 are those of tests/so3_ref.py.  The prior sum itself is held to rel 1e-10 here, as
    tests/test_gpu_relpose.py::test_relpose_phases_over_the_angle_range holds the factor sum."""
    for fv in (10, 6):
        for kw in [{}] + ([dict(jacobian_mode=0)] if angle in so3.AT_SWITCHES else []):
            sc, f0, sets, fv, fconst, keep_gauge, fac = jc.sweep_case(angle, fv)
            h = _handle(fv, **kw)
            try:
                sets.set_on(h, keep_gauge)
                assert h.upload(f0, sc)
                so = _orc_scene(orc, sc)
                ok, nrm = orc.normalize(so)
                assert ok
                sn = jr.normalised(sets, nrm)
                r = (jr.residuals(sn, so)[0] + sn.sets[0]["mean"]).reshape(-1, 6)
                assert np.linalg.norm(r, axis=1).min() > 2e-3 and np.abs(np.linalg.norm(r[:, 3:], axis=1) - angle).max() < 1e-13
                want, got = jr.energy(sn, so), h.joint_pose_prior_error()
                out = _phases(orc, h, sc, f0, 1e-4, sets, keep_gauge, fv)
                assert h.jacobian_kernel() in ((0, 1) if kw else (1, 2, 3))
                Uo = out["ref"]["blocks"][2][:, 10 - fv:, 10 - fv:]
                dU = np.sqrt(np.abs(np.einsum("mii->mi", Uo)))
                print(f"angle {angle:.12g} fv {fv} {kw}: prior sum off by {abs(got - want) / want:.2e}, frame blocks by "
                      f"{sym_scaled_err(out['U'], Uo, dU):.2e} (scaled)")
                assert got == pytest.approx(want, rel=1e-10)
            finally:
                h.close()


def test_joint_pose_prior_residuals_over_the_angle_range():
    """the host getter at every angle of the sweep, one slot each, one upload: rotation rows within 1e-13 of the reference's on
    the downloaded scene (tests/test_so3_cpu.py derives the bound), translation rows within 1e-10 of the extent"""
    sc, f0, sets, angles = jc.residual_sweep()
    h = _handle(10)
    try:
        sets.set_on(h)
        assert h.upload(f0, sc)
        world = sc.copy()
        h.download(world)
        want = np.concatenate(jr.residuals(sets, world)).reshape(-1, 6)
        got = np.concatenate(h.joint_pose_prior_residuals()).reshape(-1, 6)
        mean = np.concatenate([s["mean"] for s in sets.sets]).reshape(-1, 6)
        assert got.shape == want.shape == (angles.size, 6)
        assert np.abs(np.linalg.norm(want[:, 3:] + mean[:, 3:], axis=1) - angles).max() < 1e-13
        for k, a in enumerate(angles):
            print(f"angle {a:.12g}: rotation rows off by {np.abs(got[k, 3:] - want[k, 3:]).max():.2e}")
        assert np.abs(got[:, :3] - want[:, :3]).max() < 1e-10 * jc.extent(sc)
        assert np.abs(got[:, 3:] - want[:, 3:]).max() < 1e-13
    finally:
        h.close()


def test_jointprior_at_exactly_pi():
    """jointprior_cases.pi_case: slots half a turn about a coordinate axis and about a seeded one.  The rounding of the
    normalisation lands on either side of pi, so only what both signs of the residual share is held: everything downloaded is
    finite, the solve succeeds, the residuals have the length pi, and the prior sum (rotation information a multiple of I, no
    coupling to it, a zero mean) is the yardstick's."""
    sc, f0, sets, fv, fconst, keep_gauge, fac = jc.pi_case()
    h = _handle(fv)
    try:
        sets.set_on(h, keep_gauge)
        assert h.upload(f0, sc)
        nsc = sc.copy()
        ok, nrm = sa.normalize_scene_inplace(nsc)
        assert ok
        sn = jr.normalised(sets, nrm)
        want, got = jr.energy(sn, nsc), h.joint_pose_prior_error()
        err = h.phase_error()[0]
        h.phase_derivatives()
        V, U, W, g = (h.buffer(b).copy() for b in (B.BUF_POINT_BLOCKS, B.BUF_FRAME_BLOCKS, B.BUF_POINT_FRAME, B.BUF_GRAD))
        h.phase_schur(1e-4)
        S, rhs = h.buffer(B.BUF_RCS).copy(), h.buffer(B.BUF_RCS_RHS).copy()
        assert _finite(V, U, W, g, S, rhs) and np.isfinite(err) and np.isfinite(got)
        assert h.phase_solve()
        h.phase_backsub(1e-4)
        assert _finite(h.buffer(B.BUF_CORRECTIONS))
        res = h.joint_pose_prior_residuals()[0].reshape(-1, 6)
        ang = np.linalg.norm(res[:, 3:], axis=1)
        print(f"half a turn: residual angles - pi {ang[:2] - np.pi}, prior sum {got:.17g}, yardstick {want:.17g}")
        assert _finite(res) and np.abs(ang[:2] - np.pi).max() < 1e-13 and abs(ang[2] - 0.05) < 1e-13
        assert np.abs(np.abs(res[0, 3:]) - [np.pi, 0, 0]).max() < 1e-13  # about the first axis of R^T Rbar = diag(1, -1, -1)
        assert got == pytest.approx(want, rel=1e-10) and err > got
    finally:
        h.close()


def test_jointprior_phases_fixed_intrinsics(orc):
    """six variables a frame: the pose part is the whole block (SRK_UGS(6))"""
    sc, f0, sets, fv, fconst, keep_gauge, fac = jc.case(jc.MODE_CASE + "_fixed_k")
    h = _handle(fv)
    try:
        sets.set_on(h)
        _phases(orc, h, sc, f0, 1e-4, sets, keep_gauge, fv)
    finally:
        h.close()


def test_jointprior_phases_f32_storage_and_fp32_schur(orc):
    """W stored as float: the tolerances of tests/test_gpu_relpose.py::test_relpose_phases_f32_storage_and_fp32_schur; and fp32
    Schur sums run to the end with the sets"""
    sc, f0, sets, fv, fconst, keep_gauge, fac = jc.case(jc.MODE_CASE)
    h = _handle(fv, storage_precision=True)
    orc.set_w_storage_f32(2)
    try:
        sets.set_on(h)
        _phases(orc, h, sc, f0, 1e-4, sets, keep_gauge, fv, w_tol=1.3e-7, s_tol=1e-9)
    finally:
        orc.set_w_storage_f32(0)
        h.close()
    runs = []
    for modes in (dict(schur_precision=True), {}):
        h = _handle(fv, **modes)
        try:
            sets.set_on(h)
            runs.append(_run(h, sc, f0, 1e-10, 1e6, 6))
        finally:
            h.close()
    assert runs[0][1].iterations == runs[1][1].iterations and runs[0][1].err_final == pytest.approx(runs[1][1].err_final, rel=1e-5)


def test_jointprior_phases_huber_loss_and_information(orc):
    """no robust loss and no information acts on a prior: the energy is the weighted observation energy plus the plain sum"""
    sc, f0, sets, fv, fconst, keep_gauge, fac = jc.case(jc.MODE_CASE)
    q = cc.information(sc)
    h = _handle(fv)
    try:
        sets.set_on(h)
        h.set_robust_loss("huber", 1.0)
        h.set_observation_information(q)
        _phases(orc, h, sc, f0, 1e-4, sets, keep_gauge, fv,
                derivatives=lambda so: wr.derivatives(f0, so, q, wr.HUBER, 1.0), energy=lambda so: wr.energy(f0, so, q, wr.HUBER, 1.0))
    finally:
        h.close()


def test_jointprior_phases_with_position_priors(orc):
    sc, f0, sets, fv, fconst, keep_gauge, fac = jc.case(jc.MODE_CASE)
    pri = pc.priors_for(sc, cc._every(sc.N, 7), [3, 12])
    h = _handle(fv)
    try:
        sets.set_on(h)
        pri.set_on(h, 1)
        out = _phases(orc, h, sc, f0, 1e-4, sets, keep_gauge, fv, pri_w=pri)
        ep, ef = h.prior_error()
        assert ep > 0 and ef > 0 and h.joint_pose_prior_error() > 0
        assert out["err"] > ep + ef + h.joint_pose_prior_error()
    finally:
        h.close()


# ------------------------------------------------------------------ reordered frames, chunked solve

def _shuffled(sets, perm):
    out = []
    for s in sets.sets:
        fr = perm[s["frames"]]
        o = np.argsort(fr)
        i6 = (6 * o[:, None] + np.arange(6)[None, :]).reshape(-1)
        out.append(dict(frames=fr[o], R=s["R"][o], C=s["C"][o], mean=s["mean"][i6], info=s["info"][np.ix_(i6, i6)]))
    return jr.Sets(out)


def test_jointprior_shuffled_frames_take_the_reordering_and_agree(orc):
    """a shuffled-frame scene with set_frame_reordering(1): the slots go through the renumbering, which swaps the internal
    order of some coupled pairs (the transposed block).  Phase by phase against the yardstick on the shuffled scene, and the LM
    run against the run of the unshuffled scene (1e-7, as tests/test_gpu_relpose.py)."""
    sc, f0, sets, fv, fconst, keep_gauge, fac = jc.case(jc.REORDER_CASE)
    perm = np.concatenate([[0, 1], 2 + np.random.RandomState(0).permutation(sc.M - 2)])  # the gauge frames stay 0 and 1
    sh = sa.renumber_frames(sc, perm)
    ssh = _shuffled(sets, perm)
    assert jr.energy(ssh, sh) == pytest.approx(jr.energy(sets, sc), rel=1e-12)
    h = _handle(fv)
    try:
        sets.set_on(h)
        base = _run(h, sc, f0, 1e-10, 1e6, 8)
        h.set_frame_reordering(1)
        ssh.set_on(h)
        _phases(orc, h, sh, f0, 1e-4, ssh, keep_gauge, fv)
        order = h.frame_order()
        assert order is not None  # renumbered internally
        pairs = np.array(jr.frame_pairs(ssh))
        ia, ib = np.asarray(order)[pairs[:, 0]], np.asarray(order)[pairs[:, 1]]
        assert np.any(ia > ib)  # the internal order swaps a pair given as (lo, hi)
        ok, rep, sg, log = _run(h, sh, f0, 1e-10, 1e6, 8)
        back = sa.Scene(sg.points, sg.cam_R[perm], sg.cam_T[perm], sc.K, sc.shared_k, sc.row_ptr, sc.obs_frame, sc.obs_uv)
        _compare_runs(base, (ok, rep, back, log))
    finally:
        h.close()


def test_chunked_w8_m70_with_a_set_inside_the_band_and_one_beyond_it():
    """w8_m70 cut into chunks (band of 8 frames): a set inside the band leaves the plan alone; a set beyond it ({3, 40, 41})
    changes the plan.  The corrections agree across rcs modes to 1e-9 and with numpy on the downloaded system, as
    tests/test_gpu_relpose.py::test_chunked_scene_with_factors compares."""
    sc, f0 = jc.w8_m70()
    c = 1e-3
    for frames in ([30, 31, 33, 36], [3, 40, 41]):
        sets = jr.Sets([jc.set_for(sc, frames)])
        h = _handle(10)
        sols = {}
        try:
            assert h.upload(f0, sc)
            fill0, chunks0 = h.rcs_fill(), h.rcs_chunks()
            sets.set_on(h)
            for mode in (2, 1, 0):
                h.set_rcs_mode(mode)
                assert h.upload(f0, sc)
                if mode == 2:
                    print(f"{frames}: chunks {chunks0} -> {h.rcs_chunks()}, fill {fill0:.4f} -> {h.rcs_fill():.4f}, renumbered {h.frame_order() is not None}")
                    if frames[0] == 30:
                        assert h.rcs_fill() == fill0 and h.rcs_chunks() == chunks0
                h.phase_derivatives()
                h.phase_schur(c)
                if mode == 2:
                    S = h.buffer(B.BUF_RCS).reshape(10 * sc.M, 10 * sc.M)
                    rhs = h.buffer(B.BUF_RCS_RHS)
                assert h.phase_solve()
                h.phase_backsub(c)
                sols[mode] = h.buffer(B.BUF_CORRECTIONS)
            a, b = frames[-1], frames[0]
            assert np.abs(S[10 * a + 4:10 * a + 10, 10 * b + 4:10 * b + 10]).max() > 0
            x = np.linalg.solve(S, rhs)
            for _ in range(3):
                x = x + np.linalg.solve(S, rhs - S @ x)
            assert rel_err(sols[2][3 * sc.N:], x) < 1e-9
            assert rel_err(sols[2], sols[1]) < 1e-9 and rel_err(sols[2], sols[0]) < 1e-9
        finally:
            h.close()


# ------------------------------------------------------------------ marginalising landmarks into a prior

def _sub_scene(sc, keep):
    idx = np.flatnonzero(keep)
    rp = np.asarray(sc.row_ptr)
    obs = np.concatenate([np.arange(rp[i], rp[i + 1]) for i in idx])
    row_ptr = np.concatenate([[0], np.cumsum(rp[idx + 1] - rp[idx])]).astype(rp.dtype)
    return sa.Scene(sc.points[idx].copy(), sc.cam_R.copy(), sc.cam_T.copy(), sc.K, sc.shared_k, row_ptr,
                    np.ascontiguousarray(np.asarray(sc.obs_frame)[obs]), np.ascontiguousarray(np.asarray(sc.obs_uv)[obs]))


def test_marginalising_landmarks_into_a_prior_reproduces_the_system():
    """8 frames, calibrated, uploaded already normalised.  The landmarks are split into A (even) and B (odd).  The pose x pose
    part of A's reduced camera system at c = 0, halved (the system carries the factor 2), is the information matrix of one set
    over all 8 frames, linearised at the current poses with m = 0; with it B's reduced camera system equals the full scene's
    on the free variables, to the scaled 1e-10 of _phases (rhs excluded: the prior's gradient is zero, A's is not)."""
    spec = sa.SceneSpec(n_frames=8, grid_nx=10, grid_ny=8, vis_window=4, noise_uv_pix=0.3)
    sc = sa.generate_scene(spec)
    ok, _ = sa.normalize_scene_inplace(sc)
    assert ok
    even = np.arange(sc.N) % 2 == 0
    A, Bs = _sub_scene(sc, even), _sub_scene(sc, ~even)
    for part in (A, Bs):
        assert np.diff(part.row_ptr).min() >= 2 and np.unique(part.obs_frame).size == sc.M
    fv, M = 6, sc.M
    h = _handle(fv)
    try:
        def system(scene):
            assert h.upload(spec.f0, scene, already_normalized=True)
            h.phase_derivatives()
            U = h.buffer(B.BUF_FRAME_BLOCKS).reshape(M, fv, fv).copy()
            h.phase_schur(0.0)
            return h.buffer(B.BUF_RCS).reshape(fv * M, fv * M).copy(), U

        S_full, U_full = system(sc)
        S_A, _ = system(A)
        S_B, _ = system(Bs)
        fixed = kref.fixed_vars(M, np.zeros(M, dtype=bool), 1, fv)[kref.frame_var_index(M, fv)]
        free = ~fixed
        L = 0.5 * S_A
        assert np.array_equal(L, L.T)
        h.set_joint_pose_priors([jr.linearised_at(sc, np.arange(M), L)])
        S_Bp, _ = system(Bs)
        assert h.joint_pose_prior_error() < 1e-24
        dk = np.sqrt(np.abs(np.einsum("mii->mi", U_full))).reshape(-1)[free]
        err = sym_scaled_err(S_Bp[np.ix_(free, free)], S_full[np.ix_(free, free)], dk)
        gap = sym_scaled_err(S_B[np.ix_(free, free)], S_full[np.ix_(free, free)], dk)
        print(f"B with the prior vs the full scene: {err:.3e} (B alone: {gap:.3e})")
        assert gap > 1e-2 and err < 1e-10
    finally:
        h.close()


# ------------------------------------------------------------------ LM runs

def _same_as_yardstick(orc, gpu, sc, f0, sets, keep_gauge, fv, fconst, **kw):
    so = _orc_scene(orc, sc)
    rc_o, rep_o = jr.compute_inplace(orc, f0, so, sets, keep_gauge, fv, fconst=fconst, allowed_err_change=kw.get("allowed"),
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


@pytest.mark.parametrize("name", [jc.MODE_CASE, "gauge_frames_gauge_released"])
def test_jointprior_24_frames_ten_iterations_vs_python_lm_loop(orc, name):
    """attempt by attempt against the Python loop, with the reference's gauge and with the priors instead of it"""
    sc, f0, sets, fv, fconst, keep_gauge, fac = jc.case(name)
    assert sc.M == 24 and fac is None
    h = _handle(fv)
    try:
        sets.set_on(h, keep_gauge)
        _, rep, sg, _ = _same_as_yardstick(orc, h, sc, f0, sets, keep_gauge, fv, fconst, max_iterations=10)
        assert rep.iterations == 10
    finally:
        h.close()


# ------------------------------------------------------------------ the doubling identity

def test_doubling_identity_through_joint_covariance(orc):
    """calibrated w8_m70 at the scene the Python loop ends with; the prior built by joint_pose_prior_from_covariance from
    joint_covariance of DOUBLING_FRAMES (tests/test_jointprior_cpu.py says why {2..7} and not {58..63}).  The GPU's joint
    covariance with the prior agrees with the yardstick's at the bound tests/test_gpu_cross_covariance.py uses for
    joint_covariance (64 eps cond, every entry on the scale of its two marginal sigmas), and with Sigma / 2 within 4 d_ref plus
    that bound, relative to the largest entry of Sigma as d_ref is; in the normalised scene's variables."""
    r = doubling_reference(orc)
    assert r["d_ref"] < 1e-8, r["d_ref"]
    sc, f0, spx = r["scene"], r["f0"], 0.6
    k = 2.0 * (spx / f0) ** 2
    h = _handle(6)
    try:
        assert h.upload(f0, sc)
        h.phase_derivatives()
        g0 = h.buffer(B.BUF_GRAD).copy()
        Sw = h.joint_covariance(DOUBLING_FRAMES, [], sigma_pixels=spx)
        Sn = h.joint_covariance(DOUBLING_FRAMES, [], sigma_pixels=spx, caller_coordinates=False)
        st = B.joint_pose_prior_from_covariance(DOUBLING_FRAMES, sc, Sw, 6, spx, f0)
        h.set_joint_pose_priors([st])
        assert h.upload(f0, sc)
        # (the residual is the rounding of R R^T, of order 1e-16, against an information matrix of order 1 / Sigma: the energy and
        # the gradient change are printed; test_zero_residual_sets_leave_gradient_and_error_unchanged holds their bounds)
        h.phase_derivatives()
        g1 = h.buffer(B.BUF_GRAD)
        print(f"\nprior sum {h.joint_pose_prior_error():.3e}, gradient moved by {np.abs(g1 - g0).max():.3e} of {np.abs(g0).max():.3e}, "
              f"largest entry of L {np.abs(st['info']).max():.3e}")
        S2 =h.joint_covariance(DOUBLING_FRAMES, [], sigma_pixels=spx, caller_coordinates=False)
        tol = vc.bound(max(r["cond"], r["cond2"]))
        scaled = lambda a, b: float((np.abs(a - b) / np.sqrt(np.outer(np.diag(b), np.diag(b)))).max())  # noqa: E731 (covariance_ref.block_err's scale)
        d_y = scaled(S2 / k, r["Sigma2"])
        d_0 = scaled(Sn / k, r["Sigma"])
        d_half = float(np.abs(S2 - 0.5 * Sn).max() / np.abs(Sn).max())
        print(f"d_ref {r['d_ref']:.3e}; GPU vs yardstick without the prior {d_0:.3e}, with it {d_y:.3e}; GPU vs its own Sigma / 2 {d_half:.3e}; "
              f"bound {tol:.3e}")
        assert d_0 < tol and d_y < tol
        assert d_half < 4 * r["d_ref"] + tol
    finally:
        h.close()


# ------------------------------------------------------------------ zero residual, determinism, switched-off sets

def test_zero_residual_sets_leave_gradient_and_error_unchanged():
    sc, f0, sets, fv, fconst, keep_gauge, fac = jc.case(jc.MODE_CASE)
    zero = jr.Sets([jr.linearised_at(sc, s["frames"], s["info"]) for s in sets.sets])
    h = _handle(fv)
    try:
        assert h.upload(f0, sc)
        e0 = h.phase_error()[0]
        h.phase_derivatives()
        g0, U0 = h.buffer(B.BUF_GRAD).copy(), h.buffer(B.BUF_FRAME_BLOCKS).copy()
        zero.set_on(h)
        assert h.upload(f0, sc)
        e1, ep = h.phase_error()[0], h.joint_pose_prior_error()
        h.phase_derivatives()
        g1, U1 = h.buffer(B.BUF_GRAD), h.buffer(B.BUF_FRAME_BLOCKS)
        h.phase_schur(1e-4)
        S = h.buffer(B.BUF_RCS)
        print(f"prior sum {ep:.3e}, error {e0:.17g} -> {e1:.17g}, gradient moved by {np.abs(g1 - g0).max():.3e} of {np.abs(g0).max():.3e}")
        assert np.all(np.isfinite(g1)) and np.all(np.isfinite(U1)) and np.all(np.isfinite(S))
        assert ep < 1e-24 and e1 == pytest.approx(e0, rel=1e-14)
        assert np.abs(g1 - g0).max() < 1e-12 * np.abs(g0).max()
        assert np.abs(U1 - U0).max() > 1.0
        assert max(np.abs(r).max() for r in h.joint_pose_prior_residuals()) < 1e-12
    finally:
        h.close()


def _same_bits(a, b):
    (ok_a, rep_a, sg_a, log_a), (ok_b, rep_b, sg_b, log_b) = a, b
    assert rep_a.iterations > 0 and (ok_a, rep_a.iterations, rep_a.attempts, rep_a.status) == (ok_b, rep_b.iterations, rep_b.attempts, rep_b.status)
    assert (rep_a.err_initial, rep_a.err_final) == (rep_b.err_initial, rep_b.err_final)
    assert np.array_equal(log_a["attempts"], log_b["attempts"]) and np.array_equal(log_a["err"], log_b["err"])
    for x in ("points", "cam_R", "cam_T"):
        assert np.array_equal(getattr(sg_a, x), getattr(sg_b, x)), x


def test_deterministic_mode_gives_identical_bits_with_sets():
    sc, f0, sets, fv, fconst, keep_gauge, fac = jc.case("sixteen_frames_the_limit")
    runs = []
    for _ in range(2):
        h = _handle(fv, deterministic=True)
        try:
            sets.set_on(h)
            runs.append(_run(h, sc, f0, None, None, 6))
            assert h.deterministic() and h.joint_pose_prior_error() > 0
        finally:
            h.close()
    _same_bits(*runs)


def test_all_zero_information_gives_the_bits_of_the_run_without_that_set():
    """an all-zero information matrix is a valid, switched-off set: plan and run equal, bit for bit, those of the setting
    without it, even where its pairs would widen the skyline (deterministic mode)"""
    sc, f0, sets, fv, fconst, keep_gauge, fac = jc.case(jc.MODE_CASE)
    off = jc.set_for(sc, [2, 13, 22], seed=61)
    off["info"] = np.zeros((18, 18))
    more = jr.Sets(sets.sets + [off])
    runs, fills = [], []
    for s in (sets, more):
        h = _handle(fv, deterministic=True)
        try:
            s.set_on(h)
            runs.append(_run(h, sc, f0, None, None, 4))
            fills.append(h.rcs_fill())
            if s is more:
                assert len(h.joint_pose_priors()[0]) == sets.n + 1
                res = h.joint_pose_prior_residuals()  # the switched-off set still reports its residuals
                assert len(res) == sets.n + 1 and np.all(res[-1] != 0)
        finally:
            h.close()
    assert fills[0] == fills[1]
    _same_bits(*runs)


def test_default_is_bitwise_unchanged_after_toggling():
    """Set sets (one reaching across the scene, so that the skyline and the plans change), run, clear, run again: the second
    run equals a fresh handle's run bit for bit, fill and chunks included (deterministic mode on both handles)"""
    sc, f0 = cc.scene("nf16_10_tiles")
    fresh = sa.BundleAdjustmentKanatani(0)
    toggled = sa.BundleAdjustmentKanatani(0)
    try:
        for h in (fresh, toggled):
            h.set_deterministic(True)
        jr.Sets([jc.set_for(sc, [0, 11, sc.M - 1]), jc.set_for(sc, range(4, 10), seed=3)]).set_on(toggled)
        ok, rep, sg, _ = _run(toggled, sc, f0, None, None, 6)
        assert rep.iterations > 0 and toggled.joint_pose_prior_error() > 0
        toggled.set_joint_pose_priors(None)
        assert toggled.joint_pose_priors() is None
        runs = [_run(h, sc, f0, None, None, 12) for h in (fresh, toggled)]
        assert fresh.deterministic() and toggled.deterministic() and toggled.joint_pose_prior_error() == 0.0
        assert fresh.rcs_fill() == toggled.rcs_fill() and fresh.rcs_chunks() == toggled.rcs_chunks()
        _same_bits(*runs)
    finally:
        fresh.close()
        toggled.close()


# ------------------------------------------------------------------ getters

def test_getters_error_and_residuals_in_the_callers_units(orc):
    """joint_pose_prior_error() equals the yardstick's sum (rel 1e-12) on the library's own normalised sets, phase_error the
    observation energy plus it, and joint_pose_prior_residuals() the yardstick's r - m of the downloaded scene in the caller's
    coordinates (1e-10 of the extent), on a scene uploaded un-normalised with a rotated frame 0 and s = 2.5, before and after
    an optimisation"""
    sc, f0 = cc.scene("nf2_short_runs")
    sc = pc.rotated(sc)
    sets = jr.Sets([jc.set_for(sc, [0, 1, 2], mean=True), jc.set_for(sc, [2, 4], seed=3), jc.set_for(sc, [5], seed=7)])
    h = _handle(10)
    try:
        sets.set_on(h)
        got, kg = h.joint_pose_priors()
        assert kg is True
        for a, b in zip(got, sets.sets):
            for key in ("frames", "R", "C", "mean", "info"):
                assert np.array_equal(a[key], b[key]), key
        assert h.upload(f0, sc)
        nsc = sc.copy()
        ok, nrm = sa.normalize_scene_inplace(nsc)
        assert ok
        sn = jr.Sets(B.normalize_joint_pose_priors(nrm, sets.sets))
        so = _orc_scene(orc, nsc)
        extent = jc.extent(sc)
        for stage in ("uploaded", "optimised"):
            if stage == "optimised":
                crit = sa.BundleAdjustmentKanataniTermCriteria()
                crit.AllowedReprojErrRelativeChange(None)
                crit.MaxHessianFactor(None)
                h.optimize(crit, 3)
            got_sc = sc.copy()
            h.download(got_sc, revert_normalization=False)
            so.points[:], so.cam_R[:], so.cam_T[:] = got_sc.points, got_sc.cam_R, got_sc.cam_T
            want = jr.energy(sn, so)
            e = h.joint_pose_prior_error()
            print(f"{stage}: prior sum {e:.17g}, yardstick {want:.17g}")
            assert e == pytest.approx(want, rel=1e-12)
            assert h.phase_error()[0] == pytest.approx(orc.reproj_error(f0, so)[0] + want, rel=1e-10)
            world = sc.copy()
            h.download(world)
            res = h.joint_pose_prior_residuals()
            for r, w in zip(res, jr.residuals(sets, world)):
                r, w = r.reshape(-1, 6), w.reshape(-1, 6)
                assert np.abs(r[:, :3] - w[:, :3]).max() < 1e-10 * extent and np.abs(r[:, 3:] - w[:, 3:]).max() < 1e-10
                assert np.abs(r[:, :3]).max() > 1e-5 * extent and np.abs(r[:, 3:]).max() > 1e-5
            # the energy is invariant under the normalisation: the caller's residuals against the caller's information
            assert sum(float(r @ s["info"] @ r) for r, s in zip(res, sets.sets)) == pytest.approx(e, rel=1e-8)
        # SRK_E_STATE: the stored setting changed after the upload
        s2 = sets.copy()
        s2.sets[0]["C"][0] += 1e-3
        s2.set_on(h)
        with pytest.raises(Exception):
            h.joint_pose_prior_residuals()
        assert "changed after the upload" in h.last_error()
        assert h.joint_pose_prior_error() == pytest.approx(e, rel=1e-12)  # still the resident scene's lists
        assert h.upload(f0, sc)
        assert len(h.joint_pose_prior_residuals()) == sets.n
        h.set_profile(1)
        h.phase_derivatives(); h.phase_schur(1e-4); h.phase_error()
        ms = h.joint_pose_prior_pass_ms()
        print("pass ms", ms)
        assert all(0 < m < 5 for m in ms)
    finally:
        h.close()


# ------------------------------------------------------------------ state and refusals

SMALL = sa.SceneSpec(n_frames=6, grid_nx=5, grid_ny=4, vis_window=3)


def _small_sets(sc):
    return jr.Sets([jc.set_for(sc, [0, 1, 2]), jc.set_for(sc, [2, 4, 5], seed=3)])


def test_unsupported_combinations_are_refused_in_either_order_and_the_handle_stays_usable():
    sc = sa.generate_scene(SMALL)
    sets = _small_sets(sc)
    hook = _lib.ALLREDUCE_FN(lambda *a: 0)
    h = sa.BundleAdjustmentKanatani(0)
    try:
        sets.set_on(h)
        with pytest.raises(ValueError):
            h.set_intrinsic_groups(np.zeros(sc.M, np.int32))
        assert "joint pose priors" in h.last_error() and h.intrinsic_groups() == 0
        ok, rep, sg, _ = _run(h, sc, 600.0, 1e-10, 1e6, 3)
        assert rep.iterations > 0 and h.joint_pose_prior_error() > 0
    finally:
        h.close()
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_intrinsic_groups(np.zeros(sc.M, np.int32))
        with pytest.raises(ValueError):
            sets.set_on(h)
        assert "intrinsic groups" in h.last_error() and h.joint_pose_priors() is None and h.intrinsic_groups() == 1
        h.set_intrinsic_groups(None)
        sets.set_on(h)  # fine once the groups are gone
        ok, rep, sg, _ = _run(h, sc, 600.0, 1e-10, 1e6, 3)
        assert rep.iterations > 0 and h.joint_pose_prior_error() > 0
    finally:
        h.close()
    h = sa.BundleAdjustmentKanatani(0)
    try:
        sets.set_on(h)
        with pytest.raises(ValueError):
            h.set_allreduce(hook, 0, 2)
        assert "more than one rank" in h.last_error()
    finally:
        h.close()
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_allreduce(hook, 0, 2)
        with pytest.raises(ValueError):
            sets.set_on(h)
        assert "more than one rank" in h.last_error() and h.joint_pose_priors() is None
    finally:
        h.close()


def test_bad_arguments_leave_the_previous_setting_in_force():
    sc = sa.generate_scene(SMALL)
    sets = _small_sets(sc)
    h = sa.BundleAdjustmentKanatani(0)
    try:
        assert h.joint_pose_priors() is None
        sets.set_on(h)

        def with_(g, **kw):
            out = [dict(s) for s in sets.sets]
            out[g].update(kw)
            return out

        nan_C = sets.sets[0]["C"].copy()
        nan_C[1, 0] = np.nan
        asym = sets.sets[1]["info"].copy()
        asym[0, 9] *= 1.0 + 1e-6
        bad = {
            "size": [dict(frames=np.arange(17), R=np.tile(np.eye(3), (17, 1, 1)), C=np.zeros((17, 3)), info=np.eye(102))],
            "ascending": with_(1, frames=np.array([4, 2, 5])),
            "negative": with_(0, frames=np.array([-1, 1, 2])),
            "shared": with_(1, frames=np.array([1, 2, 5])),
            "rotation": with_(0, R=sets.sets[0]["R"] * (1.0 + 1e-6)),
            "information": with_(0, info=-np.eye(18)),
            "asymmetric": with_(1, info=asym),
            "nan": with_(0, C=nan_C),
        }
        for what, s in bad.items():
            with pytest.raises(ValueError):
                h.set_joint_pose_priors(s)
            assert "joint pose priors" in h.last_error(), what
            got, kg = h.joint_pose_priors()
            assert len(got) == 2 and all(np.array_equal(a[key], b[key]) for a, b in zip(got, sets.sets) for key in ("frames", "C", "info")), what
        with pytest.raises(ValueError):
            h._raise(h._lib.srk_ba_set_joint_pose_priors(B.C.c_void_p(h._h), B.C.c_int32(2), *[None] * 6, B.C.c_int(1)))
        with pytest.raises(ValueError):
            h.set_joint_pose_priors(sets.sets, keep_gauge=2)
        assert h.joint_pose_priors()[1] is True
        ok, rep, sg, _ = _run(h, sc, 600.0, 1e-10, 1e6, 3)
        assert rep.iterations > 0
    finally:
        h.close()


def test_index_beyond_the_scene_fails_the_upload_and_the_setting_survives_reset_and_compute_inplace():
    sc = sa.generate_scene(SMALL)
    other = sa.generate_scene(sa.SceneSpec(n_frames=4, grid_nx=3, grid_ny=3, vis_window=3))
    sets = _small_sets(sc)
    h = sa.BundleAdjustmentKanatani(0)
    try:
        sets.set_on(h)
        with pytest.raises(ValueError):
            h.upload(600.0, other)
        assert "joint pose priors" in h.last_error()
        with pytest.raises(ValueError):
            _run(h, other, 600.0, 1e-10, 1e6, 3)
        assert h.upload(600.0, sc)
        e0 = h.joint_pose_prior_error()
        assert e0 > 0
        h.reset()
        assert len(h.joint_pose_priors()[0]) == 2
        assert h.joint_pose_prior_error() == e0
        with_s = _run(h, sc, 600.0, 1e-10, 1e6, 5)  # re-applied by compute_inplace (an upload of its own)
        assert h.joint_pose_prior_error() > 0
        h.set_joint_pose_priors(None)
        assert h.joint_pose_priors() is None
        without = _run(h, sc, 600.0, 1e-10, 1e6, 5)
        assert h.joint_pose_prior_error() == 0.0
        assert np.abs(with_s[2].cam_T - without[2].cam_T).max() > 1e-6
        assert h.upload(600.0, other)  # and the other scene uploads again
    finally:
        h.close()


def test_cpp_adapter_set_joint_pose_priors(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "jointprior_adapter"
    r = subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "demos"),
                        os.path.join(HERE, "cpp", "test_jointprior_adapter.cpp"), "-o", str(exe),
                        "-L", os.path.join(ROOT, "surikatoko_amd"), "-lsrk_ba",
                        "-Wl,-rpath," + os.path.join(ROOT, "surikatoko_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "jointprior adapter ok" in r.stdout
