"""Marginalisation priors on the device (srk_ba_marginalization_prior) against tests/marginal_ref.py.

Every scene is normalised on the host and uploaded as it is, so the library's normalised variables are the yardstick's.  The
kernels are isolated through phase_marginalization (A0, b0 before the host's factor terms); the whole call through the reduced
scene with the returned prior set, against the full scene's Schur complement.
"""
import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import ba as B
from conftest import sym_scaled_err
import constant_ref as kref
import jointprior_ref as jr
import marginal_cases as mc
import marginal_ref as mr
import robust_ref as rob
from gpu_common import handle as _handle, run_lm as _run

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def _upload(h, sc, f0):
    assert h.upload(f0, sc, already_normalized=True)


def _vec_scaled_err(a, b, d, scale):
    d = np.where(d > 0, d, 1.0)
    return float((np.abs(a - b) / d).max() / max(scale, 1e-300)) if a.size else 0.0


def _check_kernels(h, case):
    """phase_marginalization's A0, b0 (and A1, b1) against the yardstick; returns both"""
    sc, f0 = case["scene"], case["f0"]
    ph = h.phase_marginalization(case["D"], case["P"])
    ref = mr.system(f0, sc, case["D"], case["P"], case.get("q"), case.get("kind", rob.NONE), case.get("delta"), case.get("pri"),
                    case.get("fac"), case.get("sets"))
    assert list(ph["kept"]) == list(ref["K"])
    assert ph["report"]["landmarks_skipped"] == ref["skipped"]
    assert ph["report"]["landmarks_used"] == int(ref["used"].sum())
    assert np.array_equal(ph["A0"], ph["A0"].T) and np.all(np.isfinite(ph["A0"])) and np.all(np.isfinite(ph["b0"]))
    for tag in ("0", "1"):
        A, b, Ar, br = ph["A" + tag], ph["b" + tag], ref["A" + tag], ref["b" + tag]
        # the scale of a variable: its own block before anything is eliminated, as the S comparisons of the other GPU tests scale;
        # the gradient's scale is d_i sqrt(E_F), since |b_i| <= sqrt(A_ii E_F)
        dk = np.sqrt(ref["U" + tag])
        err = sym_scaled_err(A, Ar, dk)
        eb = _vec_scaled_err(b, br, dk, np.sqrt(ref["E" + tag]))
        print(f"{case['name']} stage {tag}: slots {len(ref['slots'])}, |P| used {int(ref['used'].sum())}, A {err:.3e}, b {eb:.3e}")
        assert err < 1e-10 and eb < 1e-10
    return ph, ref


@pytest.mark.parametrize("name", mc.KERNEL_CASES)
def test_kernels_against_the_yardstick(name):
    case = mc.case(name)
    h = _handle(case["fv"], **case.get("modes", {}))
    try:
        mc.set_on(h, case)
        _upload(h, case["scene"], case["f0"])
        ph, ref = _check_kernels(h, case)
        assert len(ref["slots"]) == case["slots"] and int(ref["used"].sum()) == case["used"]
        assert ref["skipped"] == case.get("skipped", 0)
    finally:
        h.close()


def test_f32_storage_leaves_the_bits_unchanged():
    """the kernels read the scene, not W: the storage mode of the point-frame blocks changes no bit"""
    case = mc.case("w8_24_slots_67")
    out = []
    for f32 in (False, True):
        h = _handle(10, storage_precision=f32)
        try:
            _upload(h, case["scene"], case["f0"])
            h.phase_derivatives()
            out.append(h.phase_marginalization(case["D"], case["P"]))
        finally:
            h.close()
    assert np.array_equal(out[0]["A0"], out[1]["A0"]) and np.array_equal(out[0]["b0"], out[1]["b0"])
    ref = mr.system(case["f0"], case["scene"], case["D"], case["P"])
    assert sym_scaled_err(out[1]["A0"], ref["A0"], np.sqrt(ref["U0"])) < 1e-10


def test_landmarks_only_halves_experiment_through_the_new_call():
    """the experiment of test_marginalising_landmarks_into_a_prior_reproduces_the_system with one upload: D empty, P = the even
    landmarks; Lam equals half of A's reduced camera system on the pose rows, and with it as a set the odd landmarks' system is
    the full scene's"""
    spec = sa.SceneSpec(n_frames=8, grid_nx=10, grid_ny=8, vis_window=4, noise_uv_pix=0.3)
    sc = sa.generate_scene(spec)
    ok, _ = sa.normalize_scene_inplace(sc)
    assert ok
    even = np.arange(sc.N) % 2 == 0
    A_sc, B_sc = mc.sub_scene(sc, even), mc.sub_scene(sc, ~even)
    fv, M = 6, sc.M
    h = _handle(fv)
    try:
        def system(scene):
            _upload(h, scene, spec.f0)
            h.phase_derivatives()
            U = h.buffer(B.BUF_FRAME_BLOCKS).reshape(M, fv, fv).copy()
            h.phase_schur(0.0)
            return h.buffer(B.BUF_RCS).reshape(fv * M, fv * M).copy(), U

        S_full, U_full = system(sc)
        S_A, _ = system(A_sc)
        _upload(h, sc, spec.f0)
        prior = h.marginalization_prior([], np.flatnonzero(even))
        assert list(prior["frames"]) == list(range(M)) and prior["report"]["landmarks_used"] == int(even.sum())
        dk = np.sqrt(np.abs(np.einsum("mii->mi", U_full))).reshape(-1)
        # (the gauge variables' rows of S_A are identity rows, not information: the free rows and columns are compared)
        fixed = kref.fixed_vars(M, np.zeros(M, dtype=bool), 1, fv)[kref.frame_var_index(M, fv)]
        free = ~fixed
        err_A = sym_scaled_err(prior["info"][np.ix_(free, free)], 0.5 * S_A[np.ix_(free, free)], dk[free])
        h.set_joint_pose_priors([prior])
        S_Bp, _ = system(B_sc)
        h.set_joint_pose_priors(None)
        err = sym_scaled_err(S_Bp[np.ix_(free, free)], S_full[np.ix_(free, free)], dk[free])
        print(f"Lam vs 0.5 S_A: {err_A:.3e}; B with the prior vs the full scene: {err:.3e}")
        assert err_A < 1e-10 and err < 1e-10
    finally:
        h.close()


def _reduced(sc, D, P):
    """the scene without the frames D and the landmarks P, and the new index of every old frame (-1: dropped)"""
    keep_f = np.ones(sc.M, dtype=bool)
    keep_f[np.asarray(D, dtype=np.int64)] = False
    new = np.where(keep_f, np.cumsum(keep_f) - 1, -1)
    keep_p = np.ones(sc.N, dtype=bool)
    keep_p[np.asarray(P, dtype=np.int64)] = False
    sub = mc.sub_scene(sc, keep_p)
    assert np.all(new[np.asarray(sub.obs_frame)] >= 0)
    K = sc.K if sc.shared_k else sc.K[keep_f]
    return sa.Scene(sub.points, sc.cam_R[keep_f].copy(), sc.cam_T[keep_f].copy(), K, sc.shared_k, sub.row_ptr,
                    new[np.asarray(sub.obs_frame)].astype(np.int32), sub.obs_uv), new


def _renumbered(prior, new):
    out = dict(prior)
    out["frames"] = new[np.asarray(prior["frames"])].astype(np.int32)
    assert np.all(out["frames"] >= 0)
    return out


def _pose_system(h, sc, f0, fv=6):
    _upload(h, sc, f0)
    h.phase_derivatives()
    h.phase_schur(0.0)
    n = fv * sc.M
    return h.buffer(B.BUF_RCS).reshape(n, n).copy(), h.buffer(B.BUF_RCS_RHS)[:n].copy()


@pytest.mark.parametrize("name", mc.EQUIVALENCE_CASES)
def test_reduced_scene_with_the_prior_equals_the_full_schur_complement(name):
    """full scene: the yardstick's pose x pose system at c = 0 with D eliminated.  Reduced scene (D and P removed) with the
    returned set and the gauge released: the library's reduced camera system and right-hand side.  Equal on every kept frame's
    variables to 64 eps cond(A_DD), in the scaled measure; without the prior the gap is large."""
    case = mc.case(name)
    sc, f0, D, P = case["scene"], case["f0"], case["D"], case["P"]
    h = _handle(6)
    try:
        _upload(h, sc, f0)
        prior = h.marginalization_prior(D, P)
        red, new = _reduced(sc, D, P)
        h.set_joint_pose_priors([_renumbered(prior, new)], keep_gauge=False)
        S_red, r_red = _pose_system(h, red, f0)
        h.set_joint_pose_priors(None)
        S_gap, _ = _pose_system(h, red, f0)
    finally:
        h.close()
    S_ref, r_ref, cond = mc.full_schur_complement(f0, sc, D)
    dk = np.sqrt(np.diag(S_ref))
    bound = 64 * EPS * cond
    err = sym_scaled_err(S_red, S_ref, dk)
    eb = _vec_scaled_err(r_red, r_ref, dk, np.sqrt(2.0 * rob.energy(f0, sc)))
    gap = sym_scaled_err(S_gap, S_ref, dk)
    print(f"{name}: cond(A_DD) {cond:.3e}, bound {bound:.3e}, system {err:.3e}, gradient {eb:.3e}, gap without the prior {gap:.3e}, "
          f"defect of m {prior['report']['defect']:.3e}")
    assert gap > 1e-2
    assert err < bound and eb < bound


def test_chain_identity_absorbs_the_previous_prior():
    """marginalise frame 0, set the result on the reduced scene, marginalise frame 1 there without optimising: Lam and eta equal
    those of marginalising {0, 1} at once on the full scene (the set left by the first step is absorbed, mean included)"""
    case = mc.case("chain")
    sc, f0 = case["scene"], case["f0"]
    P0, P1 = case["P0"], case["P1"]
    h = _handle(6)
    try:
        _upload(h, sc, f0)
        both = h.marginalization_prior([0, 1], np.union1d(P0, P1))
        first = h.marginalization_prior([0], P0)
        red, new = _reduced(sc, [0], P0)
        newp = -np.ones(sc.N, dtype=np.int64)
        newp[np.setdiff1d(np.arange(sc.N), P0)] = np.arange(sc.N - len(P0))
        h.set_joint_pose_priors([_renumbered(first, new)], keep_gauge=False)
        _upload(h, red, f0)
        second = h.marginalization_prior([0], newp[P1])
        h.set_joint_pose_priors(None)
    finally:
        h.close()
    assert second["report"]["sets"] == 1
    assert list(second["frames"] + 1) == list(both["frames"])
    d_ref, cond = case["d_ref"], case["cond"]
    bound = 64 * EPS * cond
    assert d_ref < 0.1 * bound, (d_ref, bound)
    dk = np.sqrt(np.abs(np.diag(both["info"])))
    err = sym_scaled_err(second["info"], both["info"], dk)
    scale = np.sqrt(rob.energy(f0, sc))
    eb = _vec_scaled_err(second["eta"], both["eta"], dk, scale)
    print(f"chain identity: Lam {err:.3e}, eta {eb:.3e}, yardstick's own d_ref {d_ref:.3e}, bound {bound:.3e} (cond {cond:.3e})")
    assert err < bound and eb < bound


def test_two_calls_give_the_same_bits_with_either_mode():
    case = mc.case("w8_40_slots")
    out = []
    for det in (False, True):
        h = _handle(10, deterministic=det)
        try:
            _upload(h, case["scene"], case["f0"])
            for _ in range(2):
                out.append(h.phase_marginalization(case["D"], case["P"]))
        finally:
            h.close()
    for o in out[1:]:
        assert np.array_equal(o["A0"], out[0]["A0"]) and np.array_equal(o["b0"], out[0]["b0"])
        assert np.array_equal(o["A1"], out[0]["A1"]) and np.array_equal(o["b1"], out[0]["b1"])


def test_a_call_leaves_a_deterministic_lm_run_unchanged():
    case = mc.case("w12_drop0")
    sc, f0 = case["scene"], case["f0"]
    h = _handle(10, deterministic=True)
    try:
        a = _run(h, sc, f0, max_iterations=4)
        _upload(h, sc, f0)
        h.marginalization_prior(case["D"], case["P"])
        h.phase_marginalization(case["D"], case["P"])
        b = _run(h, sc, f0, max_iterations=4)
    finally:
        h.close()
    assert a[0] == b[0] and (a[1].iterations, a[1].attempts) == (b[1].iterations, b[1].attempts)
    assert a[1].err_final == b[1].err_final
    for x, y in ((a[2].points, b[2].points), (a[2].cam_R, b[2].cam_R), (a[2].cam_T, b[2].cam_T)):
        assert np.array_equal(x, y)
    assert list(a[3]["attempts"]) == list(b[3]["attempts"]) and np.array_equal(a[3]["err"], b[3]["err"])


def test_refusals_and_capacity():
    case = mc.case("w8_40_slots")
    sc, f0, D, P = case["scene"], case["f0"], case["D"], case["P"]
    h = _handle(6)
    try:
        _upload(h, sc, f0)
        for frames, points, text in (([], [], "both lists are empty"), ([3, 2], [], "ascending"), ([0], [], "is observed from the dropped frame"),
                                     ([sc.M], [], "beyond the scene"), ([], [sc.N], "beyond the scene"), ([], [4, 4], "ascending"),
                                     (list(range(9)), [], "at most 8 frames"), ([], np.arange(sc.N), "kept frames, at most 32")):
            with pytest.raises(ValueError, match=text):
                h.marginalization_plan(frames, points)
        with pytest.raises(ValueError, match="70 kept frames"):
            h.marginalization_plan([], np.arange(sc.N))
        # kept_cap too small: refused with nothing written
        import ctypes as C
        kept, _ = h.marginalization_plan(D, P)
        fr, pt = np.asarray(D, np.int32), np.asarray(P, np.int64)
        kb, info = -np.ones(len(kept), np.int32), np.full((6 * len(kept)) ** 2, 7.0)
        nk = C.c_int32(-5)
        rc = sa.lib().srk_ba_marginalization_prior(C.c_void_p(h._h), C.c_int32(len(fr)), B._p(fr), C.c_int64(len(pt)), B._p(pt),
                                                   C.c_int32(len(kept) - 1), B._p(kb), C.byref(nk), None, None, B._p(info), None, None, None)
        assert rc == -1 and "do not fit kept_cap" in h.last_error()
        assert np.all(kb == -1) and nk.value == -5 and np.all(info == 7.0)
        # a lone kept frame cannot fix a dropped frame's scale: not positive definite, nothing written
        lone = mc.case("lone_kept_frame")
        _upload(h, lone["scene"], lone["f0"])
        h.set_observation_information(lone["q"])
        with pytest.raises(np.linalg.LinAlgError):
            h.marginalization_prior(lone["D"], lone["P"])
        h.set_observation_information(None)
        h.set_constant_blocks(frames=[2], n_frames=sc.M, n_points=sc.N)
        _upload(h, sc, f0)
        with pytest.raises(ValueError, match="constant blocks"):
            h.marginalization_plan(D, P)
    finally:
        h.close()


def test_cpp_adapter_marginalization_prior(tmp_path):
    import os
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "marginal_adapter"
    r = subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(root, "include"), "-I", os.path.join(root, "demos"),
                        os.path.join(here, "cpp", "test_marginal_adapter.cpp"), "-o", str(exe),
                        "-L", os.path.join(root, "surikatoko_amd"), "-lsrk_ba",
                        "-Wl,-rpath," + os.path.join(root, "surikatoko_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "marginal adapter ok" in r.stdout


def test_end_to_end_window_slides_once(orc):
    """12 frames: optimise (two iterations, so that the reduced problem still has somewhere to go), marginalise frame 0 and its
    landmarks, upload the reduced scene with the prior and the gauge released, ten iterations attempt by attempt against the
    Python loop with the same set.  Both loops run with MaxHessianFactor 1e6: the set is gauge-free and the gauge released, and an
    LM loop that can accept no attempt raises the damping factor without end when nothing bounds it (the yardstick's own loop does
    not return from a start at the optimum)."""
    import lm_trajectory as lt
    from gpu_common import orc_scene
    case = mc.case("w12_drop0")
    sc, f0, D, P = case["scene"].copy(), case["f0"], case["D"], case["P"]
    h = _handle(6)
    try:
        _upload(h, sc, f0)
        crit = sa.BundleAdjustmentKanataniTermCriteria()
        crit.MaxHessianFactor(1e6)
        h.optimize(crit, 2)
        h.download(sc, revert_normalization=False)
        prior = h.marginalization_prior(D, P)
        red, new = _reduced(sc, D, P)
        st = _renumbered(prior, new)
        h.set_joint_pose_priors([st], keep_gauge=False)
        ok, rep, sg, log = _run(h, red, f0, max_factor=1e6, max_iterations=10)
        h.set_joint_pose_priors(None)
    finally:
        h.close()
    so = orc_scene(orc, red.copy())
    sets = jr.Sets([dict(frames=st["frames"], R=st["R"], C=st["C"], mean=st["mean"], info=st["info"])])
    rc_o, rep_o = jr.compute_inplace(orc, f0, so, sets, 0, 6, max_hessian_factor=1e6, max_iterations=10)
    assert ok == (rc_o == 0) and rep.status == rep_o.status
    assert (rep.iterations, rep.attempts) == (rep_o.iterations, rep_o.attempts)
    assert list(log["attempts"]) == rep_o.attempts_per_iteration[:rep.iterations]
    assert rep.err_initial == pytest.approx(rep_o.err_initial, rel=1e-8, abs=1e-18)
    assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-8, abs=1e-18)
    lt.assert_same_trajectory(log, rep_o.log, 1e-8, gpu_attempts=rep.attempts, err_abs=1e-18)
    assert np.abs(sg.points - so.points).max() < 1e-8
    assert np.abs(sg.cam_R - so.cam_R).max() < 1e-8
    assert np.abs(sg.cam_T - so.cam_T).max() < 1e-8
