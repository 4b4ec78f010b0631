"""Marginal covariances on the GPU (srk_ba_phase_covariance / srk_ba_covariances) against the numpy reference of
tests/covariance_ref.py on the cases of tests/covariance_cases.py (each checked by tests/test_covariance_cpu.py).

Metric: per block max |a - b| / sqrt(ref_aa ref_bb).  Bound: 64 eps cond_scaled(S_free) -- a backward-stable factorisation is
off by a few eps cond of the diagonally scaled system, Cholesky is invariant under that scaling, and the reference's own two
summation orders differ by at most 4.6 eps cond (tests/test_covariance_cpu.py allows 16).  Rows and columns of fixed
variables and the blocks of constant landmarks are exact zeros, every block exactly symmetric.  The measured errors are in
DESIGN.md section 16."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import surikatoko_amd as sa
import covariance_cases as vc
import covariance_ref as vref
import prior_cases as pc
from gpu_common import handle as _handle

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

STAGED = [(n, c) for n in vc.CASES for c in vc.dampings(n)]


def _staged(gpu, k, c):
    gpu.phase_derivatives()
    gpu.phase_schur(c)
    return gpu.phase_covariance(k.frames, k.points)


def _check(FB, PB, ref, k, what):
    rf, rp = ref["FB"][k.frames], ref["PB"][k.points]
    ef, ep = vref.block_err(FB, rf), vref.block_err(PB, rp)  # (asserts the exact zeros of fixed variables)
    lim = vc.bound(ref["cond"])
    print(f"\n{what}: cond {ref['cond']:.3e}, frame blocks off by {ef:.3e}, landmark blocks by {ep:.3e} (bound {lim:.3e}; "
          f"{max(ef, ep) / (vref.EPS * ref['cond']):.2f} eps cond)")
    assert np.array_equal(FB, FB.transpose(0, 2, 1)) and np.array_equal(PB, PB.transpose(0, 2, 1))
    assert np.all(PB[k.pconst[k.points]] == 0)
    assert np.all(np.isfinite(FB)) and np.all(np.isfinite(PB))
    assert ef < lim and ep < lim


@pytest.mark.parametrize("name,c", STAGED)
def test_phase_covariance_vs_reference(orc, name, c):
    k = vc.case(name)
    ref = vc.reference(orc, name, c)
    h = _handle(k.fv)
    try:
        vc.configure(h, k)
        assert h.upload(k.f0, k.sc) and h.frame_vars() == k.fv
        if k.shuffle:
            assert h.frame_order() is not None  # renumbered internally
        FB, PB = _staged(h, k, c)
        _check(FB, PB, ref, k, f"{name} c={c:g}")
        # the system is consumed, and built again by the next phase_schur: the same answer
        FB2, PB2 = _staged(h, k, c)
        assert vref.block_err(FB2, FB) < vc.bound(ref["cond"]) and vref.block_err(PB2, PB) < vc.bound(ref["cond"])
    finally:
        h.close()


@pytest.mark.parametrize("name", ["ragged_every_frame_fv6", "w8_every_frame_fv6", "nf16_shuffled_fv6"])
def test_covariances_convenience_call_scaled_and_mapped(orc, name):
    """covariances() = the c = 0 blocks times 2 (sigma / f0)^2, mapped to the caller's coordinates: on the scene in a rotated,
    shifted and scaled world, so that the normalisation has R0 != I and s != 1"""
    k = vc.case(name)
    ref = vc.reference(orc, name, 0.0)
    rot = pc.rotated(k.sc)
    so = orc.Scene(rot.points, rot.cam_R, rot.cam_T, rot.K, rot.shared_k, rot.row_ptr, rot.obs_frame, rot.obs_uv)
    ok, nrm = orc.normalize(so)
    assert ok and abs(nrm.world_scale - 1) > 1e-3 and abs(nrm.R0[0] - 1) > 1e-3
    sigma = 0.7
    h = _handle(k.fv)
    try:
        vc.configure(h, k)
        assert h.upload(k.f0, rot)
        before = [b.copy() for b in (rot.points, rot.cam_R, rot.cam_T)]
        FBn, PBn = h.covariances(k.frames, k.points, sigma_pixels=sigma, caller_coordinates=False)
        sf, sp = vref.scaled(k.f0, sigma, ref["FB"], ref["PB"])
        _check(FBn, PBn, dict(FB=sf, PB=sp, cond=ref["cond"]), k, name + " normalised")
        FB, PB = h.covariances(k.frames, k.points, sigma_pixels=sigma)
        mf, mp = vref.revert(nrm, sf, sp)
        _check(FB, PB, dict(FB=mf, PB=mp, cond=ref["cond"]), k, name + " caller's coordinates")
        assert np.abs(FB - FBn).max() > 0  # the map did something
        # defaults: every frame, every landmark
        FA, PA = h.covariances(sigma_pixels=sigma)
        assert FA.shape == (k.sc.M, k.fv, k.fv) and PA.shape == (k.sc.N, 3, 3)
        assert vref.block_err(FA[k.frames], mf[k.frames]) < vc.bound(ref["cond"])
        assert vref.block_err(PA[k.points], mp[k.points]) < vc.bound(ref["cond"])
        assert all(np.array_equal(a, b) for a, b in zip(before, (rot.points, rot.cam_R, rot.cam_T)))
    finally:
        h.close()


def test_rcs_modes_and_batches_give_the_same_blocks(orc):
    """rcs modes 0 (dense), 1 (one chain) and 2 (chunks): the covariance call factorises slot 0's system with the single-chain
    solver whatever the mode, and a batch cap only changes which columns travel together"""
    name, c = "w8_every_frame_fv6", 1e-4
    k = vc.case(name)
    ref = vc.reference(orc, name, c)
    out = {}
    for mode, batch in ((2, 0), (1, 0), (0, 0), (2, 96), (1, 70)):
        h = _handle(k.fv)
        try:
            vc.configure(h, k)
            h.set_rcs_mode(mode)
            h.set_covariance_batch(batch)
            assert h.upload(k.f0, k.sc)
            out[(mode, batch)] = _staged(h, k, c)
            _check(*out[(mode, batch)], ref, k, f"rcs mode {mode}, batch {batch}")
        finally:
            h.close()
    # the skyline only skips exact zeros and a batch only regroups columns: modes 1 and 2 and every batch size agree to the bit
    # when the system itself has the same bits (deterministic mode pins that below); here to the bound
    for key, (FB, PB) in out.items():
        assert vref.block_err(FB, out[(2, 0)][0]) < vc.bound(ref["cond"])
        assert vref.block_err(PB, out[(2, 0)][1]) < vc.bound(ref["cond"])


def test_deterministic_mode_same_bits(orc):
    name, c = "nf16_edges_fv10", 1e-4
    k = vc.case(name)
    ref = vc.reference(orc, name, c)
    h = _handle(k.fv, deterministic=True)
    try:
        vc.configure(h, k)
        assert h.upload(k.f0, k.sc) and h.deterministic()
        a = _staged(h, k, c)
        b = _staged(h, k, c)
        _check(*a, ref, k, name + " deterministic")
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        h.set_covariance_batch(96)  # the same system in other batches: the same bits
        d = _staged(h, k, c)
        assert np.array_equal(a[0], d[0]) and np.array_equal(a[1], d[1])
    finally:
        h.close()


def test_f32_storage(orc):
    """f32 storage of the point-frame blocks: the right-hand sides of the landmarks are formed from the float factors; the
    blocks move by the storage's rounding (2^-24 relative in W) times the conditioning, as the step tests allow"""
    name, c = "nf16_edges_fv10", 1e-4
    k = vc.case(name)
    ref = vc.reference(orc, name, c)
    h = _handle(k.fv, storage_precision=True)
    try:
        vc.configure(h, k)
        assert h.upload(k.f0, k.sc)
        FB, PB = _staged(h, k, c)
        lim = 2.0 ** -23 * ref["cond"]
        ef, ep = vref.block_err(FB, ref["FB"][k.frames]), vref.block_err(PB, ref["PB"][k.points])
        print(f"\nf32 storage: frames {ef:.3e}, landmarks {ep:.3e} (bound {lim:.3e})")
        assert ef < lim and ep < lim and np.array_equal(PB, PB.transpose(0, 2, 1))
    finally:
        h.close()


def test_prior_tightens_a_landmark(orc):
    """a landmark with a prior: Sigma_prior - Sigma_X is positive semi-definite.  In the factor-2 convention the prior alone
    gives H = 2 L, so Sigma_prior = 2 (sigma / f0)^2 (2 L)^-1 = (sigma / f0)^2 L^-1, and H_ii >= 2 L bounds the block."""
    name = "nf16_priors_fv6"
    k = vc.case(name)
    h = _handle(k.fv)
    try:
        vc.configure(h, k)
        assert h.upload(k.f0, k.sc)
        sel = k.pri.pidx[:8]
        _, PB = h.covariances([], sel, sigma_pixels=1.0)
        for i, blk in zip(range(len(sel)), PB):
            prior_cov = np.linalg.inv(k.pri.pinfo[i]) / k.f0 ** 2
            gap = prior_cov - blk
            scale = np.sqrt(np.outer(np.diag(prior_cov), np.diag(prior_cov)))
            assert np.linalg.eigvalsh(0.5 * (gap + gap.T) / scale).min() > -1e-9
            assert np.linalg.eigvalsh(blk).min() > 0
        # and without the priors the same landmarks are less certain
        h2 = _handle(k.fv)
        try:
            assert h2.upload(k.f0, k.sc)
            _, P0 = h2.covariances([], sel, sigma_pixels=1.0)
        finally:
            h2.close()
        assert np.all(np.einsum("nii->n", P0) > np.einsum("nii->n", PB))
    finally:
        h.close()


def test_covariances_after_compute_inplace(orc):
    """after ComputeInplace the result is resident: covariances() answers for it and leaves the downloaded scene untouched"""
    k = vc.case("w8_every_frame_fv6")
    h = _handle(k.fv)
    try:
        crit = sa.BundleAdjustmentKanataniTermCriteria()
        crit.AllowedReprojErrRelativeChange(1e-10)
        crit.MaxHessianFactor(1e6)
        sg = k.sc.copy()
        h.ComputeInplace(k.f0, sg, crit, 20)  # (true or false: the reference's "optimised" verdict is not the point here)
        assert h.report.iterations >= 1 and h.OptimizationStatusString() != "device error"
        kept = [a.copy() for a in (sg.points, sg.cam_R, sg.cam_T)]
        FB, PB = h.covariances(k.frames, k.points, sigma_pixels=0.3)
        assert all(np.array_equal(a, b) for a, b in zip(kept, (sg.points, sg.cam_R, sg.cam_T)))
        # the reference at the optimised scene
        so = orc.Scene(sg.points, sg.cam_R, sg.cam_T, sg.K, sg.shared_k, sg.row_ptr, sg.obs_frame, sg.obs_uv)
        ok, nrm = orc.normalize(so)
        assert ok
        z = np.zeros(sg.M, dtype=bool), np.zeros(sg.N, dtype=bool)
        restricted = vref.blocks_of(orc, k.f0, so, k.fv, *z)
        rf, rp, cond = vref.covariance_blocks(so, restricted, 0.0, k.fv, *z, 1)
        mf, mp = vref.revert(nrm, *vref.scaled(k.f0, 0.3, rf, rp))
        _check(FB, PB, dict(FB=mf, PB=mp, cond=cond), k, "after ComputeInplace")
        # a second optimise call still works on the handle (the consumed system is rebuilt by the loop)
        assert h.optimize(crit, 2) in (True, False)
    finally:
        h.close()


def test_argument_and_state_errors():
    k = vc.case("nf2_all_fv6")
    h = _handle(k.fv)
    try:
        with pytest.raises(RuntimeError):
            h._raise(h._lib.srk_ba_phase_covariance(h._h, 0, None, None, 0, None, None))  # no scene
        assert h.upload(k.f0, k.sc)
        h.phase_derivatives()
        h.phase_schur(1e-4)
        for frames, points in (([k.sc.M], []), ([-1], []), ([], [k.sc.N]), ([], [-1])):
            with pytest.raises(ValueError):
                h.phase_covariance(frames, points)
            assert "out of range" in h.last_error()
        for s in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                h.covariances([0], [0], sigma_pixels=s)
        blk = np.zeros((1, 6, 6))
        assert h._lib.srk_ba_phase_covariance(h._h, 1, None, blk.ctypes.data, 0, None, None) == -1  # NULL with a positive count
        # the refused calls left the system alone
        FB, PB = h.phase_covariance([1], [0])
        assert FB[0, 0, 0] > 0 and PB[0, 0, 0] > 0
    finally:
        h.close()
    g = _handle(10)
    try:
        g.set_intrinsic_groups(np.zeros(k.sc.M, dtype=np.int32))
        assert g.upload(k.f0, k.sc)
        with pytest.raises(ValueError):
            g.covariances([0], [0])
        assert "intrinsic groups" in g.last_error()
    finally:
        g.close()


def test_ten_variables_undamped_reports_not_positive_definite_or_answers():
    """ten variables a frame on a planar grid scene: per-frame intrinsics are close to unobservable, the scaled condition
    number of the undamped system is 1e14; the call may return 1 (LinAlgError here) and must not return garbage"""
    k = vc.case("nf16_edges_fv10")
    h = _handle(10)
    try:
        assert h.upload(k.f0, k.sc)
        try:
            FB, PB = h.covariances(k.frames, k.points)
        except np.linalg.LinAlgError:
            return
        assert np.all(np.isfinite(FB)) and np.all(np.isfinite(PB))
        assert np.array_equal(FB, FB.transpose(0, 2, 1))
    finally:
        h.close()


def test_cpp_adapter_covariances(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "covariance_adapter"
    r = subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "demos"),
                        os.path.join(HERE, "cpp", "test_covariance_adapter.cpp"), "-o", str(exe),
                        "-L", os.path.join(ROOT, "surikatoko_amd"), "-lsrk_ba",
                        "-Wl,-rpath," + os.path.join(ROOT, "surikatoko_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "covariance adapter ok" in r.stdout
