"""Robust bundle adjustment (srk_ba_set_robust_loss) without a GPU: the yardstick of tests/robust_ref.py is checked against
the oracle (unit weights, plain LM loop), against finite differences of E, and against known answers of rho and w; the C ABI
entry points exist and refuse a null handle; the C++ adapter's extension compiles."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import _lib
import robust_ref as rr
from conftest import class_rel_err
from gpu_common import orc_scene as _oscene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(orc, ragged=False, outliers=False, **kw):
    spec = sa.SceneSpec(**({"n_frames": 8, "grid_nx": 6, "grid_ny": 5, "vis_window": 4, "noise_uv_pix": 0.5} | kw))
    sc = sa.generate_scene(spec)
    if ragged:
        sc = sa.drop_observations(sc, 0.2, seed=3)
    if outliers:
        rr.inject_outliers(sc, 0.1, 20, 60, seed=5)
    so = _oscene(orc, sc)
    assert orc.normalize(so)[0]
    return spec, so


def test_abi_exports_robust_entry_points_and_refuses_null():
    L = _lib.lib()
    for name in ("srk_ba_set_robust_loss", "srk_ba_robust_loss", "srk_ba_observation_weights"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    k, d = C.c_int(0), C.c_double(0)
    assert L.srk_ba_set_robust_loss(None, 1, 2.0) == -1  # SRK_E_ARGS
    assert L.srk_ba_robust_loss(None, C.byref(k), C.byref(d)) == -1
    w = np.zeros(4)
    assert L.srk_ba_observation_weights(None, w.ctypes.data_as(C.POINTER(C.c_double)), 4) < 0


def test_rho_and_weight_known_answers():
    d = 0.01
    # w(0) = 1, rho(0) = 0, rho(s) ~ s near 0
    for kind in (rr.HUBER, rr.CAUCHY):
        rho, w = rr.rho_w(np.array([0.0, 1e-12]), kind, d)
        assert w[0] == 1.0 and rho[0] == 0.0
        assert rho[1] == pytest.approx(1e-12, rel=1e-7)
    # Huber: exactly s and w = 1 up to d^2, continuous at s = d^2 (value and slope), 2 d sqrt(s) - d^2 above
    s = np.array([0.25 * d * d, d * d, d * d * (1 + 1e-12), 4 * d * d, 100 * d * d])
    rho, w = rr.rho_w(s, rr.HUBER, d)
    assert rho[0] == s[0] and rho[1] == s[1] and w[0] == 1.0 and w[1] == 1.0
    assert rho[2] == pytest.approx(s[2], rel=1e-11) and w[2] == pytest.approx(1.0, rel=1e-11)
    assert rho[3] == pytest.approx(2 * d * 2 * d - d * d) and w[3] == pytest.approx(0.5)
    assert rho[4] == pytest.approx(2 * d * 10 * d - d * d) and w[4] == pytest.approx(0.1)
    # Cauchy: d^2 log(1 + s / d^2), w = 1 / (1 + s / d^2)
    rho, w = rr.rho_w(np.array([d * d, 3 * d * d]), rr.CAUCHY, d)
    assert rho[0] == pytest.approx(d * d * np.log(2)) and w[0] == pytest.approx(0.5)
    assert rho[1] == pytest.approx(d * d * np.log(4)) and w[1] == pytest.approx(0.25)
    # w = rho'(s) by central differences
    for kind in (rr.HUBER, rr.CAUCHY):
        for s0 in (0.5 * d * d, 3 * d * d, 50 * d * d):
            h = 1e-6 * s0
            num = (rr.rho_w(s0 + h, kind, d)[0] - rr.rho_w(s0 - h, kind, d)[0]) / (2 * h)
            assert float(rr.rho_w(s0, kind, d)[1]) == pytest.approx(float(num), rel=1e-7)


@pytest.mark.parametrize("kw", [dict(), dict(ragged=True), dict(n_frames=12, grid_nx=5, grid_ny=4, vis_window=12)])
def test_unit_weight_blocks_are_the_oracle_derivatives(orc, kw):
    spec, so = _scene(orc, **kw)
    N = so.N
    g0, V0, U0, W0 = orc.derivatives(spec.f0, so)
    g, V, U, W, w = rr.derivatives(spec.f0, so)
    assert np.all(w == 1.0)
    assert class_rel_err(g[:3 * N].reshape(-1, 3), g0[:3 * N].reshape(-1, 3), (1,)) < 1e-12
    assert class_rel_err(g[3 * N:].reshape(-1, 10), g0[3 * N:].reshape(-1, 10), (1,)) < 1e-12
    assert class_rel_err(V, V0, (1, 2)) < 1e-12
    assert class_rel_err(U, U0, (1, 2)) < 1e-12
    assert class_rel_err(W, W0, (1, 2)) < 1e-12
    e, _ = orc.reproj_error(spec.f0, so)
    assert rr.energy(spec.f0, so) == pytest.approx(e, rel=1e-13)
    # Huber with delta above every residual: the same blocks exactly
    gh, Vh, Uh, Wh, wh = rr.derivatives(spec.f0, so, rr.HUBER, 1e6)
    assert np.all(wh == 1.0) and np.array_equal(gh, g) and np.array_equal(Uh, U) and np.array_equal(Wh, W)


@pytest.mark.parametrize("kind,delta", [(rr.NONE, None), (rr.HUBER, 1e6)])
def test_lm_loop_reproduces_the_oracle_without_a_loss(orc, kind, delta):
    spec = sa.SceneSpec(n_frames=8, grid_nx=6, grid_ny=5, vis_window=4, noise_uv_pix=0.5)
    sc = sa.generate_scene(spec)
    so = _oscene(orc, sc)
    rc, rep = rr.compute_inplace(orc, spec.f0, so, kind, delta, allowed_err_change=1e-12, max_hessian_factor=1e6,
                                 max_iterations=8)
    # the oracle's loop, stopped after every iteration: the error sequence and the attempts
    errs, atts = [], []
    for k in range(1, rep.iterations + 1):
        o2 = _oscene(orc, sc)
        rc2, rep2 = orc.compute_inplace(spec.f0, o2, 1e-12, 1e6, k)
        errs.append(rep2.err_final)
        atts.append(rep2.attempts)
    assert rep.iterations >= 3
    assert np.allclose(rep.errors, errs, rtol=1e-9, atol=0)
    assert list(np.cumsum(rep.attempts_per_iteration)) == atts
    o2 = _oscene(orc, sc)
    rc2, rep2, log2 = orc.compute_inplace(spec.f0, o2, 1e-12, 1e6, 8, want_log=True)
    assert (rc, rep.iterations, rep.attempts, rep.status) == (rc2, rep2.iterations, rep2.attempts, rep2.status)
    assert np.abs(so.points - o2.points).max() < 1e-8 and np.abs(so.cam_T - o2.cam_T).max() < 1e-8
    # attempt by attempt: the same decisions and damping factors, the accepted errors as above (a rejected step is longer
    # and its error less close: 1.5e-9 measured)
    for k in ("iteration", "factor", "outcome"):
        assert np.array_equal(rep.log[k], log2[k]), k
    acc = log2["outcome"] == 1
    assert np.allclose(rep.log["err_trial"][acc], log2["err_trial"][acc], rtol=1e-9, atol=0)
    assert np.allclose(rep.log["err_value"], log2["err_value"], rtol=1e-9, atol=0)
    assert np.allclose(rep.log["err_trial"], log2["err_trial"], rtol=1e-8, atol=0)


@pytest.mark.parametrize("kind", [rr.HUBER, rr.CAUCHY])
def test_weighted_gradient_is_the_gradient_of_E(orc, kind):
    # f0 = 1: there the reference's frame closed forms are the derivatives of the error (tests/test_oracle_fd_checkers.py)
    spec = sa.SceneSpec(n_frames=6, grid_nx=5, grid_ny=4, vis_window=4, f0=1.0)
    sc = sa.generate_scene(spec)
    so = _oscene(orc, sc)
    ex, ey = rr.residuals(1.0, so)
    res = np.sqrt(ex * ex + ey * ey)
    # about half of the observations beyond the threshold, none near it (a central difference across Huber's kink, where the
    # second derivative jumps, is not the derivative): the threshold in the widest gap of the middle residuals
    r = np.sort(res)[len(res) // 4:3 * len(res) // 4]
    k = int(np.argmax(r[1:] / r[:-1]))
    delta = float(np.sqrt(r[k] * r[k + 1]))
    rr.inject_outliers(sc, 0.1, 20 * delta, 60 * delta, seed=5)
    so = _oscene(orc, sc)
    g, V, U, W, w = rr.derivatives(1.0, so, kind, delta)
    if kind == rr.HUBER:
        assert np.any(w == 1.0) and np.any(w < 0.2)  # both branches
    N, M = so.N, so.M
    E = lambda s2: rr.energy(1.0, s2, kind, delta)  # noqa: E731

    def fd(perturb, h):
        a, b = so.copy(), so.copy()
        perturb(a, -h)
        perturb(b, h)
        return (E(b) - E(a)) / (2 * h)

    for i in range(N):
        for v in range(3):
            def pp(s2, h, i=i, v=v):
                s2.points[i, v] += h
            assert g[3 * i + v] == pytest.approx(fd(pp, 1e-6), rel=1e-6, abs=1e-9 * np.abs(g[:3 * N]).max()), (i, v)
    for j in range(M):
        for v in range(10):
            def pf(s2, h, j=j, v=v):
                if v < 4:  # fx fy u0 v0: entries of the frame's K
                    s2.K[j, (0, 4, 2, 5)[v]] += h
                else:  # pose: the reference's own update (AddDeltaToFrameInplace)
                    c = np.zeros(3 * N + 10 * M)
                    c[3 * N + 10 * j + v] = h
                    orc.apply_corrections(s2, c)
            gf = g[3 * N + 10 * j + v]
            assert gf == pytest.approx(fd(pf, 1e-6), rel=1e-5, abs=1e-9 * np.abs(g[3 * N:]).max()), (j, v)


def test_fixed_intrinsics_step_uses_the_restricted_blocks(orc):
    spec, so = _scene(orc, outliers=True)
    out = rr.step(orc, spec.f0, so, 1e-3, rr.HUBER, 2.0, fv=6, want_system=True)
    assert out["ok"]
    assert np.all(out["corr10"][3 * so.N:].reshape(so.M, 10)[:, :4] == 0)
    assert out["S"].shape == (6 * so.M, 6 * so.M)


def test_adapter_header_with_set_robust_loss_compiles(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "t.cpp"
    src.write_text('#include "suriko_amd/bundle-adj-kanatani.hpp"\n'
                   "void f(suriko_amd::BundleAdjustmentKanatani& ba) { ba.SetRobustLoss(1, 2.0); ba.SetRobustLoss(0, 0); }\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
