"""Per-observation information (srk_ba_set_observation_information) without a GPU: the yardstick of tests/weighted_ref.py
equals tests/robust_ref.py bit for bit at unit information, its weighted gradient is the gradient of the weighted energy
(central differences, step and tolerance of tests/test_robust_cpu.py), and a zero entry gives the blocks of the scene
without that observation; the C ABI entry points exist and refuse a null handle; the C++ adapter's extension compiles."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import _lib
import robust_ref as rr
import weighted_ref as wr
from gpu_common import orc_scene as _oscene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(ragged=False, **kw):
    spec = sa.SceneSpec(**({"n_frames": 8, "grid_nx": 6, "grid_ny": 5, "vis_window": 4, "noise_uv_pix": 0.5} | kw))
    sc = sa.generate_scene(spec)
    if ragged:
        sc = sa.drop_observations(sc, 0.2, seed=3)
    rr.inject_outliers(sc, 0.1, 20, 60, seed=5)
    return spec, sc


def test_abi_exports_information_entry_points_and_refuses_null():
    L = _lib.lib()
    for name in ("srk_ba_set_observation_information", "srk_ba_observation_information", "srk_ba_observation_residuals"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    q = np.ones(4)
    p = q.ctypes.data_as(C.POINTER(C.c_double))
    assert L.srk_ba_set_observation_information(None, p, 4) == -1  # SRK_E_ARGS
    assert L.srk_ba_observation_information(None, p, 4) == -1
    e = np.zeros(8)
    assert L.srk_ba_observation_residuals(None, e.ctypes.data_as(C.POINTER(C.c_double)), 4) < 0


@pytest.mark.parametrize("kind,delta", [(rr.NONE, None), (rr.HUBER, 2.0), (rr.CAUCHY, 2.0)])
@pytest.mark.parametrize("ragged", [False, True])
def test_unit_information_is_robust_ref_bit_for_bit(orc, kind, delta, ragged):
    spec, sc = _scene(ragged)
    so = _oscene(orc, sc)
    assert orc.normalize(so)[0]
    q = np.ones(so.O)
    assert wr.energy(spec.f0, so, q, kind, delta) == rr.energy(spec.f0, so, kind, delta)
    assert np.array_equal(wr.weights(spec.f0, so, q, kind, delta), rr.weights(spec.f0, so, kind, delta))
    for a, b in zip(wr.derivatives(spec.f0, so, q, kind, delta), rr.derivatives(spec.f0, so, kind, delta)):
        assert np.array_equal(a, b)
    for fv in (10, 6):
        a = wr.step(orc, spec.f0, so, 1e-3, q, kind, delta, fv=fv, want_system=True)
        b = rr.step(orc, spec.f0, so, 1e-3, kind, delta, fv=fv, want_system=True)
        assert a["ok"] and b["ok"] and sorted(a) == sorted(b)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    s1, s2 = _oscene(orc, sc), _oscene(orc, sc)
    r1 = wr.compute_inplace(orc, spec.f0, s1, q, kind, delta, 1e-12, 1e6, 4)
    r2 = rr.compute_inplace(orc, spec.f0, s2, kind, delta, 1e-12, 1e6, 4)
    assert r1[0] == r2[0] and r1[1].errors == r2[1].errors and r1[1].attempts_per_iteration == r2[1].attempts_per_iteration
    assert (r1[1].status, r1[1].iterations, r1[1].err_initial) == (r2[1].status, r2[1].iterations, r2[1].err_initial)
    for k in r1[1].log:
        assert np.array_equal(r1[1].log[k], r2[1].log[k], equal_nan=True), k
    for x in ("points", "cam_R", "cam_T"):
        assert np.array_equal(getattr(s1, x), getattr(s2, x)), x


@pytest.mark.parametrize("kind", [rr.NONE, rr.HUBER, rr.CAUCHY])
def test_weighted_gradient_is_the_gradient_of_the_weighted_energy(orc, kind):
    # f0 = 1: there the reference's frame closed forms are the derivatives of the error (tests/test_oracle_fd_checkers.py)
    spec = sa.SceneSpec(n_frames=6, grid_nx=5, grid_ny=4, vis_window=4, f0=1.0)
    sc = sa.generate_scene(spec)
    so = _oscene(orc, sc)
    q = wr.make_information(sc, seed=2)
    assert np.any(q == 0) and q[q > 0].min() >= 0.25 and q.max() <= 4.0
    ex, ey = rr.residuals(1.0, so)
    res = np.sqrt(q * (ex * ex + ey * ey))  # whitened
    # about half of the observations beyond the threshold, none near it (see tests/test_robust_cpu.py): the threshold in the
    # widest gap of the middle whitened residuals
    pos = np.sort(res[q > 0])
    r = pos[len(pos) // 4:3 * len(pos) // 4]
    k = int(np.argmax(r[1:] / r[:-1]))
    delta = float(np.sqrt(r[k] * r[k + 1]))
    rr.inject_outliers(sc, 0.1, 20 * delta, 60 * delta, seed=5)
    so = _oscene(orc, sc)
    g, V, U, W, w = wr.derivatives(1.0, so, q, kind, delta)
    if kind == rr.HUBER:
        assert np.any(w[q > 0] == 1.0) and np.any(w < 0.2)  # both branches
    N, M = so.N, so.M
    E = lambda s2: wr.energy(1.0, s2, q, kind, delta)  # noqa: E731

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


@pytest.mark.parametrize("kind,delta", [(rr.NONE, None), (rr.HUBER, 2.0), (rr.CAUCHY, 2.0)])
def test_zero_information_gives_the_blocks_of_the_scene_without_the_observation(orc, kind, delta):
    spec, sc = _scene(ragged=True)
    q = wr.make_information(sc, seed=4, zero_frac=0.1)
    drop = q == 0
    assert drop.sum() >= 3
    so = _oscene(orc, sc)
    sr = wr.remove_observations(sc, drop)
    assert int(sr.row_ptr[-1]) == so.O - drop.sum() and np.diff(sr.row_ptr).min() >= 2
    s2 = _oscene(orc, sr)
    g, V, U, W, w = wr.derivatives(spec.f0, so, q, kind, delta)
    g2, V2, U2, W2, w2 = wr.derivatives(spec.f0, s2, q[~drop], kind, delta)
    assert np.all(W[drop] == 0) and np.array_equal(W[~drop], W2) and np.array_equal(w[~drop], w2)
    # sums over a landmark's / a frame's observations: the zero terms only change the order of a few additions
    for a, b in ((g, g2), (V, V2), (U, U2)):
        assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max()
    assert wr.energy(spec.f0, so, q, kind, delta) == pytest.approx(wr.energy(spec.f0, s2, q[~drop], kind, delta), rel=1e-14)


def test_adapter_header_with_set_observation_information_compiles(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "t.cpp"
    src.write_text('#include "suriko_amd/bundle-adj-kanatani.hpp"\n'
                   "void f(suriko_amd::BundleAdjustmentKanatani& ba) { std::vector<suriko_amd::Scalar> q(3, 1); "
                   "ba.SetObservationInformation(q); ba.SetObservationInformation({}); auto e = ba.ObservationResiduals(); (void)e; }\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
