"""Constant parameter blocks without a device: the yardstick of tests/constant_ref.py against the oracle where the two overlap,
the conditioning of every case the GPU tests compare, and the argument checks of the C ABI that need no GPU."""
import ctypes as C

import numpy as np
import pytest

import surikatoko_amd as sa
import calibrated_ref as cref
import constant_cases as cc
import constant_ref as kref
import weighted_ref as wr


def _orc_scene(orc, sc):
    so = orc.Scene(sc.points, sc.cam_R, sc.cam_T, sc.K, sc.shared_k, sc.row_ptr, sc.obs_frame, sc.obs_uv)
    assert orc.normalize(so)[0]
    return so


@pytest.mark.parametrize("c", [1e-4, 1e-1])
@pytest.mark.parametrize("name", ["nf2_short_runs", "nf16_10_tiles"])
def test_numpy_schur_path_equals_two_phase_for_the_empty_set_and_for_the_gauge(orc, name, c):
    """With an empty constant set the numpy route's system (all 10 M frame variables, nothing removed) holds orc.two_phase's
    system at the rows and columns the gauge leaves, to 1e-10 (symmetric-scaled), and with the fixed variables equal to the
    gauge its dense solve and back-substitution give orc.two_phase's corrections, to 1e-10"""
    sc, f0 = cc.scene(name)
    so = _orc_scene(orc, sc)
    N, M = so.N, so.M
    gradE, V, U, W = orc.derivatives(f0, so)
    ok_o, corr_o, S_o, rhs_o = orc.two_phase(so, gradE, V, U, W, c, want_system=True)
    assert ok_o
    red = cref.reduced_full_index(M)
    keep = red >= 0
    none = np.zeros(M, dtype=bool), np.zeros(N, dtype=bool)
    S, rhs, Einv = kref.schur(so, gradE, V, U, W, c)
    d = np.sqrt(np.diag(S_o))
    assert np.abs((S[np.ix_(keep, keep)] - S_o) / d[:, None] / d[None, :]).max() < 1e-10
    gs = 2.0 * np.sqrt(orc.reproj_error(f0, so)[0])
    assert np.abs((rhs[keep] - rhs_o) / (d * gs)).max() < 1e-10
    ok, corr = kref.solve(so, gradE, W, S, rhs, Einv, kref.gauge_vars(M))
    assert ok
    # the yardstick's keep_gauge = 1 route with nothing constant is two_phase itself
    res = kref.step_blocks(orc, so, (gradE, V, U, W), c, *none, keep_gauge=1, want_system=True)
    assert np.array_equal(res["corr"], corr_o) and np.array_equal(res["fixed"], kref.gauge_vars(M))
    # Corrections: the oracle's Householder QR on the unscaled system is itself off by d_solver (up to 2e-8 on these scenes at
    # c = 1e-4; tests/test_gpu_parity.py::_check), so both routes are held against the exact solution of the oracle's system:
    # the numpy route to 1e-10, and the two routes against each other to max(1e-10, 4 d_solver)
    print(f"{name} c={c:g}: oracle QR off by {res['d_solver']:.3e}, numpy route off by "
          f"{kref.rel_err(corr[3 * N:], res['dc_exact']):.3e}, routes differ by {kref.rel_err(corr, corr_o):.3e}")
    assert kref.rel_err(corr[3 * N:], res["dc_exact"]) < 1e-10
    assert kref.rel_err(corr, corr_o) < max(1e-10, 4 * res["d_solver"])


def _blocks(orc, sc, so, f0, weighted):
    if not weighted:
        return orc.derivatives(f0, so)
    return wr.derivatives(f0, so, cc.information(sc), wr.HUBER, 1.0)[:4]


@pytest.mark.parametrize("c", [1e-4, 1e-1])
@pytest.mark.parametrize("name", list(cc.CASES))
def test_every_gpu_case_is_positive_definite_and_well_conditioned(orc, name, c):
    """np.linalg.cholesky of the reference system's free part succeeds and its condition number after symmetric diagonal
    scaling is below 1e10, for every (scene, constant set, keep_gauge) the GPU tests use (the loss + information variant of
    the mode case included)"""
    sc, f0, fconst, pconst, keep_gauge, fv = cc.case(name)
    so = _orc_scene(orc, sc)
    for weighted in ((False, True) if name == cc.MODE_CASE else (False,)):
        g, V, U, W = kref.restrict(*_blocks(orc, sc, so, f0, weighted), so, fconst, pconst)
        if fv == 6:
            g, V, U, W = cref.restrict(g, V, U, W, so.N)
        if so.N * so.M > 100000:  # C1: the C oracle's system (keep_gauge = 1) instead of the numpy loop
            assert keep_gauge == 1
            _, _, Sr, _ = orc.two_phase(so, g, V, U, W, c, want_system=True)
            red = cref.reduced_full_index(so.M)
            S = np.zeros((10 * so.M, 10 * so.M))
            S[np.ix_(red >= 0, red >= 0)] = Sr
        else:
            S, _, _ = kref.schur(so, g, V, U, W, c)
        fixed = kref.fixed_vars(so.M, fconst, keep_gauge, fv)
        cond = kref.system_check(S, fixed, 1e10)
        print(f"{name} c={c:g}{' (loss + information)' if weighted else ''}: cond {cond:.3e}")
        # the damped point blocks of the free landmarks are invertible as well
        E = V[~pconst].copy()
        E[:, np.arange(3), np.arange(3)] *= 1 + c
        assert np.all(np.linalg.det(E) > 0), cond


@pytest.mark.parametrize("c", [1e-4, 1e-1])
@pytest.mark.parametrize("k22_f0,fv", [(False, 10), (True, 6)])
def test_sliding_window_cases_are_positive_definite_and_well_conditioned(orc, k22_f0, fv, c):
    """the same condition for the two sliding-window scenes of the GPU tests (first 8 of 24 frames constant, no gauge kept)"""
    spec, sc, _, _, _, fconst = cc.sliding_window(k22_f0)
    so = _orc_scene(orc, sc)
    pconst = np.zeros(so.N, dtype=bool)
    g, V, U, W = kref.restrict_all(so, orc.derivatives(spec.f0, so), fconst, pconst, fv)
    S, _, _ = kref.schur(so, g, V, U, W, c)
    cond = kref.system_check(S, kref.fixed_vars(so.M, fconst, 0, fv), 1e10)
    print(f"sliding window k22_f0={k22_f0} fv={fv} c={c:g}: cond {cond:.3e}")


def test_restrict_makes_constant_blocks_identity_and_zero(orc):
    sc, f0, fconst, pconst, _, _ = cc.case(cc.MODE_CASE)
    so = _orc_scene(orc, sc)
    g, V, U, W = kref.restrict(*orc.derivatives(f0, so), so, fconst, pconst)
    assert np.all(U[fconst] == np.eye(10)) and np.all(V[pconst] == np.eye(3))
    fr, pt = np.asarray(so.obs_frame), kref.obs_points(so)
    assert np.all(W[fconst[fr] | pconst[pt]] == 0) and np.any(W[~(fconst[fr] | pconst[pt])] != 0)
    assert np.all(g[3 * so.N:].reshape(-1, 10)[fconst] == 0) and np.all(g[:3 * so.N].reshape(-1, 3)[pconst] == 0)
    res = kref.step_blocks(orc, so, orc.derivatives(f0, so), 1e-4, fconst, pconst, 1)
    assert res["ok"]
    assert np.all(res["corr"][:3 * so.N].reshape(-1, 3)[pconst] == 0)
    assert np.all(res["corr"][3 * so.N:].reshape(-1, 10)[fconst] == 0)


# ------------------------------------------------------------------ C ABI without a device

def test_symbols_are_exported_and_null_handles_are_refused():
    L = sa.lib()
    for name in ("srk_ba_set_constant_blocks", "srk_ba_constant_blocks", "srk_ba_constant_counts", "srk_ba_constant_pass_ms"):
        assert hasattr(L, name), name
    flags = np.ones(3, dtype=np.uint8)
    p = flags.ctypes.data_as(C.c_void_p)
    assert L.srk_ba_set_constant_blocks(None, p, C.c_int32(3), None, C.c_int64(0), C.c_int(1)) == -1   # SRK_E_ARGS
    assert L.srk_ba_set_constant_blocks(None, None, C.c_int32(0), None, C.c_int64(0), C.c_int(1)) == -1
    kg = C.c_int(7)
    assert L.srk_ba_constant_blocks(None, None, None, C.byref(kg)) == -1 and kg.value == 7
    assert L.srk_ba_constant_counts(None, None, None) == -1
    assert L.srk_ba_constant_pass_ms(None, None, None) == -3                                           # SRK_E_STATE
