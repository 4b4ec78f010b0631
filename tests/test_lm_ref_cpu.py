"""CPU only: the one Python LM loop (tests/lm_ref.py) is the C oracle's loop bit for bit, every yardstick's compute_inplace
around it reproduces the results recorded from the six separate loops it replaced, and robust_ref is weighted_ref at unit
information bit for bit.

tests/golden/lm_ref_parent.npz: the runs of PARENT_RUNS, recorded by running the functions of this table against the
yardstick modules of the commit before the loops were merged (its tests/ directory first on sys.path) and saving, per run,
the fields _record() lists."""
import numpy as np
import pytest

import surikatoko_amd as sa
from conftest import load_golden, rel_err
import calibrated_ref as cref
import constant_cases as cc
import constant_ref as kref
from gpu_common import orc_scene as _oscene
import lm_exit_cases as cases
import lm_ref
import lm_trajectory as lt
import prior_cases as pc
import prior_ref as pref
import robust_ref as rr
import shared_k_ref as skr
import weighted_ref as wr

SMALL_FUSED = sa.SceneSpec(n_frames=12, grid_nx=10, grid_ny=10, vis_window=5)
ALLOWED, CAP = 1e-12, 1e6


def _with_outliers(sc):
    sc = sc.copy()
    rr.inject_outliers(sc, 0.05, 20, 60, 7)
    return sc


# ------------------------------------------------------------------ 1. the shared loop is the oracle's loop

def _plain_loop(orc, f0, so, allowed, cap, max_it):
    """lm_ref.loop with the oracle's own pieces: ten variables a frame, nothing restricted"""
    rep = lm_ref.Report()
    ok, nrm = orc.normalize(so)
    assert ok
    rc = lm_ref.loop(rep, so, energy=lambda: orc.reproj_error(f0, so)[0], prepare=lambda: orc.derivatives(f0, so),
                     solve=lambda blocks, c: orc.two_phase(so, *blocks, c),
                     apply=lambda corr: orc.apply_corrections(so, corr),
                     allowed_err_change=allowed, max_hessian_factor=cap, max_iterations=max_it)
    orc.revert(so, nrm)
    return rc, rep


ORACLE_CASES = {name: (name,) + tuple(v[2:6]) for name, v in cases.CASES.items()}
# allowed_err_change above the initial error (1.3e-5): "abs err threshold" before the first iteration
ORACLE_CASES["abs_err_threshold"] = ("max_iterations", 1.0, 1e6, 8, "abs err threshold")


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_shared_loop_is_the_oracle_loop_bit_for_bit(orc, name):
    scene, allowed, cap, max_it, status = ORACLE_CASES[name]
    f0 = cases.CASES[scene][0].f0
    sc = cases.scene(scene)
    so_c, so_py = _oscene(orc, sc), _oscene(orc, sc)
    rc_c, rep_c, log_c = orc.compute_inplace(f0, so_c, allowed, cap, max_it, want_log=True)
    rc_py, rep_py = _plain_loop(orc, f0, so_py, allowed, cap, max_it)
    assert orc.status_string(rep_c.status) == status
    if name == "abs_err_threshold":
        assert (rep_c.iterations, rep_c.attempts) == (0, 0) and rep_c.err_initial < allowed
    assert (rc_py, rep_py.status, rep_py.iterations, rep_py.attempts) == (rc_c, rep_c.status, rep_c.iterations, rep_c.attempts)
    assert rep_py.hessian_factor == rep_c.hessian_factor
    assert (rep_py.err_initial, rep_py.err_final) == (rep_c.err_initial, rep_c.err_final)
    for k in lt.FIELDS:
        assert rep_py.log[k].dtype == log_c[k].dtype and np.array_equal(rep_py.log[k], log_c[k], equal_nan=True), k
    for k in ("points", "cam_R", "cam_T"):
        assert np.array_equal(getattr(so_py, k), getattr(so_c, k)), k


# ------------------------------------------------------------------ 2. each adapter reproduces its parent

def _small(orc, outliers=False):
    sc = sa.generate_scene(SMALL_FUSED)
    return _oscene(orc, _with_outliers(sc) if outliers else sc), SMALL_FUSED.f0


def _calibrated(skyline):
    def run(orc):
        so, f0 = _small(orc)
        return cref.compute_inplace(orc, f0, so, ALLOWED, CAP, 4, skyline=skyline) + (so,)
    return run


def _robust(kind, fv):
    def run(orc):
        so, f0 = _small(orc, outliers=True)
        return rr.compute_inplace(orc, f0, so, kind, 2.0, ALLOWED, CAP, 4, fv=fv) + (so,)
    return run


def _weighted(kind, fv):
    def run(orc):
        so, f0 = _small(orc, outliers=True)
        q = wr.make_information(so, 21)
        return wr.compute_inplace(orc, f0, so, q, kind, 2.0, ALLOWED, CAP, 4, fv=fv) + (so,)
    return run


def _shared_k(orc):
    sc = sa.generate_scene(SMALL_FUSED)
    so = skr.per_frame_scene(orc, sc, SMALL_FUSED.f0)
    groups = (np.arange(sc.M) % 2).astype(np.int32)
    return skr.compute_inplace(orc, SMALL_FUSED.f0, so, groups, ALLOWED, CAP, 4) + (so,)


def _constant(case):
    def run(orc):
        sc, f0, fconst, pconst, keep_gauge, fv = cc.case(case)
        so = _oscene(orc, sc)
        return kref.compute_inplace(orc, f0, so, fconst, pconst, keep_gauge, fv, ALLOWED, CAP, 3) + (so,)
    return run


def _prior(case):
    def run(orc):
        sc, f0, pri, keep_gauge, fv = pc.case(case)
        so = _oscene(orc, sc)
        return pref.compute_inplace(orc, f0, so, pri, keep_gauge, fv, ALLOWED, CAP, 3) + (so,)
    return run


PARENT_RUNS = {
    "calibrated_qr": _calibrated(False),
    "calibrated_skyline": _calibrated(True),
    "robust_huber_fv10": _robust(rr.HUBER, 10),
    "robust_cauchy_fv6": _robust(rr.CAUCHY, 6),
    "weighted_none_fv10": _weighted(rr.NONE, 10),
    "weighted_huber_fv6": _weighted(rr.HUBER, 6),
    "shared_k_two_groups": _shared_k,
    "constant_nf16_ten_iterations": _constant("nf16_ten_iterations"),
    "constant_nf16_frames_and_landmarks_fixed_k": _constant("nf16_frames_and_landmarks_fixed_k"),
    "prior_nf16_ten_iterations_free_gauge": _prior("nf16_ten_iterations_free_gauge"),
    "prior_nf16_frames_and_landmarks_fixed_k": _prior("nf16_frames_and_landmarks_fixed_k"),
}
EXACT = ("rc", "status", "iterations", "attempts", "attempts_per_iteration", "log_iteration", "log_factor", "log_outcome",
         "hessian_factor")
CLOSE = ("err_initial", "err_final", "log_err_trial", "log_err_value", "points", "cam_R", "cam_T", "K")


def _record(rc, rep, so):
    out = dict(rc=rc, status=rep.status, iterations=rep.iterations, attempts=rep.attempts,
               attempts_per_iteration=rep.attempts_per_iteration, hessian_factor=rep.hessian_factor,
               err_initial=rep.err_initial, err_final=rep.err_final, points=so.points, cam_R=so.cam_R, cam_T=so.cam_T, K=so.K)
    out.update({"log_" + k: rep.log[k] for k in lt.FIELDS})
    return {k: np.asarray(v) for k, v in out.items()}


@pytest.fixture(scope="module")
def parent():
    return load_golden("lm_ref_parent")


@pytest.mark.parametrize("name", list(PARENT_RUNS))
def test_adapter_reproduces_the_separate_loop_it_replaced(orc, parent, name):
    got = _record(*PARENT_RUNS[name](orc))
    assert got["iterations"] >= 3 and got["attempts"] > got["iterations"]
    for k in EXACT:
        want = parent[f"{name}/{k}"]
        assert got[k].shape == want.shape and np.array_equal(got[k], want), k
    for k in CLOSE:
        want = parent[f"{name}/{k}"]
        ok = ~np.isnan(want)  # a failed solve's trial error
        assert got[k].shape == want.shape and np.array_equal(np.isnan(got[k]), ~ok), k
        assert rel_err(got[k][ok], want[ok]) < 1e-8, k


# ------------------------------------------------------------------ 3. robust = weighted at unit information

@pytest.mark.parametrize("fv", [10, 6])
@pytest.mark.parametrize("kind", [rr.NONE, rr.HUBER, rr.CAUCHY])
def test_robust_is_weighted_with_unit_information_bit_for_bit(orc, kind, fv):
    """robust_ref without q and weighted_ref with q = 1 share one body now; this holds the two entry points (q = None and an
    array of ones, through weighted_ref's argument order) to the same bits, as the two separate bodies gave"""
    so_r, f0 = _small(orc, outliers=True)
    so_w, _ = _small(orc, outliers=True)
    rc_r, rep_r = rr.compute_inplace(orc, f0, so_r, kind, 2.0, ALLOWED, CAP, 4, fv=fv)
    rc_w, rep_w = wr.compute_inplace(orc, f0, so_w, np.ones(so_w.O), kind, 2.0, ALLOWED, CAP, 4, fv=fv)
    assert rep_r.iterations >= 3
    assert (rc_r, rep_r.status, rep_r.iterations, rep_r.attempts) == (rc_w, rep_w.status, rep_w.iterations, rep_w.attempts)
    assert rep_r.attempts_per_iteration == rep_w.attempts_per_iteration and rep_r.errors == rep_w.errors
    assert (rep_r.err_initial, rep_r.err_final, rep_r.hessian_factor) == (rep_w.err_initial, rep_w.err_final, rep_w.hessian_factor)
    for k in lt.FIELDS:
        assert np.array_equal(rep_r.log[k], rep_w.log[k], equal_nan=True), k
    for k in ("points", "cam_R", "cam_T"):
        assert np.array_equal(getattr(so_r, k), getattr(so_w, k)), k
