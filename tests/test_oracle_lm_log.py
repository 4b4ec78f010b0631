"""The per-attempt log of the reference LM loops (oracle.compute_inplace(..., want_log=True) and the yardstick loops):
it agrees with the loop's own report, does not depend on the oracle's thread count, and the exit cases of
tests/lm_exit_cases.py end as stated there, on decisions clear of rounding."""
import numpy as np
import pytest

import surikatoko_amd as sa
import calibrated_ref as cref
import lm_exit_cases as cases
import lm_trajectory as lt
import shared_k_ref as skr
from gpu_common import orc_scene as _oscene


RUNS = {
    "pixel_noise": (sa.SceneSpec(n_frames=12, grid_nx=10, grid_ny=10, vis_window=5, noise_uv_pix=0.5), 1e-12, 1e6, 12),
    "ragged_wave": (sa.SceneSpec(n_frames=30, grid_nx=23, grid_ny=17, vis_window=7), 1e-7, 1e6, 40),
    "tiny_to_convergence": (sa.SceneSpec(n_frames=5, grid_nx=4, grid_ny=3, vis_window=3), 1e-12, 1e6, 0),
}


@pytest.mark.parametrize("name", list(RUNS))
def test_oracle_log_agrees_with_the_report(orc, name):
    spec, allowed, cap, max_it = RUNS[name]
    so = _oscene(orc, sa.generate_scene(spec))
    rc, rep, log = orc.compute_inplace(spec.f0, so, allowed, cap, max_it, want_log=True)
    assert rep.attempts > rep.iterations >= 3
    lt.check_log_consistent(log, rep, cap)
    assert int(lt.fold(log)["attempts"].sum()) == np.count_nonzero(log["iteration"] < rep.iterations)
    # the log observes the loop and does not steer it: the same run without it
    so2 = _oscene(orc, sa.generate_scene(spec))
    rc2, rep2 = orc.compute_inplace(spec.f0, so2, allowed, cap, max_it)
    assert (rc2, rep2.iterations, rep2.attempts, rep2.status, rep2.err_final, rep2.hessian_factor) == \
        (rc, rep.iterations, rep.attempts, rep.status, rep.err_final, rep.hessian_factor)
    assert np.array_equal(so.points, so2.points) and np.array_equal(so.cam_T, so2.cam_T)


def test_oracle_log_longer_than_its_first_buffer(orc):
    """more attempts than the first log buffer holds (4096): the run is repeated from the same scene with a bigger one"""
    spec = sa.SceneSpec(n_frames=10, grid_nx=12, grid_ny=9, vis_window=5)
    so = _oscene(orc, sa.generate_scene(spec))
    rc, rep, log = orc.compute_inplace(spec.f0, so, 1e-14, 1e6, 2100, want_log=True)
    assert rep.attempts > 4096
    lt.check_log_consistent(log, rep, 1e6)
    so2 = _oscene(orc, sa.generate_scene(spec))
    rc2, rep2 = orc.compute_inplace(spec.f0, so2, 1e-14, 1e6, 2100)
    assert (rep2.attempts, rep2.err_final) == (rep.attempts, rep.err_final)
    assert np.array_equal(so.points, so2.points)


def test_oracle_log_is_bit_identical_at_1_and_8_threads(orc):
    spec = sa.SceneSpec(n_frames=30, grid_nx=23, grid_ny=17, vis_window=7, noise_uv_pix=0.3)
    sc = sa.drop_observations(sa.generate_scene(spec), 0.2, seed=3)
    threads = orc.get_threads()
    logs = {}
    try:
        for n in (1, 8):
            for solver in (0, 1):
                orc.set_threads(n)
                orc.set_solver(solver)
                so = _oscene(orc, sc)
                rc, rep, log = orc.compute_inplace(spec.f0, so, 1e-10, 1e6, 10, want_log=True)
                lt.check_log_consistent(log, rep, 1e6)
                logs[n, solver] = (log, so.points.copy(), rep.attempts)
    finally:
        orc.set_threads(threads)
        orc.set_solver(0)
    for solver in (0, 1):
        a, b = logs[1, solver], logs[8, solver]
        assert a[2] > 10
        for k in lt.FIELDS:
            assert np.array_equal(a[0][k], b[0][k], equal_nan=True), (solver, k)
        assert np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", list(cases.CASES))
def test_exit_cases_end_as_stated_on_clear_decisions(orc, name):
    spec, drop, allowed, cap, max_it, status, counts = cases.CASES[name]
    so = _oscene(orc, cases.scene(name))
    rc, rep, log = orc.compute_inplace(spec.f0, so, allowed, cap, max_it, want_log=True)
    assert orc.status_string(rep.status) == status
    assert (rep.iterations, rep.attempts) == counts
    lt.check_log_consistent(log, rep, cap)
    out = log["outcome"]
    want_last = {"err converged to limit value": lt.CONVERGED, "hessian overflow": lt.CAP_OVERFLOW,
                 "small relative err change": lt.ACCEPTED, "max iterations": lt.ACCEPTED}[status]
    assert out[-1] == want_last
    if status in ("err converged to limit value", "hessian overflow"):
        assert rep.iterations >= 1 and np.count_nonzero(log["iteration"] == rep.iterations) >= 2  # after a rejection
    assert np.abs(lt.margins(log)).min() >= 1e-5
    if allowed is not None:  # every comparison with allowed_err_change is clear of it
        acc = out == lt.ACCEPTED
        ratios = list(np.abs(log["err_trial"] - log["err_value"])[acc] / allowed)
        it = log["iteration"]
        for i in range(rep.iterations + 1):
            rej = np.flatnonzero((it == i) & (out != lt.ACCEPTED))
            ratios += list(np.abs(np.diff(log["err_trial"][rej])) / allowed)
        ratios = np.array(ratios)
        assert np.all(np.abs(ratios - 1) >= 0.04), ratios[np.abs(ratios - 1) < 0.04]
        assert rep.err_initial > 1.04 * allowed


def test_calibrated_yardstick_log(orc):
    spec = sa.SceneSpec(n_frames=8, grid_nx=6, grid_ny=5, vis_window=4, noise_uv_pix=0.5)
    so = _oscene(orc, sa.generate_scene(spec))
    rc, rep = cref.compute_inplace(orc, spec.f0, so, 1e-12, 1e-1, 30)
    assert rep.iterations >= 3 and rep.attempts > rep.iterations
    lt.check_log_consistent(rep.log, rep, 1e-1)
    assert list(lt.fold(rep.log)["attempts"]) == rep.attempts_per_iteration[:rep.iterations]


def test_shared_k_yardstick_log(orc):
    spec = sa.SceneSpec(n_frames=8, grid_nx=6, grid_ny=5, vis_window=4, noise_uv_pix=0.5)
    so = _oscene(orc, sa.generate_scene(spec))
    rc, rep = skr.compute_inplace(orc, spec.f0, so, np.zeros(so.M, dtype=np.int32), 1e-12, 1e6, 6)
    assert rep.iterations >= 3
    lt.check_log_consistent(rep.log, rep, 1e6)
    assert list(lt.fold(rep.log)["attempts"]) == rep.attempts_per_iteration[:rep.iterations]


def test_assert_same_trajectory_catches_equal_totals_in_another_order(orc):
    """two runs with the same (iterations, attempts) but another accept / reject sequence, a wrong factor or a wrong error"""
    spec = sa.SceneSpec(n_frames=12, grid_nx=10, grid_ny=10, vis_window=5, noise_uv_pix=0.5)
    so = _oscene(orc, sa.generate_scene(spec))
    rc, rep, log = orc.compute_inplace(spec.f0, so, 1e-12, 1e6, 12, want_log=True)
    good = lt.fold(log)
    assert lt.assert_same_trajectory(good, log, 1e-12, gpu_attempts=rep.attempts) is None
    a = good["attempts"]
    i, j = int(np.flatnonzero(a != a[0])[0]), 0  # swap two iterations with different attempt counts: same totals
    swapped = dict(good, attempts=a.copy())
    swapped["attempts"][[i, j]] = a[[j, i]]
    with pytest.raises(AssertionError, match=f"accepted iteration {min(i, j)}: attempts"):
        lt.assert_same_trajectory(swapped, log, 1e-6, gpu_attempts=rep.attempts)
    fac = dict(good, hessian_factor=good["hessian_factor"].copy())
    fac["hessian_factor"][3] = np.nextafter(fac["hessian_factor"][3], 1.0)
    with pytest.raises(AssertionError, match="accepted iteration 3: hessian_factor"):
        lt.assert_same_trajectory(fac, log, 1e-6)
    err = dict(good, err=good["err"] * (1 + 1e-5))
    with pytest.raises(AssertionError, match="accepted iteration 0: accepted err"):
        lt.assert_same_trajectory(err, log, 1e-6)
    with pytest.raises(AssertionError, match="attempts"):
        lt.assert_same_trajectory(good, log, 1e-6, gpu_attempts=rep.attempts + 1)
    # a fork is a tie only where the reference's margin at the differing decision is below 1e-10
    with pytest.raises(AssertionError, match="not a tie"):
        lt.assert_same_trajectory(swapped, log, 1e-6, allow_tie_fork=True)
