"""Every exit of the library's LM loop against the oracle's loop, attempt by attempt (tests/lm_exit_cases.py: small
scenes and criteria that end the reference run with "err converged to limit value", "small relative err change",
"hessian overflow" from the MaxHessianFactor cap after rejected attempts, and "max iterations"; "hessian overflow" from a
failed solve is test_gpu_parity.py::test_failed_solve_is_hessian_overflow_as_in_the_reference_and_leaves_no_residue).

Each case runs with speculative pairs on and off: with speculation on,
the converged and capped exits are decided while the pair's second attempt is already computed (or, at the cap, must
not be started), which is where attempt counting and slot handling can go wrong.  Every run is compared with the oracle
by lm_trajectory.assert_same_trajectory plus ComputeInplace's return value, status, attempt count and final error; then
the same handle is reset() and runs again, and must repeat itself.

Deterministic mode does not take these scenes: it needs every landmark on the run-based derivative and Schur kernels
(srk_ba_upload_scene builds its ordered-sum tables only then), which scenes of a few hundred landmarks with ragged tracks
do not give -- the handle reports deterministic() False and runs the default path.  The deterministic loop is compared
with the oracle attempt by attempt on the bench scene (test_gpu_parity.py::
test_c3_bench_run_vs_the_oracle_loop_attempt_by_attempt, exit "max iterations") and bit for bit against itself after
reset() (test_reset_after_a_warm_up_reproduces_a_fresh_run)."""
import numpy as np
import pytest

import surikatoko_amd as sa
import lm_exit_cases as cases
import lm_trajectory as lt

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _oracle(orc, name):
    if name not in _ORACLE:
        spec, _, allowed, cap, max_it = cases.CASES[name][:5]
        sc = cases.scene(name)
        so = orc.Scene(sc.points, sc.cam_R, sc.cam_T, sc.K, sc.shared_k, sc.row_ptr, sc.obs_frame, sc.obs_uv)
        _ORACLE[name] = orc.compute_inplace(spec.f0, so, allowed, cap, max_it, want_log=True) + (so,)
    return _ORACLE[name]


@pytest.mark.parametrize("speculation", [True, False], ids=["pairs", "sequential"])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_exit_matches_the_oracle_attempt_by_attempt(orc, name, speculation):
    spec, _, allowed, cap, max_it, status, counts = cases.CASES[name]
    rc_o, rep_o, log_o, so = _oracle(orc, name)
    assert orc.status_string(rep_o.status) == status and (rep_o.iterations, rep_o.attempts) == counts
    crit = sa.BundleAdjustmentKanataniTermCriteria()
    crit.AllowedReprojErrRelativeChange(allowed)
    crit.MaxHessianFactor(cap)
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_speculation(speculation)
        sg = cases.scene(name)
        ok = h.ComputeInplace(spec.f0, sg, crit, max_it)
        rep = h.report
        assert ok == (rc_o == 0)
        assert h.OptimizationStatusString() == status
        assert (rep.iterations, rep.attempts) == counts
        lt.assert_same_trajectory(h.iteration_log(), log_o, 1e-9, gpu_attempts=rep.attempts)
        assert rep.err_final == pytest.approx(rep_o.err_final, rel=1e-9)
        assert rep.hessian_factor == rep_o.hessian_factor
        assert np.abs(sg.points - so.points).max() < 1e-6 and np.abs(sg.cam_T - so.cam_T).max() < 1e-6
        first = (rep.iterations, rep.attempts, rep.status, rep.err_final, h.iteration_log())
        # the handle still works: reset() to the uploaded scene and the same run again
        h.reset()
        ok2 = h.optimize(crit, max_iterations=max_it)
        rep = h.report
        assert ok2 == ok and (rep.iterations, rep.attempts, rep.status) == first[:3]
        lt.assert_same_trajectory(h.iteration_log(), log_o, 1e-9, gpu_attempts=rep.attempts)
        assert rep.err_final == pytest.approx(first[3], rel=1e-12)
    finally:
        h.close()
