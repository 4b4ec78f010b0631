"""Helpers the GPU test files share: the oracle's view of a scene, a handle with its modes set, a plain LM run of the
library and the comparison of two such runs.  The mode-specific runs (robust loss, observation information), every _phases
and every _same_as_yardstick stay in their test files: their tolerances differ per mode on purpose."""
import numpy as np
import pytest

import surikatoko_amd as sa


def orc_scene(orc, sc):
    return orc.Scene(sc.points, sc.cam_R, sc.cam_T, sc.K, sc.shared_k, sc.row_ptr, sc.obs_frame, sc.obs_uv)


def handle(fv=10, **modes):
    h = sa.BundleAdjustmentKanatani(0)
    if fv == 6:
        h.set_fixed_intrinsics(True)
    for k, v in modes.items():
        getattr(h, "set_" + k)(v)
    return h


def run_lm(gpu, sc, f0, allowed=None, max_factor=None, max_iterations=0):
    crit = sa.BundleAdjustmentKanataniTermCriteria()
    crit.AllowedReprojErrRelativeChange(allowed)
    crit.MaxHessianFactor(max_factor)
    sg = sc.copy()
    ok = gpu.ComputeInplace(f0, sg, crit, max_iterations)
    return ok, gpu.report, sg, gpu.iteration_log()


def compare_runs(a, b, tol=1e-7):
    (ok_a, rep_a, sg_a, log_a), (ok_b, rep_b, sg_b, log_b) = a, b
    assert ok_a == ok_b and rep_a.status == rep_b.status
    assert (rep_a.iterations, rep_a.attempts) == (rep_b.iterations, rep_b.attempts)
    assert list(log_a["attempts"]) == list(log_b["attempts"])
    assert rep_a.err_final == pytest.approx(rep_b.err_final, rel=tol)
    assert np.abs(sg_a.points - sg_b.points).max() < tol
    assert np.abs(sg_a.cam_R - sg_b.cam_R).max() < tol
    assert np.abs(sg_a.cam_T - sg_b.cam_T).max() < tol
