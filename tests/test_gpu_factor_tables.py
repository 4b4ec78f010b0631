"""The upload through the factor-settings unit (surikatoko_amd/csrc/srk_factors.cpp) gives the results the commit before the unit
existed gave: cases of tests/factor_table_cases.py, one optimise call of 3 iterations each, against arrays recorded from that
commit on an MI355X (tests/golden/factor_tables_parent_gpu.npz, written by running record() below with that commit's library).
Deterministic mode: bit for bit.  Otherwise (fp64 atomics) the end-to-end tolerances of tests/test_gpu_scene_plan.py: the same
attempts per iteration and damping factors, errors rel 1e-6, the scene abs 1e-6 in normalised units."""
import os

import numpy as np
import pytest

import surikatoko_amd as sa
import factor_table_cases as ftc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "factor_tables_parent_gpu.npz")
# (case, ask for deterministic mode); deterministic mode refuses fixed intrinsics, so the two fixed_k cases run without it only
RUNS = [(name, det) for name in ("all_five_nf16_10_tiles", "c_nf16_reordered", "p_nf16_reordered", "r_nf16_reordered", "j_reordered")
        for det in (1, 0)] + [("j_sixteen_frames_fixed_k", 0), ("r_ragged_21_22_42_43_fixed_k", 0)]


def _family_errors(ba):
    return np.array([*ba.prior_error(), ba.relative_pose_error(), ba.joint_pose_prior_error()])


def run_case(name, det):
    c = ftc.case(name)
    sc = c["scene"].copy()
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        ba.set_deterministic(bool(det))
        ftc.apply(ba, c)
        assert ba.upload(c["f0"], sc)
        before = _family_errors(ba)
        ba.optimize(max_iterations=3)
        after = _family_errors(ba)
        log = ba.iteration_log()
        ba.download(sc, revert_normalization=False)
        return dict(det=np.int64(ba.deterministic()), pts=sc.points, R=sc.cam_R, T=sc.cam_T, attempts=log["attempts"], err=log["err"],
                    factor=log["hessian_factor"], before=before, after=after)
    finally:
        ba.close()


def record(path):
    np.savez(path, **{f"{name}.{det}.{k}": v for name, det in RUNS for k, v in run_case(name, det).items()})


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.gpu
@pytest.mark.parametrize("name,det", RUNS)
def test_results_are_the_parent_commits(golden, name, det):
    got = run_case(name, det)
    want = {k: golden[f"{name}.{det}.{k}"] for k in got}
    for k in ("err", "factor", "before", "after"):
        print(name, det, k, got[k], want[k])
    assert got["det"] == want["det"] == det
    assert len(got["attempts"]) > 0 and np.array_equal(got["attempts"], want["attempts"])
    if det:
        for k in ("pts", "R", "T", "err", "factor", "before", "after"):
            assert got[k].tobytes() == want[k].tobytes(), k
    else:
        assert np.array_equal(got["factor"], want["factor"])
        assert got["err"] == pytest.approx(want["err"], rel=1e-6)
        assert got["before"] == pytest.approx(want["before"], rel=1e-6) and got["after"] == pytest.approx(want["after"], rel=1e-6)
        for k in ("pts", "R", "T"):
            assert np.abs(got[k] - want[k]).max() < 1e-6, k
