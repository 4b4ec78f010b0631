"""The upload through the scene planner gives the results the commit before the planner existed gave: the branch-taking cases of
tests/scene_plan_cases.py, one optimise call of 3 iterations each, against arrays recorded from that commit on an MI355X
(tests/golden/scene_plan_parent_gpu.npz, written by running record() below with that commit's library).  Deterministic mode
where the scene runs that way: bit for bit.  Otherwise (fp64 atomics) the end-to-end tolerances of tests/test_gpu_parity.py:
the same attempts per iteration, errors rel 1e-6, the scene abs 1e-6 in normalised units."""
import os

import numpy as np
import pytest

import surikatoko_amd as sa
import scene_plan_cases as spc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_plan_parent_gpu.npz")
# (case, ask for deterministic mode): (a) and (b) with it are the cases (j); (d) has long tracks and falls back to atomics
RUNS = [("a_uniform", 1), ("b_ragged", 1), ("d_all_visible_30", 1), ("h_shuffled_auto", 1), ("h_shuffled_given", 1),
        ("a_uniform", 0), ("b_ragged", 0)]


def run_case(name, det):
    sc, o = spc.case(name)
    sc = sc.copy()
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        ba.set_deterministic(bool(det))
        ba.set_jacobian_mode(o["jac_mode"])
        ba.set_frame_reordering(o["frame_order_mode"])
        if o["frame_order"] is not None:
            ba.set_frame_order(o["frame_order"])
        assert ba.upload(600.0, sc)
        ba.optimize(max_iterations=3)
        log = ba.iteration_log()
        ba.download(sc, revert_normalization=False)
        return dict(det=np.int64(ba.deterministic()), kernel=np.int64(ba.jacobian_kernel()), pts=sc.points, R=sc.cam_R, T=sc.cam_T,
                    attempts=log["attempts"], err=log["err"], factor=log["hessian_factor"])
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
    assert got["det"] == want["det"] and got["kernel"] == want["kernel"]
    assert got["det"] == (1 if det and name != "d_all_visible_30" else 0)
    assert len(got["attempts"]) > 0 and np.array_equal(got["attempts"], want["attempts"])
    if got["det"]:
        for k in ("pts", "R", "T", "err", "factor"):
            assert got[k].tobytes() == want[k].tobytes(), k
    else:
        assert np.array_equal(got["factor"], want["factor"])
        assert got["err"] == pytest.approx(want["err"], rel=1e-6)
        for k in ("pts", "R", "T"):
            assert np.abs(got[k] - want[k]).max() < 1e-6, k
