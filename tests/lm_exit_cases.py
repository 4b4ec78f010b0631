"""Small scenes and termination criteria on which the reference loop ends with each of its statuses; shared by the CPU
test that pins the choice (tests/test_oracle_lm_log.py) and the GPU test that runs them (tests/test_gpu_lm_exits.py).

Every decision of these runs is clear of rounding: the smallest |margin| (err_value - err_trial) / err_value of any
attempt is >= 1e-5, and every |change| compared with allowed_err_change is at least 4 % away from it, so a library whose
errors agree with the oracle's to 1e-12 must take the same decisions.  Found by scanning the SceneSpec families (pixel
noise, dropped observations, perturbed starts) over criteria with the oracle.

- "err converged to limit value" (status 4) is rare: it needs two consecutive rejections in one iteration that differ by
  less than allowed_err_change while every accepted change before them differs by more.  On the noise-free and
  low-noise scenes the accepted changes shrink faster than the rejected ones, and "small relative err change" comes first.
  Of the scanned scenes one, 1 px noise with 40 % of the observations dropped, has it with a 5 % gap either side, in
  its second iteration: there the library's first round is a speculative pair and both its attempts are rejected.
- "hessian overflow" from the cap: after a rejection the factor x10 exceeds MaxHessianFactor (1e-2 and 1e-3: the run
  stops in its 11th and 3rd iteration).
"""
import surikatoko_amd as sa

NOISY_WAVE = sa.SceneSpec(n_frames=20, grid_nx=12, grid_ny=9, vis_window=6, noise_uv_pix=1.0)
PIXEL_NOISE = sa.SceneSpec(n_frames=12, grid_nx=10, grid_ny=10, vis_window=5, noise_uv_pix=0.5)

# name: (spec, fraction of observations dropped (seed 5), allowed_err_change, max_hessian_factor, max_iterations,
#        expected status, expected (iterations, attempts))
CASES = {
    "err_converged": (NOISY_WAVE, 0.4, 6.06e-4, None, 0, "err converged to limit value", (1, 5)),
    "small_err_change": (PIXEL_NOISE, 0.0, 1e-8, None, 0, "small relative err change", (22, 46)),
    "cap_overflow_1e-2": (PIXEL_NOISE, 0.0, None, 1e-2, 0, "hessian overflow", (10, 23)),
    "cap_overflow_1e-3": (PIXEL_NOISE, 0.0, None, 1e-3, 0, "hessian overflow", (2, 6)),
    "max_iterations": (PIXEL_NOISE, 0.2, 1e-12, 1e6, 8, "max iterations", (8, 18)),
}


def scene(name):
    spec, drop = CASES[name][:2]
    sc = sa.generate_scene(spec)
    return sa.drop_observations(sc, drop, seed=5) if drop else sc
