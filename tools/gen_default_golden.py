"""Golden outputs of the default (10-variable) path in deterministic mode, for tests/test_gpu_calibrated.py: the library of a
checkout (ROOT, default: this repository) runs the seeded scenes below to the iteration cap with ordered sums
(srk_ba_set_deterministic), and the scene after the run, the error and the attempt sequence are written to an .npz.
tests/golden/default_det_before_fixed_intrinsics.npz was made with the library of the commit before fixed intrinsics were
added (a checkout of that revision, this file copied into its tools/ and run there on an MI355X):

    python tools/gen_default_golden.py OUT.npz [ROOT]
"""
import os
import sys

import numpy as np

SCENES = {  # name -> (SceneSpec args, f0 override, iterations)
    "C1_dino_standin": (None, 600.0, 20),
    "nf20_runs": (dict(n_frames=30, grid_nx=33, grid_ny=31, vis_window=20), None, 20),
}


def run(sa, name):
    spec_args, f0, iters = SCENES[name]
    if spec_args is None:
        sc = sa.config_scene(name)
        f0 = f0 if f0 is not None else sa.CONFIGS[name].f0
    else:
        spec = sa.SceneSpec(**spec_args)
        sc = sa.generate_scene(spec)
        f0 = spec.f0
    h = sa.BundleAdjustmentKanatani(0)
    try:
        h.set_deterministic(True)
        crit = sa.BundleAdjustmentKanataniTermCriteria()
        s2 = sc.copy()
        h.ComputeInplace(f0, s2, crit, iters)
        log = h.iteration_log()
        r = h.report
        return {f"{name}__det": np.array(h.deterministic()), f"{name}__points": s2.points, f"{name}__cam_R": s2.cam_R,
                f"{name}__cam_T": s2.cam_T, f"{name}__err": np.array([r.err_initial, r.err_final]),
                f"{name}__counts": np.array([r.iterations, r.attempts, r.status]), f"{name}__attempts": log["attempts"],
                f"{name}__log_err": log["err"]}
    finally:
        h.close()


def main():
    out = sys.argv[1]
    root = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import surikatoko_amd as sa
    arrays = {}
    for name in SCENES:
        arrays.update(run(sa, name))
        print(name, "deterministic:", bool(arrays[f"{name}__det"]), "counts:", arrays[f"{name}__counts"].tolist(),
              "err_final: %.17g" % arrays[f"{name}__err"][1])
    np.savez(out, **arrays)


if __name__ == "__main__":
    main()
