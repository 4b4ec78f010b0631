"""Robust bundle adjustment (srk_ba_set_robust_loss) against plain least squares on the same seeded scenes: device time by
phase (profile level 1, speculation off) per attempt, and the derivative pass per iteration (one derivative pass an
iteration with speculation off).  The losses take different numbers of iterations, so compare per attempt / per pass, not
iterations / s.  Prints one JSON line per (config, loss) and writes them all to --out.

    python tools/robust_rate.py [--configs C1_dino_standin,C2_200cam_20kpt,C3_1kcam_100kpt,C5_4kcam_1Mpt] [--steps 10]
                                [--delta 2.0] [--out profiles/robust/robust_rate.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ("ms_jacobian", "ms_schur", "ms_solve", "ms_backsub", "ms_apply", "ms_error")


def one(sa, name, loss, delta, steps):
    spec = sa.CONFIGS[name]
    f0 = 600.0 if name == "C1_dino_standin" else spec.f0
    sc = sa.config_scene(name)
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        ba.set_speculation(False)
        ba.set_profile(1)
        ba.set_robust_loss(loss, delta)
        assert ba.upload(f0, sc)
        ba.optimize(None, max_iterations=2)  # warm-up
        ba.reset()
        import torch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ba.optimize(None, max_iterations=steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        r = ba.report
        att, it = max(int(r.attempts), 1), max(int(r.iterations), 1)
        out = {"config": name, "loss": loss or "none", "delta_pixels": delta if loss else None, "jacobian_kernel": ba.jacobian_kernel(),
               "iterations": int(r.iterations), "attempts": int(r.attempts), "seconds": dt, "err_initial": r.err_initial,
               "err_final": r.err_final}
        out["per_attempt"] = {k: getattr(r, k) / att for k in PHASES}
        out["per_attempt"]["total"] = sum(out["per_attempt"].values())
        out["per_attempt"]["error_pass"] = r.ms_error / (att + 1)  # the initial error and one a attempt
        out["derivative_pass"] = r.ms_jacobian / it
        return out
    finally:
        ba.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1_dino_standin,C2_200cam_20kpt,C3_1kcam_100kpt,C5_4kcam_1Mpt")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--delta", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import surikatoko_amd as sa
    rows = []
    for name in a.configs.split(","):
        for loss in (None, "huber"):
            r = one(sa, name, loss, a.delta, a.steps)
            print(json.dumps(r), flush=True)
            rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
