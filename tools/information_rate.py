"""Per-observation information (srk_ba_set_observation_information) against the same run without it, in one process on the
same seeded scenes: device time by phase (profile level 1, speculation off) per attempt, the derivative pass per iteration
and the error pass, for no loss against information alone and for Huber against Huber with information.  The information is
seeded (log-uniform in [0.25, 4], about 3 % of the observations switched off, at most one per landmark and only where four or
more are left).  Runs with and without information take different numbers of attempts, so compare per attempt / per pass.
Prints one JSON line per (config, loss, information) and writes them all to --out.

    python tools/information_rate.py [--configs C1_dino_standin,C2_200cam_20kpt,C3_1kcam_100kpt,C5_4kcam_1Mpt] [--steps 10]
                                     [--delta 2.0] [--seed 21] [--out profiles/information/information_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ("ms_jacobian", "ms_schur", "ms_solve", "ms_backsub", "ms_apply", "ms_error")


def make_information(row_ptr, seed, zero_frac=0.03):
    rng = np.random.RandomState(seed)
    rp = np.asarray(row_ptr)
    O = int(rp[-1])
    q = np.exp(rng.uniform(np.log(0.25), np.log(4.0), size=O))
    cnt = np.diff(rp)
    cand = np.flatnonzero(cnt >= 4)
    pick = rng.choice(cand, size=min(len(cand), int(round(zero_frac * O))), replace=False)
    q[rp[pick] + (rng.randint(1 << 30, size=len(pick)) % cnt[pick])] = 0.0
    return q


def one(sa, name, loss, delta, steps, q):
    spec = sa.CONFIGS[name]
    f0 = 600.0 if name == "C1_dino_standin" else spec.f0
    sc = sa.config_scene(name)
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        ba.set_speculation(False)
        ba.set_profile(1)
        ba.set_robust_loss(loss, delta)
        ba.set_observation_information(q)
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
        out = {"config": name, "loss": loss or "none", "delta_pixels": delta if loss else None, "information": q is not None,
               "jacobian_kernel": ba.jacobian_kernel(), "iterations": int(r.iterations), "attempts": int(r.attempts),
               "seconds": dt, "err_initial": r.err_initial, "err_final": r.err_final}
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
    ap.add_argument("--seed", type=int, default=21)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import surikatoko_amd as sa
    rows = []
    for name in a.configs.split(","):
        q = make_information(sa.config_scene(name).row_ptr, a.seed)
        for loss in (None, "huber"):
            pair = [one(sa, name, loss, a.delta, a.steps, info) for info in (None, q)]
            for r in pair:
                print(json.dumps(r), flush=True)
                rows.append(r)
            base, info = pair
            rel = {"config": name, "loss": loss or "none", "information_over_none": {
                "attempt": info["per_attempt"]["total"] / base["per_attempt"]["total"],
                "derivative_pass": info["derivative_pass"] / base["derivative_pass"],
                "error_pass": info["per_attempt"]["error_pass"] / base["per_attempt"]["error_pass"]}}
            print(json.dumps(rel), flush=True)
            rows.append(rel)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
