"""Position priors (srk_ba_set_position_priors) against the run without them on the same seeded scenes, in one process:
per-attempt device time by phase (profile level 1, speculation off) and the two prior passes' own device time (event pairs
around k_prior_add and k_prior_error, srk_ba_prior_pass_ms).  Four settings: no priors, a centre prior on every frame, a prior
on every hundredth landmark, a prior on every landmark (the reference's gauge kept in all).  Priors sit at the scene's own
positions moved by a seeded 1e-3, with L = 10 (landmarks) and L = 100 (centres).
Prints one JSON line per (config, setting) and writes them all to --out.

    python tools/prior_rate.py [--configs C1_dino_standin,C3_1kcam_100kpt] [--steps 10] [--out profiles/priors/prior_rate.json]
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
SETTINGS = ("none", "every_frame", "every_100th_landmark", "every_landmark")


def prior_set(sc, which):
    """(points, frames) arguments of set_position_priors"""
    rs = np.random.RandomState(11)
    if which == "none":
        return None, None
    if which == "every_frame":
        R, T = sc.cam_R.reshape(-1, 3, 3), sc.cam_T.reshape(-1, 3)
        C = -np.einsum("jba,jb->ja", R, T)
        return None, (np.arange(sc.M), C + rs.uniform(-1e-3, 1e-3, size=C.shape), {"info": 100.0 * np.eye(3)[None]})
    idx = np.arange(0, sc.N, 100 if which == "every_100th_landmark" else 1)
    return (idx, sc.points[idx] + rs.uniform(-1e-3, 1e-3, size=(idx.size, 3)), {"info": 10.0 * np.eye(3)[None]}), None


def pass_times(ba, n=20):
    """median device ms of the two prior passes over n staged derivative / error phases at the resident scene"""
    a, b = [], []
    for _ in range(n):
        ba.phase_derivatives()
        ba.phase_error()
        x, y = ba.prior_pass_ms()
        a.append(x)
        b.append(y)
    return float(np.median(a)), float(np.median(b))


def one(sa, name, which, steps):
    spec = sa.CONFIGS[name]
    f0 = 600.0 if name == "C1_dino_standin" else spec.f0
    sc = sa.config_scene(name)
    pts, frs = prior_set(sc, which)
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        ba.set_position_priors(pts, frs, keep_gauge=True)
        ba.set_speculation(False)
        ba.set_profile(1)
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
        att = max(int(r.attempts), 1)
        out = {"config": name, "priors": which, "frame_priors": 0 if frs is None else int(len(frs[0])),
               "landmark_priors": 0 if pts is None else int(len(pts[0])), "iterations": int(r.iterations),
               "attempts": int(r.attempts), "seconds": dt, "err_initial": r.err_initial, "err_final": r.err_final,
               "per_attempt": {k: getattr(r, k) / att for k in PHASES}}
        out["per_attempt"]["total"] = sum(out["per_attempt"].values())
        ba.reset()
        out["k_prior_add_ms"], out["k_prior_error_ms"] = pass_times(ba)
        return out
    finally:
        ba.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1_dino_standin,C3_1kcam_100kpt")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "priors", "prior_rate.json"))
    a = ap.parse_args()
    import surikatoko_amd as sa
    rows = []
    for name in a.configs.split(","):
        for which in SETTINGS:
            r = one(sa, name, which, a.steps)
            print(json.dumps(r), flush=True)
            rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
