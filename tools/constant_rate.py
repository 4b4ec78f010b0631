"""Constant parameter blocks (srk_ba_set_constant_blocks) against the run without them on the same seeded scenes, in one
process: per-attempt device time by phase (profile level 1, speculation off), the two masking passes' own device time (event
pairs around k_const_points / k_const_frames, srk_ba_constant_pass_ms) and iterations / s with the defaults.  Two constant
sets: the first 10 % of the frames, and a seeded random 10 % of the landmarks (the reference's gauge kept in both).
Prints one JSON line per (config, set, mode) and writes them all to --out.

    python tools/constant_rate.py [--configs C1_dino_standin,C3_1kcam_100kpt] [--steps 10] [--out profiles/constant/constant_rate.json]
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


def constant_set(sc, which):
    """(frame mask or None, landmark mask or None)"""
    if which == "none":
        return None, None
    if which == "frames_first_10pct":
        m = np.zeros(sc.M, dtype=bool)
        m[:max(2, sc.M // 10)] = True
        return m, None
    if which == "landmarks_random_10pct":
        m = np.zeros(sc.N, dtype=bool)
        m[np.random.RandomState(11).choice(sc.N, max(1, sc.N // 10), replace=False)] = True
        return None, m
    raise ValueError(which)


def pass_times(ba, n=20):
    """median device ms of the two masking passes over n staged derivative / assembly phases at the resident scene"""
    pts, frs = [], []
    for _ in range(n):
        ba.phase_derivatives()
        ba.phase_schur(1e-4)
        a, b = ba.constant_pass_ms()
        pts.append(a)
        frs.append(b)
    return float(np.median(pts)), float(np.median(frs))


def one(sa, name, which, steps, profile):
    spec = sa.CONFIGS[name]
    f0 = 600.0 if name == "C1_dino_standin" else spec.f0
    sc = sa.config_scene(name)
    fm, pm = constant_set(sc, which)
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        ba.set_constant_blocks(fm, pm, keep_gauge=True)
        if profile:
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
        out = {"config": name, "constant": which, "constant_frames": int(fm.sum()) if fm is not None else 0,
               "constant_landmarks": int(pm.sum()) if pm is not None else 0, "iterations": int(r.iterations),
               "attempts": int(r.attempts), "seconds": dt, "err_initial": r.err_initial, "err_final": r.err_final}
        if profile:
            att = max(int(r.attempts), 1)
            out["per_attempt"] = {k: getattr(r, k) / att for k in PHASES}
            out["per_attempt"]["total"] = sum(out["per_attempt"].values())
            ba.reset()
            kp, kf = pass_times(ba)
            out["k_const_points_ms"], out["k_const_frames_ms"] = kp, kf
        else:
            out["iterations_per_s"] = r.iterations / dt if dt > 0 else None
        return out
    finally:
        ba.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1_dino_standin,C3_1kcam_100kpt")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constant", "constant_rate.json"))
    a = ap.parse_args()
    import surikatoko_amd as sa
    rows = []
    for name in a.configs.split(","):
        for which in ("none", "frames_first_10pct", "landmarks_random_10pct"):
            for profile in (True, False):
                r = one(sa, name, which, a.steps, profile)
                r["mode"] = "profile" if profile else "defaults"
                print(json.dumps(r), flush=True)
                rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
