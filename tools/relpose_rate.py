"""Relative-pose factors (srk_ba_set_relative_pose_factors) against the run without them on the same seeded scenes, in one
process: per-attempt device time by phase (profile level 1, speculation off) and the three factor passes' own device time
(event pairs around k_relpose_add, k_relpose_couple and k_relpose_error, srk_ba_relative_pose_pass_ms).  Three settings: no
factors, a chain on every consecutive pair of frames, the chain plus one loop closure between the first and the last frame
(frame reordering automatic, as a caller has it).  The measurements are the scene's own relative poses with the translation
moved by a seeded 1e-3, with L_tt = 100 and L_rr = 100.  Also recorded: the fill of the skyline, the chunk count and whether the
frames were renumbered.  Prints one JSON line per (config, setting) and writes them all to --out.

    python tools/relpose_rate.py [--configs C1_dino_standin,C3_1kcam_100kpt] [--steps 10] [--out profiles/relpose/relpose_rate.json]
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
SETTINGS = ("none", "chain", "chain_and_loop_closure")


def factor_set(B, sc, which):
    """(pairs, rel_R, rel_t, info) of set_relative_pose_factors, or None"""
    if which == "none":
        return None
    pairs = [(j, j + 1) for j in range(sc.M - 1)]
    if which == "chain_and_loop_closure":
        pairs.append((0, sc.M - 1))
    pairs.sort(key=lambda p: (min(p), max(p)))
    rs = np.random.RandomState(11)
    Z, z = zip(*[B.relative_pose(sc, a, b) for a, b in pairs])
    z = np.array(z) + rs.uniform(-1e-3, 1e-3, size=(len(pairs), 3))
    return np.array(pairs), np.array(Z), z, 100.0 * np.eye(6)[None]


def pass_times(ba, n=20):
    """median device ms of the three passes over n staged derivative / Schur / error phases at the resident scene"""
    out = []
    for _ in range(n):
        ba.phase_derivatives()
        ba.phase_schur(1e-4)
        ba.phase_error()
        out.append(ba.relative_pose_pass_ms())
    return [float(x) for x in np.median(np.array(out), axis=0)]


def one(sa, name, which, steps):
    from surikatoko_amd import ba as B
    spec = sa.CONFIGS[name]
    f0 = 600.0 if name == "C1_dino_standin" else spec.f0
    sc = sa.config_scene(name)
    fs = factor_set(B, sc, which)
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        if fs is not None:
            ba.set_relative_pose_factors(fs[0], fs[1], fs[2], info=fs[3])
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
        out = {"config": name, "factors": which, "n_factors": 0 if fs is None else int(len(fs[0])), "iterations": int(r.iterations),
               "attempts": int(r.attempts), "seconds": dt, "err_initial": r.err_initial, "err_final": r.err_final,
               "rcs_fill": ba.rcs_fill(), "rcs_chunks": ba.rcs_chunks(), "renumbered": ba.frame_order() is not None,
               "per_attempt": {k: getattr(r, k) / att for k in PHASES}}
        out["per_attempt"]["total"] = sum(out["per_attempt"].values())
        ba.reset()
        out["k_relpose_add_ms"], out["k_relpose_couple_ms"], out["k_relpose_error_ms"] = pass_times(ba) if fs is not None else (0.0, 0.0, 0.0)
        return out
    finally:
        ba.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1_dino_standin,C3_1kcam_100kpt")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relpose", "relpose_rate.json"))
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
