"""Joint Gaussian pose priors (srk_ba_set_joint_pose_priors) against the run without them on the same seeded scenes, in one
process: per-attempt device time by phase (profile level 1, speculation off) and the three passes' own device time (event
pairs around k_jprior_form + k_jprior_add, k_jprior_couple and k_jprior_error, srk_ba_joint_pose_prior_pass_ms).  Settings:
no set, one set of 16 consecutive frames (the limit: a 96 x 96 information matrix, 120 coupled pairs) and, on C3 only, 60 sets
of 16 consecutive frames chained one shared frame apart (set g holds frames 15 g .. 15 g + 15).  The sets are linearised at the
scene's own poses with the centres moved by a seeded 1e-3; the information matrices are dense, positive definite, of order 100.
Also recorded: the fill of the skyline, the chunk count and whether the frames were renumbered.  Prints one JSON line per
(config, setting) and writes them all to --out.

    python tools/jointprior_rate.py [--configs C1_dino_standin,C3_1kcam_100kpt] [--steps 10] [--out profiles/jointprior/jointprior_rate.json]
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
SETTINGS = ("none", "one_set_of_16", "60_sets_of_16_chained")


def prior_sets(sc, which):
    """the list of sets of set_joint_pose_priors, or None"""
    if which == "none":
        return None
    n_sets = 1 if which == "one_set_of_16" else 60
    if 15 * (n_sets - 1) + 16 > sc.M:
        return ()
    rs = np.random.RandomState(11)
    R = np.asarray(sc.cam_R, dtype=np.float64).reshape(-1, 3, 3)
    T = np.asarray(sc.cam_T, dtype=np.float64).reshape(-1, 3)
    Cn = -np.einsum("jba,jb->ja", R, T)
    A = rs.uniform(-1, 1, size=(96, 96))
    L = 100.0 * (A @ A.T / 96 + 0.5 * np.eye(96))
    out = []
    for g in range(n_sets):
        fr = np.arange(15 * g, 15 * g + 16)
        out.append(dict(frames=fr, R=R[fr], C=Cn[fr] + rs.uniform(-1e-3, 1e-3, size=(16, 3)), info=L))
    return out


def pass_times(ba, n=20):
    """median device ms of the three passes over n staged derivative / Schur / error phases at the resident scene"""
    out = []
    for _ in range(n):
        ba.phase_derivatives()
        ba.phase_schur(1e-4)
        ba.phase_error()
        out.append(ba.joint_pose_prior_pass_ms())
    return [float(x) for x in np.median(np.array(out), axis=0)]


def one(sa, name, which, steps):
    spec = sa.CONFIGS[name]
    f0 = 600.0 if name == "C1_dino_standin" else spec.f0
    sc = sa.config_scene(name)
    sets = prior_sets(sc, which)
    if sets == ():
        return None  # the scene has too few frames for this setting
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        if sets is not None:
            ba.set_joint_pose_priors(sets)
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
        out = {"config": name, "sets": which, "n_sets": 0 if sets is None else len(sets), "iterations": int(r.iterations),
               "attempts": int(r.attempts), "seconds": dt, "err_initial": r.err_initial, "err_final": r.err_final,
               "rcs_fill": ba.rcs_fill(), "rcs_chunks": ba.rcs_chunks(), "renumbered": ba.frame_order() is not None,
               "per_attempt": {k: getattr(r, k) / att for k in PHASES}}
        out["per_attempt"]["total"] = sum(out["per_attempt"].values())
        ba.reset()
        out["k_jprior_form_add_ms"], out["k_jprior_couple_ms"], out["k_jprior_error_ms"] = pass_times(ba) if sets is not None else (0.0, 0.0, 0.0)
        return out
    finally:
        ba.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1_dino_standin,C3_1kcam_100kpt")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jointprior", "jointprior_rate.json"))
    a = ap.parse_args()
    import surikatoko_amd as sa
    rows = []
    for name in a.configs.split(","):
        for which in SETTINGS:
            r = one(sa, name, which, a.steps)
            if r is None:
                continue
            print(json.dumps(r), flush=True)
            rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
