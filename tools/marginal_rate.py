"""Marginalisation priors (srk_ba_marginalization_prior) timed on the benchmark scenes with six variables a frame (fixed
intrinsics), beside the only route callers had before it on the same scene: joint_covariance of the kept frames plus numpy's
inverse (which also counts the observations that stay in the window, so it is a price tag, not the same quantity).

Per config, after two LM iterations on the seeded scene: frame 0 is dropped with the landmarks marginalization_landmarks(max_kept=16)
chooses, the dropped frame's other observations switched off through set_observation_information.  Recorded: the two kernels' device
times from the call's event pairs, the host part (factor terms, elimination, revert map), the wall time of the call (median of
--reps; it synchronises), and the wall time of joint_covariance(K, []) + numpy.linalg.inv.  One JSON line per config, all of them
to --out.

    python tools/marginal_rate.py [--configs C1_dino_standin,C3_1kcam_100kpt] [--reps 5] [--out profiles/marginal/marginal_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out))


def one(sa, name, reps):
    spec = sa.CONFIGS[name]
    f0 = 600.0 if name == "C1_dino_standin" else spec.f0
    sc = sa.config_scene(name)
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        ba.set_fixed_intrinsics(True)
        assert ba.upload(f0, sc)
        ba.optimize(None, max_iterations=2)
        drop = [0]
        P, q = sa.marginalization_landmarks(sc, drop, max_kept=16)
        ba.set_observation_information(q)
        kept, counts = ba.marginalization_plan(drop, P)
        ba.marginalization_prior(drop, P)  # warm-up: allocations, code objects
        reports = []

        def call():
            reports.append(ba.marginalization_prior(drop, P)["report"])

        ms_call = median_ms(call, reps)
        med = lambda key: float(np.median([r[key] for r in reports]))  # noqa: E731
        out = {"config": name, "n_frames": sc.M, "n_points": sc.N, "dropped": drop, "kept": [int(k) for k in kept], "landmarks": int(len(P)),
               "landmarks_used": int(reports[-1]["landmarks_used"]), "observations": int(counts["n_observations"]), "strip_rows": 4 * int(len(P)),
               "strip_columns": 6 * (len(drop) + len(kept)) + 1, "reps": reps, "k_marg_rows_ms": med("ms_rows"), "k_marg_gram_ms": med("ms_gram"),
               "host_ms": med("ms_host"), "call_ms": ms_call, "defect": float(reports[-1]["defect"])}
        ba.set_observation_information(None)
        ba.joint_covariance(kept[:2], [])

        def covariance_route():
            cov = ba.joint_covariance(kept, [])
            np.linalg.inv(cov)

        out["joint_covariance_plus_inverse_ms"] = median_ms(covariance_route, reps)
        return out
    finally:
        ba.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1_dino_standin,C3_1kcam_100kpt")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marginal", "marginal_rate.json"))
    a = ap.parse_args()
    import surikatoko_amd as sa
    rows = []
    for name in a.configs.split(","):
        r = one(sa, name, a.reps)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
