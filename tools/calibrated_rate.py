"""Calibrated bundle adjustment (srk_ba_set_fixed_intrinsics) against the default 10-variable layout on the same seeded
scenes: per-attempt device time by phase (profile level 1, speculation off) and iterations / s with the defaults.
Prints one JSON line per (config, mode) and writes them all to --out.

    python tools/calibrated_rate.py [--configs C1_dino_standin,C2_200cam_20kpt,C3_1kcam_100kpt,C5_4kcam_1Mpt] [--steps 10]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ("ms_jacobian", "ms_schur", "ms_solve", "ms_backsub", "ms_apply", "ms_error")


def one(sa, name, fixed, steps, profile):
    spec = sa.CONFIGS[name]
    f0 = 600.0 if name == "C1_dino_standin" else spec.f0
    sc = sa.config_scene(name)
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        ba.set_fixed_intrinsics(fixed)
        if profile:
            ba.set_speculation(False)
            ba.set_profile(1)
        assert ba.upload(f0, sc)
        fv = ba.frame_vars()
        ba.optimize(None, max_iterations=2)  # warm-up
        ba.reset()
        import torch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ba.optimize(None, max_iterations=steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        r = ba.report
        ld = (fv * sc.M + 255) // 256 * 256
        out = {"config": name, "frame_vars": fv, "ld": ld, "iterations": int(r.iterations), "attempts": int(r.attempts),
               "seconds": dt, "err_initial": r.err_initial, "err_final": r.err_final}
        if profile:
            att = max(int(r.attempts), 1)
            out["per_attempt"] = {k: getattr(r, k) / att for k in PHASES}
            out["per_attempt"]["total"] = sum(out["per_attempt"].values())
        else:
            out["iterations_per_s"] = r.iterations / dt if dt > 0 else None
        return out
    finally:
        ba.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1_dino_standin,C2_200cam_20kpt,C3_1kcam_100kpt,C5_4kcam_1Mpt")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import surikatoko_amd as sa
    rows = []
    for name in a.configs.split(","):
        for fixed in (False, True):
            for profile in (True, False):
                r = one(sa, name, fixed, a.steps, profile)
                r["mode"] = "profile" if profile else "defaults"
                print(json.dumps(r), flush=True)
                rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
