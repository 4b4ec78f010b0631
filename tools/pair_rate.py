"""Two-view pose refinement (srk_refine_pairs, srk_relate_frames_refined) timed on the synthetic batch of tools/relate_rate.py:
1000 pairs of 2000 matches each (2 000 000 matches), every pair with its own motion, one pixel of noise, 30 % of the matches
replaced by uniform points.

Recorded (median of --reps, device time of the refinement's kernels from the call's event pair, and the wall time of the call with
its uploads): evaluate-only (attempts = 0: one pass over the matches), ten attempts without a loss and ten attempts with a Cauchy
loss at the inlier threshold, all three from relate's poses; and the chained call (256 hypotheses, the refinement on the winner's
inliers with the Cauchy loss), whose relate time is read from relate's own event pair in the same run: how much the refinement
adds to a relate call is the figure users ask for.  Beside each: the attempts used and the median errors to the truth before and
after.  One JSON object to --out.

    python tools/pair_rate.py [--reps 7] [--out profiles/pair/pair_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from relate_rate import F0, K, batch  # noqa: E402

TAU = 4.0


def errors(R, T, truth):
    Rt, Tt = truth
    rot = np.arccos(np.clip(0.5 * (np.einsum("nij,nij->n", R, Rt) - 1.0), -1.0, 1.0))
    direction = np.arccos(np.clip(np.einsum("ni,ni->n", T, Tt), -1.0, 1.0))
    return float(np.median(rot)), float(np.median(direction))


def timed_refine(sa, PR, ba, reps, row_ptr, ua, ub, start, truth, **kw):
    sa.refine_pairs(ba, F0, row_ptr, ua, ub, K, K, start.R, start.T, **kw)   # warm-up: allocations, code objects
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = sa.refine_pairs(ba, F0, row_ptr, ua, ub, K, K, start.R, start.T, **kw)
        wall.append(1e3 * (time.perf_counter() - t0))
        dev.append(PR.last_kernel_ms(ba))
    ms, O = float(np.median(dev)), int(row_ptr[-1])
    passes = float(np.sum(res.quality[:, 5] + 1.0) / len(res.status))             # walks of the matches per pair: the start and one per attempt
    rot, direction = errors(res.R, res.T, truth)
    return {"kernel_ms": ms, "call_ms": float(np.median(wall)), "mean_attempts": float(res.quality[:, 5].mean()), "matches_walked_per_s": passes * O / (1e-3 * ms),
            "not_converged": int(np.count_nonzero(res.status & 8)), "degenerate": int(np.count_nonzero(res.status & 2)),
            "median_rms_pixels": float(np.median(res.quality[:, 0])), "median_rotation_error_rad": rot, "median_direction_error_rad": direction}


def timed_chain(sa, PR, RL, ba, reps, row_ptr, ua, ub, truth, hypotheses, refine):
    kw = dict(hypotheses=hypotheses, inlier_pixels=TAU)
    sa.relate_frames(ba, F0, row_ptr, ua, ub, K, K, refine=refine, **kw)
    dev, rel, wall = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        related, res = sa.relate_frames(ba, F0, row_ptr, ua, ub, K, K, refine=refine, **kw)
        wall.append(1e3 * (time.perf_counter() - t0))
        dev.append(PR.last_kernel_ms(ba))
        rel.append(RL.last_kernel_ms(ba)[0])
    plain = []
    for _ in range(reps):                                                         # relate alone, the same batch, the same run
        t0 = time.perf_counter()
        before = sa.relate_frames(ba, F0, row_ptr, ua, ub, K, K, **kw)
        plain.append((RL.last_kernel_ms(ba)[0], 1e3 * (time.perf_counter() - t0)))
    ms, rms = float(np.median(dev)), float(np.median(rel))
    rot, direction = errors(res.R, res.T, truth)
    rot0, direction0 = errors(before.R, before.T, truth)
    return {"refine_kernel_ms": ms, "relate_kernel_ms_in_the_chain": rms, "relate_kernel_ms_alone": float(np.median([p[0] for p in plain])),
            "refinement_adds_share_of_relate": ms / rms, "call_ms": float(np.median(wall)), "relate_call_ms_alone": float(np.median([p[1] for p in plain])),
            "mean_attempts": float(res.quality[:, 5].mean()), "pairs_not_related": int(np.count_nonzero(related.status)),
            "median_rotation_error_rad_before": rot0, "median_direction_error_rad_before": direction0, "median_rotation_error_rad": rot,
            "median_direction_error_rad": direction}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--matches", type=int, default=2000)
    ap.add_argument("--hypotheses", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair", "pair_rate.json"))
    a = ap.parse_args()
    import surikatoko_amd as sa
    from surikatoko_amd import pair as PR
    from surikatoko_amd import relate as RL
    rng = np.random.default_rng(24)
    row_ptr, ua, ub, R, T, moved = batch(a.pairs, a.matches, rng)
    out = {"scene": "synthetic pairs, one pixel of noise, 30 % of the matches replaced", "n_pairs": a.pairs, "n_matches": int(row_ptr[-1]), "reps": a.reps,
           "inlier_pixels": TAU, "hypotheses": a.hypotheses}
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        start = sa.relate_frames(ba, F0, row_ptr, ua, ub, K, K, hypotheses=a.hypotheses, inlier_pixels=TAU)
        ok = start.status == 0                                                    # a pair that was not related has no unit T to start from
        start.R[~ok], start.T[~ok] = np.eye(3), np.array([1.0, 0.0, 0.0])
        out["start"] = dict(zip(("median_rotation_error_rad", "median_direction_error_rad"), errors(start.R, start.T, (R, T))))
        for name, kw in (("evaluate_only", dict(attempts=0)), ("ten_attempts", dict(attempts=10)),
                         ("ten_attempts_cauchy", dict(attempts=10, loss="cauchy", delta=TAU))):
            out[name] = timed_refine(sa, PR, ba, a.reps, row_ptr, ua, ub, start, (R, T), **kw)
            print(name, json.dumps(out[name]), flush=True)
        out["chained"] = timed_chain(sa, PR, RL, ba, a.reps, row_ptr, ua, ub, (R, T), a.hypotheses,
                                     dict(attempts=10, loss="cauchy", delta=TAU, inliers_only=True))
        print("chained", json.dumps(out["chained"]), flush=True)
    finally:
        ba.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
