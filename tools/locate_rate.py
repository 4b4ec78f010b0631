"""Resection without a start pose (srk_locate_frames) timed on the landmarks of the benchmark scene C3 (100 000 landmarks) with 1000
extra frames of 2000 observations each: frame j sees what C3's frame j sees, the ground-truth landmark projected into the
ground-truth camera with 0.3 px of noise, 30 % of the observations moved by 20 .. 60 px; no pose is given.

Recorded per variant (64 and 256 hypotheses for the batch, 256 and 1024 for one frame alone, each without and with ten refinement
attempts under a Cauchy loss): the kernels' device time from the call's event pair (median of --reps), the hypothesis-and-score
kernel's own time and its share, the wall time of the call, and projections per second (hypotheses x observations / time) beside
the double-precision vector peak.  A projection is 9 multiply-adds for the pack, 3 for the depth, one division, 2 multiply-adds
and 5 more operations for the error and the truncated sum: about 35 flop, so the peak in projections is the flop peak / 35.  One
JSON object to --out.

    python tools/locate_rate.py [--reps 7] [--out profiles/locate/locate_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FP64_VECTOR_PEAK = 78.6e12   # flop / s: half the 157.3 TFLOPS single-precision vector peak of the MI355X data sheet
FLOP_PER_PROJECTION = 35


def timed(sa, LC, ba, reps, f0, row_ptr, point, uv, X, K, truth, **kw):
    sa.locate_frames(ba, f0, row_ptr, point, uv, X, K, **kw)   # warm-up: allocations, code objects
    dev, score, wall = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = sa.locate_frames(ba, f0, row_ptr, point, uv, X, K, **kw)
        wall.append(1e3 * (time.perf_counter() - t0))
        ms = LC.last_kernel_ms(ba)
        dev.append(ms[0])
        score.append(ms[1])
    ms, sms, O = float(np.median(dev)), float(np.median(score)), int(row_ptr[-1])
    rate = kw["hypotheses"] * O / (1e-3 * sms)
    Rt, Tt = truth
    centre = np.linalg.norm(np.einsum("nji,nj->ni", res.R, res.T) - np.einsum("nji,nj->ni", Rt, Tt), axis=1)
    return {"kernel_ms": ms, "score_kernel_ms": sms, "score_share": sms / ms, "call_ms": float(np.median(wall)), "projections_per_s": rate,
            "share_of_fp64_vector_peak": rate * FLOP_PER_PROJECTION / FP64_VECTOR_PEAK, "frames_not_located": int(np.count_nonzero(res.located_status)),
            "median_inlier_share": float(np.median(res.located[:, 2] / np.maximum(res.located[:, 1], 1))),
            "median_centre_error": float(np.median(centre)), "max_centre_error": float(centre.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate", "locate_rate.json"))
    a = ap.parse_args()
    import surikatoko_amd as sa
    from surikatoko_amd import locate as LC
    from resect_rate import frames_of_c3
    sc, f0, row_ptr, point, uv, pts, K = frames_of_c3(sa)
    _, _, Rg, Tg = sa.config_scene("C3_1kcam_100kpt", with_gt=True)
    Rg, Tg = Rg.reshape(-1, 3, 3), Tg.reshape(-1, 3)
    rng = np.random.default_rng(10)
    moved = rng.random(len(uv)) < 0.3
    ang, mag = rng.uniform(0, 2 * np.pi, len(uv)), rng.uniform(20, 60, len(uv))
    uv = uv + moved[:, None] * np.column_stack([mag * np.cos(ang), mag * np.sin(ang)])
    out = {"scene": "C3_1kcam_100kpt landmarks, one extra frame per C3 frame, 30 % of the observations moved", "n_frames": int(sc.M),
           "n_landmarks": int(sc.N), "n_observations": int(row_ptr[-1]), "reps": a.reps, "fp64_vector_peak_flops": FP64_VECTOR_PEAK,
           "flop_per_projection": FLOP_PER_PROJECTION}
    refine = dict(attempts=10, rel_change=0.0, loss="cauchy", delta=2.0)
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        for fine in (None, refine):
            for H in (64, 256):
                label = f"batch_H{H}" + ("_refined" if fine else "")
                out[label] = timed(sa, LC, ba, a.reps, f0, row_ptr, point, uv, pts, K, (Rg, Tg), hypotheses=H, refine=fine)
                print(label, json.dumps(out[label]), flush=True)
            j = sc.M // 2
            o0, o1 = row_ptr[j], row_ptr[j + 1]
            for H in (256, 1024):
                label = f"one_frame_H{H}" + ("_refined" if fine else "")
                out[label] = timed(sa, LC, ba, a.reps, f0, np.array([0, o1 - o0]), point[o0:o1], uv[o0:o1], pts, K[j:j + 1], (Rg[j:j + 1], Tg[j:j + 1]),
                                   hypotheses=H, refine=fine)
                print(label, json.dumps(out[label]), flush=True)
    finally:
        ba.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
