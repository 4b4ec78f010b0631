"""Map alignment (srk_align_points) timed on the landmarks of the benchmark scene C3 (100 000 landmarks): 1000 sets of 2000
correspondences each, 2 000 000 in all.  Set j holds the landmarks C3's frame j sees; their targets are the landmarks under a
random similarity of the set's own (scale 0.5 .. 2) with 0.01 of noise, and 30 % of the targets are replaced (moved by 20 .. 200
tau, tau = 0.05).

Recorded per variant (64 and 256 hypotheses for the batch, 256 and 1024 for one set alone, each with refine_rounds 0 and 2): the
kernels' device time from the call's event pair (median of --reps), the hypothesis-and-score kernel's own time and its share, the
wall time of the call, and evaluations per second (hypotheses x correspondences / the score kernel's time) beside the
double-precision vector peak.  An evaluation, counted from srk_align_term and the loop around it: three rows of s R a + t and the
subtraction from b (3 x 7 flop: a multiply and two multiply-adds, the addition of t, the subtraction), r^2 (a multiply and two
multiply-adds, 5), q r^2 (1) and the two truncated sums (2): 29 flop and no division, so the peak in evaluations is the flop peak
/ 29.  The yardstick is k_locate_score on the same shapes in the same run (35 flop and a division per projection,
tools/locate_rate.py): its projections per second are recorded beside.  One JSON object to --out.

    python tools/align_rate.py [--reps 7] [--out profiles/align/align_rate.json]
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
FLOP_PER_EVALUATION = 29
FLOP_PER_PROJECTION = 35     # tools/locate_rate.py
TAU, NOISE = 0.05, 0.01


def rotations(rng, n):
    q = rng.normal(size=(n, 4))
    w, x, y, z = (q / np.linalg.norm(q, axis=1)[:, None]).T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)


def timed(sa, AL, ba, reps, row_ptr, a, b, truth, **kw):
    sa.align_points(ba, row_ptr, a, b, inlier_distance=TAU, **kw)   # warm-up: allocations, code objects
    dev, score, wall = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = sa.align_points(ba, row_ptr, a, b, inlier_distance=TAU, **kw)
        wall.append(1e3 * (time.perf_counter() - t0))
        ms = AL.last_kernel_ms(ba)
        dev.append(ms[0])
        score.append(ms[1])
    ms, sms, O = float(np.median(dev)), float(np.median(score)), int(row_ptr[-1])
    rate = kw["hypotheses"] * O / (1e-3 * sms)
    s, R, t = truth
    angle = np.arccos(np.clip((np.einsum("nij,nij->n", res.R, R) - 1.0) / 2.0, -1.0, 1.0))
    return {"kernel_ms": ms, "score_kernel_ms": sms, "score_share": sms / ms, "call_ms": float(np.median(wall)), "evaluations_per_s": rate,
            "share_of_fp64_vector_peak": rate * FLOP_PER_EVALUATION / FP64_VECTOR_PEAK, "sets_not_aligned": int(np.count_nonzero(res.status)),
            "median_inlier_share": float(np.median(res.aligned[:, 2] / np.maximum(res.aligned[:, 1], 1))),
            "median_rounds": float(np.median(res.aligned[:, 5])), "median_rotation_error_rad": float(np.median(angle)),
            "median_scale_error": float(np.median(np.abs(res.s / s - 1.0))), "median_inlier_rms": float(np.nanmedian(res.aligned[:, 7]))}


def locate_timed(sa, LC, ba, reps, f0, row_ptr, point, uv, X, K, hypotheses):
    sa.locate_frames(ba, f0, row_ptr, point, uv, X, K, hypotheses=hypotheses)
    score = []
    for _ in range(reps):
        sa.locate_frames(ba, f0, row_ptr, point, uv, X, K, hypotheses=hypotheses)
        score.append(LC.last_kernel_ms(ba)[1])
    sms = float(np.median(score))
    rate = hypotheses * int(row_ptr[-1]) / (1e-3 * sms)
    return {"score_kernel_ms": sms, "projections_per_s": rate, "share_of_fp64_vector_peak": rate * FLOP_PER_PROJECTION / FP64_VECTOR_PEAK}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align", "align_rate.json"))
    a = ap.parse_args()
    import surikatoko_amd as sa
    from surikatoko_amd import align as AL
    from surikatoko_amd import locate as LC
    from resect_rate import frames_of_c3
    sc, f0, row_ptr, point, uv, pts, K = frames_of_c3(sa)
    n, O = len(row_ptr) - 1, int(row_ptr[-1])
    rng = np.random.default_rng(12)
    s, R, t = rng.uniform(0.5, 2.0, n), rotations(rng, n), rng.uniform(-3, 3, (n, 3))
    of = np.repeat(np.arange(n), np.diff(row_ptr))
    src = np.ascontiguousarray(pts[point])
    dst = s[of, None] * np.einsum("oij,oj->oi", R[of], src) + t[of] + NOISE * rng.normal(size=(O, 3))
    moved = rng.random(O) < 0.3
    d = rng.normal(size=(O, 3))
    dst += moved[:, None] * d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(20 * TAU, 200 * TAU, O)[:, None]
    uvm = uv + (rng.random(len(uv)) < 0.3)[:, None] * rng.uniform(20, 60, (len(uv), 2))     # locate's workload: 30 % moved as well
    out = {"scene": "C3_1kcam_100kpt landmarks, one set per C3 frame under a similarity of its own, 30 % of the targets replaced", "n_sets": n,
           "n_landmarks": int(sc.N), "n_correspondences": O, "reps": a.reps, "fp64_vector_peak_flops": FP64_VECTOR_PEAK,
           "flop_per_evaluation": FLOP_PER_EVALUATION, "flop_per_projection": FLOP_PER_PROJECTION, "inlier_distance": TAU, "noise": NOISE}
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        j = n // 2
        o0, o1 = row_ptr[j], row_ptr[j + 1]
        one = np.array([0, o1 - o0])
        for rounds in (0, 2):
            for H in (64, 256):
                label = f"batch_H{H}_rounds{rounds}"
                out[label] = timed(sa, AL, ba, a.reps, row_ptr, src, dst, (s, R, t), hypotheses=H, refine_rounds=rounds)
                print(label, json.dumps(out[label]), flush=True)
            for H in (256, 1024):
                label = f"one_set_H{H}_rounds{rounds}"
                out[label] = timed(sa, AL, ba, a.reps, one, src[o0:o1], dst[o0:o1], (s[j:j + 1], R[j:j + 1], t[j:j + 1]), hypotheses=H, refine_rounds=rounds)
                print(label, json.dumps(out[label]), flush=True)
        for H in (64, 256):                                       # the yardstick: k_locate_score on the same shapes
            out[f"locate_batch_H{H}"] = locate_timed(sa, LC, ba, a.reps, f0, row_ptr, point, uvm, pts, K, H)
            print(f"locate_batch_H{H}", json.dumps(out[f"locate_batch_H{H}"]), flush=True)
        for H in (256, 1024):
            out[f"locate_one_frame_H{H}"] = locate_timed(sa, LC, ba, a.reps, f0, one, point[o0:o1], uvm[o0:o1], pts, K[j:j + 1], H)
            print(f"locate_one_frame_H{H}", json.dumps(out[f"locate_one_frame_H{H}"]), flush=True)
    finally:
        ba.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
