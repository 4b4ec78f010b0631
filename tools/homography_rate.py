"""The two-view homography (srk_relate_homography) timed on the shapes of tools/align_rate.py: 1000 pairs of 2000 matches each,
2 000 000 in all.  Pair j sees 2000 points of the plane z = 6 + 0.2 x - 0.1 y from (I, 0) and from a motion of its own, with one
pixel of noise in both images, and 30 % of the targets are replaced by uniform points of the frame.

Recorded per variant (64 and 256 hypotheses for the batch and for one pair of 2000 alone, each with refine_rounds 0 and 4): the
kernels' device time from the call's event pair (median of --reps), the hypothesis-and-score kernel's own time and its share, the
wall time of the call, and evaluations per second (hypotheses x matches / the score kernel's time) beside the double-precision
vector peak.  An evaluation, counted from srk_homog_term and the loop around it: G p_a and Gi p_b (2 x 3 rows of three multiplies
and two additions, 30 flop), the two quotients f0 / y_3 and f0 / x_3 (two divisions, counted apart), the four residuals (a multiply
and a subtraction each, 8), s (four multiplies and three additions, 7), q s (1) and the two truncated sums (2): 48 flop and two
divisions, so the peak in evaluations is at most the flop peak / 48.  For comparison k_align_score (29 flop, tools/align_rate.py) on
3D correspondences of the same shapes and k_relate_score on the same matches, in the same run.  One JSON object to --out.

    python tools/homography_rate.py [--reps 7] [--out profiles/homography/homography_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_VECTOR_PEAK = 78.6e12   # flop / s: half the 157.3 TFLOPS single-precision vector peak of the MI355X data sheet
FLOP_PER_EVALUATION = 48     # and two divisions
FLOP_PER_ALIGN_EVALUATION = 29
F0, TAU = 600.0, 6.0
KA = np.array([[1.25, 0.0, 0.53], [0.0, 1.3, 0.4], [0.0, 0.0, 1.0]])
KB = np.array([[1.1, 0.01, 0.5], [0.0, 1.15, 0.42], [0.0, 0.0, 1.0]])


def rotations(rng, n, angle):
    w = rng.normal(size=(n, 3))
    w *= (rng.uniform(0.01, angle, n) / np.linalg.norm(w, axis=1))[:, None]
    th = np.linalg.norm(w, axis=1)[:, None, None]
    k = np.zeros((n, 3, 3))
    k[:, 0, 1], k[:, 0, 2], k[:, 1, 0], k[:, 1, 2], k[:, 2, 0], k[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    k /= th
    return np.eye(3) + np.sin(th) * k + (1.0 - np.cos(th)) * (k @ k)


def pixels(K, x):
    p = x @ K.T
    return F0 * p[..., :2] / p[..., 2:3]


def workload(n, per, rng):
    R = rotations(rng, n, 0.3)
    T = rng.normal(size=(n, 3))
    T /= np.linalg.norm(T, axis=1)[:, None]
    X = np.stack([rng.uniform(-2, 2, (n, per)), rng.uniform(-1.5, 1.5, (n, per)), np.zeros((n, per))], -1)
    X[..., 2] = 6.0 + 0.2 * X[..., 0] - 0.1 * X[..., 1]
    Y = np.einsum("nij,npj->npi", R, X) + T[:, None, :]
    ua = pixels(KA, X).reshape(-1, 2) + rng.normal(size=(n * per, 2))
    ub = pixels(KB, Y).reshape(-1, 2) + rng.normal(size=(n * per, 2))
    moved = rng.random(n * per) < 0.3
    ub[moved] = np.column_stack([rng.uniform(-100, 700, moved.sum()), rng.uniform(-150, 600, moved.sum())])
    N = np.array([-0.2, 0.1, 1.0])
    G = KB @ (R + T[:, :, None] * N[None, None, :] / 6.0) @ np.linalg.inv(KA)
    return ua, ub, moved, G, X.reshape(-1, 3), Y.reshape(-1, 3)


def corner_distance(G, G0):
    c = np.array([[0.0, 0.0, F0], [640.0, 0.0, F0], [0.0, 480.0, F0], [640.0, 480.0, F0]])
    a, b = c @ np.swapaxes(G, 1, 2), c @ np.swapaxes(G0, 1, 2)
    return np.sqrt(((F0 * a[..., :2] / a[..., 2:3] - F0 * b[..., :2] / b[..., 2:3]) ** 2).sum(-1)).max(-1)


def timed(sa, HG, ba, reps, row_ptr, ua, ub, moved, G, **kw):
    run = lambda: sa.relate_homography(ba, F0, row_ptr, ua, ub, KA, KB, inlier_pixels=TAU, want_inliers=True, **kw)  # noqa: E731
    run()                                                       # warm-up: allocations, code objects
    dev, score, wall = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = run()
        wall.append(1e3 * (time.perf_counter() - t0))
        ms = HG.last_kernel_ms(ba)
        dev.append(ms[0])
        score.append(ms[1])
    ms, sms, O = float(np.median(dev)), float(np.median(score)), int(row_ptr[-1])
    rate = kw["hypotheses"] * O / (1e-3 * sms)
    flags = res.inliers.astype(bool)
    return {"kernel_ms": ms, "score_kernel_ms": sms, "score_share": sms / ms, "call_ms": float(np.median(wall)), "evaluations_per_s": rate,
            "share_of_fp64_vector_peak": rate * FLOP_PER_EVALUATION / FP64_VECTOR_PEAK, "pairs_without_model": int(np.count_nonzero(res.status)),
            "unmoved_flagged": float(flags[~moved].mean()), "moved_flagged": float(flags[moved].mean()),
            "median_rounds": float(np.median(res.homog[:, 5])), "median_corner_pixels_to_truth": float(np.median(corner_distance(res.G, G))),
            "median_inlier_rms_pixels": float(np.nanmedian(res.homog[:, 7])), "pairs_with_two_poses": int(np.count_nonzero(res.n_poses == 2))}


def other_timed(call, last_ms, reps, hypotheses, O, flop):
    call()
    score = []
    for _ in range(reps):
        call()
        score.append(last_ms()[1])
    sms = float(np.median(score))
    out = {"score_kernel_ms": sms, "evaluations_per_s": hypotheses * O / (1e-3 * sms)}
    if flop:
        out["share_of_fp64_vector_peak"] = out["evaluations_per_s"] * flop / FP64_VECTOR_PEAK
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--matches", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography", "homography_rate.json"))
    a = ap.parse_args()
    import surikatoko_amd as sa
    from surikatoko_amd import align as AL
    from surikatoko_amd import homography as HG
    from surikatoko_amd import relate as RL
    n, per = a.pairs, a.matches
    rng = np.random.default_rng(27)
    ua, ub, moved, G, X, Y = workload(n, per, rng)
    row_ptr = per * np.arange(n + 1, dtype=np.int64)
    O = n * per
    out = {"scene": "pairs of matches on the plane z = 6 + 0.2 x - 0.1 y, one pixel of noise, 30 % of the targets replaced", "n_pairs": n,
           "n_matches": O, "reps": a.reps, "fp64_vector_peak_flops": FP64_VECTOR_PEAK, "flop_per_evaluation": FLOP_PER_EVALUATION,
           "divisions_per_evaluation": 2, "flop_per_align_evaluation": FLOP_PER_ALIGN_EVALUATION, "inlier_pixels": TAU}
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        one = np.array([0, per], np.int64)
        for rounds in (0, 4):
            for H in (64, 256):
                label = f"batch_H{H}_rounds{rounds}"
                out[label] = timed(sa, HG, ba, a.reps, row_ptr, ua, ub, moved, G, hypotheses=H, refine_rounds=rounds)
                print(label, json.dumps(out[label]), flush=True)
                label = f"one_pair_H{H}_rounds{rounds}"
                out[label] = timed(sa, HG, ba, a.reps, one, ua[:per], ub[:per], moved[:per], G[:1], hypotheses=H, refine_rounds=rounds)
                print(label, json.dumps(out[label]), flush=True)
        Ym = Y + moved[:, None] * rng.uniform(1.0, 3.0, (O, 3))     # align's workload on the same shapes: 30 % moved as well
        for H in (64, 256):
            out[f"align_batch_H{H}"] = other_timed(lambda: sa.align_points(ba, row_ptr, X, Ym, hypotheses=H, inlier_distance=0.05, refine_rounds=0),
                                                   lambda: AL.last_kernel_ms(ba), a.reps, H, O, FLOP_PER_ALIGN_EVALUATION)
            print(f"align_batch_H{H}", json.dumps(out[f"align_batch_H{H}"]), flush=True)
            out[f"relate_batch_H{H}"] = other_timed(lambda: sa.relate_frames(ba, F0, row_ptr, ua, ub, KA, KB, hypotheses=H, inlier_pixels=4.0),
                                                    lambda: RL.last_kernel_ms(ba), a.reps, H, O, 0)
            print(f"relate_batch_H{H}", json.dumps(out[f"relate_batch_H{H}"]), flush=True)
    finally:
        ba.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
