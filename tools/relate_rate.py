"""Two-view relative pose (srk_relate_frames) timed on a synthetic batch: 1000 pairs of 2000 matches each (2 000 000 matches), every
pair with its own motion (rotations up to 0.3 rad, a unit baseline against depths of 4 to 8), one pixel of noise, 30 % of the
matches replaced by uniform points.

Recorded per variant (64 and 256 hypotheses for the batch, 256 and 1024 for one pair alone): the kernels' device time from the
call's event pair (median of --reps), the score kernel's own time from the second pair, the rest (gather, the five-point solve
and the pick: the solve but for two short kernels) and its share, the wall time of the call with its uploads, and Sampson
evaluations per second (hypotheses x matches / score time) beside the double-precision vector peak.  A Sampson evaluation is 9
multiply-adds for F p_a, 6 for two rows of F^T p_b, 3 for the residual, 4 for the denominator, a division and 4 more operations
for the weight, the truncation and the sum: about 50 flop, so the peak in evaluations is the flop peak / 50.  One JSON object to
--out.

    python tools/relate_rate.py [--reps 7] [--out profiles/relate/relate_rate.json]
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
FLOP_PER_SAMPSON = 50
F0 = 600.0
K = np.array([[1.25, 0.0, 0.53], [0.0, 1.3, 0.4], [0.0, 0.0, 1.0]])


def rotations(w):
    """Rodrigues, batched: w [n][3]"""
    th = np.linalg.norm(w, axis=1)[:, None, None]
    k = w / np.linalg.norm(w, axis=1, keepdims=True)
    kx = np.zeros((len(w), 3, 3))
    kx[:, 0, 1], kx[:, 0, 2], kx[:, 1, 0], kx[:, 1, 2], kx[:, 2, 0], kx[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3) + np.sin(th) * kx + (1.0 - np.cos(th)) * (kx @ kx)


def batch(n_pairs, n_matches, rng, share=0.3, sigma=1.0):
    w = rng.normal(size=(n_pairs, 3))
    R = rotations(w / np.linalg.norm(w, axis=1, keepdims=True) * rng.uniform(0.01, 0.3, (n_pairs, 1)))
    T = rng.normal(size=(n_pairs, 3))
    T /= np.linalg.norm(T, axis=1, keepdims=True)
    X = np.stack([rng.uniform(-2.0, 2.0, (n_pairs, n_matches)), rng.uniform(-1.5, 1.5, (n_pairs, n_matches)), rng.uniform(4.0, 8.0, (n_pairs, n_matches))], axis=2)

    def pixels(x):
        p = x @ K.T
        return F0 * p[..., :2] / p[..., 2:3]
    ua = pixels(X) + sigma * rng.normal(size=(n_pairs, n_matches, 2))
    ub = pixels(np.einsum("nij,nmj->nmi", R, X) + T[:, None, :]) + sigma * rng.normal(size=(n_pairs, n_matches, 2))
    moved = rng.random((n_pairs, n_matches)) < share
    ub[moved] = np.column_stack([rng.uniform(-100.0, 700.0, moved.sum()), rng.uniform(-150.0, 600.0, moved.sum())])
    return np.arange(n_pairs + 1, dtype=np.int64) * n_matches, ua.reshape(-1, 2), ub.reshape(-1, 2), R, T, moved.reshape(-1)


def timed(sa, RL, ba, reps, row_ptr, ua, ub, truth, moved, **kw):
    sa.relate_frames(ba, F0, row_ptr, ua, ub, K, K, **kw)   # warm-up: allocations, code objects
    dev, score, wall = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = sa.relate_frames(ba, F0, row_ptr, ua, ub, K, K, want_inliers=True, **kw)
        wall.append(1e3 * (time.perf_counter() - t0))
        ms = RL.last_kernel_ms(ba)
        dev.append(ms[0])
        score.append(ms[1])
    ms, sms, O = float(np.median(dev)), float(np.median(score)), int(row_ptr[-1])
    rate = kw["hypotheses"] * O / (1e-3 * sms)
    Rt, Tt = truth
    rot = np.arccos(np.clip(0.5 * (np.einsum("nij,nij->n", res.R, Rt) - 1.0), -1.0, 1.0))
    direction = np.arccos(np.clip(np.einsum("ni,ni->n", res.T, Tt), -1.0, 1.0))
    return {"kernel_ms": ms, "score_kernel_ms": sms, "solve_and_rest_ms": ms - sms, "solve_share": (ms - sms) / ms, "call_ms": float(np.median(wall)),
            "sampson_per_s": rate, "share_of_fp64_vector_peak": rate * FLOP_PER_SAMPSON / FP64_VECTOR_PEAK,
            "pairs_not_related": int(np.count_nonzero(res.status)), "median_inlier_share": float(np.median(res.related[:, 2] / np.maximum(res.related[:, 1], 1))),
            "moved_among_inliers": float(res.inliers[moved].mean()), "median_rotation_error_rad": float(np.median(rot)),
            "median_direction_error_rad": float(np.median(direction)), "median_models_per_hypothesis": float(np.median(res.related[:, 4]) / kw["hypotheses"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--matches", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relate", "relate_rate.json"))
    a = ap.parse_args()
    import surikatoko_amd as sa
    from surikatoko_amd import relate as RL
    rng = np.random.default_rng(24)
    row_ptr, ua, ub, R, T, moved = batch(a.pairs, a.matches, rng)
    out = {"scene": "synthetic pairs, one pixel of noise, 30 % of the matches replaced", "n_pairs": a.pairs, "n_matches": int(row_ptr[-1]), "reps": a.reps,
           "inlier_pixels": 4.0, "fp64_vector_peak_flops": FP64_VECTOR_PEAK, "flop_per_sampson": FLOP_PER_SAMPSON}
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        for H in (64, 256):
            out[f"batch_H{H}"] = timed(sa, RL, ba, a.reps, row_ptr, ua, ub, (R, T), moved, hypotheses=H, inlier_pixels=4.0)
            print(f"batch_H{H}", json.dumps(out[f"batch_H{H}"]), flush=True)
        j = a.pairs // 2
        s = slice(int(row_ptr[j]), int(row_ptr[j + 1]))
        for H in (256, 1024):
            out[f"one_pair_H{H}"] = timed(sa, RL, ba, a.reps, np.array([0, a.matches]), ua[s], ub[s], (R[j:j + 1], T[j:j + 1]), moved[s], hypotheses=H,
                                          inlier_pixels=4.0)
            print(f"one_pair_H{H}", json.dumps(out[f"one_pair_H{H}"]), flush=True)
    finally:
        ba.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
