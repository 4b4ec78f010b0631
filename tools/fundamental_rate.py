"""The two-view fundamental matrix (srk_relate_uncalibrated) timed on the shapes of tools/homography_rate.py: 1000 pairs of 2000
matches each, 2 000 000 in all.  Pair j sees 2000 general points from (I, 0) and from a motion of its own, with half a pixel of
noise in both images, and 30 % of the targets are replaced by uniform points of the frame.

Recorded per variant (64 and 256 hypotheses for the batch and for one pair of 2000 alone, each with refine_rounds 0 and 8): the
kernels' device time from the call's event pair (median of --reps), the score kernel's own time and its share, the solve kernel's
time and its share, the wall time of the call, and evaluations per second (hypotheses x matches / the score kernel's time) beside
the double-precision vector peak.  An evaluation, counted from srk_relate_sampson, srk_relate_term and the loop around them: F p_a
(three rows of three multiplies and two additions, 15 flop), two entries of F^T p_b (10), e = p_b . l (5), e e (1), the denominator
(four multiplies and three additions, 7), one division (counted apart), q s (1) and the truncated sum with its count (2): 41 flop
and one division, so the peak in evaluations is at most the flop peak / 41.  For comparison k_relate_score (the same evaluation)
and k_homog_score (48 flop and two divisions, tools/homography_rate.py) on the same matches, in the same run.  One JSON object to
--out.

    python tools/fundamental_rate.py [--reps 7] [--out profiles/fundamental/fundamental_rate.json]
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
FLOP_PER_EVALUATION = 41     # and one division
FLOP_PER_HOMOGRAPHY_EVALUATION = 48
F0, TAU = 600.0, 2.0
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
    X = np.stack([rng.uniform(-2, 2, (n, per)), rng.uniform(-1.5, 1.5, (n, per)), rng.uniform(4.0, 8.0, (n, per))], -1)
    Y = np.einsum("nij,npj->npi", R, X) + T[:, None, :]
    ua = pixels(KA, X).reshape(-1, 2) + 0.5 * rng.normal(size=(n * per, 2))
    ub = pixels(KB, Y).reshape(-1, 2) + 0.5 * rng.normal(size=(n * per, 2))
    moved = rng.random(n * per) < 0.3
    ub[moved] = np.column_stack([rng.uniform(-100, 700, moved.sum()), rng.uniform(-150, 600, moved.sum())])
    Tx = np.zeros((n, 3, 3))
    Tx[:, 0, 1], Tx[:, 0, 2], Tx[:, 1, 0], Tx[:, 1, 2], Tx[:, 2, 0], Tx[:, 2, 1] = -T[:, 2], T[:, 1], T[:, 2], -T[:, 0], -T[:, 1], T[:, 0]
    F = np.linalg.inv(KB).T @ (Tx @ R) @ np.linalg.inv(KA)
    F /= np.linalg.norm(F, axis=(1, 2))[:, None, None]
    return ua, ub, moved, F


def distance_to_truth(F, F0_):
    """per pair, the smaller of |F - F_true| and |F + F_true| (largest entry)"""
    return np.minimum(np.abs(F - F0_).max(axis=(1, 2)), np.abs(F + F0_).max(axis=(1, 2)))


def timed(sa, FD, ba, reps, row_ptr, ua, ub, moved, Ft, **kw):
    run = lambda: sa.relate_uncalibrated(ba, F0, row_ptr, ua, ub, inlier_pixels=TAU, want_inliers=True, **kw)  # noqa: E731
    run()                                                       # warm-up: allocations, code objects
    dev, score, solve, wall = [], [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = run()
        wall.append(1e3 * (time.perf_counter() - t0))
        ms = FD.last_kernel_ms(ba)
        dev.append(ms[0])
        score.append(ms[1])
        solve.append(FD.last_solve_ms(ba))
    ms, sms, vms, O = float(np.median(dev)), float(np.median(score)), float(np.median(solve)), int(row_ptr[-1])
    rate = kw["hypotheses"] * O / (1e-3 * sms)
    flags = res.inliers.astype(bool)
    return {"kernel_ms": ms, "score_kernel_ms": sms, "score_share": sms / ms, "solve_kernel_ms": vms, "solve_share": vms / ms,
            "call_ms": float(np.median(wall)), "evaluations_per_s": rate, "share_of_fp64_vector_peak": rate * FLOP_PER_EVALUATION / FP64_VECTOR_PEAK,
            "pairs_without_model": int(np.count_nonzero(res.status)), "unmoved_flagged": float(flags[~moved].mean()),
            "moved_flagged": float(flags[moved].mean()), "median_attempts_used": float(np.median(res.fund[:, 7])),
            "median_attempts_accepted": float(np.median(res.fund[:, 6])), "median_entry_distance_to_truth": float(np.median(distance_to_truth(res.F, Ft))),
            "median_inlier_rms_pixels": float(np.nanmedian(res.fund[:, 8])), "median_cond_1": float(np.nanmedian(res.fund[:, 10])),
            "winners_with_three_roots": int(np.count_nonzero(res.fund[:, 11] == 3))}


def other_timed(call, last_ms, reps, hypotheses, O, flop):
    call()
    score = []
    for _ in range(reps):
        call()
        score.append(last_ms()[1])
    sms = float(np.median(score))
    rate = hypotheses * O / (1e-3 * sms)
    return {"score_kernel_ms": sms, "evaluations_per_s": rate, "share_of_fp64_vector_peak": rate * flop / FP64_VECTOR_PEAK}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--matches", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fundamental", "fundamental_rate.json"))
    a = ap.parse_args()
    import surikatoko_amd as sa
    from surikatoko_amd import fundamental as FD
    from surikatoko_amd import homography as HG
    from surikatoko_amd import relate as RL
    n, per = a.pairs, a.matches
    rng = np.random.default_rng(28)
    ua, ub, moved, Ft = workload(n, per, rng)
    row_ptr = per * np.arange(n + 1, dtype=np.int64)
    O = n * per
    out = {"scene": "pairs of matches on general points, half a pixel of noise, 30 % of the targets replaced", "n_pairs": n, "n_matches": O,
           "reps": a.reps, "fp64_vector_peak_flops": FP64_VECTOR_PEAK, "flop_per_evaluation": FLOP_PER_EVALUATION, "divisions_per_evaluation": 1,
           "flop_per_homography_evaluation": FLOP_PER_HOMOGRAPHY_EVALUATION, "inlier_pixels": TAU}
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        one = np.array([0, per], np.int64)
        for rounds in (0, 8):
            for H in (64, 256):
                label = f"batch_H{H}_rounds{rounds}"
                out[label] = timed(sa, FD, ba, a.reps, row_ptr, ua, ub, moved, Ft, hypotheses=H, refine_rounds=rounds)
                print(label, json.dumps(out[label]), flush=True)
                label = f"one_pair_H{H}_rounds{rounds}"
                out[label] = timed(sa, FD, ba, a.reps, one, ua[:per], ub[:per], moved[:per], Ft[:1], hypotheses=H, refine_rounds=rounds)
                print(label, json.dumps(out[label]), flush=True)
        for H in (64, 256):
            out[f"relate_batch_H{H}"] = other_timed(lambda: sa.relate_frames(ba, F0, row_ptr, ua, ub, KA, KB, hypotheses=H, inlier_pixels=TAU),
                                                    lambda: RL.last_kernel_ms(ba), a.reps, H, O, FLOP_PER_EVALUATION)
            print(f"relate_batch_H{H}", json.dumps(out[f"relate_batch_H{H}"]), flush=True)
            out[f"homography_batch_H{H}"] = other_timed(lambda: sa.relate_homography(ba, F0, row_ptr, ua, ub, KA, KB, hypotheses=H, inlier_pixels=6.0,
                                                                                     refine_rounds=0),
                                                        lambda: HG.last_kernel_ms(ba), a.reps, H, O, FLOP_PER_HOMOGRAPHY_EVALUATION)
            print(f"homography_batch_H{H}", json.dumps(out[f"homography_batch_H{H}"]), flush=True)
    finally:
        ba.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
