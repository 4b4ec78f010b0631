"""Batched camera resection (srk_resect_frames) timed on the landmarks of the benchmark scene C3 (100 000 landmarks) with 1000
extra frames of 2000 observations each: frame j sees what C3's frame j sees, the ground-truth landmark projected into the
ground-truth camera with 0.3 px of noise, and starts from the scene's noisy camera.  Beside it the only route callers had before
it: the same frames uploaded into a scene with every landmark constant (set_constant_blocks, fixed intrinsics, keep_gauge=False)
and optimised.

Recorded per variant (0, 5 and 10 attempts at rel_change 0, so every attempt runs; without a loss and with Huber at 2 px): the
kernels' device time from the call's event pair (median of --reps), the wall time of the call (uploads of the observations and
landmarks and download of the results included), observations per second and walk (an attempt walks the frame once, the start is
one more walk).  The same for one frame alone: the tracking case, at latency scale.  One JSON object to --out.

    python tools/resect_rate.py [--reps 7] [--out profiles/resect/resect_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frames_of_c3(sa):
    """CSR by frame over C3's observations: (row_ptr, point, uv from the ground truth + 0.3 px), the ground-truth landmarks"""
    sc, pts, Rg, Tg = sa.config_scene("C3_1kcam_100kpt", with_gt=True)
    f0 = sa.CONFIGS["C3_1kcam_100kpt"].f0
    lm = np.repeat(np.arange(sc.N), np.diff(sc.row_ptr))
    order = np.argsort(sc.obs_frame, kind="stable")
    frame, point = sc.obs_frame[order], lm[order].astype(np.int32)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(frame, minlength=sc.M))]).astype(np.int64)
    K = np.asarray(sc.K, np.float64).reshape(-1, 3, 3)
    h = np.einsum("nij,nj->ni", K[frame], np.einsum("nij,nj->ni", Rg.reshape(-1, 3, 3)[frame], pts[point]) + Tg.reshape(-1, 3)[frame])
    uv = f0 * h[:, :2] / h[:, 2:] + 0.3 * np.random.default_rng(9).normal(size=(len(frame), 2))
    return sc, f0, row_ptr, point, uv, pts, K


def timed(sa, RS, ba, reps, f0, row_ptr, point, uv, X, K, R0, T0, **kw):
    sa.resect_frames(ba, f0, row_ptr, point, uv, X, K, R0, T0, **kw)   # warm-up: allocations, code objects
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        R, T, quality, info, status = sa.resect_frames(ba, f0, row_ptr, point, uv, X, K, R0, T0, **kw)
        wall.append(1e3 * (time.perf_counter() - t0))
        dev.append(RS.last_kernel_ms(ba))
    ms, O, walks = float(np.median(dev)), int(row_ptr[-1]), kw["attempts"] + 1
    return {"kernel_ms": ms, "call_ms": float(np.median(wall)), "observations_per_s_and_walk": O * walks / (1e-3 * ms),
            "median_rms_pixels": float(np.nanmedian(quality[:, 0])), "frames_flagged": int(np.count_nonzero(status & ~np.uint32(8)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resect", "resect_rate.json"))
    a = ap.parse_args()
    import surikatoko_amd as sa
    from surikatoko_amd import resect as RS
    sc, f0, row_ptr, point, uv, pts, K = frames_of_c3(sa)
    R0, T0 = sc.cam_R.reshape(-1, 3, 3), sc.cam_T.reshape(-1, 3)
    out = {"scene": "C3_1kcam_100kpt landmarks, one extra frame per C3 frame", "n_frames": int(sc.M), "n_landmarks": int(sc.N),
           "n_observations": int(row_ptr[-1]), "observations_per_frame": [int(np.diff(row_ptr).min()), int(np.diff(row_ptr).max())], "reps": a.reps}
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        for loss in (None, "huber"):
            for attempts in (0, 5, 10):
                kw = dict(attempts=attempts, rel_change=0.0, loss=loss, delta=2.0 if loss else None)
                label = f"attempts{attempts}" + ("_huber" if loss else "")
                out[label] = timed(sa, RS, ba, a.reps, f0, row_ptr, point, uv, pts, K, R0, T0, **kw)
                j = sc.M // 2
                o0, o1 = row_ptr[j], row_ptr[j + 1]
                out[label + "_one_frame"] = timed(sa, RS, ba, a.reps, f0, np.array([0, o1 - o0]), point[o0:o1], uv[o0:o1], pts, K[j:j + 1], R0[j:j + 1],
                                                  T0[j:j + 1], **kw)
                print(label, json.dumps(out[label]), json.dumps(out[label + "_one_frame"]), flush=True)
    finally:
        ba.close()
    # the existing way: the same frames as a scene whose landmarks are all constant, optimised (10 LM iterations at most)
    g = sa.BundleAdjustmentKanatani(0)
    try:
        t0 = time.perf_counter()
        fixed = sa.Scene(pts, sc.cam_R, sc.cam_T, sc.K, sc.shared_k, sc.row_ptr, sc.obs_frame, uv[np.argsort(np.argsort(sc.obs_frame, kind="stable"))])
        g.set_fixed_intrinsics(True)
        g.set_constant_blocks(points=np.ones(sc.N, bool), keep_gauge=False, n_frames=sc.M, n_points=sc.N)
        t1 = time.perf_counter()
        assert g.upload(f0, fixed)
        t2 = time.perf_counter()
        g.optimize(max_iterations=10)
        t3 = time.perf_counter()
        r = g.report
        out["scene_with_constant_landmarks"] = {"host_scene_ms": 1e3 * (t1 - t0), "upload_and_plan_ms": 1e3 * (t2 - t1), "optimize_ms": 1e3 * (t3 - t2),
                                                "iterations": int(r.iterations), "attempts": int(r.attempts)}
        out["ratio_optimize_over_call_10_attempts"] = out["scene_with_constant_landmarks"]["optimize_ms"] / out["attempts10"]["call_ms"]
        out["ratio_upload_plan_optimize_over_call_10_attempts"] = (1e3 * (t3 - t1)) / out["attempts10"]["call_ms"]
        print(json.dumps(out["scene_with_constant_landmarks"]), flush=True)
    finally:
        g.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
