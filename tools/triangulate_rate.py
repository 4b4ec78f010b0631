"""Batched triangulation (srk_triangulate_tracks) timed on the tracks of the benchmark scenes (C3: 100 000 tracks / 2 000 000
observations of 20 views each; the same cameras with tracks of 8 to 32 views, C3_ragged_8to32; C1: 4983 / 16432), beside the
only route callers had before it: a host loop over srk_triangulate_least_squares with caller-built K [R | T] per observation
(timed on a sample of tracks, scaled to the whole batch).

Per config: linear only, linear plus 5 refinement attempts (refine_rel_change = 0, so every attempt runs), with and without
information weights.  Recorded: the kernels' device time from the call's event pair (median of --reps), the wall time of the
call (uploads of the tracks and download of the results included), observations / s on the device time and the fraction of the
HBM peak (8 TB/s) on the algorithmic bytes: 16 B uv + 4 B frame (+ 8 B q) an observation, 24 B X + 32 B quality + 4 B status and
8 B row_ptr a track, the poses (72 + 24 + 72 B a frame) counted once.  One JSON line per config, all of them to --out.

    python tools/triangulate_rate.py [--configs C1_dino_standin,C3_1kcam_100kpt,C3_ragged_8to32] [--reps 7] [--out profiles/triangulate/triangulate_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes / s


def ragged_c3(sa):
    """C3's cameras and landmarks with 100 000 tracks of 8 to 32 consecutive views (2 000 000 observations on average): the
    ground-truth landmark projected into the ground-truth cameras, 0.3 px of noise; triangulated over the scene's noisy cameras"""
    from types import SimpleNamespace
    sc, pts, Rg, Tg = sa.config_scene("C3_1kcam_100kpt", with_gt=True)
    rng = np.random.default_rng(8)
    L = rng.integers(8, 33, sc.N)
    row_ptr = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
    first = np.minimum(sc.obs_frame[sc.row_ptr[:-1]], sc.M - L)
    frame = (np.repeat(first, L) + np.arange(row_ptr[-1]) - np.repeat(row_ptr[:-1], L)).astype(np.int32)
    X = np.repeat(pts, L, axis=0)
    Rf, Tf, Kf = Rg.reshape(-1, 3, 3)[frame], Tg.reshape(-1, 3)[frame], np.asarray(sc.K, np.float64).reshape(-1, 3, 3)[frame]
    h = np.einsum("nij,nj->ni", Kf, np.einsum("nij,nj->ni", Rf, X) + Tf)
    uv = sa.CONFIGS["C3_1kcam_100kpt"].f0 * h[:, :2] / h[:, 2:] + 0.3 * rng.normal(size=(len(frame), 2))
    return SimpleNamespace(N=sc.N, M=sc.M, row_ptr=row_ptr, obs_frame=frame, obs_uv=uv, cam_R=sc.cam_R, cam_T=sc.cam_T, K=sc.K)


def one(sa, name, reps, sample):
    from surikatoko_amd import io as sio
    from surikatoko_amd import triangulate as T
    spec = sa.CONFIGS["C3_1kcam_100kpt" if name == "C3_ragged_8to32" else name]
    f0 = 600.0 if name == "C1_dino_standin" else spec.f0
    sc = ragged_c3(sa) if name == "C3_ragged_8to32" else sa.config_scene(name)
    R, Tt, K = sc.cam_R.reshape(-1, 3, 3), sc.cam_T.reshape(-1, 3), np.asarray(sc.K, np.float64).reshape(-1, 3, 3)
    n, O, M = sc.N, int(sc.row_ptr[-1]), sc.M
    q = np.random.default_rng(0).uniform(0.5, 2.0, O)
    ba = sa.BundleAdjustmentKanatani(0)
    out = {"config": name, "n_tracks": int(n), "n_observations": O, "n_frames": int(M), "longest_track": int(np.diff(sc.row_ptr).max()), "reps": reps,
           "hbm_peak_bytes_per_s": HBM_PEAK}
    try:
        for label, w, attempts in (("linear", None, 0), ("linear_q", q, 0), ("refine5", None, 5), ("refine5_q", q, 5)):
            args = dict(q=w, refine_attempts=attempts, refine_rel_change=0.0)
            sa.triangulate_tracks(ba, f0, sc.row_ptr, sc.obs_frame, sc.obs_uv, R, Tt, K, **args)  # warm-up: allocations, code objects
            dev, wall = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                X, quality, status = sa.triangulate_tracks(ba, f0, sc.row_ptr, sc.obs_frame, sc.obs_uv, R, Tt, K, **args)
                wall.append(1e3 * (time.perf_counter() - t0))
                dev.append(T.last_kernel_ms(ba))
            ms = float(np.median(dev))
            nbytes = O * (20 + (8 if w is not None else 0)) + n * (60 + 8) + M * 168
            out[label] = {"kernel_ms": ms, "call_ms": float(np.median(wall)), "observations_per_s": O / (1e-3 * ms), "algorithmic_bytes": int(nbytes),
                          "fraction_of_hbm_peak": nbytes / (1e-3 * ms) / HBM_PEAK, "tracks_flagged": int(np.count_nonzero(status & ~np.uint32(16))),
                          "median_rms_pixels": float(np.nanmedian(quality[:, 0]))}
        # the host loop on a sample of tracks, K [R | T] per observation built by the caller as before
        pick = np.linspace(0, n - 1, min(sample, n)).astype(np.int64)
        P = np.concatenate([K @ R, (K @ Tt[:, :, None])], axis=2).reshape(M, 12)
        t0 = time.perf_counter()
        for i in pick:
            o0, o1 = sc.row_ptr[i], sc.row_ptr[i + 1]
            sio.triangulate_least_squares(sc.obs_uv[o0:o1], P[sc.obs_frame[o0:o1]], f0)
        per_track = (time.perf_counter() - t0) / len(pick)
        out["host_loop"] = {"sampled_tracks": int(len(pick)), "ms_per_track": 1e3 * per_track, "ms_whole_batch_extrapolated": 1e3 * per_track * n}
        return out
    finally:
        ba.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1_dino_standin,C3_1kcam_100kpt,C3_ragged_8to32")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangulate", "triangulate_rate.json"))
    a = ap.parse_args()
    import surikatoko_amd as sa
    rows = []
    for name in a.configs.split(","):
        r = one(sa, name, a.reps, a.sample)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
