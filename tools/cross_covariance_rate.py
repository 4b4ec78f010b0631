"""Cross-covariances and relative-pose covariances (srk_ba_cross_covariances, srk_ba_relative_pose_covariances) timed on the
benchmark scenes with six variables a frame (fixed intrinsics), beside the marginal call (srk_ba_covariances) in the same process
and against the column-by-column alternative: one srk_ba_phase_solve per distinct column of the inverse.

Per config, after two LM iterations on the seeded scene, the wall time (the calls synchronise), median of --reps calls, each
call including the derivative pass, the undamped system and its factorisation, of

  (a) covariances() of every frame                                    -- the existing call
  (b) relative_pose_covariances() of all M - 1 consecutive pairs      -- every frame's marginal and M - 1 cross blocks
  (c) cross_covariances() of 1000 random frame pairs (seeded)
  (d) joint_covariance() of a window of 10 consecutive frames and 100 of their landmarks (Python assembly included)

and the median time of one srk_ba_phase_solve on the same system (the system rebuilt, untimed, before every solve) times the
number of distinct columns each call needs, as tools/covariance_rate.py measures it.  (b) - (a) is what the cross blocks cost on
top of the marginals.  Prints one JSON line per config and writes them all to --out.

    python tools/cross_covariance_rate.py [--configs C1_dino_standin,C3_1kcam_100kpt] [--reps 5] [--out profiles/cross_covariance/cross_covariance_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FV = 6


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
        M, N = sc.M, sc.N
        every = np.arange(M, dtype=np.int32)
        consecutive = np.stack([every[:-1], every[1:]], axis=1)
        rs = np.random.RandomState(7)
        random_pairs = rs.randint(0, M, size=(1000, 2)).astype(np.int32)
        w0 = M // 2
        window = np.arange(w0, min(w0 + 10, M), dtype=np.int32)
        rp, fr = np.asarray(sc.row_ptr), np.asarray(sc.obs_frame)
        seen = np.flatnonzero([np.any((fr[rp[i]:rp[i + 1]] >= window[0]) & (fr[rp[i]:rp[i + 1]] <= window[-1])) for i in range(N)])
        landmarks = seen[np.linspace(0, len(seen) - 1, min(100, len(seen))).astype(np.int64)]
        ba.relative_pose_covariances(consecutive[:1])  # warm-up: allocations, code objects
        ba.joint_covariance(window[:2], landmarks[:2])
        ba.covariances([w0], [])
        out = {"config": name, "frame_vars": FV, "n_frames": M, "n_points": N, "n": FV * M, "rcs_fill": ba.rcs_fill(), "reps": reps}
        out["shared_part_ms"] = median_ms(lambda: ba.covariances([], []), reps)

        def solve_once():
            ba.phase_schur(0.0)
            t0 = time.perf_counter()
            ok = ba.phase_solve()
            dt = 1e3 * (time.perf_counter() - t0)
            assert ok
            return dt

        ba.phase_derivatives()
        solve_once()
        solve = out["phase_solve_ms"] = float(np.median([solve_once() for _ in range(max(reps, 9))]))

        def row(ms, columns, **more):
            return dict(ms=ms, distinct_columns=int(columns), column_by_column_ms=columns * solve, speedup=columns * solve / ms, **more)

        out["a_covariances_all_frames"] = row(median_ms(lambda: ba.covariances(every, []), reps), FV * M)
        out["b_relative_pose_consecutive"] = row(median_ms(lambda: ba.relative_pose_covariances(consecutive), reps), FV * M, pairs=M - 1)
        out["b_minus_a_ms"] = out["b_relative_pose_consecutive"]["ms"] - out["a_covariances_all_frames"]["ms"]
        out["c_1000_random_frame_pairs"] = row(median_ms(lambda: ba.cross_covariances(random_pairs), reps),
                                               FV * len(np.unique(random_pairs)), pairs=1000)
        nb = len(window) + len(landmarks)
        out["d_joint_10_frames_100_landmarks"] = row(median_ms(lambda: ba.joint_covariance(window, landmarks), reps),
                                                     FV * len(window) + 3 * len(landmarks), pairs=nb * (nb + 1) // 2,
                                                     frames=len(window), landmarks=len(landmarks))
        # the figure a gate would use: the translational sigma of consecutive relative poses for one pixel of noise
        rel = ba.relative_pose_covariances(consecutive)
        st = np.sqrt(np.einsum("nii->n", rel[:, :3, :3]))
        out["relative_translation_sigma_world_units_1px"] = {"median": float(np.median(st)), "max": float(st.max())}
        return out
    finally:
        ba.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1_dino_standin,C3_1kcam_100kpt")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_covariance", "cross_covariance_rate.json"))
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
