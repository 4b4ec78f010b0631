"""Marginal covariances (srk_ba_covariances) timed on the benchmark scenes with six variables a frame (fixed intrinsics), against
the alternative the library offered before: one srk_ba_phase_solve per column of the inverse, measured in the same process.

Per config, after two LM iterations on the seeded scene: the wall time (the calls synchronise) of covariances() for one
frame, for every frame, and for every frame plus 1000 landmarks -- each the median of --reps calls, each call including the
derivative pass, the undamped system and its factorisation; that shared part alone (a call with empty selections); and the
median time of one srk_ba_phase_solve on the same system (the system rebuilt, untimed, before every solve), times the number
of columns each selection has.  Also recorded: the skyline's fill, the chunk count of the solver's own plan (the covariance call
always takes the single chain) and the batches a call needed.  Prints one JSON line per config and writes them all to --out.

    python tools/covariance_rate.py [--configs C1_dino_standin,C3_1kcam_100kpt] [--reps 5] [--out profiles/covariance/covariance_rate.json]
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
CAP_BYTES = 256 << 20


def median_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out))


def batches(ld, columns):
    """batches of a call with that many columns (groups never straddle a batch, so this is a lower bound that is exact for
    frame-only selections whose cap is a multiple of six columns or not reached)"""
    cap = max(64, CAP_BYTES // (8 * ld) // 64 * 64)
    return int(-(-columns // cap))


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
        n = FV * M
        ld = -(-n // 256) * 256
        pts = np.linspace(0, N - 1, min(1000, N)).astype(np.int64)
        every = np.arange(M, dtype=np.int32)
        ba.covariances([M // 2], [])  # warm-up: allocations, code objects
        sets = {"one_frame": ([M // 2], []), "all_frames": (every, []), "all_frames_1000_landmarks": (every, pts)}
        out = {"config": name, "frame_vars": FV, "n_frames": M, "n_points": N, "n": n, "rcs_fill": ba.rcs_fill(),
               "rcs_chunks": ba.rcs_chunks(), "reps": reps}
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
        out["phase_solve_ms"] = float(np.median([solve_once() for _ in range(max(reps, 9))]))
        for key, (fr, pt) in sets.items():
            cols = FV * len(fr) + 3 * len(pt)
            ms = median_ms(lambda: ba.covariances(fr, pt), reps)
            out[key] = {"columns": cols, "batches": batches(ld, cols), "covariances_ms": ms,
                        "column_by_column_ms": cols * out["phase_solve_ms"],
                        "speedup": cols * out["phase_solve_ms"] / ms}
        FB, _ = ba.covariances(every, [])
        d = np.sqrt(np.einsum("nii->ni", FB)[:, :3].sum(axis=1))
        out["centre_sigma_world_units_1px"] = {"median": float(np.median(d[2:])), "max": float(d.max())}
        return out
    finally:
        ba.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1_dino_standin,C3_1kcam_100kpt")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariance", "covariance_rate.json"))
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
