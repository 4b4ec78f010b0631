"""Scenes that each send the scene planner (surikatoko_amd/csrc/srk_plan.cpp) down a named branch, shared by
tests/test_scene_plan_cpu.py (tables against the parent commit's) and tests/test_gpu_scene_plan.py (results against the
parent commit's).  A case = (Scene, options); the options are those of SrkPlanOptions that the case sets."""
import numpy as np

import surikatoko_amd as sa
from surikatoko_amd.ba import Scene

OPTION_DEFAULTS = dict(fixed_k=0, deterministic=0, jac_mode=-1, frame_order_mode=-1, frame_order=None, multi_rank=0, check_sort=0)


def _select(M, nx, ny, frames_of):
    """The all-visible circle-grid scene of M frames and nx * ny landmarks, cut down to landmark i seeing frames_of[i]."""
    sc = sa.generate_scene(sa.SceneSpec(n_frames=M, grid_nx=nx, grid_ny=ny, vis_window=0, noise_uv_pix=0.3))
    assert sc.N == len(frames_of) and np.all(np.diff(sc.row_ptr) == M)
    frames_of = [np.asarray(sorted(f), np.int64) for f in frames_of]
    idx = np.concatenate([i * M + f for i, f in enumerate(frames_of)]).astype(np.int64)
    row_ptr = np.concatenate([[0], np.cumsum([len(f) for f in frames_of])]).astype(np.int64)
    return Scene(sc.points, sc.cam_R, sc.cam_T, sc.K, sc.shared_k, row_ptr,
                 np.concatenate(frames_of).astype(np.int32), sc.obs_uv[idx])


def _random_geometry(M, frames_of, seed):
    """Tracks alone matter to the planner: any numbers for the geometry (scenes too large for the generator)."""
    rng = np.random.RandomState(seed)
    N = len(frames_of)
    row_ptr = np.concatenate([[0], np.cumsum([len(f) for f in frames_of])]).astype(np.int64)
    obs_frame = np.concatenate(frames_of).astype(np.int32)
    return Scene(rng.standard_normal((N, 3)), rng.standard_normal((M, 9)), rng.standard_normal((M, 3)),
                 rng.standard_normal((M, 9)), False, row_ptr, obs_frame, rng.standard_normal((int(row_ptr[-1]), 2)))


def _uniform():  # (a) two frame lists, 24 landmarks each: a third list's worth of widening is refused at 24, so both runs are uniform
    return _select(6, 8, 6, [range(0, 4)] * 24 + [range(2, 6)] * 24)


def _ragged_tracks(M=12, nx=20, ny=15, seed=7):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(nx * ny):
        n = rng.randint(2, 7)
        s = rng.randint(0, M - n + 1)
        f = np.arange(s, s + n)
        keep = rng.rand(n) >= 0.25
        keep[0] = keep[-1] = True
        out.append(f[keep])
    return out


def _ragged():  # (b)
    return _select(12, 20, 15, _ragged_tracks())


SHUFFLE_12 = np.random.RandomState(11).permutation(12)  # (h) frame j of (b) becomes frame SHUFFLE_12[j]


def _build(name):
    o = dict(OPTION_DEFAULTS)
    if name == "a_uniform":
        o["jac_mode"] = 1
        return _uniform(), o
    if name == "b_ragged":  # (mode 2: the Schur runs of so small a scene are cut into parts of 8 landmarks, too few observations a task otherwise)
        o["jac_mode"] = 2
        return _ragged(), o
    if name == "c_mid_wide":  # tracks of 21 frames, and of 22..24
        o["fixed_k"] = 1
        fr = [range(i % 3, i % 3 + 21) for i in range(30)] + [range(i % 5, i % 5 + 22 + i % 3) for i in range(30)]
        return _select(30, 10, 6, fr), o
    if name == "d_all_visible_30":  # (mode 2: without it the uniform tasks are long enough and no union task is looked at)
        o["jac_mode"] = 2
        return _select(30, 10, 10, [range(30)] * 100), o
    if name == "e_all_visible_40":  # tracks over more than 32 frames: the derivative kernel's own runs are refused
        o["jac_mode"] = 2
        return _select(40, 10, 10, [range(40)] * 100), o
    if name == "e_all_visible_60":  # 60 frames: a workgroup's window is 48 frames or more, so mode 0 leaves the two-kernel path
        o["jac_mode"] = 0
        return _select(60, 8, 5, [range(60)] * 40), o
    if name == "f_over_4096":
        rng = np.random.RandomState(3)
        fr = [np.arange(4097)] + [np.arange(s, s + 3) for s in rng.randint(0, 4097, 50)]
        return _random_geometry(4100, fr, 4), o
    if name == "g_long_fb16":  # 103 runs: 16 landmarks over the same 64 frames, the next 64 frames would widen the run past its allowance
        fr = [np.arange(64 * r, 64 * r + 64) for r in range(103) for _ in range(16)]
        return _random_geometry(64 * 103, fr, 5), o
    if name in ("h_shuffled_auto", "h_shuffled_given"):
        sc = sa.renumber_frames(_ragged(), SHUFFLE_12)
        o["jac_mode"] = 2
        if name == "h_shuffled_auto":
            o["frame_order_mode"] = 1
        else:
            o["frame_order"] = np.argsort(SHUFFLE_12).astype(np.int32)
        return sc, o
    if name == "i_threaded_sort":
        rng = np.random.RandomState(9)
        fr = np.sort(np.argsort(rng.rand(40000, 50), axis=1)[:, :3], axis=1)
        o["frame_order_mode"] = 0
        o["check_sort"] = 1
        return _random_geometry(50, list(fr), 10), o
    if name == "j_uniform_det":
        o["jac_mode"] = 1
        o["deterministic"] = 1
        return _uniform(), o
    if name == "j_ragged_det":
        o["jac_mode"] = 2
        o["deterministic"] = 1
        return _ragged(), o
    if name == "k_empty_multi_rank":
        fr = _ragged_tracks()
        fr[len(fr) // 2] = fr[-1] = np.zeros(0, np.int64)
        o["multi_rank"] = 1
        return _select(12, 20, 15, fr), o
    raise KeyError(name)


NAMES = ["a_uniform", "b_ragged", "c_mid_wide", "d_all_visible_30", "e_all_visible_40", "e_all_visible_60", "f_over_4096",
         "g_long_fb16", "h_shuffled_auto", "h_shuffled_given", "i_threaded_sort", "j_uniform_det", "j_ragged_det",
         "k_empty_multi_rank"]
GPU_NAMES = ["a_uniform", "b_ragged", "d_all_visible_30", "h_shuffled_auto", "h_shuffled_given", "j_uniform_det", "j_ragged_det"]
_cache = {}


def case(name):
    """(Scene, options); built once, not to be changed by the caller"""
    if name not in _cache:
        _cache[name] = _build(name)
    return _cache[name]


def write_case(path, name):
    """The case as the raw binary file tests/cpp/test_scene_plan.cpp reads: 12 int64 of header, then the arrays."""
    sc, o = case(name)
    K = np.ascontiguousarray(np.broadcast_to(np.asarray(sc.K, np.float64).reshape(-1, 9), (sc.M, 9)))
    order = o["frame_order"]
    head = np.array([sc.N, sc.M, sc.O, o["fixed_k"], o["deterministic"], 0, o["jac_mode"], o["frame_order_mode"],
                     0 if order is None else 1, o["multi_rank"], o["check_sort"], 0], np.int64)
    with open(path, "wb") as f:
        for a, t in ((head, np.int64), (sc.row_ptr, np.int64), (sc.obs_frame, np.int32), (sc.obs_uv, np.float64),
                     (sc.points, np.float64), (sc.cam_R, np.float64), (sc.cam_T, np.float64), (K, np.float64)):
            f.write(np.ascontiguousarray(a, dtype=t).tobytes())
        if order is not None:
            f.write(np.ascontiguousarray(order, dtype=np.int32).tobytes())
