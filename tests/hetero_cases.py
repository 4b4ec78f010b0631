"""Scenes whose frames (or intrinsic groups) carry different intrinsics, shared by tests/test_hetero_cpu.py (the gate: the
yardstick stays inside the existing tolerances on them) and tests/test_gpu_hetero.py (every kernel and host path that reads
a camera pack, against the yardsticks).

srk_scene_generate writes the same K into every frame, so a kernel or a host table that took another frame's (or group's)
intrinsics would not be noticed on its scenes.  per_frame_intrinsics() gives every frame its own fx, fy, u0, v0 and maps every
observation by the affine map of its frame that keeps it the projection of the same ray:

    x = (fx X/Z + u0) / K22 = u / f0   ->   u' = f0 (fx' (u K22 / f0 - u0) / fx + u0') / K22     (likewise v)

so the rays, and with them the geometry of the bundle adjustment problem, stay as they were (residuals are scaled by fx'/fx
and fy'/fy per frame).  Both conventions of K work (K(2,2) = 1 with K divided by f0, and K(2,2) = f0); shared_k = 0 only,
zero skew only (what the generator and the golden inputs carry).
"""
import numpy as np

import surikatoko_amd as sa

SPREAD = 0.15


def _with_draws(sc, f0, spread, d):
    """the scene with frame j's intrinsics changed by the draws d[j] = (fx, fy, u0, v0), each in [-1, 1]"""
    assert sc.shared_k == 0, "one K per frame is needed"
    K = sc.K.reshape(-1, 9).copy()
    assert K.shape[0] == sc.M and d.shape == (sc.M, 4)
    assert np.all(K[:, [1, 3, 6, 7]] == 0), "zero skew, affine K only"
    fx, fy, u0, v0, k22 = (K[:, k].copy() for k in (0, 4, 2, 5, 8))
    fx2 = fx * (1.0 + spread * d[:, 0])
    fy2 = fy * (1.0 + spread * d[:, 1])
    u02 = u0 + spread * fx * d[:, 2]
    v02 = v0 + spread * fy * d[:, 3]
    K[:, 0], K[:, 4], K[:, 2], K[:, 5] = fx2, fy2, u02, v02
    j = sc.obs_frame
    uv = sc.obs_uv.reshape(-1, 2)
    uv2 = np.empty_like(uv)
    uv2[:, 0] = f0 * (fx2[j] * (uv[:, 0] * k22[j] / f0 - u0[j]) / fx[j] + u02[j]) / k22[j]
    uv2[:, 1] = f0 * (fy2[j] * (uv[:, 1] * k22[j] / f0 - v0[j]) / fy[j] + v02[j]) / k22[j]
    return sa.Scene(sc.points, sc.cam_R, sc.cam_T, K, 0, sc.row_ptr, sc.obs_frame, uv2)


def per_frame_intrinsics(sc, f0, spread=SPREAD, seed=0):
    """a copy of `sc` in which every frame has its own fx, fy, u0 and v0 (four independent seeded draws a frame: fx, fy scaled by
    1 + spread U(-1, 1), u0 / v0 shifted by spread fx U(-1, 1) / spread fy U(-1, 1)), the observations mapped with them"""
    d = np.random.RandomState(seed).uniform(-1.0, 1.0, size=(sc.M, 4))
    return _with_draws(sc, f0, spread, d)


def per_group_intrinsics(sc, f0, groups, spread=SPREAD, seed=0):
    """the same with one draw per intrinsic group: distinct K from group to group, identical bits inside a group (what
    set_intrinsic_groups asks of an upload)"""
    groups = np.asarray(groups, dtype=np.int64)
    assert groups.shape == (sc.M,)
    d = np.random.RandomState(seed).uniform(-1.0, 1.0, size=(int(groups.max()) + 1, 4))
    return _with_draws(sc, f0, spread, d[groups])


def distinct_intrinsics(sc):
    """number of distinct values of (fx, fy, u0, v0) over the frames"""
    K = sc.K.reshape(-1, 9)
    return tuple(len(np.unique(K[:, k])) for k in (0, 4, 2, 5))


def block_first_frames(sc, block=1024):
    """Smallest frame of every `block` consecutive observations in the library's landmark order (landmarks sorted by first
    frame, track length, then the rest of the frame list; frames as the caller numbers them): the first frame of the camera
    window a workgroup of the fused derivative kernel and of the staged error kernel keeps in LDS."""
    rp, of = sc.row_ptr, sc.obs_frame
    keys = []
    for i in range(sc.N):
        f = of[rp[i]:rp[i + 1]]
        keys.append((len(f) > 0, int(f[0]) if len(f) else -1, len(f), tuple(int(x) for x in f[1:]), i))
    seq = np.concatenate([of[rp[k[-1]]:rp[k[-1] + 1]] for k in sorted(keys)])
    return np.array([int(seq[o:o + block].min()) for o in range(0, len(seq), block)])


def groups_of(M, G):
    """G groups: alternating frames for two, runs of consecutive frames otherwise (as tests/test_gpu_shared_k.py)"""
    if G == 1:
        return np.zeros(M, dtype=np.int32)
    if G == 2:
        return (np.arange(M) % 2).astype(np.int32)
    return (np.arange(M) * G // M).astype(np.int32)


def _gen(seed, drop=0.0, drop_seed=7, **spec):
    def make():
        s = sa.SceneSpec(**spec)
        sc = sa.generate_scene(s)
        if drop > 0:
            sc = sa.drop_observations(sc, drop, seed=drop_seed)
        return sc, s.f0, seed
    return make


def _loop_90():
    return sa.loop_scene(sa.SceneSpec(n_frames=90, grid_nx=20, grid_ny=15, vis_window=0), window=6), 600.0, 36


def _gauge_on(a, b):
    """frames a and b trade numbers with frames 0 and 1, which carry the gauge, AFTER the intrinsics were drawn"""
    def post(sc):
        p = np.arange(sc.M)
        p[[0, a]] = p[[a, 0]]
        p[[1, b]] = p[[b, 1]]
        return sa.renumber_frames(sc, p)
    return post


def _shuffle(seed):
    """frames renumbered at random AFTER the intrinsics were drawn: every K has to travel with its frame"""
    return lambda sc: sa.renumber_frames(sc, np.random.RandomState(seed).permutation(sc.M))


# The oracle's Householder QR on the unscaled system lands 5e-9 .. 4e-8 from the exact solution at c = 1e-4 on most scenes of
# this kind, from one draw of the intrinsics to the next (with one K for all frames as well); tests/test_hetero_cpu.py holds
# four times that below the correction tolerance of the GPU test that takes the case (corr_tol() below).
# - Which two frames carry the gauge decides the scale of the normalised world and with it how the unscaled QR fares: with the
#   gauge on frames 51 and 49 (as the shuffle of shuffled_60 happens to put it) the distance is 7e-11 .. 2e-10 for every draw
#   tried, on the 60-frame band and on the 90-frame loop alike.  The loop of tests/test_gpu_parity.py::UNORDERED as it stands
#   (gauge on its frames 0 and 1) gives 9e-9 .. 4e-8 and cannot meet the 1e-8 of the renumbered-frame tests, nor can it with
#   60 or 45 frames, pixel noise or a random shuffle; loop_90 here is that loop with frames 51 and 49 renumbered to 0 and 1.
# - schur_grouped_23 and runs_nf16 have no such handle (they must stay in time order).  The seed of schur_grouped_23 was taken
#   from the draws that leave a margin under 1e-7 (4.5e-9; other draws give up to 4e-8); runs_nf16 gives 1.7e-9 against the
#   2.5e-9 that the deterministic-mode test's 1e-8 asks for.  Both are properties of the yardstick alone (plain C, no BLAS),
#   asserted on the CPU.
# name -> maker of (same-K scene, f0, seed of the intrinsics), derivative mode to set, derivative kernel expected
# (srk_ba_jacobian_kernel: 0 two kernels, 1 fused, 2 uniform runs, 3 runs over frame unions)[, what is done to the scene after
# it got its intrinsics]
CASES = {
    # derivative and error kernels, one case a kernel
    "two_kernel_60": (_gen(11, n_frames=60, grid_nx=12, grid_ny=10, vis_window=50), 0, 0),
    "fused_12": (_gen(12, n_frames=12, grid_nx=30, grid_ny=20, vis_window=5), 0, 1),    # 3000 observations: three workgroups
    "runs_nf16": (_gen(13, n_frames=24, grid_nx=30, grid_ny=20, vis_window=16), 1, 2),
    "union_ragged_20": (_gen(14, drop=0.15, drop_seed=5, n_frames=60, grid_nx=40, grid_ny=30, vis_window=20), 2, 3),
    # Schur kernels: they do not read K, the W they sum now differs from frame to frame
    "schur_mm_ragged_7": (_gen(15, drop=0.25, n_frames=30, grid_nx=23, grid_ny=17, vis_window=7), -1, None),
    "schur_grouped_23": (_gen(38, drop=0.10, n_frames=50, grid_nx=24, grid_ny=20, vis_window=23), -1, None),
    # (70 frames with a window of 40, k_schur_long's case elsewhere, fails the gate of tests/test_hetero_cpu.py: the oracle's QR
    # is 9e-7 from the exact solution there, 5e-6 with one K; on this one 7e-9)
    "schur_long_34": (_gen(17, drop=0.25, drop_seed=11, n_frames=44, grid_nx=14, grid_ny=12, vis_window=34), -1, None),
    # the 12-frame scene with pixel noise of the issue's table
    "pixel_noise_12": (_gen(18, n_frames=12, grid_nx=10, grid_ny=10, vis_window=5, noise_uv_pix=0.5), -1, None),
    # shared intrinsics: 48 frames (2 and 32 groups)
    "groups_48": (_gen(19, n_frames=48, grid_nx=20, grid_ny=15, vis_window=8, noise_uv_pix=0.3), -1, None),
    # frames in another order than time (tests/test_gpu_parity.py::UNORDERED): renumbered inside by reverse Cuthill-McKee
    "shuffled_60": (_gen(21, n_frames=60, grid_nx=20, grid_ny=15, vis_window=6, noise_uv_pix=0.3), -1, None, _shuffle(1)),
    "loop_90": (_loop_90, -1, None, _gauge_on(51, 49)),
}
UNORDERED_CASES = ("shuffled_60", "loop_90")
DERIVATIVE_CASES = ("two_kernel_60", "fused_12", "runs_nf16", "union_ragged_20")
SCHUR_CASES = ("schur_mm_ragged_7", "schur_grouped_23", "schur_long_34")
DAMPINGS = (1e-4, 10.0)
CORR_TOL = 1e-7  # the corr_tol tests/test_gpu_parity.py gives _check on its synthetic scenes


def corr_tol(name):
    """the smallest correction tolerance a GPU test holds this case to before _check's widening by the yardstick's own error:
    1e-8 (the default of tests/test_gpu_parity.py::_check) where the case goes through test_phases_with_renumbered_frames_vs_oracle
    or the deterministic-mode test, 1e-7 elsewhere"""
    return 1e-8 if name in UNORDERED_CASES + ("runs_nf16",) else CORR_TOL

_cache = {}


def _post(name, sc):
    return CASES[name][3](sc) if len(CASES[name]) > 3 else sc


def same_k(name):
    """(copy of the case's scene with the generator's one K for all frames, f0)"""
    if name not in _cache:
        _cache[name] = CASES[name][0]()
    sc, f0, _ = _cache[name]
    return _post(name, sc.copy()), f0


def case(name):
    """(copy of the case's scene with per-frame intrinsics, f0)"""
    key = ("hetero", name)
    if key not in _cache:
        sc, f0, seed = _cache[name] if name in _cache else _cache.setdefault(name, CASES[name][0]())
        _cache[key] = _post(name, per_frame_intrinsics(sc, f0, SPREAD, seed))
    return _cache[key].copy(), _cache[name][1]


def huber_information_case(name="union_ragged_20"):
    """(the case with 5 % of its observations moved by 20 .. 60 px, f0, information with some q = 0) -- the outliers and the
    information of tests/test_gpu_information.py"""
    import robust_ref as rr
    import weighted_ref as wr
    sc, f0 = case(name)
    rr.inject_outliers(sc, 0.05, 20, 60, 7)
    return sc, f0, wr.make_information(sc, 21)


def c1():
    """the C1 stand-in (36 frames, 4983 landmarks, 16432 observations) with per-frame intrinsics"""
    if "C1" not in _cache:
        _cache["C1"] = per_frame_intrinsics(sa.config_scene("C1_dino_standin"), 600.0, SPREAD, 20)
    return _cache["C1"].copy(), 600.0


def solver_distance(S, rhs, x):
    """(distance of the solution x of S x = rhs from the exact one -- numpy's solve refined six times in long double, as
    tests/test_gpu_parity.py::_check does -- relative to the largest entry, condition number of the diagonally scaled S)"""
    xe = np.linalg.solve(S, rhs)
    Sl, rl = S.astype(np.longdouble), rhs.astype(np.longdouble)
    for _ in range(6):
        xe = xe + np.linalg.solve(S, (rl - Sl @ xe.astype(np.longdouble)).astype(np.float64))
    d = float(np.abs(np.asarray(x) - xe).max() / max(float(np.abs(xe).max()), 1e-300))
    dsc = 1.0 / np.sqrt(np.abs(np.diag(S)))
    return d, float(np.linalg.cond(S * dsc[:, None] * dsc[None, :]))
