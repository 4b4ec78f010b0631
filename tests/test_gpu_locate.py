"""Resection without a start pose on the device: the kernels of srk_locate.hip against the numpy yardstick
(tests/locate_ref.py) on the cases of tests/locate_cases.py, the hand-off to the refinement, the bits, the status words, the
resident scene, the argument checks and the C++ adapter."""
import ctypes as C
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import _lib
from surikatoko_amd import ba as B
from surikatoko_amd import locate as LC
import hetero_cases
import locate_cases as lc
import locate_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def h():
    ba = sa.BundleAdjustmentKanatani(0)
    yield ba
    ba.close()


@pytest.fixture(scope="module")
def floor():
    """the largest pose distance between the host walk and the yardstick on the ragged cases, a CPU run (locate_cases.host_floor)"""
    if lc.cxx() is None:
        pytest.skip("no host C++ compiler")
    return lc.host_floor()


def _run(h, b, q="own", **kw):
    return sa.locate_frames(h, b.f0, b.row_ptr, b.point, b.uv, b.X, b.K, q=b.q if isinstance(q, str) else q, **kw)


def _got(res):
    return SimpleNamespace(R=res.R, T=res.T, located=res.located, status=res.located_status)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1)


def _same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ------------------------------------------------------------------ accuracy
def test_noise_free(h, floor):
    """n from 4 to 300 at 64 hypotheses: the located pose within ten times the host walk's distance from the truth on the same
    cases (a CPU run: 3.8e-11), located[0] below 1e-6 px"""
    b = lc.accuracy()
    res = _run(h, b, hypotheses=64, want_inliers=True)
    bound = 10 * lc.accuracy_floor()
    err = [max(lc.pose_error(res.R[i], res.T[i], f)) for i, f in enumerate(b.frames)]
    print(f"noise-free frames, device: largest distance from the truth {max(err):.3e} (bound {bound:.3e}), located[0] {res.located[:, 0].max():.3e} px")
    assert not res.located_status.any()
    assert max(err) <= bound and res.located[:, 0].max() < 1e-6
    assert np.array_equal(res.located[:, 2], res.located[:, 1]) and res.inliers.all()
    for i in range(b.n):   # every returned R passes the resection's rotation check
        assert np.abs(res.R[i].T @ res.R[i] - np.eye(3)).max() <= 1e-9 and abs(np.linalg.det(res.R[i]) - 1) <= 1e-9


@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("hypotheses", lc.HYPOTHESES)
def test_every_length_against_the_yardstick(h, floor, hypotheses, holes):
    """weighted lengths 0 .. 300 at every hypothesis count: status, winner, inlier count and flags, the number of hypotheses with a
    pose, the score to 1e-12 at the device's own pose, the pose within ten times the CPU floor"""
    b = lc.small(holes)
    res = _run(h, b, hypotheses=hypotheses, seed=lc.SAMPLER_SEED[hypotheses], want_inliers=True)
    worst = lc.agree(b, lc.small_yardstick(holes, hypotheses), _got(res), res.inliers)
    print(f"H = {hypotheses}, holes {holes}: largest pose distance to the yardstick {worst:.3e}, bound {10 * floor:.3e}")
    assert worst <= 10 * floor
    if holes:
        assert not res.inliers[b.q == 0].any()


@pytest.mark.parametrize("n_frames", lc.BATCH_SIZES)
def test_batches_against_the_yardstick(h, floor, n_frames):
    """batches of 1, 3, 5 and 257 frames at 65 hypotheses (a full wave and one lane); the yardstick walks every eighth frame, and
    every frame has the bits it has alone in test_a_frames_bits_do_not_depend_on_the_batch"""
    b = lc.rows(lc.ragged(False), range(n_frames))
    res = _run(h, b, hypotheses=lc.BIG_HYPOTHESES, seed=lc.SAMPLER_SEED[lc.BIG_HYPOTHESES], want_inliers=True)
    ys = {i: y for i, y in lc.big_yardstick(False).items() if i < n_frames}
    worst = lc.agree(b, ys, _got(res), res.inliers)
    assert worst <= 10 * floor
    lengths = np.diff(b.row_ptr)
    assert np.array_equal(res.located_status, np.where(lengths < 4, LC.LOCATE_FEW_POINTS, 0))


@pytest.mark.parametrize("share", [0.3, 0.5])
def test_outliers(h, share):
    """eight frames of 200 points with 30 % / 50 % of the observations moved: every located pose within twice the yardstick's own
    largest error on these frames (computed in the cases file), no moved observation marked an inlier; refined with a Cauchy loss,
    no worse than resect_frames started 3 degrees off"""
    b = lc.outliers(share)
    H = lc.outlier_hypotheses(share)
    assert H == -(-sa.ransac_hypotheses(0.3, 0.999) // 64) * 64 if share == 0.3 else H == 256
    ys, bound = lc.outlier_yardstick(share)
    res = _run(h, b, hypotheses=H, want_inliers=True)
    err = np.array([lc.pose_error(res.R[i], res.T[i], f) for i, f in enumerate(b.frames)])
    print(f"outliers {share}: H = {H}, located pose error {err[:, 0].max():.2e} rad, {err[:, 1].max():.2e} of the depth; bound {bound[0]:.2e}, {bound[1]:.2e}")
    assert not res.located_status.any()
    assert err[:, 0].max() <= bound[0] and err[:, 1].max() <= bound[1]
    assert not res.inliers[b.moved].any()
    lc.agree(b, ys, _got(res), res.inliers)
    fine = _run(h, b, hypotheses=H, refine=lc.OUTLIER_REFINE)
    import resect_cases as rc
    rng = np.random.default_rng(5)
    starts = [rc.off_pose(f.R_true, f.T_true, rng, np.radians(3), 0.1) for f in b.frames]
    R, T = sa.resect_frames(h, b.f0, b.row_ptr, b.point, b.uv, b.X, b.K, np.stack([s[0] for s in starts]), np.stack([s[1] for s in starts]),
                            **lc.OUTLIER_REFINE)[:2]
    e_fine = np.array([lc.pose_error(fine.R[i], fine.T[i], f) for i, f in enumerate(b.frames)])
    e_pred = np.array([lc.pose_error(R[i], T[i], f) for i, f in enumerate(b.frames)])
    print(f"  refined: {e_fine.max(0)}, resect_frames from 3 degrees off: {e_pred.max(0)}")
    # Both runs end in the same minimum of the Cauchy energy and stop when an accepted attempt changes E by less than 1e-9 E:
    # E ~ 300 px^2 and the Hessian's smallest eigenvalue in these pose variables ~ 1e6 px^2 (100 inliers x (880 px / rad)^2 / 100 for
    # the weakest direction), so the stopping point is sqrt(2 x 3e-7 / 1e6) ~ 1e-6 from the minimum: "at most" is read to that
    # resolution.  Measured on an MI355X: 30 % moved 1.05879e-3 against 1.05886e-3 rad; 50 % moved 2.30926e-3 against 2.30925e-3.
    assert np.all(e_fine.max(0) <= e_pred.max(0) + 1e-6)


# ------------------------------------------------------------------ the hand-off to the refinement
@pytest.mark.parametrize("opts", [dict(attempts=10), dict(loss="cauchy", delta=2.0, attempts=20), dict(loss="huber", delta=2.0, attempts=0)])
def test_chaining_is_resect_frames_from_the_located_poses(h, opts):
    b = lc.rows(lc.ragged(True), range(40))
    plain = _run(h, b, hypotheses=65, want_inliers=True)
    fine = _run(h, b, hypotheses=65, refine=opts, want_inliers=True, want_weights=True)
    assert _same_bits((plain.located, plain.located_status, plain.inliers), (fine.located, fine.located_status, fine.inliers))
    assert plain.quality is None and plain.weights is None
    own = sa.resect_frames(h, b.f0, b.row_ptr, b.point, b.uv, b.X, b.K, plain.R, plain.T, q=b.q, want_weights=True, **opts)
    assert _same_bits((fine.R, fine.T, fine.quality, fine.info, fine.status, fine.weights), own)
    assert np.array_equal((fine.status & 1).astype(bool), plain.located[:, 1] < 3)      # a frame that was not located is refined like any other


# ------------------------------------------------------------------ bits
def _out(res):
    return (res.R, res.T, res.located, res.located_status)


def test_a_frames_bits_do_not_depend_on_the_batch(h):
    b = lc.rows(lc.ragged(True), range(60))
    kw = dict(hypotheses=130, seed=3, want_inliers=True)
    a = _run(h, b, **kw)
    assert _same_bits(_out(a) + (a.inliers,), _out(_run(h, b, **kw)) + (_run(h, b, **kw).inliers,))          # two runs
    order = np.arange(b.n)[::-1]
    r = _run(h, lc.rows(b, order), **kw)
    assert _same_bits([x[order] for x in _out(a)], _out(r))                                                  # the reversed batch
    for i in (0, 4, 7, 8, 17, 59):                                                                           # alone
        one = _run(h, lc.rows(b, [i]), **kw)
        assert _same_bits([x[i:i + 1] for x in _out(a)], _out(one)), i
        assert np.array_equal(one.inliers, a.inliers[b.row_ptr[i]:b.row_ptr[i + 1]])
    whole = _run(h, lc.ragged(True), **kw)                                                                   # inside 257 frames
    assert _same_bits([x[:b.n] for x in _out(whole)], _out(a))
    other = _run(h, b, hypotheses=130, seed=4)
    located = a.located_status == 0
    assert np.any(other.located[located, 3] != a.located[located, 3])                                        # the seed matters


def test_unit_information_is_no_information_and_zero_is_absence(h):
    b = lc.rows(lc.ragged(True), range(60))
    short, keep = lc.without_holes(b)
    kw = dict(hypotheses=65, seed=2, want_inliers=True)
    a, c = _run(h, b, **kw), _run(h, short, **kw)
    assert _same_bits(_out(a), _out(c)) and np.array_equal(a.inliers[keep], c.inliers) and not a.inliers[~keep].any()
    one, none = _run(h, short, q=np.ones_like(short.q), **kw), _run(h, short, q=None, **kw)
    assert _same_bits(_out(one) + (one.inliers,), _out(none) + (none.inliers,))


# ------------------------------------------------------------------ status
def test_status_words(h):
    rng = np.random.default_rng(31)
    f = [lc.frame(n, rng, sigma=0.5) for n in (0, 3, 4, 4, 8)]
    f[2].q = np.array([1.0, 0.0, 1.0, 1.0])                      # four observations, one switched off
    line = np.linspace(-1, 1, 8)
    f[4].X = np.column_stack([line, 0.5 * line, lc.DEPTH + 0.3 * line])    # collinear landmarks
    import resect_cases as rc
    f[4].uv = rc.project(f[4].K, f[4].R_true, f[4].T_true, f[4].X)
    b = lc.batch(f, seed=5)
    res = _run(h, b, hypotheses=64, want_inliers=True)
    for i in (0, 1, 2):
        assert res.located_status[i] == LC.LOCATE_FEW_POINTS and res.located[i, 1] == (0, 3, 3)[i]
        assert np.array_equal(res.R[i], np.eye(3)) and np.array_equal(res.T[i], np.zeros(3))
        assert np.isnan(res.located[i, [0, 3, 5]]).all() and res.located[i, 2] == 0 and res.located[i, 4] == 0
    assert res.located_status[3] == 0 and res.located[3, 1] == 4
    # a line determines no pose: NO_MODEL with (I, 0), or some finite pose; never a non-finite pose without a status bit
    if res.located_status[4] == 0:
        assert np.all(np.isfinite(res.R[4])) and np.all(np.isfinite(res.T[4])) and np.isfinite(res.located[4]).all()
    else:
        assert res.located_status[4] == LC.LOCATE_NO_MODEL and np.array_equal(res.R[4], np.eye(3)) and res.located[4, 4] == 0
    assert not res.inliers[b.row_ptr[0]:b.row_ptr[3]].any()
    fine = _run(h, b, hypotheses=64, refine=dict(attempts=3))   # the refinement runs on such frames as on any other
    assert np.array_equal(fine.located_status, res.located_status) and fine.status[0] & 1 and not fine.status[1] & 1


def test_one_hypothesis_of_wrong_matches(h):
    """H = 1 and the single sample is all outliers: the call returns, and few observations agree with its pose"""
    b = lc.rows(lc.outliers(0.5), [0])
    moved = set(b.frames[0].moved.tolist())
    seed = next(s for s in range(1, 2000) if set(ref.sample(s, 0, 200)[:3]) <= moved)
    res = _run(h, b, hypotheses=1, seed=seed)
    y = lc.yardstick(b, 0, 1, seed)
    assert res.located_status[0] == y["status"] and res.located[0, 4] == y["located"][4]
    assert res.located[0, 2] <= 20
    if y["status"] == 0:
        assert res.located[0, 3] == 0 and res.located[0, 2] == y["located"][2]


# ------------------------------------------------------------------ the resident scene
def _held_out(reorder, n_extra=2, share=0.3, hetero=False):
    """An all-visible scene; its last n_extra frames are held out: their observations, `share` of them moved by 20 .. 60 px,
    become the frames to locate.  hetero: the full scene gets per-frame intrinsics before it is split, so the held-out frames carry
    K distinct from each other and from the resident frames."""
    spec = sa.SceneSpec(n_frames=12, grid_nx=12, grid_ny=9, vis_window=0, noise_uv_pix=0.3)
    full = sa.generate_scene(spec)
    if hetero:
        full = hetero_cases.per_frame_intrinsics(full, spec.f0)
        assert min(hetero_cases.distinct_intrinsics(full)) == full.M
    M = full.M - n_extra
    lm = np.repeat(np.arange(full.N), np.diff(full.row_ptr))
    inside = full.obs_frame < M
    rp = np.concatenate([[0], np.cumsum(np.bincount(lm[inside], minlength=full.N))]).astype(np.int64)
    sc = sa.Scene(full.points, full.cam_R[:M], full.cam_T[:M], full.K[:M], 0, rp, full.obs_frame[inside], full.obs_uv[inside])
    if reorder:
        sc = sa.renumber_frames(sc, np.random.default_rng(3).permutation(sc.M))
    rng = np.random.default_rng(9)
    frames = []
    for j in range(M, full.M):
        sel = np.flatnonzero(full.obs_frame == j)
        uv = full.obs_uv[sel].copy()
        lc.move_share(uv, share, rng)
        frames.append((lm[sel].astype(np.int32), uv))
    row_ptr = np.concatenate([[0], np.cumsum([len(p) for p, _ in frames])]).astype(np.int64)
    extra = dict(row_ptr=row_ptr, point=np.concatenate([p for p, _ in frames]), uv=np.concatenate([m for _, m in frames]),
                 K=full.K[M:].reshape(-1, 3, 3))
    g = sa.BundleAdjustmentKanatani(0)
    if reorder:
        g.set_frame_reordering(1)
    assert g.upload(spec.f0, sc)
    g.optimize(max_iterations=3)
    return g, sc, spec.f0, extra


SCENE_BUFFERS = (B.BUF_POINTS, B.BUF_CAM_R, B.BUF_CAM_T)


@pytest.mark.parametrize("reorder", [False, True])
def test_resident_scene_equals_the_downloaded_landmarks(h, reorder):
    """ba.locate in the normalised coordinates against locate_frames on the downloaded landmarks: the same winner and inlier
    count; the poses within ten times the distance between the yardstick's own runs in the two coordinate systems (a CPU run)"""
    _equals_the_downloaded_landmarks(h, reorder, False)


@pytest.mark.parametrize("reorder", [False, True])
def test_resident_scene_with_per_frame_intrinsics_equals_the_downloaded_landmarks(h, reorder):
    _equals_the_downloaded_landmarks(h, reorder, True)


def _equals_the_downloaded_landmarks(h, reorder, hetero):
    g, sc, f0, e = _held_out(reorder, hetero=hetero)
    assert not hetero or len(np.unique(e["K"][:, 1, 2])) == len(e["K"])
    try:
        before = [g.buffer(w).copy() for w in SCENE_BUFFERS]
        kw = dict(hypotheses=128, seed=5, want_inliers=True)
        res = g.locate(e["row_ptr"], e["point"], e["uv"], e["K"], revert_normalization=True, **kw)
        raw = g.locate(e["row_ptr"], e["point"], e["uv"], e["K"], revert_normalization=False, **kw)
        assert all(np.array_equal(a.view(np.uint8), g.buffer(w).view(np.uint8)) for a, w in zip(before, SCENE_BUFFERS))
        got = sc.copy()
        g.download(got, revert_normalization=True)
        own = sa.locate_frames(h, f0, e["row_ptr"], e["point"], e["uv"], got.points, e["K"], **kw)
        norm = got.copy()                                    # the yardstick's own second coordinate system: the normalised scene
        ok, nrm = sa.normalize_scene_inplace(norm)
        assert ok
        assert not res.located_status.any() and not own.located_status.any()
        assert np.array_equal(res.located[:, 1:4], own.located[:, 1:4]) and np.array_equal(res.inliers, own.inliers)
        assert np.array_equal(raw.located[:, 1:5], res.located[:, 1:5]) and not np.array_equal(raw.T, res.T)
        from surikatoko_amd import resect as RS
        unit, here = 0.0, []
        for i in range(len(res.R)):
            o0, o1 = e["row_ptr"][i], e["row_ptr"][i + 1]
            ya = ref.locate_frame(f0, e["uv"][o0:o1], got.points[e["point"][o0:o1]], None, e["K"][i], 128, 4.0, 5)
            yn = ref.locate_frame(f0, e["uv"][o0:o1], norm.points[e["point"][o0:o1]], None, e["K"][i], 128, 4.0, 5)
            assert ya["located"][3] == yn["located"][3] == res.located[i, 3] and ya["located"][2] == res.located[i, 2]
            Rb, Tb, _ = RS.revert(nrm, yn["R"][None], yn["T"][None])
            unit = max(unit, lc.pose_gap(Rb[0], Tb[0], ya))
            here.append(max(ref.pose_distance(res.R[i], res.T[i], own.R[i], own.T[i], lc.DEPTH)))
        # the distance is rounding through one ill- or well-conditioned triple per frame (measured 4e-15 .. 9e-12 on these four
        # frames), so the unit is the yardstick's largest over the scene's frames, not each frame's own draw
        print(f"resident against the caller's landmarks {here}; the yardstick's two runs differ by {unit:.3e}")
        assert max(here) <= 10 * unit
        if reorder:
            order = g.frame_order()
            assert order is not None and not np.array_equal(order, np.arange(sc.M))
        fine = g.locate(e["row_ptr"], e["point"], e["uv"], e["K"], refine=dict(loss="cauchy", delta=2.0, attempts=10), **kw)
        chained = g.resect(e["row_ptr"], e["point"], e["uv"], e["K"], res.R, res.T, loss="cauchy", delta=2.0, attempts=10)
        assert np.array_equal(fine.located, res.located)
        assert np.abs(fine.R - chained[0]).max() <= 1e-6 and np.abs(fine.T - chained[1]).max() <= 1e-6     # the start went through two maps: the same minimum, not the same bits
    finally:
        g.close()


def test_resident_scene_refusals():
    g, sc, f0, e = _held_out(False)
    args = (e["row_ptr"], e["point"], e["uv"], e["K"])
    try:
        bad = e["point"].copy()
        bad[5] = sc.N
        with pytest.raises(ValueError):
            g.locate(e["row_ptr"], bad, *args[2:])
        assert "out of range" in g.last_error()
        hook = _lib.ALLREDUCE_FN(lambda *a: 0)
        g.set_allreduce(hook, 0, 2)
        with pytest.raises(ValueError):
            g.locate(*args)
        assert "more than one rank" in g.last_error()
    finally:
        g.close()
    g = sa.BundleAdjustmentKanatani(0)
    try:
        with pytest.raises(RuntimeError):   # no scene
            g.locate(*args)
    finally:
        g.close()


# ------------------------------------------------------------------ bad arguments
def test_bad_arguments_launch_nothing(h):
    """one case per check: the text is set, the outputs and the kernel time of the last good call stay what they were"""
    b = lc.rows(lc.ragged(True), range(12))
    _run(h, b, hypotheses=64)
    ms = LC.last_kernel_ms(h)
    assert ms[0] > 0 and 0 < ms[1] <= ms[0]
    O = int(b.row_ptr[-1])
    out = [np.full((b.n, 9), 7.0), np.full((b.n, 3), 7.0), np.full((b.n, 6), 7.0), np.full(b.n, 7, np.uint32), np.full(O, 7, np.uint8),
           np.full((b.n, 6), 7.0), np.full((b.n, 36), 7.0), np.full(b.n, 7, np.uint32), np.full(O, 7.0)]
    good = dict(rp=b.row_ptr, pt=b.point, uv=b.uv, q=b.q, X=b.X, K=b.K, lo=(64, 4.0, 1), ro=(10, 1e-9, 0, 0.0), f0=b.f0, outs=tuple(range(9)))

    def call(**kw):
        a = dict(good, **kw)
        arr = {k: None if a[k] is None else np.ascontiguousarray(a[k], {"rp": np.int64, "pt": np.int32}.get(k, np.float64)) for k in
               ("rp", "pt", "uv", "q", "X", "K")}
        lo = _lib.LocateOptions(*a["lo"])
        ro = None if a["ro"] is None else _lib.ResectOptions(*a["ro"])
        p = {k: None if v is None else B._p(v) for k, v in arr.items()}
        code = sa.lib().srk_locate_frames(C.c_void_p(h._h), C.c_double(a["f0"]), C.c_int32(b.n), p["rp"], p["pt"], p["uv"], p["q"], C.c_int64(len(b.X)),
                                          p["X"], p["K"], C.c_int(0), C.byref(lo), None if ro is None else C.byref(ro),
                                          *[B._p(o) if k in a["outs"] else None for k, o in enumerate(out)])
        return code, h.last_error()

    def changed(name, index, value):
        a = np.array(good[name], copy=True)
        a[index] = value
        return {name: a}
    cases = [
        (changed("rp", 0, 1), "row_ptr[0]"), (changed("rp", 4, b.row_ptr[3] - 1), "decreases"), (changed("pt", 17, len(b.X)), "out of range"),
        (changed("q", 3, -1.0), "q of observation 3"), (changed("q", 3, np.nan), "q of observation 3"), (changed("uv", (40, 1), np.nan), "uv of observation 40"),
        (changed("X", (2, 0), np.inf), "landmark 2"), (changed("K", (1, 1, 1), np.nan), "K of frame 1 is not finite"),
        (changed("K", (1, 2), np.zeros(3)), "K of frame 1 is singular"),
        (dict(lo=(0, 4.0, 1)), "hypotheses"), (dict(lo=(4097, 4.0, 1)), "hypotheses"), (dict(lo=(64, 0.0, 1)), "inlier_pixels"),
        (dict(lo=(64, np.inf, 1)), "inlier_pixels"), (dict(ro=(65, 1e-9, 0, 0.0)), "refine attempts"), (dict(ro=(10, -1.0, 0, 0.0)), "refine rel_change"),
        (dict(ro=(10, 1e-9, 3, 1.0)), "refine loss_kind"), (dict(ro=(10, 1e-9, 1, 0.0)), "refine loss needs"),
        (dict(uv=None), "NULL observation array"), (dict(X=None), "landmark array is NULL"), (dict(K=None), "intrinsics array is NULL"), (dict(f0=0.0), "f0"),
        (dict(outs=(1, 2, 3, 4, 5, 6, 7, 8)), "NULL output array"), (dict(outs=(0, 1, 3, 4, 5, 6, 7, 8)), "NULL output array"),
        (dict(outs=(0, 1, 2, 3, 4, 5, 7, 8)), "NULL output array of the refinement"),
    ]
    for kw, text in cases:
        code, why = call(**kw)
        assert code == -1 and text in why, (text, code, why)
        assert LC.last_kernel_ms(h) == ms
    assert all(np.all(a == 7) for a in out)                    # nothing written
    code, _ = call(ro=None, outs=(0, 1, 2, 3))                 # without refinement its outputs may be NULL
    assert code == 0 and not np.any(out[0] == 7) and np.all(out[5] == 7) and np.all(out[4] == 7)
    code, _ = call()                                           # and the same call with good arguments runs
    assert code == 0 and not np.any(out[5] == 7) and not np.any(out[4] == 7) and LC.last_kernel_ms(h)[0] > 0


# ------------------------------------------------------------------ the C++ adapter
def test_cpp_adapter_locate(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "locate_adapter"
    r = subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "demos"),
                        os.path.join(ROOT, "tests", "cpp", "test_locate_adapter.cpp"), "-o", str(exe),
                        "-L", os.path.join(ROOT, "surikatoko_amd"), "-lsrk_ba",
                        "-Wl,-rpath," + os.path.join(ROOT, "surikatoko_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "locate adapter ok" in r.stdout
