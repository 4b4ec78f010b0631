"""Map alignment on the device: the kernels of srk_align.hip against the numpy yardstick (tests/align_ref.py,
Umeyama's SVD route) on the cases of tests/align_cases.py, the bits, the status words, the outliers, the resident scene, the
bootstrap end to end, the argument checks and the C++ adapter."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import _lib
from surikatoko_amd import align as AL
from surikatoko_amd import ba as B
import align_cases as ac
import align_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def h():
    ba = sa.BundleAdjustmentKanatani(0)
    yield ba
    ba.close()


@pytest.fixture(scope="module")
def floor():
    """the largest model distance between the host walk and the yardstick on the ragged cases, a CPU run (align_cases.host_floor)"""
    return ac.host_floor()


def _run(h, b, q="own", **kw):
    kw.setdefault("inlier_distance", ac.TAU)
    return sa.align_points(h, b.row_ptr, b.a, b.b, q=b.q if isinstance(q, str) else q, **kw)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1)


def _same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _out(res):
    return (res.s, res.R, res.t, res.aligned, res.status)


def _proper(R):
    R = np.asarray(R).reshape(3, 3)
    return np.abs(R.T @ R - np.eye(3)).max() <= 1e-9 and abs(np.linalg.det(R) - 1) <= 1e-9


# ------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("scale", ac.SCALES)
@pytest.mark.parametrize("with_scale", [True, False])
def test_noise_free(h, with_scale, scale):
    """n from 3 to 300, a coplanar set and a set 1e6 from the origin at 64 hypotheses: the model within ten times the host walk's
    distance from the truth on the same cases (a CPU run in this process), every R a proper rotation"""
    b = ac.accuracy(with_scale, scale)
    res = _run(h, b, hypotheses=64, inlier_distance=ac.accuracy_tau(b), with_scale=with_scale, want_inliers=True)
    bound = 10 * ac.accuracy_floor(with_scale, scale)
    err = [ref.distance(ac.model_of(res, i), f.truth, f.b) for i, f in enumerate(b.sets)]
    print(f"noise-free sets, with_scale {with_scale}, scale {scale}: largest distance from the truth {max(err):.3e} (bound {bound:.3e})")
    assert not res.status.any()
    assert max(err) <= bound
    assert np.array_equal(res.aligned[:, 2], res.aligned[:, 1]) and res.inliers.all()
    assert all(_proper(R) for R in res.R)
    if not with_scale:
        assert np.all(res.s == 1.0)


@pytest.mark.parametrize("rounds", [0, 2])
@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("hypotheses", ac.HYPOTHESES)
def test_every_length_against_the_yardstick(h, floor, hypotheses, holes, rounds):
    """weighted lengths 0 .. 300 at every hypothesis count, refined and not: status, winner, the model count, the inlier count and
    flags, the rounds accepted, the score to 1e-12 at the device's own model, the model within ten times the CPU floor"""
    b = ac.small(holes)
    res = _run(h, b, hypotheses=hypotheses, seed=ac.SAMPLER_SEED[hypotheses], refine_rounds=rounds, want_inliers=True)
    worst = ac.agree(b, ac.small_yardstick(holes, hypotheses), res, res.inliers, stage=rounds == 0)
    print(f"H = {hypotheses}, holes {holes}, rounds {rounds}: largest model distance to the yardstick {worst:.3e}, bound {10 * floor:.3e}")
    assert worst <= 10 * floor
    if holes:
        assert not res.inliers[b.q == 0].any()


@pytest.mark.parametrize("n_sets", ac.BATCH_SIZES)
def test_batches_against_the_yardstick(h, floor, n_sets):
    """batches of 1, 3, 5 and 257 sets at 65 hypotheses (a full wave and one lane); the yardstick walks every eighth set"""
    b = ac.rows(ac.ragged(False), range(n_sets))
    res = _run(h, b, hypotheses=ac.BIG_HYPOTHESES, seed=ac.SAMPLER_SEED[ac.BIG_HYPOTHESES], want_inliers=True)
    ys = {i: y for i, y in ac.big_yardstick(False).items() if i < n_sets}
    worst = ac.agree(b, ys, res, res.inliers)
    print(f"{n_sets} sets: largest model distance to the yardstick {worst:.3e}, bound {10 * floor:.3e}")
    assert worst <= 10 * floor
    assert np.array_equal(res.status, np.where(np.diff(b.row_ptr) < 3, AL.ALIGN_FEW_POINTS, 0))


# ------------------------------------------------------------------ bits
def test_a_sets_bits_do_not_depend_on_the_batch(h):
    b = ac.rows(ac.ragged(True), range(60))
    kw = dict(hypotheses=130, seed=3, want_inliers=True)
    a = _run(h, b, **kw)
    again = _run(h, b, **kw)
    assert _same_bits(_out(a) + (a.inliers,), _out(again) + (again.inliers,))                                # two runs
    order = np.arange(b.n)[::-1]
    r = _run(h, ac.rows(b, order), **kw)
    assert _same_bits([x[order] for x in _out(a)], _out(r))                                                  # the reversed batch
    for i in (0, 4, 7, 8, 17, 59):                                                                           # alone
        one = _run(h, ac.rows(b, [i]), **kw)
        assert _same_bits([x[i:i + 1] for x in _out(a)], _out(one)), i
        assert np.array_equal(one.inliers, a.inliers[b.row_ptr[i]:b.row_ptr[i + 1]])
    whole = _run(h, ac.ragged(True), **kw)                                                                   # inside 257 sets
    assert _same_bits([x[:b.n] for x in _out(whole)], _out(a))
    other = _run(h, b, hypotheses=130, seed=4)
    ok = a.status == 0
    assert np.any(other.aligned[ok, 3] != a.aligned[ok, 3])                                                  # the seed matters


def test_unit_information_is_no_information_and_zero_is_absence(h):
    b = ac.rows(ac.ragged(True), range(60))
    short, keep = ac.without_holes(b)
    kw = dict(hypotheses=65, seed=2, want_inliers=True)
    a, c = _run(h, b, **kw), _run(h, short, **kw)
    assert _same_bits(_out(a), _out(c)) and np.array_equal(a.inliers[keep], c.inliers) and not a.inliers[~keep].any()
    one, none = _run(h, short, q=np.ones_like(short.q), **kw), _run(h, short, q=None, **kw)
    assert _same_bits(_out(one) + (one.inliers,), _out(none) + (none.inliers,))


def test_no_rounds_leave_the_hypothesis_stage_as_it_is(h):
    """refine_rounds = 0: the winner, its score and its counts are those the refined run started from; where no round is accepted
    the two runs have the same bits"""
    b = ac.rows(ac.ragged(True), range(60))
    kw = dict(hypotheses=65, seed=2, want_inliers=True)
    plain, fine = _run(h, b, refine_rounds=0, **kw), _run(h, b, refine_rounds=2, **kw)
    assert np.all(plain.aligned[:, 5] == 0) and np.isnan(plain.aligned[:, 6]).all()
    assert _same_bits((plain.status, plain.aligned[:, [1, 3, 4]]), (fine.status, fine.aligned[:, [1, 3, 4]]))
    same = fine.aligned[:, 5] == 0
    assert same.any() and not same.all()
    assert _same_bits([x[same] for x in _out(plain)], [x[same] for x in _out(fine)])
    ok = plain.status == 0
    assert np.all(fine.aligned[ok, 0] <= plain.aligned[ok, 0])                                               # never worse than the winner
    for i in np.flatnonzero(ok):                                                                             # and it is the hypothesis' model
        y = ref.align_set(*ac.set_obs(b, i)[:2], ac.set_obs(b, i)[2], 65, ac.TAU, 2, True, 0)
        if int(plain.aligned[i, 3]) == y["aligned"][3]:
            assert ref.distance(ac.model_of(plain, i), (y["s"], y["R"], y["t"]), ac.set_obs(b, i)[1]) <= 1e-9


# ------------------------------------------------------------------ status
def test_status_words(h):
    rng = np.random.default_rng(31)
    f = [ac.make_set(n, rng, sigma=ac.NOISE) for n in (0, 2, 3, 3, 8, 50)]
    f[2].q = np.array([1.0, 0.0, 1.0])                           # three correspondences, one switched off
    line = np.linspace(-1, 1, 8)
    f[4].a = np.column_stack([line, 0.5 * line, 0.3 * line])     # exactly collinear sources
    f[4].b = ac.apply(f[4].truth, f[4].a)
    mirror = np.diag([1.0, 1.0, -1.0])
    f[5].b = ac.apply(f[5].truth, f[5].a @ mirror)               # a mirrored set: no proper rotation fits it
    b = ac.batch(f)
    res = _run(h, b, hypotheses=64, want_inliers=True)
    for i in (0, 1, 2):
        assert res.status[i] == AL.ALIGN_FEW_POINTS and res.aligned[i, 1] == (0, 2, 2)[i]
    assert res.status[3] == 0 and res.aligned[3, 1] == 3
    assert res.status[4] == AL.ALIGN_NO_MODEL and res.aligned[4, 1] == 8 and res.aligned[4, 4] == 0
    for i in (0, 1, 2, 4):
        assert res.s[i] == 1.0 and np.array_equal(res.R[i], np.eye(3)) and np.array_equal(res.t[i], np.zeros(3))
        assert np.isnan(res.aligned[i, [0, 3, 6, 7]]).all() and res.aligned[i, 2] == 0 and res.aligned[i, 5] == 0
        assert not res.inliers[b.row_ptr[i]:b.row_ptr[i + 1]].any()
    # the mirrored set: a proper rotation, finite outputs, and an error of the size of the set, not of the noise
    assert res.status[5] == 0 and _proper(res.R[5]) and np.isfinite(res.aligned[5, :6]).all() and res.s[5] > 0
    assert res.aligned[5, 2] < 25 and res.aligned[5, 0] > 0.5 * ac.TAU
    assert AL.align_status_names(res.status[4]) == ["NO_MODEL"]


def test_collinear_inliers_report_a_gap_of_zero(h):
    """Forty collinear points and one off the line whose target is moved by 2 tau away from the line, without scale: every sample
    with a model holds the moved point; the winner's inliers are the forty on the line, the closed form over them is accepted (it
    fits the line exactly) and its eigenvalue gap is 0: the rotation about the line is not determined, and the library says so
    instead of refusing.  The gap is a difference of two eigenvalues of size lambda1, each good to a few eps."""
    rng = np.random.default_rng(7)
    tau = 0.05
    u = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    w = np.cross(u, [0.0, 0.0, 1.0])
    w /= np.linalg.norm(w)
    a = np.concatenate([np.outer(np.linspace(-1.5, 1.5, 40), u), [0.2 * u + 1.0 * w]])
    truth = ac.similarity(rng, 1.0)
    bt = ac.apply(truth, a)
    bt[40] += 2 * tau * (truth[1] @ w)
    kw = dict(hypotheses=256, inlier_distance=tau, seed=1, with_scale=False, want_inliers=True)
    y = ref.align_set(a, bt, None, 256, tau, 1, False, 2)
    res = sa.align_points(h, [0, 41], a, bt, **kw)
    print(f"collinear inliers: gap {res.aligned[0, 6]:.3e} (yardstick {y['aligned'][6]:.3e}), rounds {res.aligned[0, 5]}, inliers {res.aligned[0, 2]}")
    assert y["aligned"][2] == 40 and y["aligned"][5] >= 1 and not y["inliers"][40]
    assert res.status[0] == 0 and res.aligned[0, 2] == 40 and res.aligned[0, 5] >= 1 and not res.inliers[40] and res.inliers[:40].all()
    assert 0.0 <= res.aligned[0, 6] <= 1e-12 and _proper(res.R[0])
    assert res.aligned[0, 7] <= 1e-12                                                                        # the line itself is fitted exactly


# ------------------------------------------------------------------ outliers
@pytest.mark.parametrize("share", [0.3, 0.5])
def test_outliers(h, floor, share):
    """eight sets of 200 correspondences with 30 % / 50 % of the targets moved by 20 .. 200 tau, at the reference's hypothesis count
    rounded up to a wave: no moved correspondence is an inlier and every unmoved one is; the refined model agrees with Umeyama over
    the unmoved correspondences within ten times the floor; the refined score is never above the unrefined one"""
    b = ac.outliers(share)
    H = ac.outlier_hypotheses(share)
    assert H == -(-sa.ransac_hypotheses(share, 0.999, 3) // 64) * 64
    res = _run(h, b, hypotheses=H, want_inliers=True)
    plain = _run(h, b, hypotheses=H, refine_rounds=0)
    assert not res.status.any()
    moved = np.zeros(len(res.inliers), bool)
    moved[b.moved] = True
    assert not res.inliers[moved].any() and res.inliers[~moved].all()
    worst = ac.agree(b, ac.outlier_yardstick(share), res, res.inliers)
    gaps = []
    for i, f in enumerate(b.sets):
        keep = np.setdiff1d(np.arange(200), f.moved)
        best, _ = ref.umeyama(f.a[keep], f.b[keep], np.ones(len(keep)), True)
        gaps.append(ref.distance(ac.model_of(res, i), best, f.b))
    print(f"outliers {share}: H = {H}, to the yardstick {worst:.3e}, to Umeyama over the unmoved {max(gaps):.3e}, bound {10 * floor:.3e}, "
          f"rounds {res.aligned[:, 5]}")
    assert worst <= 10 * floor and max(gaps) <= 10 * floor
    assert np.all(res.aligned[:, 0] <= plain.aligned[:, 0]) and np.all(res.aligned[:, 5] >= 1)


# ------------------------------------------------------------------ the resident scene
def _resident(share=0.2):
    spec = sa.SceneSpec(n_frames=8, grid_nx=12, grid_ny=9, vis_window=0, noise_uv_pix=0.3)
    sc, pts_gt, _, _ = sa.generate_scene(spec, with_gt=True)
    rng = np.random.default_rng(11)
    truth = ac.similarity(rng, 3.0)
    target = ac.apply(truth, pts_gt)
    tau = 0.05 * 3.0
    moved = ac.move_share(target, share, rng, tau)
    order = rng.permutation(sc.N).astype(np.int32)          # the correspondences in an order of their own
    g = sa.BundleAdjustmentKanatani(0)
    assert g.upload(spec.f0, sc)
    return g, sc, order, target[order], np.isin(order, moved), tau, truth


SCENE_BUFFERS = (B.BUF_POINTS, B.BUF_CAM_R, B.BUF_CAM_T)


def test_resident_scene_equals_the_downloaded_landmarks(h, floor):
    """ba.align over the resident landmarks against align_points on the downloaded ones, before and after ten LM iterations: the
    same winner, counts and flags, the model within the floor; the scene's buffers keep their bits"""
    g, sc, point, target, wrong, tau, truth = _resident()
    try:
        kw = dict(hypotheses=128, inlier_distance=tau, seed=5, want_inliers=True)
        seen = []
        for step in range(2):
            before = [g.buffer(w).copy() for w in SCENE_BUFFERS]
            res = g.align(point, target, **kw)
            raw = g.align(point, target, revert_normalization=False, **kw)
            assert all(np.array_equal(a.view(np.uint8), g.buffer(w).view(np.uint8)) for a, w in zip(before, SCENE_BUFFERS))
            got = sc.copy()
            g.download(got, revert_normalization=True)
            own = sa.align_points(h, [0, len(point)], got.points[point], target, **kw)
            assert res.status[0] == 0 and own.status[0] == 0
            assert np.array_equal(res.aligned[:, 1:6], own.aligned[:, 1:6]) and np.array_equal(res.inliers, own.inliers)
            assert np.array_equal(raw.aligned[:, 1:6], res.aligned[:, 1:6]) and not np.array_equal(raw.t, res.t)
            assert not res.inliers[wrong].any() and res.inliers[~wrong].all()
            gap = ref.distance(ac.model_of(res), ac.model_of(own), target)
            print(f"resident scene, step {step}: align() against align_points on the download {gap:.3e} (floor {floor:.3e}); "
                  f"from the generating similarity {ref.distance(ac.model_of(res), truth, target):.3e}")
            assert gap <= floor
            seen.append(ac.model_of(res))
            if step == 0:
                g.optimize(max_iterations=10)
        assert ref.distance(seen[0], seen[1], target) > 100 * floor                                          # it read the refined landmarks
        bad = point.copy()
        bad[5] = sc.N
        with pytest.raises(ValueError):
            g.align(bad, target, **kw)
        assert "beyond the map" in g.last_error()
        with pytest.raises(ValueError):
            g.align(point, target, hypotheses=128)
        assert "inlier_distance" in g.last_error()
        hook = _lib.ALLREDUCE_FN(lambda *a: 0)
        g.set_allreduce(hook, 0, 2)
        with pytest.raises(ValueError):
            g.align(point, target, **kw)
        assert "more than one rank" in g.last_error()
    finally:
        g.close()
    g = sa.BundleAdjustmentKanatani(0)
    try:
        with pytest.raises(RuntimeError):   # no scene
            g.align(point, target, **kw)
    finally:
        g.close()


# ------------------------------------------------------------------ end to end
def test_bootstrap_end_to_end(h, floor):
    """two_view_scene on the relate test's pair of 150 landmarks, its points aligned to the true landmarks under a known similarity
    with 20 % of the identities shuffled, then apply_similarity.  Asserted: the device's model within ten times the floor of the
    yardstick's on the same input.  The recovered baseline length and camera centre against the truth are measured and printed
    (profiles/align/test_figures.json records them), not asserted against a number chosen here."""
    from test_gpu_relate import _bootstrap_case
    import relate_cases as rc
    c = _bootstrap_case()
    tv = sa.two_view_scene(h, rc.F0, c.uv_a, c.uv_b, rc.K0, rc.K0, hypotheses=sa.ransac_hypotheses(0.2, 0.999, 5), inlier_pixels=rc.TAU)
    rng = np.random.default_rng(2490)
    X = rc.points(150, rng)
    X[:, 2] *= 0.6                                              # the landmarks of _bootstrap_case, frame a = (I, 0), |T| = 1
    world = ac.similarity(np.random.default_rng(8), 4.0)        # the main map's coordinates
    target = ac.apply(world, X[tv.match])
    n = len(target)
    mixed = np.random.default_rng(9).choice(n, size=n // 5, replace=False)
    target[mixed] = target[np.roll(mixed, 1)]                   # 20 % of the identities shuffled
    tau = 0.05 * world[0]
    kw = dict(hypotheses=sa.ransac_hypotheses(0.2, 0.999, 3) * 4, inlier_distance=tau, seed=1)
    res = sa.align_points(h, [0, n], tv.points, target, want_inliers=True, **kw)
    y = ref.align_set(tv.points, target, None, kw["hypotheses"], tau, 1, True, 2)
    assert res.status[0] == 0 and y["status"] == 0
    assert int(res.aligned[0, 3]) in ac.near_ties(y) and ac.winner_is_clear(y)
    gap = ref.distance(ac.model_of(res), (y["s"], y["R"], y["t"]), target)
    assert np.array_equal(res.aligned[0, [2, 5]], y["aligned"][[2, 5]]) and np.array_equal(res.inliers.astype(bool), y["inliers"])
    pts, cam_R, cam_T = AL.apply_similarity(*ac.model_of(res), tv.points, tv.cam_R, tv.cam_T)
    centre = -cam_R[1].T @ cam_T[1]
    true_R = c.R @ world[1].T
    true_centre = ac.apply(world, (-c.R.T @ c.T)[None])[0]
    figures = dict(landmarks=n, inliers=int(res.aligned[0, 2]), rounds=int(res.aligned[0, 5]), inlier_rms=float(res.aligned[0, 7]), tau=tau,
                   baseline=float(np.linalg.norm(centre - (-cam_R[0].T @ cam_T[0]))), baseline_true=float(world[0]),
                   centre_error=float(np.linalg.norm(centre - true_centre)), rotation_error_rad=float(ref.distance((1.0, cam_R[1], np.zeros(3)),
                                                                                                                   (1.0, true_R, np.zeros(3)), np.ones(3))),
                   device_to_yardstick=gap, host_floor=floor)
    print("ALIGN_FIGURES " + json.dumps(figures))
    assert gap <= 10 * floor
    assert not res.inliers[mixed].any()


# ------------------------------------------------------------------ bad arguments
def test_bad_arguments_launch_nothing(h):
    """one case per check through the handle: the text is set, the outputs and the kernel time of the last good call stay what they were"""
    b = ac.rows(ac.ragged(True), range(12))
    _run(h, b, hypotheses=64)
    ms = AL.last_kernel_ms(h)
    assert ms[0] > 0 and 0 < ms[1] <= ms[0]
    O = int(b.row_ptr[-1])
    out = [np.full(b.n, 7.0), np.full((b.n, 9), 7.0), np.full((b.n, 3), 7.0), np.full((b.n, 8), 7.0), np.full(b.n, 7, np.uint32), np.full(O, 7, np.uint8)]
    good = dict(rp=b.row_ptr, a=b.a, b=b.b, q=b.q, lo=(64, ac.TAU, 1, 1, 2), outs=tuple(range(6)))

    def call(**kw):
        a = dict(good, **kw)
        arr = {k: None if a[k] is None else np.ascontiguousarray(a[k], np.int64 if k == "rp" else np.float64) for k in ("rp", "a", "b", "q")}
        lo = _lib.AlignOptions(*a["lo"])
        p = {k: None if v is None else B._p(v) for k, v in arr.items()}
        code = sa.lib().srk_align_points(C.c_void_p(h._h), C.c_int32(b.n), p["rp"], p["a"], p["b"], p["q"], C.byref(lo),
                                         *[B._p(o) if k in a["outs"] else None for k, o in enumerate(out)])
        return code, h.last_error()

    def changed(name, index, value):
        a = np.array(good[name], copy=True)
        a[index] = value
        return {name: a}
    cases = [
        (changed("rp", 0, 1), "row_ptr[0]"), (changed("rp", 4, b.row_ptr[3] - 1), "decreases"), (changed("rp", 1, -1), "decreases at set 0"),
        (changed("q", 3, -1.0), "q of correspondence 3"), (changed("q", 3, np.nan), "q of correspondence 3"),
        (changed("a", (40, 1), np.nan), "a of correspondence 40"), (changed("b", (2, 0), np.inf), "b of correspondence 2"),
        (dict(lo=(0, ac.TAU, 1, 1, 2)), "hypotheses"), (dict(lo=(4097, ac.TAU, 1, 1, 2)), "hypotheses"), (dict(lo=(64, 0.0, 1, 1, 2)), "inlier_distance"),
        (dict(lo=(64, np.inf, 1, 1, 2)), "inlier_distance"), (dict(lo=(64, ac.TAU, 1, 1, 17)), "refine_rounds"), (dict(lo=(64, ac.TAU, 1, 2, 2)), "with_scale"),
        (dict(a=None), "NULL correspondence array"), (dict(b=None), "NULL correspondence array"),
        (dict(outs=(1, 2, 3, 4, 5)), "NULL output array"), (dict(outs=(0, 1, 2, 4, 5)), "NULL output array"), (dict(outs=(0, 1, 2, 3, 5)), "NULL output array"),
    ]
    for kw, text in cases:
        code, why = call(**kw)
        assert code == -1 and text in why, (text, code, why)
        assert AL.last_kernel_ms(h) == ms
    assert all(np.all(a == 7) for a in out)                    # nothing written
    code, _ = call(outs=(0, 1, 2, 3, 4))                       # inlier_out may be NULL
    assert code == 0 and not np.any(out[1] == 7) and np.all(out[5] == 7)
    code, _ = call()                                           # and the same call with good arguments runs
    assert code == 0 and not np.any(out[5] == 7) and AL.last_kernel_ms(h)[0] > 0
    with pytest.raises(ValueError):
        sa.align_points(h, b.row_ptr, b.a, b.b)                # the Python entry: inlier_distance has no default
    assert "inlier_distance" in h.last_error()


# ------------------------------------------------------------------ the C++ adapter
def test_cpp_adapter_align(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "align_adapter"
    r = subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "demos"),
                        os.path.join(ROOT, "tests", "cpp", "test_align_adapter.cpp"), "-o", str(exe),
                        "-L", os.path.join(ROOT, "surikatoko_amd"), "-lsrk_ba",
                        "-Wl,-rpath," + os.path.join(ROOT, "surikatoko_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "align adapter ok" in r.stdout
