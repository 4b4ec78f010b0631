"""Two-view relative pose on the device: the kernels of srk_relate.hip against the numpy yardstick
(tests/relate_ref.py) on the cases of tests/relate_cases.py, the bits, the status words, the argument checks and the bootstrap of a
two-frame scene end to end, and the C++ adapter."""
import ctypes as C
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import _lib
from surikatoko_amd import relate as RL
import relate_cases as rc
import relate_ref as ref

pytestmark = pytest.mark.gpu
# the distance allowed between the device's pose and the yardstick's at the same winner: both are double-precision solutions of one
# minimal problem polished on the constraints themselves, so they differ by rounding (1e-16) times the conditioning of the sample,
# which the noise-free samples of the CPU test put at 1e5 and less; two more digits for a sample of noisy matches
POSE_BOUND = 1e-9


@pytest.fixture(scope="module")
def h():
    ba = sa.BundleAdjustmentKanatani(0)
    yield ba
    ba.close()


def _run(h, b, q="own", **kw):
    kw.setdefault("inlier_pixels", rc.TAU)
    return sa.relate_frames(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb, q=b.q if isinstance(q, str) else q, want_inliers=True, **kw)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1)


def _pair_bits(res, b, i):
    s = slice(int(b.row_ptr[i]), int(b.row_ptr[i + 1]))
    return np.concatenate([_bits(res.R[i]), _bits(res.T[i]), _bits(res.E[i]), _bits(res.related[i]), _bits(res.status[i:i + 1]), res.inliers[s]])


# ------------------------------------------------------------------ accuracy
def test_noise_free(h):
    """40 noise-free matches, general, planar and forward motion: R and T within max(1e-13, 64 x the yardstick's own distance from
    the truth on the same pair); every match an inlier in front of both cameras.  The pure rotation: the call succeeds, R within
    the same bound, the parallax below 1e-6 rad, nothing asserted on T."""
    b = rc.accuracy()
    ys = rc.batch_yardstick("accuracy", 64)
    res = _run(h, b, hypotheses=64)
    assert np.all(res.status == 0)
    for i, kind in enumerate(rc.ACCURACY_KINDS):
        dr, dt = rc.pose_error(res.R[i], res.T[i], b.R[i], b.T[i])
        yr, yt = rc.pose_error(ys[i]["R"], ys[i]["T"], b.R[i], b.T[i])
        print(f"{kind}: rotation {dr:.2e} rad (yardstick {yr:.2e}), direction {dt:.2e} rad (yardstick {yt:.2e}), parallax {res.related[i, 7]:.3e}")
        assert dr <= max(1e-13, 64.0 * yr), (i, dr, yr)
        assert res.related[i, 2] == 40 and res.inliers[40 * i:40 * i + 40].all()
        if kind == "rotation":
            assert res.related[i, 7] < 1e-6
            continue
        assert dt <= max(1e-13, 64.0 * yt), (i, dt, yt)
        assert res.related[i, 6] == 40 and res.related[i, 0] < 1e-6
        assert abs(np.linalg.norm(res.T[i]) - 1.0) <= 1e-12 and np.abs(res.E[i] - ref.skew(res.T[i]) @ res.R[i]).max() <= 1e-15


# ------------------------------------------------------------------ every length, every hypothesis count
@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("hypotheses", rc.HYPOTHESES)
def test_every_length_against_the_yardstick(h, holes, hypotheses):
    b = rc.ragged(holes)
    worst = rc.agree(b, rc.ragged_yardstick(holes, hypotheses), _run(h, b, hypotheses=hypotheses), POSE_BOUND)
    print(f"holes {holes}, {hypotheses} hypotheses: largest pose distance to the yardstick {worst:.3e}")


@pytest.mark.parametrize("count", rc.BATCH_SIZES)
def test_batches_of_unequal_pairs(h, count):
    b = rc.many(count)
    rc.agree(b, rc.batch_yardstick((count,), 65), _run(h, b, hypotheses=65), POSE_BOUND)


# ------------------------------------------------------------------ the bits
def test_a_pairs_bits_do_not_depend_on_the_batch(h):
    big = rc.many(17)
    whole = _run(h, big, hypotheses=65)
    for i in (0, 5, 16):
        alone = _run(h, rc.rows(big, [i]), hypotheses=65)
        assert np.array_equal(_pair_bits(alone, rc.rows(big, [i]), 0), _pair_bits(whole, big, i)), i
        for order in ([i, 1, 3, 9], [1, 3, 9, i], [7, 2, i, 11, 4]):        # first, last, among pairs of other lengths (2 is empty)
            sub = rc.rows(big, order)
            res = _run(h, sub, hypotheses=65)
            assert np.array_equal(_pair_bits(res, sub, order.index(i)), _pair_bits(whole, big, i)), (i, order)


def test_q_zero_is_the_pair_without_the_match(h):
    b = rc.ragged(True)
    short, keep = rc.without_holes(b)
    a, c = _run(h, b, hypotheses=65, seed=7), _run(h, short, hypotheses=65, seed=7)
    for x, y in ((a.R, c.R), (a.T, c.T), (a.E, c.E), (a.related, c.related), (a.status, c.status), (a.inliers[keep], c.inliers)):
        assert np.array_equal(_bits(x), _bits(y))
    assert not a.inliers[~keep].any()
    one, none = _run(h, short, q=np.ones_like(short.q), hypotheses=65), _run(h, short, q=None, hypotheses=65)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(one, none))


# ------------------------------------------------------------------ outliers
@pytest.mark.parametrize("share", [0.3, 0.5])
def test_outliers(h, share):
    """200 matches, a share of them replaced by uniform points, one pixel of noise, ransac_hypotheses(share, 0.999, 5) samples, a
    threshold of four pixels: the yardstick recovers at least 95 % of the matches that were not moved and flags at most 5 % of
    the moved ones (asserted here on the CPU side; the seeds of relate_cases were chosen for it), and the device returns the
    yardstick's winner and inlier flags, so it meets the same figures."""
    key = "out3" if share == 0.3 else "out5"
    b, H = rc.outliers(share), RL.ransac_hypotheses(share, 0.999, 5)
    assert H == rc.outlier_hypotheses(share)
    ys = rc.batch_yardstick(key, H)
    moved = np.zeros(int(b.row_ptr[-1]), bool)
    moved[b.moved] = True
    for i, y in enumerate(ys):
        s = slice(int(b.row_ptr[i]), int(b.row_ptr[i + 1]))
        inl, mv = y["inliers"].astype(bool), moved[s]
        assert inl[~mv].mean() >= 0.95 and inl[mv].mean() <= 0.05, (i, inl[~mv].mean(), inl[mv].mean())
    rc.agree(b, ys, _run(h, b, hypotheses=H, inlier_pixels=rc.OUTLIER_TAU), POSE_BOUND)


# ------------------------------------------------------------------ the status words
def test_status_words(h):
    rng = np.random.default_rng(2470)
    five = rc.pair(8, rng, sigma=0.5)                                  # eight matches, five of them weighted
    same = rc.pair(12, rng)
    same.uv_a[:], same.uv_b[:] = same.uv_a[0], same.uv_b[0]            # one point twelve times: no essential matrix
    good = rc.pair(30, rng, sigma=0.5)
    b = rc.batch([good, five, rc.pair(0, rng), same, good])
    b.q = np.ones(int(b.row_ptr[-1]))
    b.q[30:33] = 0.0
    res = _run(h, b, hypotheses=65)
    assert res.status.tolist() == [0, RL.RELATE_FEW_POINTS, RL.RELATE_FEW_POINTS, RL.RELATE_NO_MODEL, 0]
    for i in (1, 2, 3):
        assert np.array_equal(res.R[i], np.eye(3)) and not res.T[i].any() and not res.E[i].any()
        assert np.isnan(res.related[i, [0, 3, 5, 7]]).all() and res.related[i, 2] == 0 and res.related[i, 6] == 0
        assert not res.inliers[b.row_ptr[i]:b.row_ptr[i + 1]].any()
    assert res.related[1, 1] == 5 and res.related[2, 1] == 0 and res.related[3, 1] == 12 and res.related[3, 4] == 0
    alone = _run(h, rc.rows(b, [0]), hypotheses=65)                     # the neighbours' bits are those of the pair alone
    assert np.array_equal(_pair_bits(alone, rc.rows(b, [0]), 0), _pair_bits(res, b, 0))
    assert np.array_equal(_pair_bits(alone, rc.rows(b, [0]), 0)[:-30], _pair_bits(res, b, 4)[:-30])
    assert RL.relate_status_names(res.status[3]) == ["NO_MODEL"]


# ------------------------------------------------------------------ bad arguments
def test_bad_arguments_launch_nothing(h):
    """one case per check: SRK_E_ARGS, the text is set, the outputs and the kernel time of the last good call stay what they were"""
    b = rc.ragged(True)
    _run(h, b, hypotheses=5)
    ms = RL.last_kernel_ms(h)
    assert ms[0] > 0 and 0 < ms[1] <= ms[0]
    n, O = b.n, int(b.row_ptr[-1])
    L = _lib.lib()
    out = [np.full((n, 9), -7.5), np.full((n, 3), -7.5), np.full((n, 9), -7.5), np.full((n, 8), -7.5), np.full(n, 7, np.uint32), np.full(O, 7, np.uint8)]
    base = dict(f0=b.f0, row_ptr=b.row_ptr.copy(), uv_a=b.uv_a.copy(), uv_b=b.uv_b.copy(), q=b.q.copy(), Ka=b.Ka.copy(), Kb=b.Kb.copy(),
                opts=(64, rc.TAU, 1), null=())

    def call(**kw):
        a = {**base, **kw}
        lo = _lib.RelateOptions(*a["opts"])
        ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
        outs = [None if k in a["null"] else ptr(o) for k, o in enumerate(out)]
        code = L.srk_relate_frames(C.c_void_p(h._h), C.c_double(a["f0"]), C.c_int32(n), ptr(a["row_ptr"]), ptr(a["uv_a"]), ptr(a["uv_b"]), ptr(a["q"]),
                                   ptr(a["Ka"]), ptr(a["Kb"]), C.c_int(0), C.byref(lo), *outs)
        return code, h.last_error()

    def changed(key, where, value):
        x = base[key].copy()
        x[where] = value
        return {key: x}
    cases = [(changed("row_ptr", 3, b.row_ptr[2] - 1), "decreases at pair 2"), (changed("row_ptr", 0, -1), "row_ptr[0]"),
             (changed("uv_a", (4, 0), np.nan), "uv_a of match 4"), (changed("uv_b", (5, 1), np.inf), "uv_b of match 5"),
             (changed("Ka", (1, 0, 0), np.nan), "K_a of pair 1 is not finite"), (changed("Kb", (2, 2), 0.0), "K_b of pair 2 is singular"),
             (changed("q", 3, -0.5), "q of match 3"), (changed("q", 3, np.inf), "q of match 3"),
             (dict(opts=(0, rc.TAU, 1)), "hypotheses outside"), (dict(opts=(4097, rc.TAU, 1)), "hypotheses outside"),
             (dict(opts=(64, 0.0, 1)), "inlier_pixels"), (dict(opts=(64, np.nan, 1)), "inlier_pixels"), (dict(f0=0.0), "f0"),
             (dict(null=(0,)), "NULL output"), (dict(null=(2,)), "NULL output"), (dict(null=(3,)), "NULL output"), (dict(null=(4,)), "NULL output"),
             (dict(uv_b=None), "NULL match array"), (dict(Ka=None), "intrinsics array is NULL")]
    for kw, text in cases:
        code, why = call(**kw)
        assert code == -1, (text, code)                      # SRK_E_ARGS
        assert text in why, (text, why)
        assert RL.last_kernel_ms(h) == ms
    assert all(np.all((a == 7) | (a == -7.5)) for a in out)    # nothing written
    code, _ = call(null=(5,))                                  # inlier_out may be NULL
    assert code == 0 and not np.any(out[3] == -7.5) and not np.any(out[4] == 7) and np.all(out[5] == 7) and RL.last_kernel_ms(h)[0] > 0


# ------------------------------------------------------------------ the bootstrap, end to end
def _bootstrap_case(Kb=rc.K0, seed=2490):
    rng = np.random.default_rng(seed)
    R = rc.rotation(np.array([0.05, -0.12, 0.04]))
    T = np.array([0.55, 0.75, 0.36])
    T /= np.linalg.norm(T)
    X = rc.points(150, rng)
    X[:, 2] *= 0.6
    ua, ub = rc.pixels(rc.K0, X) + 0.5 * rng.normal(size=(150, 2)), rc.pixels(Kb, X @ R.T + T) + 0.5 * rng.normal(size=(150, 2))
    moved = rng.choice(150, 30, replace=False)
    ub[moved] = np.column_stack([rng.uniform(-100.0, 700.0, 30), rng.uniform(-150.0, 600.0, 30)])
    return SimpleNamespace(R=R, T=T, uv_a=ua, uv_b=ub, moved=moved)


def test_bootstrap_end_to_end(h):
    """150 landmarks in two frames, 0.5 px of noise, 20 % wrong matches: two_view_scene, the result uploaded calibrated with frame 0
    constant, ten LM iterations.  The inlier RMS reprojection error ends below 1.5 x the noise, the relative rotation within 0.5
    degrees of the truth and the translation direction within 2 degrees."""
    _bootstrap(h, rc.K0)


def test_bootstrap_end_to_end_with_two_cameras(h):
    """the same with K_a = K0 and K_b = K1: two_view_scene hands [K_a, K_b] on to the triangulation as a two-frame K array, and the
    two-frame scene is uploaded with its two K (shared_k = 0).  The three figures are those of the one-camera case.  The wrong matches
    are uniform points, and one in 200 of those lies within two pixels of its epipolar line: with seed 2490 and K1, match 110 does (a
    host run of RL.host_pair shows it), so this case draws with 2491, where none does.

    The two K are uploaded in the form K f0 (K(2,2) = f0, the same cameras): the adjuster's closed-form pose derivatives are those
    of the error in that form only ("Derivative convention").  In the form K / f0 it rejects every attempt
    on this scene ('hessian overflow', 0 iterations, 153 attempts) and the figures stay two_view_scene's own -- RMS 0.450 px,
    rotation 0.998 degrees, direction 1.281 degrees -- where the one-camera case in that form moves its error by 1e-3 of it in ten
    iterations and passes on two_view_scene's result.  In the form K f0 the adjuster ends, after seven accepted iterations, at
    RMS 0.260 px, 0.141 and 0.106 degrees (an MI355X): to three digits the minimum a scipy adjustment of the same two-view problem
    with the whole K, skew included, reaches on the host."""
    _bootstrap(h, rc.K1, 2491)


def _bootstrap(h, Kb, seed=2490):
    c = _bootstrap_case(Kb, seed)
    K = (rc.K0, Kb)
    H = RL.ransac_hypotheses(0.2, 0.999, 5)
    tv = sa.two_view_scene(h, rc.F0, c.uv_a, c.uv_b, rc.K0, Kb, hypotheses=H, inlier_pixels=rc.TAU)
    assert tv.relate.status[0] == 0 and len(tv.points) >= 100 and not np.isin(tv.match, c.moved).any()
    if Kb is rc.K0:
        scene = sa.Scene(tv.points, tv.cam_R, tv.cam_T, rc.K0.reshape(1, 9), 1, tv.row_ptr, tv.obs_frame, tv.obs_uv)
    else:
        scene = sa.Scene(tv.points, tv.cam_R, tv.cam_T, np.stack(K).reshape(2, 9) * rc.F0, 0, tv.row_ptr, tv.obs_frame, tv.obs_uv)
    ba = sa.BundleAdjustmentKanatani(0)
    try:
        ba.set_fixed_intrinsics(True)
        ba.set_constant_blocks(frames=[0], n_frames=2, n_points=len(tv.points))
        assert ba.upload(rc.F0, scene)
        ba.optimize(max_iterations=10)
        r = ba.report
        print(f"bootstrap: the adjuster ended '{ba.OptimizationStatusString()}' after {r.iterations} iterations, {r.attempts} attempts, "
              f"error {r.err_initial:.6e} -> {r.err_final:.6e}")
        assert r.iterations > 0 and r.err_final < r.err_initial     # it did adjust: the figures below are not two_view_scene's alone
        ba.download(scene)
    finally:
        ba.close()
    Rs, Ts = scene.cam_R.reshape(2, 3, 3), scene.cam_T.reshape(2, 3)
    Rrel = Rs[1] @ Rs[0].T
    Trel = Ts[1] - Rrel @ Ts[0]
    err = []
    for f in range(2):
        uv = rc.pixels(K[f], scene.points @ Rs[f].T + Ts[f])
        err.append(uv - tv.obs_uv.reshape(-1, 2, 2)[:, f])
    rms = float(np.sqrt(np.mean(np.sum(np.concatenate(err) ** 2, axis=1)) / 2.0))   # per coordinate, as the noise is
    dr, dt = np.degrees(ref.rotation_angle(Rrel, c.R)), np.degrees(ref.direction_angle(Trel, c.T))
    print(f"bootstrap: {len(tv.points)} landmarks, RMS {rms:.3f} px per coordinate, rotation {dr:.3f} deg, direction {dt:.3f} deg")
    assert rms < 1.5 * 0.5 and dr < 0.5 and dt < 2.0


# ------------------------------------------------------------------ the C++ adapter
def test_cpp_adapter_relate(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "relate_adapter"
    r = subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(rc.ROOT, "include"), "-I", os.path.join(rc.ROOT, "demos"),
                        os.path.join(rc.ROOT, "tests", "cpp", "test_relate_adapter.cpp"), "-o", str(exe),
                        "-L", os.path.join(rc.ROOT, "surikatoko_amd"), "-lsrk_ba",
                        "-Wl,-rpath," + os.path.join(rc.ROOT, "surikatoko_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "relate adapter ok" in r.stdout
