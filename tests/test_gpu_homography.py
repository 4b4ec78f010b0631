"""The two-view homography on the device: the kernels of srk_homog.hip against the numpy yardstick
(tests/homography_ref.py: DLT, lstsq, SVD) on the cases of tests/homography_cases.py, the bits, the status words, the outliers, one
case end to end next to relate_frames, the argument checks and the C++ adapter."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import _lib
from surikatoko_amd import ba as B
from surikatoko_amd import homography as HG
import homography_cases as hc
import homography_ref as ref
from homography_cases import bounds, outlier_conditions

pytestmark = pytest.mark.gpu
ROOT = hc.ROOT


@pytest.fixture(scope="module")
def h():
    ba = sa.BundleAdjustmentKanatani(0)
    yield ba
    ba.close()


def _run(h, b, q="own", **kw):
    kw.setdefault("inlier_pixels", hc.TAU)
    kw.setdefault("want_inliers", True)
    return sa.relate_homography(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb, q=b.q if isinstance(q, str) else q, **kw)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1)


def _same_bits(a, b, fields=("G", "H", "n_poses", "R", "T", "N", "front", "homog", "status")):
    return all(np.array_equal(_bits(getattr(a, f)), _bits(getattr(b, f))) for f in fields)


def _pair(res, i, s=None):
    """pair i of a result as a result of one pair (inliers: the slice s)"""
    return HG.HomographyResult(*[res[k][i:i + 1] for k in range(9)], None if s is None else res.inliers[s])


# ------------------------------------------------------------------ against the yardstick
@pytest.mark.parametrize("rounds", hc.ROUNDS)
@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("hypotheses", hc.HYPOTHESES)
def test_every_length_against_the_yardstick(h, hypotheses, holes, rounds):
    b = hc.ragged(holes)
    got = _run(h, b, hypotheses=hypotheses, seed=hc.SAMPLER_SEED[(holes, hypotheses)], refine_rounds=rounds)
    worst = hc.agree(b, hc.ragged_yardstick(holes, hypotheses, rounds), got, *bounds())
    print(f"H {hypotheses} holes {holes} rounds {rounds}: score {worst[0]:.3e} relative, corners {worst[1]:.3e} px; bounds {bounds()}")


@pytest.mark.parametrize("n_pairs", hc.BATCH_SIZES)
def test_batches_of_unequal_pairs(h, n_pairs):
    b = hc.many(n_pairs)
    got = _run(h, b, hypotheses=64)
    hc.agree(b, hc.many_yardstick(n_pairs), got, *bounds())
    if n_pairs > 4:
        assert got.status[2] == HG.HOMOGRAPHY_FEW_POINTS and got.homog[2, 1] == 0


def test_a_pairs_bits_do_not_depend_on_the_batch(h):
    b = hc.many(17)
    whole = _run(h, b, hypotheses=65, seed=5)
    for i in range(b.n):
        one = hc.rows(b, [i])
        alone = _run(h, one, hypotheses=65, seed=5)
        s = slice(int(b.row_ptr[i]), int(b.row_ptr[i + 1]))
        assert _same_bits(alone, _pair(whole, i)), i
        assert np.array_equal(alone.inliers, whole.inliers[s]), i
    shared = hc.SimpleNamespace(**{**vars(b), "Ka": b.Ka[:1], "Kb": b.Kb[:1]})       # one K for all: the same bits again
    assert _same_bits(_run(h, shared, hypotheses=65, seed=5), whole)


def test_unit_information_is_no_information_and_zero_is_absence(h):
    b = hc.ragged(True)
    short, keep = hc.without_holes(b)
    x, y = _run(h, b, hypotheses=65, seed=7), _run(h, short, hypotheses=65, seed=7)
    assert _same_bits(x, y)
    assert np.array_equal(x.inliers[keep], y.inliers) and not x.inliers[~keep].any()
    one, none = _run(h, short, q=np.ones_like(short.q), hypotheses=65, seed=7), _run(h, short, q=None, hypotheses=65, seed=7)
    assert _same_bits(one, none) and np.array_equal(one.inliers, none.inliers)


def test_no_rounds_return_the_winning_hypothesis_and_rounds_never_raise_the_score(h):
    b = hc.ragged(False)
    base = _run(h, b, hypotheses=64, seed=3, refine_rounds=0)
    host = hc.host_walk(b, 64, 3, rounds=0)
    assert not base.homog[:, 5].any() and np.array_equal(base.homog[:, [1, 2, 4, 5]], host.homog[:, [1, 2, 4, 5]]) and np.array_equal(base.inliers, host.inliers)
    big = base.homog[:, 1] >= 8                  # below eight matches the samples repeat and the winner is one of a tie
    assert np.array_equal(base.homog[big, 3], host.homog[big, 3])
    last = base.homog[:, 0]
    for rounds in (1, 4, 16):
        got = _run(h, b, hypotheses=64, seed=3, refine_rounds=rounds)
        assert np.array_equal(got.homog[:, 3], base.homog[:, 3]) and (got.homog[:, 5] <= rounds).all() and (got.homog[:, 0] <= last).all()
        last = got.homog[:, 0]
    assert (last < base.homog[:, 0]).any()


# ------------------------------------------------------------------ noise-free pairs
def test_noise_free_planes(h):
    b, ps = hc.planar_pairs()
    got = _run(h, b, hypotheses=64, inlier_pixels=hc.OUTLIER_TAU)
    for i, p in enumerate(ps):
        assert got.status[i] == 0 and got.n_poses[i] == 2 and got.homog[i, 2] == 40 and got.inliers[40 * i:40 * i + 40].all()
        hc.check_poses(got, i)
        d = [max(np.abs(got.R[i, k] - p.R).max(), np.abs(got.T[i, k] - p.T / hc.PLANE_D).max(), np.abs(got.N[i, k] - hc.PLANE_N).max()) for k in range(2)]
        print(f"plane {i}: the candidates' distances from the truth {d[0]:.3e}, {d[1]:.3e}")
        assert min(d) <= 1e-9 and max(d) > 1e-3 and got.front[i, 0] == 40
        assert ref.corner_distance(got.G[i], hc.true_homography(p), hc.F0) <= 1e-9


def test_noise_free_rotations(h):
    b, ps = hc.rotation_pairs()
    got = _run(h, b, hypotheses=64, inlier_pixels=hc.OUTLIER_TAU)
    for i, p in enumerate(ps):
        assert got.status[i] == 0 and got.n_poses[i] == 1 and got.homog[i, 6] <= 1e-10
        assert np.abs(got.R[i, 0] - p.R).max() <= 1e-9 and not got.T[i].any() and not got.N[i].any() and not got.R[i, 1].any()
        assert got.homog[i, 2] == 40 and got.inliers[40 * i:40 * i + 40].all()
        hc.check_poses(got, i)


@pytest.mark.parametrize("share", [0.3, 0.5])
def test_outliers(h, share):
    b, ps = hc.outliers(share)
    got = _run(h, b, hypotheses=hc.outlier_hypotheses(share), inlier_pixels=hc.OUTLIER_TAU, refine_rounds=hc.OUTLIER_ROUNDS)
    have = outlier_conditions(b, ps, dict(inliers=[got.inliers[:200], got.inliers[200:]], G=got.G))
    print(f"share {share}: (unmoved flagged, moved flagged, corner px) {have}, rounds {got.homog[:, 5]}")
    hc.agree(b, hc.outlier_yardstick(share), got, *bounds())


# ------------------------------------------------------------------ status words
def test_status_words(h):
    b = hc.status_cases()
    got = _run(h, b, hypotheses=64)
    assert got.status.tolist() == [HG.HOMOGRAPHY_FEW_POINTS, HG.HOMOGRAPHY_FEW_POINTS, HG.HOMOGRAPHY_NO_MODEL, 0]
    assert got.homog[:, 1].tolist() == [0, 3, 4, 8] and got.homog[2, 4] == 0
    for i in range(3):
        assert np.array_equal(got.G[i], np.eye(3)) and np.array_equal(got.H[i], np.eye(3)) and got.n_poses[i] == 0
        assert not got.R[i].any() and not got.T[i].any() and not got.N[i].any() and not got.front[i].any()
        assert np.isnan(got.homog[i, [0, 3, 6, 7]]).all() and got.homog[i, 2] == 0 and got.homog[i, 5] == 0
    assert not got.inliers[:7].any() and got.n_poses[3] == 2
    host = hc.host_walk(b, 64, 1)
    assert np.array_equal(host.status, got.status) and np.array_equal(host.homog[:3], got.homog[:3], equal_nan=True)


# ------------------------------------------------------------------ end to end, next to relate
def test_plane_end_to_end_next_to_relate(h):
    """A planar pair of 120 matches with half a pixel of noise through relate_frames and relate_homography; the homography's
    candidate nearer to the truth, then triangulate_tracks from (I, 0) and (R, T / d): in those units the plane is N^T X = 1.
    A depth from two views carries z^2 sigma / (f b): z = 1, sigma = 0.5 sqrt(2) px, f = 750 px, b = |T| / d = 0.17 give 0.006; the
    test allows the RMS twice and the largest of 120 five times that.  Both calls' inlier counts and RMS go to test_figures.json;
    nothing is asserted between the two models."""
    rng = np.random.default_rng(2780)
    p = hc.hpair(120, rng, "planar", sigma=0.5)
    b = hc.batch([p])
    hg = _run(h, b, hypotheses=64)
    rel = sa.relate_frames(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb, hypotheses=256, inlier_pixels=2.0, want_inliers=True)
    assert hg.status[0] == 0 and hg.n_poses[0] == 2
    k = int(np.argmin([np.abs(hg.R[0, c] - p.R).max() + np.abs(hg.N[0, c] - hc.PLANE_N).max() for c in range(2)]))
    R, T, N = hg.R[0, k], hg.T[0, k], hg.N[0, k]
    keep = np.flatnonzero(hg.inliers)
    n = len(keep)
    row_ptr = 2 * np.arange(n + 1, dtype=np.int64)
    frame = np.tile(np.array([0, 1], np.int32), n)
    uv = np.stack([b.uv_a[keep], b.uv_b[keep]], axis=1).reshape(-1, 2)
    X, quality, status = sa.triangulate_tracks(h, b.f0, row_ptr, frame, uv, np.array([np.eye(3), R]), np.array([np.zeros(3), T]), np.array([p.Ka, p.Kb]))[:3]
    assert not status.any()
    off = X @ N - 1.0
    print(f"end to end: homography {int(hg.homog[0, 2])} inliers, RMS {hg.homog[0, 7]:.3f} px; relate {int(rel.related[0, 2])} inliers, "
          f"RMS truncated {rel.related[0, 0]:.3f} px; plane offsets RMS {np.sqrt((off ** 2).mean()):.4f}, largest {np.abs(off).max():.4f}")
    assert np.sqrt((off ** 2).mean()) <= 0.012 and np.abs(off).max() <= 0.03
    hc.write_figures("plane_end_to_end", dict(matches=120, homography_inliers=int(hg.homog[0, 2]), homography_inlier_rms_pixels=float(hg.homog[0, 7]),
                                              homography_rms_truncated_pixels=float(hg.homog[0, 0]), relate_inliers=int(rel.related[0, 2]),
                                              relate_rms_truncated_pixels=float(rel.related[0, 0]), plane_offset_rms=float(np.sqrt((off ** 2).mean())),
                                              plane_offset_largest=float(np.abs(off).max())))


# ------------------------------------------------------------------ bad arguments
def test_bad_arguments_launch_nothing(h):
    """one case per check through the handle: the text is set, the outputs and the kernel time of the last good call stay what they were"""
    b = hc.ragged(True)
    _run(h, b, hypotheses=64)
    ms = HG.last_kernel_ms(h)
    assert ms[0] > 0 and 0 < ms[1] <= ms[0]
    O, n = int(b.row_ptr[-1]), b.n
    out = [np.full((n, 9), 7.0), np.full((n, 9), 7.0), np.full(n, 7, np.int32), np.full((n, 18), 7.0), np.full((n, 6), 7.0), np.full((n, 6), 7.0),
           np.full((n, 2), 7, np.int32), np.full((n, 8), 7.0), np.full(n, 7, np.uint32), np.full(O, 7, np.uint8)]
    good = dict(rp=b.row_ptr, a=b.uv_a, b=b.uv_b, q=b.q, ka=b.Ka, kb=b.Kb, f0=b.f0, lo=(64, hc.TAU, 1, 4), outs=tuple(range(10)))

    def call(**kw):
        a = dict(good, **kw)
        arr = {k: None if a[k] is None else np.ascontiguousarray(a[k], np.int64 if k == "rp" else np.float64) for k in ("rp", "a", "b", "q", "ka", "kb")}
        lo = _lib.HomographyOptions(*a["lo"])
        p = {k: None if v is None else B._p(v) for k, v in arr.items()}
        code = sa.lib().srk_relate_homography(C.c_void_p(h._h), C.c_double(a["f0"]), C.c_int32(n), p["rp"], p["a"], p["b"], p["q"], p["ka"], p["kb"],
                                              C.c_int(0), C.byref(lo), *[B._p(o) if k in a["outs"] else None for k, o in enumerate(out)])
        return code, h.last_error()

    def changed(name, index, value):
        a = np.array(good[name], copy=True)
        a[index] = value
        return {name: a}
    cases = [
        (changed("rp", 0, 1), "row_ptr[0]"), (changed("rp", 4, b.row_ptr[3] - 1), "decreases"), (changed("rp", 1, -1), "decreases at pair 0"),
        (changed("q", 3, -1.0), "q of match 3"), (changed("q", 3, np.nan), "q of match 3"),
        (changed("a", (40, 1), np.nan), "uv_a of match 40"), (changed("b", (2, 0), np.inf), "uv_b of match 2"),
        (changed("ka", (1, 0, 0), np.nan), "K_a of pair 1 is not finite"), (changed("kb", (2, 2, 2), 0.0), "K_b of pair 2 is singular"),
        (dict(lo=(0, hc.TAU, 1, 4)), "hypotheses"), (dict(lo=(4097, hc.TAU, 1, 4)), "hypotheses"), (dict(lo=(64, 0.0, 1, 4)), "inlier_pixels"),
        (dict(lo=(64, np.inf, 1, 4)), "inlier_pixels"), (dict(lo=(64, hc.TAU, 1, 17)), "refine_rounds"), (dict(lo=(64, hc.TAU, 1, -1)), "refine_rounds"),
        (dict(f0=0.0), "f0"), (dict(f0=np.nan), "f0"), (dict(a=None), "NULL match array"), (dict(kb=None), "intrinsics array is NULL"),
    ] + [(dict(outs=tuple(k for k in range(10) if k != miss)), "NULL output array") for miss in range(9)]
    for kw, text in cases:
        code, why = call(**kw)
        assert code == -1 and text in why, (text, code, why)
        assert HG.last_kernel_ms(h) == ms
    assert all(np.all(a == 7) for a in out)                    # nothing written
    code, _ = call(outs=tuple(range(9)))                       # inlier_out may be NULL
    assert code == 0 and not np.any(out[0] == 7) and np.all(out[9] == 7)
    code, _ = call()                                           # and the same call with good arguments runs
    assert code == 0 and not np.any(out[9] == 7) and HG.last_kernel_ms(h)[0] > 0


# ------------------------------------------------------------------ the C++ adapter
def test_cpp_adapter_homography(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "homog_adapter"
    r = subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "demos"),
                        os.path.join(ROOT, "tests", "cpp", "test_homog_adapter.cpp"), "-o", str(exe),
                        "-L", os.path.join(ROOT, "surikatoko_amd"), "-lsrk_ba",
                        "-Wl,-rpath," + os.path.join(ROOT, "surikatoko_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "homography adapter ok" in r.stdout
