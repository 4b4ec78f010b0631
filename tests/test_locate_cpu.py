"""Resection without a start pose, without a GPU: the yardstick (tests/locate_ref.py), the guards that keep
the compared decisions away from rounding, and the host half (surikatoko_amd/csrc/srk_locate.cpp) through a stand-alone program
(tests/cpp/test_locate_host.cpp): the sampler, srk_ransac_hypotheses, P3P alone, the argument checks, and a walk of every frame
on the host in the kernels' own order of operations."""
import json
import os
import subprocess

import numpy as np
import pytest

from surikatoko_amd import locate as LC
import locate_cases as lc
import locate_ref as ref

FIGURES = os.path.join(lc.ROOT, "profiles", "locate", "test_figures.json")


@pytest.fixture(scope="module")
def program():
    if lc.cxx() is None:
        pytest.skip("no host C++ compiler")
    return lc.host_program()


# ------------------------------------------------------------------ the sampler
@pytest.mark.parametrize("n", [4, 5, 64, 1000])
def test_sampler_against_the_yardstick(program, tmp_path, n):
    out = str(tmp_path / "ranks.bin")
    for seed in (1, 0xFFFFFFFFFFFFFFFF):
        r = subprocess.run([program, "sampler", out, str(seed), str(n), "4096"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = np.fromfile(out, np.int64).reshape(4096, 4)
        want = np.array([ref.sample(seed, h, n) for h in range(4096)])
        assert np.array_equal(got, want)
        assert got.min() >= 0 and got.max() < n
        assert all(len(set(row)) == 4 for row in got.tolist())
    if n > 4:
        assert len({tuple(row) for row in got.tolist()}) > 100          # and the draws differ from one another


# ------------------------------------------------------------------ srk_ransac_hypotheses
def test_ransac_hypotheses_against_the_formula():
    assert LC.ransac_hypotheses(0.3, 0.999) == 26 and LC.ransac_hypotheses(0.5, 0.99) == 72
    for e in (0.05, 0.2, 0.3, 0.5, 0.7, 0.9):
        for p in (0.5, 0.9, 0.99, 0.999):
            for s in (1, 3, 4, 7):
                assert LC.ransac_hypotheses(e, p, s) == max(1, ref.ransac_hypotheses(e, p, s)), (e, p, s)
    assert LC.ransac_hypotheses(0.0, 0.99) == 1
    for e, p in ((1.0, 0.9), (-0.1, 0.9), (1.5, 0.9), (0.3, 0.0), (0.3, 1.0), (0.3, -1.0), (np.nan, 0.9), (0.3, np.nan)):
        with pytest.raises(ValueError):
            LC.ransac_hypotheses(e, p)
    with pytest.raises(ValueError):
        LC.ransac_hypotheses(0.3, 0.9, 0)


# ------------------------------------------------------------------ P3P alone
def test_p3p_against_the_yardstick(program, tmp_path):
    """2000 noise-free triples: the host build's nearest solution to the truth against the yardstick's (Grunert's quartic through
    numpy.roots, the pose through an SVD).  Triples where the yardstick's own error exceeds 1e-6 are left out, at most 1 % of
    them; on the rest the host's error is held to ten times the yardstick's at the same quantiles.  Measured (a CPU run):
    left out 0.05 %; median 2.2e-13 against the yardstick's 2.7e-13, maximum 6.5e-7 against 8.7e-7."""
    tr = lc.p3p_triples()
    n = len(tr.X)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        np.array([n], np.int64).tofile(f)
        np.array([lc.F0]).tofile(f)
        np.ascontiguousarray(lc.K0).tofile(f)
        tr.X.tofile(f)
        tr.uv.tofile(f)
    r = subprocess.run([program, "p3p", src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(dst, np.uint8)
    R = raw[:n * 288].view(np.float64).reshape(n, 4, 3, 3)
    T = raw[n * 288:n * 384].view(np.float64).reshape(n, 4, 3)
    ok = raw[n * 384:].view(np.int32).reshape(n, 4)
    yard, host = np.full(n, np.inf), np.full(n, np.inf)
    for i in range(n):
        poses, _ = ref.p3p(tr.X[i], ref.bearings(lc.K0, tr.uv[i], lc.F0))
        yard[i] = min([lc.p3p_error(Ry, Ty, tr.R[i], tr.T[i]) for Ry, Ty in poses] or [np.inf])
        for k in range(4):
            if ok[i, k]:
                Rk = R[i, k]                                                    # the resection's own rotation check
                assert np.abs(Rk.T @ Rk - np.eye(3)).max() <= 1e-9 and abs(np.linalg.det(Rk) - 1.0) <= 1e-9, (i, k)
                host[i] = min(host[i], lc.p3p_error(Rk, T[i, k], tr.R[i], tr.T[i]))
    keep = yard <= 1e-6
    left_out = 1.0 - np.count_nonzero(keep) / n
    figures = dict(triples=n, left_out=left_out, yardstick_median=float(np.median(yard[keep])), yardstick_max=float(yard[keep].max()),
                   host_median=float(np.median(host[keep])), host_max=float(host[keep].max()))
    print("P3P alone:", json.dumps(figures))
    assert left_out <= 0.01
    for quantile in (0.5, 0.9, 0.99, 1.0):
        assert np.quantile(host[keep], quantile) <= 10.0 * np.quantile(yard[keep], quantile), quantile
    if os.path.exists(FIGURES):   # the recorded figures are these, to two digits
        rec = json.load(open(FIGURES))["p3p_cpu"]
        assert all(abs(rec[k] - v) <= 0.05 * abs(v) for k, v in figures.items()), (rec, figures)


# ------------------------------------------------------------------ the guards
def _frames(ys):
    return ys.items() if isinstance(ys, dict) else enumerate(ys)


def _all_cases():
    for holes in (False, True):
        for H in lc.HYPOTHESES:
            yield lc.small(holes), lc.small_yardstick(holes, H), (holes, H)
    yield lc.ragged(False), lc.big_yardstick(False), ("big", lc.BIG_HYPOTHESES)


def test_cases_have_no_frame_at_a_threshold():
    """On every frame the yardstick walks: no hypothesis whose existence hangs on rounding (a nearly double root of the quartic, a
    depth at zero), no observation at the inlier threshold of the located pose, and a clear winner -- the last on the frames of
    more than five points.  A frame of four or five points draws the permutations of one triple again and again (120 ordered
    samples of five points against 63 and more hypotheses), and these give one pose up to rounding and scores that differ in the
    last bits: no seed avoids that, so there the chosen h is held to the yardstick's near-ties (locate_cases.agree)."""
    located = 0
    for b, ys, name in _all_cases():
        for i, y in _frames(ys):
            assert not y["fragile"], (name, i)
            if y["status"]:
                continue
            located += 1
            assert lc.inliers_are_clear(b, i, y), (name, i)
            assert y["located"][1] <= 5 or lc.winner_is_clear(y), (name, i)
    assert located > 60


def test_outlier_cases_mark_no_moved_observation():
    """the yardstick itself on the outlier frames: within 5e-3 rad and 5e-3 of the depth of the truth (its own errors set the GPU
    test's bound), and no moved observation among its inliers"""
    for share in (0.3, 0.5):
        b = lc.outliers(share)
        ys, bound = lc.outlier_yardstick(share)
        print(f"outliers {share}: H = {lc.outlier_hypotheses(share)}, bound {bound[0]:.2e} rad, {bound[1]:.2e} of the depth")
        assert lc.outlier_hypotheses(share) == (64 if share == 0.3 else 256)
        assert bound[0] <= 2e-2 and bound[1] <= 2e-2
        inl = np.concatenate([y["inliers"] for y in ys])
        assert not inl[b.moved].any() and len(b.moved) == int(round(share * 200)) * 8
        assert all(y["status"] == 0 and y["located"][2] >= 0.8 * (1 - share) * 200 for y in ys)


# ------------------------------------------------------------------ the host half
def test_checks_defaults_and_the_hypothesis_count(program):
    r = subprocess.run([program, "unit"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0 failure(s)", r.stdout + r.stderr


def test_unit_runs_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan: the unit checks and a ragged batch with q = 0 in between"""
    if lc.cxx() is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "test_locate_host_san"
    r = lc.build_host_program(exe, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), "unit"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0 failure(s)", r.stdout + r.stderr
    b = lc.small(True)
    got = lc.host_walk(b, 65, 1, program=str(exe))
    assert len(got.status) == b.n


def test_host_walk_against_the_yardstick_on_the_ragged_cases(program):
    """the kernels' order of operations on the host: the same status, winner, inlier count and number of poses as the yardstick,
    the score to 1e-12 at the walk's own pose; the largest pose distance is the floor the GPU tests use"""
    worst = 0.0
    for b, ys, name in _all_cases():
        got = lc.host_walk(b, name[1], lc.SAMPLER_SEED[name[1]])
        worst = max(worst, lc.agree(b, ys, got, got.inliers))
    print(f"host walk against the yardstick: largest pose distance {worst:.3e}; host_floor() {lc.host_floor():.3e}")
    assert worst <= 1e-6    # measured 1.2e-9: two double-precision solutions of one quartic; the device gets 10 x host_floor()
    assert lc.host_floor() <= worst


def test_host_walk_noise_free(program):
    b = lc.accuracy()
    got = lc.host_walk(b, 64, 1)
    floor = lc.accuracy_floor()
    print(f"noise-free frames, host walk: largest distance from the truth {floor:.3e}, largest located[0] {got.located[:, 0].max():.3e} px")
    assert np.all(got.status == 0) and got.located[:, 0].max() < 1e-6 and floor < 1e-6
    assert np.array_equal(got.located[:, 2], got.located[:, 1])


def test_host_walk_q_zero_is_the_frame_without_the_observation(program):
    b = lc.rows(lc.ragged(True), range(40))
    short, keep = lc.without_holes(b)
    a, c = lc.host_walk(b, 65, 7), lc.host_walk(short, 65, 7)
    for x, y in ((a.R, c.R), (a.T, c.T), (a.located, c.located), (a.scores, c.scores), (a.status, c.status), (a.inliers[keep], c.inliers)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert not a.inliers[~keep].any()
    one = lc.SimpleNamespace(**{**vars(short), "q": np.ones_like(short.q)})
    none = lc.SimpleNamespace(**{**vars(short), "q": None})
    a, c = lc.host_walk(one, 65, 7), lc.host_walk(none, 65, 7)
    assert np.array_equal(a.R.view(np.uint8), c.R.view(np.uint8)) and np.array_equal(a.located.view(np.uint8), c.located.view(np.uint8))


# ------------------------------------------------------------------ the Python checks
def test_python_check_frames_and_names():
    b = lc.small(True)
    args = (b.row_ptr, b.point, b.uv, b.X, b.K)
    assert LC.check_frames(*args, q=b.q) is None
    assert LC.check_frames(*args, q=b.q, refine=dict(loss="cauchy", delta=2.0, attempts=20)) is None

    def bad(i, f, **kw):
        a = [np.array(x, copy=True) for x in args]
        f(a[i])
        return LC.check_frames(*a, **kw)
    assert "row_ptr[0]" in bad(0, lambda a: a.__setitem__(0, 1))
    assert "decreases at frame 3" in bad(0, lambda a: a.__setitem__(4, a[3] - 1))
    assert "out of range" in bad(1, lambda a: a.__setitem__(5, len(b.X)))
    assert "out of range" in bad(1, lambda a: a.__setitem__(5, -1))
    assert "uv of observation 7" in bad(2, lambda a: a.__setitem__((7, 1), np.nan))
    assert "landmark 3 is not finite" in bad(3, lambda a: a.__setitem__((3, 0), np.inf))
    assert "K of frame 2 is not finite" in bad(4, lambda a: a.__setitem__((2, 1, 1), np.nan))
    assert "K of frame 2 is singular" in bad(4, lambda a: a.__setitem__((2, 2), np.zeros(3)))
    q = b.q.copy()
    q[9] = -1.0
    assert "q of observation 9" in LC.check_frames(*args, q=q)
    assert "hypotheses outside 1..4096" in LC.check_frames(*args, hypotheses=0) and "hypotheses" in LC.check_frames(*args, hypotheses=4097)
    assert "inlier_pixels" in LC.check_frames(*args, inlier_pixels=0.0) and "inlier_pixels" in LC.check_frames(*args, inlier_pixels=np.nan)
    assert "refine attempts" in LC.check_frames(*args, refine=dict(attempts=65))
    assert "refine rel_change" in LC.check_frames(*args, refine=dict(rel_change=-1.0))
    assert "refine loss needs" in LC.check_frames(*args, refine=dict(loss="huber"))
    assert LC.default_locate_options() == dict(hypotheses=256, inlier_pixels=4.0, seed=1)
    assert LC.locate_status_names(LC.LOCATE_FEW_POINTS | LC.LOCATE_NO_MODEL) == ["FEW_POINTS", "NO_MODEL"]
    with pytest.raises(ValueError):
        LC.check_frames(b.row_ptr, b.point[:5], b.uv, b.X, b.K)
    with pytest.raises(ValueError):
        LC.check_frames(*args, refine=dict(steps=3))
