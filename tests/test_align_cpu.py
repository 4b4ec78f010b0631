"""Map alignment without a GPU: the yardstick (tests/align_ref.py), the guards that keep the compared
decisions away from rounding, and the host half (surikatoko_amd/csrc/srk_align.cpp): the argument checks, a walk of every set on
the host in the kernels' own order of operations (srk_align_host_set), srk_similarity_apply, and through a stand-alone program
(tests/cpp/test_align_host.cpp) the sampler and the unit checks, the latter also under the sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import align as AL
import align_cases as ac
import align_ref as ref


def cxx():
    return shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def build_host_program(out, extra=()):
    return subprocess.run([cxx(), "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ac.ROOT, "tests", "cpp", "test_align_host.cpp"),
                           os.path.join(ac.ROOT, "surikatoko_amd", "csrc", "srk_align.cpp"), "-o", str(out)], capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if cxx() is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("align_bin") / "test_align_host"
    r = build_host_program(exe)
    assert r.returncode == 0, r.stderr
    return str(exe)


# ------------------------------------------------------------------ the sampler
@pytest.mark.parametrize("n", [3, 4, 64, 2 ** 40])
def test_sampler_against_the_yardstick(program, tmp_path, n):
    out = str(tmp_path / "ranks.bin")
    for seed in (1, 0xFFFFFFFFFFFFFFFF):
        r = subprocess.run([program, "sampler", out, str(seed), str(n), "4096"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = np.fromfile(out, np.int64).reshape(4096, 3)
        want = np.array([ref.sample(seed, h, n) for h in range(4096)], dtype=np.int64)
        assert np.array_equal(got, want)
        assert got.min() >= 0 and got.max() < n
        assert all(len(set(row)) == 3 for row in got.tolist())
    if n > 4:
        assert len({tuple(row) for row in got.tolist()}) > 100          # and the draws differ from one another


# ------------------------------------------------------------------ the stand-alone program
def test_unit_checks_of_the_host_half(program):
    r = subprocess.run([program, "unit"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0 failure(s)", r.stdout + r.stderr


def test_unit_runs_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan: the checks, three walks and srk_similarity_apply"""
    if cxx() is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "test_align_host_san"
    r = build_host_program(exe, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), "unit"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0 failure(s)", r.stdout + r.stderr


# ------------------------------------------------------------------ the guards
def _all_cases():
    for holes in (False, True):
        for H in ac.HYPOTHESES:
            yield ac.small(holes), ac.small_yardstick(holes, H), (holes, H)
    yield ac.ragged(False), ac.big_yardstick(False), ("big", ac.BIG_HYPOTHESES)


def test_cases_have_no_set_at_a_threshold():
    """On every set the yardstick walks: no correspondence at the inlier threshold of a model whose inliers are taken, no
    candidate's score within rounding of the score it has to beat (an exactly equal score is a repeated model and is refused on
    both sides), and on the sets of more than four correspondences a clear winner.  Sets of three and four draw the orderings of
    one or four triples again and again; there the chosen h is held to the yardstick's near-ties (align_cases.agree)."""
    aligned = 0
    for b, ys, name in _all_cases():
        for i, y in (ys.items() if isinstance(ys, dict) else enumerate(ys)):
            if y["status"]:
                continue
            aligned += 1
            assert y["edge"] >= 1e-6 and y["stage"]["edge"] >= 1e-6, (name, i)
            assert not 0.0 < y["margin"] < 1e-9, (name, i)
            assert y["aligned"][1] <= 4 or ac.winner_is_clear(y), (name, i)
    assert aligned > 100


def test_outlier_cases_meet_the_condition_on_the_yardstick():
    """the yardstick alone on the outlier sets: no moved correspondence is an inlier and every unmoved one is, at H = the
    reference's count for three-point samples rounded up to a wave"""
    for share in (0.3, 0.5):
        b, ys = ac.outliers(share), ac.outlier_yardstick(share)
        assert ac.outlier_hypotheses(share) == -(-ref_count(share) // 64) * 64 == 64
        inl = np.concatenate([y["inliers"] for y in ys])
        moved = np.zeros(len(inl), bool)
        moved[b.moved] = True
        assert len(b.moved) == int(round(share * 200)) * 8
        assert not inl[moved].any() and inl[~moved].all()
        assert all(y["status"] == 0 and y["edge"] >= 1e-6 and ac.winner_is_clear(y) for y in ys)


def ref_count(share):
    return int(np.ceil(np.log(1 - 0.999) / np.log(1 - (1 - share) ** 3)))


# ------------------------------------------------------------------ the host walk
def test_host_walk_against_the_yardstick_on_the_ragged_cases():
    """the kernels' order of operations on the host against the SVD route: the same status, winner, counts, rounds and flags, the
    score to 1e-12 at the walk's own model; the largest model distance is the floor the GPU tests use"""
    worst = 0.0
    for b, ys, name in _all_cases():
        for rounds in (0, 2):
            got = ac.host_walk(b, name[1], ac.SAMPLER_SEED[name[1]], refine_rounds=rounds)
            worst = max(worst, ac.agree(b, ys, got, got.inliers, stage=rounds == 0))
    print(f"host walk against the yardstick: largest model distance {worst:.3e}; host_floor() {ac.host_floor():.3e}")
    # two double-precision routes to one least-squares problem whose conditioning (the triad's 1 / sin, the inliers' spread) is of
    # order 10 to 100 on these sets: a few hundred roundings
    assert worst <= 1e-12
    assert 0.0 < ac.host_floor() <= worst


@pytest.mark.parametrize("with_scale", [True, False])
def test_host_walk_noise_free(with_scale):
    for scale in ac.SCALES:
        b = ac.accuracy(with_scale, scale)
        got = ac.host_walk(b, 64, 1, tau=ac.accuracy_tau(b), with_scale=with_scale)
        floor = ac.accuracy_floor(with_scale, scale)
        print(f"noise-free sets, with_scale {with_scale}, scale {scale}: the host walk's largest distance from the truth {floor:.3e}")
        # the far set: coordinates of 1e6 carry 1e6 eps = 2e-10 absolute, over an extent of 4 s
        assert np.all(got.status == 0) and floor < 1e-7
        assert np.array_equal(got.aligned[:, 2], got.aligned[:, 1]) and got.inliers.all()
        if not with_scale:
            assert np.all(got.s == 1.0)


def test_host_walk_q_zero_is_the_set_without_the_correspondence():
    b = ac.rows(ac.ragged(True), range(40))
    short, keep = ac.without_holes(b)
    x, y = ac.host_walk(b, 65, 7), ac.host_walk(short, 65, 7)
    for u, v in ((x.s, y.s), (x.R, y.R), (x.t, y.t), (x.aligned, y.aligned), (x.status, y.status), (x.inliers[keep], y.inliers)):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    assert not x.inliers[~keep].any()
    one = ac.SimpleNamespace(**{**vars(short), "q": np.ones_like(short.q)})
    none = ac.SimpleNamespace(**{**vars(short), "q": None})
    x, y = ac.host_walk(one, 65, 7), ac.host_walk(none, 65, 7)
    assert np.array_equal(x.R.view(np.uint8), y.R.view(np.uint8)) and np.array_equal(x.aligned.view(np.uint8), y.aligned.view(np.uint8))


# ------------------------------------------------------------------ apply_similarity
def test_apply_similarity_keeps_every_reprojection_and_round_trips():
    spec = sa.SceneSpec(n_frames=6, grid_nx=6, grid_ny=5, vis_window=0, noise_uv_pix=0.0)
    sc = sa.generate_scene(spec)
    rng = np.random.default_rng(4)
    s, R, t = ac.similarity(rng, 2.5)

    def project(points, cam_R, cam_T):
        out = np.zeros((sc.O, 2))
        lm = np.repeat(np.arange(sc.N), np.diff(sc.row_ptr))
        for o in range(sc.O):
            j = sc.obs_frame[o]
            x = sc.K[j].reshape(3, 3) @ (cam_R[j].reshape(3, 3) @ points[lm[o]] + cam_T[j])
            out[o] = spec.f0 * x[:2] / x[2]
        return out
    before = project(sc.points, sc.cam_R, sc.cam_T)
    X, cR, cT = AL.apply_similarity(s, R, t, sc.points, sc.cam_R, sc.cam_T)
    assert np.abs(X - ac.apply((s, R, t), sc.points)).max() <= 1e-14 * np.abs(X).max()
    assert np.abs(project(X, cR, cT) - before).max() <= 1e-12
    Xb, cRb, cTb = AL.apply_similarity(1.0 / s, R.T, -R.T @ t / s, X, cR, cT)
    assert np.abs(Xb - sc.points).max() <= 1e-14 and np.abs(cRb.reshape(-1, 9) - sc.cam_R.reshape(-1, 9)).max() <= 1e-15
    assert np.abs(cTb - sc.cam_T).max() <= 1e-14
    only, none_R, none_T = AL.apply_similarity(s, R, t, points=sc.points)
    assert np.array_equal(only, X) and none_R is None and none_T is None
    assert AL.apply_similarity(s, R, t, cam_R=sc.cam_R, cam_T=sc.cam_T)[0] is None
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            AL.apply_similarity(bad, R, t, sc.points)
    with pytest.raises(ValueError):
        AL.apply_similarity(s, R, t, cam_R=sc.cam_R)


# ------------------------------------------------------------------ the Python checks
def test_python_check_sets_and_names():
    b = ac.small(True)
    args = (b.row_ptr, b.a, b.b)
    good = dict(q=b.q, inlier_distance=0.05)
    assert AL.check_sets(*args, **good) is None
    assert AL.check_sets(b.row_ptr, None, b.b, point=np.zeros(len(b.b), np.int32), n_points=1, **good) is None

    def bad(i, f, **kw):
        x = [np.array(v, copy=True) for v in args]
        f(x[i])
        return AL.check_sets(*x, **{**good, **kw})
    assert "row_ptr[0]" in bad(0, lambda v: v.__setitem__(0, 1))
    assert "decreases at set 3" in bad(0, lambda v: v.__setitem__(4, v[3] - 1))
    assert "decreases at set 0" in bad(0, lambda v: v.__setitem__(1, -1))
    assert "a of correspondence 7 is not finite" in bad(1, lambda v: v.__setitem__((7, 1), np.nan))
    assert "b of correspondence 9 is not finite" in bad(2, lambda v: v.__setitem__((9, 2), np.inf))
    q = b.q.copy()
    q[9] = -1.0
    assert "q of correspondence 9" in AL.check_sets(*args, q=q, inlier_distance=0.05)
    q[9] = np.nan
    assert "q of correspondence 9" in AL.check_sets(*args, q=q, inlier_distance=0.05)
    assert "hypotheses outside 1..4096" in AL.check_sets(*args, hypotheses=0, **good) and "hypotheses" in AL.check_sets(*args, hypotheses=4097, **good)
    assert "inlier_distance" in AL.check_sets(*args, q=b.q) and "inlier_distance" in AL.check_sets(*args, q=b.q, inlier_distance=0.0)
    assert "inlier_distance" in AL.check_sets(*args, q=b.q, inlier_distance=np.nan)
    assert "refine_rounds outside 0..16" in AL.check_sets(*args, refine_rounds=17, **good) and "refine_rounds" in AL.check_sets(*args, refine_rounds=-1, **good)
    pt = np.zeros(len(b.b), np.int32)
    pt[5] = 3
    assert "correspondence 5 is beyond the map" in AL.check_sets(b.row_ptr, None, b.b, point=pt, n_points=3, **good)
    pt[5] = -1
    assert "beyond the map" in AL.check_sets(b.row_ptr, None, b.b, point=pt, n_points=3, **good)
    assert "split the batch" in AL.check_sets(np.zeros((1 << 16) + 2, np.int64), np.zeros((0, 3)), np.zeros((0, 3)), hypotheses=4096, inlier_distance=1.0)
    d = AL.default_align_options()
    assert d == dict(hypotheses=256, inlier_distance=0.0, seed=1, with_scale=True, refine_rounds=2)
    assert AL.align_status_names(AL.ALIGN_FEW_POINTS | AL.ALIGN_NO_MODEL) == ["FEW_POINTS", "NO_MODEL"]
    assert sa.ransac_hypotheses(0.3, 0.999, 3) == 17 and sa.ransac_hypotheses(0.5, 0.999, 3) == 52
    with pytest.raises(ValueError):
        AL.check_sets(b.row_ptr, b.a[:5], b.b, **good)
    with pytest.raises(ValueError):
        AL.host_set(b.a[:5], b.b[:4], inlier_distance=0.05)
    with pytest.raises(ValueError):
        AL.host_set(b.a[:5], b.b[:5])          # the checks refuse a set without inlier_distance
