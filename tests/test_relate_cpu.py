"""Two-view relative pose without a GPU: the yardstick (tests/relate_ref.py), the guards that keep the
compared decisions away from rounding, and the host half (surikatoko_amd/csrc/srk_relate.cpp) through a stand-alone program
(tests/cpp/test_relate_host.cpp): the sampler, the five-point solve alone, the decomposition, the argument checks, and a walk of
every pair on the host in the kernels' own order of operations."""
import json
import os
import subprocess

import numpy as np
import pytest

from surikatoko_amd import relate as RL
import relate_cases as rc
import relate_ref as ref

FIGURES = os.path.join(rc.ROOT, "profiles", "relate", "test_figures.json")


@pytest.fixture(scope="module")
def program():
    if rc.cxx() is None:
        pytest.skip("no host C++ compiler")
    return rc.host_program()


# ------------------------------------------------------------------ the sampler
@pytest.mark.parametrize("n", [6, 7, 64, 10 ** 6])
def test_sampler_against_the_yardstick(program, tmp_path, n):
    out = str(tmp_path / "ranks.bin")
    for seed in (1, 0xFFFFFFFFFFFFFFFF):
        r = subprocess.run([program, "sampler", out, str(seed), str(n), "4096"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = np.fromfile(out, np.int64).reshape(4096, 6)
        want = np.array([ref.sample(seed, h, n) for h in range(4096)])
        assert np.array_equal(got, want)
        assert got.min() >= 0 and got.max() < n
        assert all(len(set(row)) == 6 for row in got.tolist())
    if n > 6:
        assert len({tuple(row) for row in got.tolist()}) > 1000          # and the draws differ from one another


def test_the_stream_is_not_locates():
    import locate_ref
    assert ref.sample(1, 0, 1000)[:4] != locate_ref.sample(1, 0, 1000)


# ------------------------------------------------------------------ the five-point solve alone
def test_five_point_against_the_yardstick(program):
    """300 noise-free samples, a third planar, rotations 0.01-0.6 rad.  The exact E is among the host build's solutions, the number
    of real roots equals the yardstick's, and per sample min ||+-E - E_true||_F <= max(1e-13, 64 x the yardstick's own distance);
    samples where the yardstick itself is above 1e-7 are left out, at most 5 % of them.  The yardstick is the action matrix of
    Stewenius from an SVD null space (relate_ref.five_point).  Measured (a CPU run): see profiles/relate/test_figures.json."""
    sm = rc.samples()
    n = len(sm.E)
    E, rec, roots = rc.host_solve(sm.uv_a, sm.uv_b)
    ra = np.array([ref.rays(rc.K0, sm.uv_a[i], rc.F0) for i in range(n)])
    rb = np.array([ref.rays(rc.K0, sm.uv_b[i], rc.F0) for i in range(n)])
    Ey, real, _ = ref.five_point(ra[:, :5], rb[:, :5])
    host = np.array([min([ref.essential_distance(E[i, k], sm.E[i]) for k in range(roots[i])] or [np.inf]) for i in range(n)])
    yard = np.array([min([ref.essential_distance(Ey[i, k], sm.E[i]) for k in np.flatnonzero(real[i])] or [np.inf]) for i in range(n)])
    keep = yard <= 1e-7
    left_out = 1.0 - np.count_nonzero(keep) / n
    ratio = host[keep] / np.maximum(yard[keep], 1e-13 / 64.0)
    same_count = roots[keep] == real[keep].sum(axis=1)
    figures = dict(samples=n, left_out=left_out, yardstick_median=float(np.median(yard[keep])), yardstick_max=float(yard[keep].max()),
                   host_median=float(np.median(host[keep])), host_max=float(host[keep].max()), largest_ratio=float(ratio.max()),
                   root_counts_differ=int(np.count_nonzero(~same_count)))
    print("five-point alone:", json.dumps(figures))
    assert left_out <= 0.05
    assert same_count.all(), np.flatnonzero(keep)[~same_count]
    assert (ratio <= 64.0).all(), (np.flatnonzero(keep)[ratio > 64.0], ratio.max())
    assert rec[:, 19].all() and np.sqrt(rec[:, 18]).max() < 1e-6        # the sixth match picks an E that fits it
    if os.path.exists(FIGURES):   # the recorded figures are these, to two digits
        saved = json.load(open(FIGURES))["five_point_cpu"]
        assert all(abs(saved[k] - v) <= 0.05 * abs(v) + 1e-300 for k, v in figures.items() if k in ("samples", "left_out", "root_counts_differ")), saved


# ------------------------------------------------------------------ the decomposition
def test_decomposition_returns_the_pose(program):
    rng = np.random.default_rng(2401)
    poses = [rc.motion(rng, hi=3.0) for _ in range(500)]
    E = np.array([ref.skew(T) @ R for R, T in poses])
    Rs, Ts = rc.host_poses(E)
    for (R, T), Ri, Ti in zip(poses, Rs, Ts):
        assert min(max(np.abs(Ri[k] - R).max(), np.abs(Ti[k] - T).max()) for k in range(4)) <= 1e-12
        for k in range(4):
            assert np.abs(Ri[k].T @ Ri[k] - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(Ri[k]) - 1.0) <= 1e-12
        assert np.abs(ref.skew(Ti[0]) @ Ri[0] - ref.skew(T) @ R).max() <= 1e-12 and np.abs(ref.skew(Ti[3]) @ Ri[3] - ref.skew(T) @ R).max() <= 1e-12
        assert np.abs(ref.skew(Ti[1]) @ Ri[1] + ref.skew(T) @ R).max() <= 1e-12 and np.abs(ref.skew(Ti[2]) @ Ri[2] + ref.skew(T) @ R).max() <= 1e-12


def test_the_vote_picks_the_pose(program):
    """noise-free pairs walked on the host: the pose is the truth, every match an inlier in front of both cameras"""
    b = rc.accuracy()
    got = rc.host_walk(b, 64, 1)
    assert np.all(got.status == 0)
    for i, kind in enumerate(rc.ACCURACY_KINDS):
        dr, dt = rc.pose_error(got.R[i], got.T[i], b.R[i], b.T[i])
        print(f"host walk, {kind}: rotation {dr:.2e} rad, direction {dt:.2e} rad, parallax {got.related[i, 7]:.3e} rad")
        assert got.related[i, 2] == 40
        if kind != "rotation":
            assert dr <= 1e-9 and dt <= 1e-9 and got.related[i, 6] == 40 and got.related[i, 0] < 1e-6
            assert np.abs(got.E[i] - ref.skew(got.T[i]) @ got.R[i]).max() <= 1e-15


# ------------------------------------------------------------------ the guards
def _ragged_cases():
    for holes in (False, True):
        for H in rc.HYPOTHESES:
            yield rc.ragged(holes), rc.ragged_yardstick(holes, H), (holes, H)


def test_cases_have_no_pair_at_a_threshold():
    """On the ragged pairs: no hypothesis whose real roots hang on rounding, no match at the inlier threshold of the winner, and
    for every pair with n >= 8 the yardstick's best and second-best scores differ by more than 1e-6 relative.  Pairs of six or
    seven matches draw permutations of nearly one sample, whose scores differ by rounding only."""
    clear = 0
    for b, ys, name in _ragged_cases():
        for i, y in enumerate(ys):
            assert y["status"] == 0 and not y["fragile"], (name, i)
            assert y["margin"] > 1e-6 * rc.TAU ** 2, (name, i, y["margin"])
            if y["related"][1] >= 8:
                assert rc.winner_is_clear(y), (name, i)
                clear += 1
    assert clear == 2 * len(rc.HYPOTHESES) * 5


# ------------------------------------------------------------------ the host half
def test_checks_and_defaults(program):
    r = subprocess.run([program, "unit"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0 failure(s)", r.stdout + r.stderr


def test_unit_runs_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan: the unit checks, the sampler, a solve and a ragged batch with
    q = 0 in between"""
    if rc.cxx() is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "test_relate_host_san"
    r = rc.build_host_program(exe, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), "unit"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0 failure(s)", r.stdout + r.stderr
    sm = rc.samples()
    assert len(rc.host_solve(sm.uv_a[:20], sm.uv_b[:20], program=str(exe))[2]) == 20
    b = rc.ragged(True)
    got = rc.host_walk(b, 5, 1, program=str(exe))
    assert len(got.status) == b.n


def test_host_walk_against_the_yardstick_on_the_ragged_cases(program):
    """the kernels' order of operations on the host: the same status, winner, inlier flags and counts as the yardstick, the score to
    1e-9 relative; the largest pose distance is printed"""
    worst = 0.0
    for b, ys, name in _ragged_cases():
        got = rc.host_walk(b, name[1], 1)
        worst = max(worst, rc.agree(b, ys, got, 1e-6))
    print(f"host walk against the yardstick: largest pose distance {worst:.3e}")


def test_host_walk_q_zero_is_the_pair_without_the_match(program):
    b = rc.ragged(True)
    short, keep = rc.without_holes(b)
    a, c = rc.host_walk(b, 65, 7), rc.host_walk(short, 65, 7)
    for x, y in ((a.R, c.R), (a.T, c.T), (a.E, c.E), (a.related, c.related), (a.scores, c.scores), (a.status, c.status), (a.inliers[keep], c.inliers)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert not a.inliers[~keep].any()
    one = rc.SimpleNamespace(**{**vars(short), "q": np.ones_like(short.q)})
    none = rc.SimpleNamespace(**{**vars(short), "q": None})
    a, c = rc.host_walk(one, 65, 7), rc.host_walk(none, 65, 7)
    for x, y in ((a.R, c.R), (a.T, c.T), (a.E, c.E), (a.related, c.related), (a.scores, c.scores), (a.inliers, c.inliers)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_host_pair_through_the_library_is_the_program(program):
    b = rc.rows(rc.ragged(True), [3])
    got, lib = rc.host_walk(b, 64, 3), RL.host_pair(b.f0, b.uv_a, b.uv_b, b.Ka[0], b.Kb[0], q=b.q, hypotheses=64, seed=3, inlier_pixels=rc.TAU)
    assert lib.status[0] == got.status[0] and lib.related[0, 3] == got.related[0, 3] and np.array_equal(lib.inliers, got.inliers)
    assert np.abs(lib.R - got.R).max() <= 1e-9 and abs(lib.related[0, 0] - got.related[0, 0]) <= 1e-9 * got.related[0, 0]


# ------------------------------------------------------------------ the Python checks
def test_python_check_pairs_and_names():
    b = rc.ragged(True)
    args = (b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb)
    assert RL.check_pairs(*args, q=b.q) is None

    def bad(i, f, **kw):
        a = [np.array(x, copy=True) for x in args]
        f(a[i])
        return RL.check_pairs(*a, **kw)
    assert "row_ptr[0]" in bad(0, lambda a: a.__setitem__(0, 1))
    assert "decreases at pair 3" in bad(0, lambda a: a.__setitem__(4, a[3] - 1))
    assert "decreases at pair 0" in bad(0, lambda a: a.__setitem__(1, -1))
    assert "uv_a of match 7" in bad(1, lambda a: a.__setitem__((7, 1), np.nan))
    assert "uv_b of match 9" in bad(2, lambda a: a.__setitem__((9, 0), np.inf))
    assert "K_a of pair 2 is not finite" in bad(3, lambda a: a.__setitem__((2, 1, 1), np.nan))
    assert "K_b of pair 2 is singular" in bad(4, lambda a: a.__setitem__((2, 2), np.zeros(3)))
    q = b.q.copy()
    q[9] = -1.0
    assert "q of match 9" in RL.check_pairs(*args, q=q)
    q[9] = np.inf
    assert "q of match 9" in RL.check_pairs(*args, q=q)
    assert "hypotheses outside 1..4096" in RL.check_pairs(*args, hypotheses=0) and "hypotheses" in RL.check_pairs(*args, hypotheses=4097)
    assert "inlier_pixels" in RL.check_pairs(*args, inlier_pixels=0.0) and "inlier_pixels" in RL.check_pairs(*args, inlier_pixels=np.nan)
    assert RL.default_relate_options() == dict(hypotheses=256, inlier_pixels=2.0, seed=1)
    assert RL.relate_status_names(RL.RELATE_FEW_POINTS | RL.RELATE_NO_MODEL) == ["FEW_POINTS", "NO_MODEL"]
    with pytest.raises(ValueError):
        RL.check_pairs(b.row_ptr, b.uv_a[:5], b.uv_b, b.Ka, b.Kb)
    with pytest.raises(ValueError):
        RL.check_pairs(b.row_ptr, b.uv_a, b.uv_b, b.Ka[:3], b.Kb)


def test_ransac_hypotheses_of_five():
    assert RL.ransac_hypotheses(0.3, 0.999, 5) == 38 and RL.ransac_hypotheses(0.5, 0.999, 5) == 218
    for e in (0.05, 0.2, 0.3, 0.5, 0.7):
        for p in (0.5, 0.9, 0.99, 0.999):
            assert RL.ransac_hypotheses(e, p, 5) == max(1, ref.ransac_hypotheses(e, p, 5)), (e, p)
