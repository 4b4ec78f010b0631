"""The gate of the distinct-intrinsics cases of pair refinement and the homography (tests/twoview_k_cases.py), without a GPU: the
guards that the existing CPU tests put on their own cases hold on these, the host walks agree with the yardsticks on them within
the bounds of their own CPU tests, and -- the point of the cases -- on the noise-free batches the yardstick with the next pair's
K_a, the next pair's K_b, or K_a and K_b exchanged misses the truth by at least a thousand times the bound
tests/test_gpu_twoview_k.py applies to that pair with its own K.  Then the homography's decomposition over its range: baselines from
1 down to below the gap's bound, both double singular values, rotations up to pi."""
import json
import os

import numpy as np

from surikatoko_amd import homography as HG
import homography_cases as hc
import homography_ref as href
import pair_cases as pc
import pair_ref
import resect_cases
import twoview_k_cases as tk

FIGURES = os.path.join(hc.ROOT, "profiles", "frontend_intrinsics", "test_figures.json")


# ------------------------------------------------------------------ the cases are what they claim to be
def test_every_entry_of_K_differs_from_pair_to_pair():
    entries = ((0, 0), (1, 1), (0, 2), (1, 2), (0, 1))
    batches = [tk.pair_ragged(False), tk.pair_ragged(True), tk.pair_truth(), tk.pair_big(), tk.homog_ragged(False), tk.homog_ragged(True),
               tk.homog_many(), tk.homog_truth()[0], tk.decomposition_batch()]
    for b in batches:
        for K in (b.Ka, b.Kb, np.concatenate([b.Ka, b.Kb])):
            for r, c in entries:
                assert len(np.unique(K[:, r, c])) == len(K)
            assert np.all(K[:, 2, 2] == 1.0) and np.all(K[:, 1, 0] == 0.0) and np.all(K[:, 2, :2] == 0.0)
    for s in (tk.pair_shared(), tk.homog_shared()):
        assert np.all(s.Ka == s.Ka[0]) and np.all(s.Kb == s.Kb[0]) and not np.array_equal(s.Ka[0], s.Kb[0]) and s.n > 4
    m = tk.mixed_form(tk.homog_many(), ("Ka", "Kb"))
    assert np.count_nonzero(m.Ka[:, 2, 2] == hc.F0) == 6 and np.count_nonzero(m.Kb[:, 2, 2] == hc.F0) == 5
    assert not np.any((m.Ka[:, 2, 2] == hc.F0) & (m.Kb[:, 2, 2] == hc.F0))
    assert tuple(np.diff(tk.pair_ragged(False).row_ptr)) == pc.LENGTHS and tuple(np.diff(tk.homog_ragged(False).row_ptr)) == hc.LENGTHS
    big = np.diff(tk.pair_big().row_ptr)
    assert len(big) == tk.BIG == 257 and big.min() >= 8 and big.max() <= 20 and max(tk.ALONE) == 256 and {3, 4, 5, 255} <= set(tk.ALONE)
    assert np.all((np.diff(tk.pair_truth().row_ptr) >= 40) & (np.diff(tk.pair_truth().row_ptr) <= 60)) and tk.pair_truth().n == 6
    b, ps = tk.homog_truth()
    assert np.all(np.diff(b.row_ptr) == 40) and [bool(p.T.any()) for p in ps] == [k == "planar" for k in tk.HOMOG_TRUTH_KINDS]
    assert tk.HOMOG_TRUTH_KINDS.count("planar") == 4 and tk.HOMOG_TRUTH_KINDS.count("rotation") == 2
    assert tk.homog_many().n == 17 and tk.homog_many().row_ptr[2] == tk.homog_many().row_ptr[3]


# ------------------------------------------------------------------ pair refinement
def test_pair_cases_have_no_pair_at_a_threshold():
    """the guards of tests/test_pair_cpu.py on the own-K ragged batches: no pair is excused by the filter of pair_cases.agree"""
    for holes in (False, True):
        rel_change = tk.PAIR_OPTIONS[holes][1]
        ys = tk.pair_ragged_yardstick(holes)
        assert len(ys) == len(pc.LENGTHS) and [int(y["quality"][1]) for y in ys] == list(pc.LENGTHS)
        for i, y in enumerate(ys):
            assert resect_cases.margins_ok(y["log"], rel_change), (holes, i, y["log"])
        live = [y for y in ys if not y["status"] & pair_ref.FEW_POINTS]
        capped = sum(bool(y["status"] & pair_ref.NOT_CONVERGED) for y in live)
        assert len(live) == 8 and 0 < capped < len(live)


def test_pair_host_walk_against_the_yardstick():
    worst = tk.pair_host_floor()
    print(f"pair host walk against the yardstick: {worst:.3e} Newton steps")
    assert worst <= 1.0            # the bound of test_host_walk_against_the_yardstick_on_the_ragged_cases


def test_pair_truth_and_a_neighbours_K():
    b = tk.pair_truth()
    ys = tk.pair_truth_yardstick(b)
    got = pc.host_walk(b, tk.PAIR_TRUTH_ATTEMPTS, 0.0)[0]
    own = max(tk.pose_gap(y["R"], y["T"], b.R[i], b.T[i]) for i, y in enumerate(ys))
    walk = max(tk.pose_gap(got.R[i], got.T[i], b.R[i], b.T[i]) for i in range(b.n))
    print(f"pair truth: the yardstick {own:.3e}, the host walk {walk:.3e} from the truth; bound {tk.POSE_BOUND:.0e}")
    assert own <= 1e-3 * tk.POSE_BOUND and walk <= tk.POSE_BOUND and not np.any(got.status & pair_ref.FEW_POINTS)
    ratio = tk.pair_wrong_K()
    assert sorted(ratio) == ["Ka_rolled", "Kb_rolled", "swapped"]
    for name, r in ratio.items():
        print(f"pair refinement, {name}: the yardstick misses the truth by at least {r.min():.3e} x the bound")
        assert len(r) == b.n and np.all(np.isfinite(r)) and np.all(r >= tk.WRONG_K_FACTOR), (name, r)


# ------------------------------------------------------------------ the homography
def _homog_ragged_cases():
    for holes in (False, True):
        for H in hc.HYPOTHESES:
            for rounds in hc.ROUNDS:
                yield holes, H, rounds


def _guard(A, y, where):
    assert hc.at_a_threshold(A, y) is None, (where, hc.at_a_threshold(A, y))
    assert y["homog"][1] < 8 or hc.winner_is_clear(y), where


def test_homog_cases_have_a_clear_winner_and_no_pair_at_a_threshold():
    """test_cases_have_a_clear_winner_and_no_pair_at_a_threshold of tests/test_homography_cpu.py on the own-K batches, the batch of
    17 included; no pair is skipped"""
    walked = 0
    for holes, H, rounds in _homog_ragged_cases():
        for i, (A, y) in enumerate(zip(tk.homog_ragged_scored(holes, H), tk.homog_ragged_yardstick(holes, H, rounds))):
            assert y["status"] == 0, (holes, H, i)
            _guard(A, y, (holes, H, rounds, i))
            walked += 1
    assert walked == 2 * len(hc.HYPOTHESES) * len(hc.ROUNDS) * len(hc.LENGTHS)
    for rounds in hc.ROUNDS:
        for i, (A, y) in enumerate(zip(tk.homog_many_scored(), tk.homog_many_yardstick(rounds))):
            assert (y["status"] != 0) == (i == 2)
            if i != 2:
                assert y["homog"][1] >= 8
                _guard(A, y, ("many", rounds, i))


def test_homog_host_walk_against_the_yardstick():
    """the bounds the GPU tests use (homography_cases.bounds()) hold for the host walk on the own-K batches"""
    figures = []
    for holes, H, rounds in _homog_ragged_cases():
        b = tk.homog_ragged(holes)
        got = hc.host_walk(b, H, tk.HOMOG_SAMPLER_SEED[(holes, H)], rounds=rounds)
        hc.agree(b, tk.homog_ragged_yardstick(holes, H, rounds), got, *hc.bounds(), figures)
    b = tk.homog_many()
    hc.agree(b, tk.homog_many_yardstick(), hc.host_walk(b, tk.HOMOG_MANY_HYPOTHESES, tk.HOMOG_MANY_SAMPLER_SEED), *hc.bounds(), figures)
    print(f"homography host walk against the yardstick over {len(figures)} pairs: score {max(f[0] for f in figures):.3e} relative, "
          f"corners {max(f[1] for f in figures):.3e} px; bounds {hc.bounds()}")


def test_homog_truth_and_a_neighbours_K():
    """the assertions of test_host_walk_noise_free_planes and test_host_walk_noise_free_rotations on pairs with their own K, and
    the yardstick with another K on every pair"""
    b, ps = tk.homog_truth()
    got = hc.host_walk(b, 64, 1, tau=hc.OUTLIER_TAU)
    for i, p in enumerate(ps):
        planar = bool(p.T.any())
        assert got.status[i] == 0 and got.n_poses[i] == (2 if planar else 1) and got.homog[i, 2] == 40 and got.inliers[40 * i:40 * i + 40].all()
        hc.check_poses(got, i)
        d = tk.truth_distances(got, i, tk.homog_truth_of(p))
        assert min(d) <= tk.POSE_BOUND and (not planar or (max(d) > 1e-3 and got.front[i, 0] == 40)), (i, d)
        assert planar or got.homog[i, 6] <= 1e-10
        assert href.corner_distance(got.G[i], hc.true_homography(p), hc.F0) <= 1e-9
    ratio = tk.homog_wrong_K()
    assert sorted(ratio) == ["Ka_rolled", "Kb_rolled", "own", "swapped"] and np.all(ratio["own"] <= 1e-3)
    for name, r in ratio.items():
        if name != "own":
            print(f"homography, {name}: the yardstick misses the truth by at least {r.min():.3e} x the bound")
            assert len(r) == b.n and np.all(np.isfinite(r)) and np.all(r >= tk.WRONG_K_FACTOR), (name, r)


# ------------------------------------------------------------------ the two forms of K, and the record
def test_the_form_of_K_changes_the_host_walks_by_rounding_only():
    """a third of the matrices stored as K f0, other pairs for K_b than for K_a: the same status words, counts, winners and inlier
    flags (asserted where the change is measured), the poses apart by the figures the GPU test gives a factor of ten"""
    fig = tk.cpu_figures()
    print(json.dumps(fig, indent=1))
    assert fig["pair"]["form_change"] <= 1e-9 and fig["homography"]["form_change"] <= 1e-9
    # the record holds these figures as one run measured them; they are maxima of rounding errors, so only their kind is compared
    rec = json.load(open(FIGURES))
    for front in ("pair", "homography"):
        assert sorted(rec[front]["cpu"]) == sorted(fig[front])
        assert sorted(rec[front]["cpu"]["wrong_K_smallest_ratio"]) == sorted(fig[front]["wrong_K_smallest_ratio"])


# ------------------------------------------------------------------ the decomposition over its range
def test_decomposition_table_is_what_it_claims():
    cases, ys = tk.decomposition_cases(), tk.decomposition_yardstick()
    names = [p.name for p in cases]
    assert len(set(names)) == len(names) == len(tk.DECOMPOSITION_BASELINES) + 2 * len(tk.DECOMPOSITION_DOUBLES) + len(tk.DECOMPOSITION_ANGLES)
    assert tk.DECOMPOSITION_BASELINES == (1.0, 1e-1, 1e-3, 1e-5, 1e-7, 1e-9, 1e-11) and any(s < 0 for s in tk.DECOMPOSITION_SCALES)
    for p, y in zip(cases, ys):
        w = np.linalg.svd(p.H, compute_uv=False) ** 2
        w /= w[1]
        assert len(p.uv_a) == 40 and abs(np.linalg.norm(p.N) - 1.0) <= 1e-15
        # no case at the gap's bound: 1e-9 a factor 20 above, 1e-11 a factor 5 below, every other case decades away; the gap
        # itself is good to a few eps
        assert y.gap >= 10.0 * href.GAP or y.gap <= 0.25 * href.GAP, (p.name, y.gap)
        assert y.n_poses == (1 if p.name == "baseline_1e-11" else 2), p.name
        if p.name.startswith("baseline"):
            assert abs(y.gap / (2.0 * p.size) - 1.0) <= 0.5, (p.name, y.gap)
        if p.name.startswith("double_upper"):
            assert abs(w[1] - w[2]) <= 8 * pair_ref.EPS and w[0] - w[1] > 1e-3, (p.name, w)
        if p.name.startswith("double_lower"):
            assert abs(w[0] - w[1]) <= 8 * pair_ref.EPS and w[1] - w[2] > 1e-3, (p.name, w)
        if p.name.startswith("rotation"):
            assert p.R[2, 2] == 1.0 and abs(p.size - 0.1) <= 1e-15
    assert cases[-1].R[0, 0] == -1.0 and np.array_equal(cases[-4].R, np.eye(3))


def test_decomposition_over_its_range():
    """HG.decompose_homography on the exact H = R + t N^T of every case times every factor, against the yardstick and the truth:
    the same number of poses and gap, the properties of check_poses without exception, below the gap's bound the rotation alone,
    every pose one of the yardstick's and the nearer one at the truth within the case's bound: ten times the yardstick's own
    distance from the truth, never below 1e-13.  That distance grows like eps / gap along the baselines (1e-13 at |t| = 1e-3, 1e-7
    at 1e-9) and is about sqrt(eps / gap) at the double singular values."""
    cases, ys = tk.decomposition_cases(), tk.decomposition_yardstick()
    figures = {}
    for p, y in zip(cases, ys):
        ds = [HG.decompose_homography(s * p.H, p.xa, p.xb) for s in tk.DECOMPOSITION_SCALES]
        got = tk.as_result(ds)
        truth = tk.decomposition_truth(p, y.n_poses)
        own, other = [], []
        for k, (d, (Hy, gap, poses)) in enumerate(zip(ds, y.runs)):
            assert d.n_poses == len(poses) == y.n_poses and abs(d.gap - gap) <= 1e-12, (p.name, k, d.n_poses, d.gap, gap)
            assert np.abs(d.H - Hy).max() <= 1e-13, (p.name, k)
            hc.check_poses(got, k)
            if d.n_poses == 1:
                assert not d.T.any() and not d.N.any() and not d.R[1].any(), (p.name, k)
            own.append(tk.nearest([(d.R[c], d.T[c], d.N[c]) for c in range(d.n_poses)], truth))
            other.append(max(tk.one_of(d.R[c], d.T[c], d.N[c], d.front[c], len(p.xa), poses) for c in range(d.n_poses)))
        figures[p.name] = dict(gap=y.gap, n_poses=y.n_poses, yardstick_from_truth=y.distance, bound=y.bound, host_from_truth=max(own),
                               host_from_yardstick=max(other))
        print(f"{p.name:22s} gap {y.gap:.3e}, poses {y.n_poses}: the yardstick {y.distance:.3e} from the truth, bound {y.bound:.3e}; "
              f"the host function {max(own):.3e} from the truth, {max(other):.3e} from the yardstick")
    hc.write_figures("decomposition_range", figures)
    for name, f in figures.items():
        assert f["host_from_truth"] <= f["bound"] and f["host_from_yardstick"] <= f["bound"], (name, f)
    assert sorted(hc.committed_figures()["decomposition_range"]) == sorted(figures)
