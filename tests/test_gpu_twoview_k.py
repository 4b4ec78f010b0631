"""Pair refinement and the homography on the device (DESIGN.md sections 26 and 27) on batches whose pairs carry distinct intrinsics,
one shared K_a and K_b, or the same cameras stored as K f0 (tests/twoview_k_cases.py).  The host walks and the yardsticks take one
K per pair, so these are the tests that see which K a kernel read: k_pair_pack, k_pair_refine, k_homog_pick and the chained
relate_frames(..., refine=...).  tests/test_twoview_k_cpu.py shows that on the noise-free batches a neighbour's K, or K_a for K_b,
misses the bounds used here by eight decades, and computes the floors.  Last, the homography's decomposition over its range."""
import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import pair as PR
from surikatoko_amd import relate as RL
import homography_cases as hc
import homography_ref as href
import pair_cases as pc
import pair_ref
import relate_cases as rl
import resect_cases
import test_gpu_homography as gpu_homog
import test_gpu_pair as gpu_pair
import twoview_k_cases as tk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def h():
    ba = sa.BundleAdjustmentKanatani(0)
    yield ba
    ba.close()


def _refine(h, b, Ka=None, Kb=None, **kw):
    kw.setdefault("want_weights", True)
    return sa.refine_pairs(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka if Ka is None else Ka, b.Kb if Kb is None else Kb, b.R0, b.T0, q=b.q, **kw)


def _homog(h, b, Ka=None, Kb=None, **kw):
    kw.setdefault("inlier_pixels", hc.TAU)
    kw.setdefault("want_inliers", True)
    return sa.relate_homography(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka if Ka is None else Ka, b.Kb if Kb is None else Kb, q=b.q, **kw)


def _figure(front, what, value):
    print(f"twoview_k figure: {front} {what} {value:.3e}")


def _live(res):
    return np.flatnonzero((res.status & PR.PAIR_FEW_POINTS) == 0)


# ------------------------------------------------------------------ pair refinement
def test_pair_recovers_the_truth(h):
    """noise-free pairs from 3 and 5 degrees off, run to the end: rotation and direction within 1e-9 of the truth, the bound of
    tests/test_gpu_relate.py; with the next pair's K_a or K_b, or the two exchanged, the yardstick ends 0.1 rad away"""
    b = tk.pair_truth()
    res = _refine(h, b, attempts=tk.PAIR_TRUTH_ATTEMPTS, rel_change=0.0)
    assert len(_live(res)) == b.n and not np.any(res.status & PR.PAIR_DEGENERATE)
    worst = 0.0
    for i in range(b.n):
        dr, dt = pc.pose_error(res.R[i], res.T[i], b.R[i], b.T[i])
        worst = max(worst, dr, dt)
        assert dr <= tk.POSE_BOUND and dt <= tk.POSE_BOUND, (i, dr, dt)
        assert res.quality[i, 4] == res.quality[i, 1] == b.row_ptr[i + 1] - b.row_ptr[i] and res.quality[i, 0] < 1e-6, (i, res.quality[i])
    _figure("pair", "truth", worst)


@pytest.mark.parametrize("holes", [False, True])
def test_pair_against_the_yardstick(h, holes):
    """as test_every_length_against_the_yardstick of tests/test_gpu_pair.py, every pair with its own K_a and K_b"""
    b = tk.pair_ragged(holes)
    floor = tk.pair_host_floor()
    attempts, rel_change = tk.PAIR_OPTIONS[holes]
    ys = pc.tagged(list(tk.pair_ragged_yardstick(holes)), rel_change)
    assert all(resect_cases.margins_ok(y["log"], rel_change) for y in ys)          # no named case is excused
    got = _refine(h, b, attempts=attempts, rel_change=rel_change)
    worst = pc.agree(got, ys, b, bound=10 * floor)
    walk = pc.host_walk(b, attempts, rel_change, want_weights=True)[0]
    for i, y in enumerate(ys):
        assert got.status[i] == walk.status[i] and np.array_equal(got.quality[i, [1, 4, 5]], walk.quality[i, [1, 4, 5]], equal_nan=True), i
        assert np.abs(got.info[i] - y["info"]).max() <= 1e-9 * max(np.abs(y["info"]).max(), 1e-300) * max(1.0, 10 * floor), i
    assert np.abs(got.weights - np.concatenate([y["w"] for y in ys])).max() <= 1e-10
    _figure("pair", f"yardstick_newton_steps_holes_{int(holes)}", worst)
    print(f"pose distance in Newton steps: host walk {floor:.3e}, device {worst:.3e}, bound {10 * floor:.3e}")


def test_pair_evaluate_only_on_257_pairs(h):
    """attempts = 0 sees the K with no iteration in between: the start pose comes back, E = [T0]x R0, and the error figure and the
    information of every eighth pair and of the pairs at the block edges are the yardstick's terms at the start with the pair's own
    K, within the bounds of pair_cases.agree and of the ragged test"""
    b = tk.pair_big()
    got = _refine(h, b, attempts=0)
    assert np.array_equal(got.R, b.R0) and np.array_equal(got.T, b.T0) and not got.quality[:, 5].any() and not got.status.any()
    worst = 0.0
    for i in sorted(set(tk.CHECKED) | set(tk.ALONE)):
        uva, uvb, q = pc.pair_obs(b, i)
        E, H, _, w = pair_ref.terms(b.f0, uva, uvb, q, b.Ka[i], b.Kb[i], b.R0[i], b.T0[i])
        n = got.quality[i, 1]
        assert n == len(uva) and np.abs(got.E[i] - pair_ref.skew(b.T0[i]) @ b.R0[i]).max() <= 4 * pair_ref.EPS, i
        have = got.quality[i, 0] ** 2 * n
        tol = pc.energy_tolerance(b, i, E, n)
        worst = max(worst, abs(have - E) / tol)
        assert abs(have - E) <= tol, (i, have, E, tol)
        assert np.abs(got.info[i] * b.f0 ** 2 - H).max() <= 1e-9 * np.abs(H).max(), i
        assert np.abs(got.weights[b.row_ptr[i]:b.row_ptr[i + 1]] - w).max() <= 1e-10, i
    _figure("pair", "evaluate_only_in_energy_tolerances", worst)


def test_pair_bits_at_the_block_edges_and_with_shared_K(h):
    """pairs 0, 3, 4, 5, 255 and 256 of the 257 alone give the bits they have in the batch; one K_a and one K_b for all give the bits
    of the call that repeats them per pair, sent right after a call of the same shapes with distinct K (the handle's K buffers keep
    what the last call left behind the first nine doubles); and other per-pair arrays do not give those bits"""
    b = tk.pair_big()
    attempts, rel_change = tk.PAIR_BIG_OPTIONS
    whole = _refine(h, b, attempts=attempts, rel_change=rel_change)
    for i in tk.ALONE:
        one = pc.rows(b, [i])
        assert np.array_equal(gpu_pair._pair_bits(_refine(h, one, attempts=attempts, rel_change=rel_change), one, 0), gpu_pair._pair_bits(whole, b, i)), i
    assert len(_live(whole)) == b.n and np.count_nonzero(whole.quality[:, 5] > 1) > b.n // 2
    s, other = tk.pair_shared(), tk.pair_ragged(False)
    Ka, Kb = s.Ka[:1], s.Kb[:1]
    assert RL.relate_pair_args(s.row_ptr, s.uv_a, s.uv_b, s.q, Ka, Kb)[7] is True and s.n == other.n > 4 and not np.array_equal(Ka, Kb)
    assert RL.relate_pair_args(s.row_ptr, s.uv_a, s.uv_b, s.q, s.Ka, s.Kb)[7] is False
    for kw in (dict(attempts=3), dict(attempts=5, loss="cauchy", delta=2.0)):
        _refine(h, other, attempts=1)
        got = _refine(h, s, Ka=Ka, Kb=Kb, **kw)
        want = _refine(h, s, **kw)
        assert gpu_pair._same(got, want)
        wrong = _refine(h, s, Ka=tk.rolled(other.Ka), Kb=tk.rolled(other.Kb), **kw)            # the comparison can fail
        live = _live(want)
        assert len(live) == 8
        for i in live:
            assert not np.array_equal(gpu_pair._pair_bits(wrong, s, i), gpu_pair._pair_bits(want, s, i)), i
            assert not np.array_equal(wrong.R[i], want.R[i]) and not np.array_equal(wrong.info[i], want.info[i]), i


def test_pair_form_of_K(h):
    """a third of the K_a and another third of the K_b stored as K f0: the same statuses and counters; the poses apart by at most
    ten times what the host walk shows"""
    b = tk.pair_ragged(False)
    opts = dict(zip(("attempts", "rel_change"), tk.PAIR_OPTIONS[False]))
    a, m = _refine(h, b, **opts), _refine(h, tk.mixed_form(b, ("Ka", "Kb")), **opts)
    assert np.array_equal(a.status, m.status) and np.array_equal(a.quality[:, [1, 4, 5]], m.quality[:, [1, 4, 5]], equal_nan=True)
    got, floor = tk.pair_form_units(a.status, (a.R, a.T), (m.R, m.T)), tk.pair_form_change()
    _figure("pair", "form_change", got)
    assert got <= 10 * floor, (got, floor)


@pytest.mark.parametrize("inliers_only", [False, True])
def test_pair_chained_call_is_its_two_halves(h, inliers_only):
    """test_chained_call_is_its_two_halves of tests/test_gpu_pair.py with the K of every pair its own: the K handed through
    srk_relate_frames_refined to both halves is the pair's"""
    b = tk.pair_ragged(True)
    kw = dict(hypotheses=64, inlier_pixels=rl.TAU, seed=3)
    rel = sa.relate_frames(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb, q=b.q, want_inliers=True, **kw)
    opts = dict(attempts=4, rel_change=1e-6, loss="huber", delta=1.5)
    both, res = sa.relate_frames(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb, q=b.q, want_inliers=True,
                                 refine=dict(opts, inliers_only=inliers_only, want_weights=True), **kw)
    assert np.count_nonzero(rel.status) == 3 and np.count_nonzero(rel.status == 0) == 7       # 0, 4 and 5 matches are not related
    assert gpu_pair._same((both.related, both.status, both.inliers), (rel.related, rel.status, rel.inliers))
    R0, T0 = gpu_pair._start_of(rel)
    q = b.q * rel.inliers if inliers_only else b.q
    alone = sa.refine_pairs(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb, R0, T0, q=q, want_weights=True, **opts)
    assert gpu_pair._same(res, alone) and gpu_pair._same((both.R, both.T, both.E), (alone.R, alone.T, alone.E))
    _, lean = sa.relate_frames(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb, q=b.q, refine=dict(opts, inliers_only=inliers_only), **kw)
    assert gpu_pair._same(lean[:7], alone[:7]) and lean.weights is None
    # and the related poses are those of the pairs' own cameras: near the truth, which another K misses by 0.1 rad
    for i in np.flatnonzero((rel.status == 0) & (np.diff(b.row_ptr) > 40)):
        assert max(pc.pose_error(alone.R[i], alone.T[i], b.R[i], b.T[i])) <= 0.05, i


# ------------------------------------------------------------------ the homography
def test_homog_recovers_the_truth(h):
    """the assertions of test_noise_free_planes and test_noise_free_rotations of tests/test_gpu_homography.py, every pair with its
    own K_a and K_b"""
    b, ps = tk.homog_truth()
    got = _homog(h, b, hypotheses=64, inlier_pixels=hc.OUTLIER_TAU)
    worst = [0.0, 0.0]
    for i, p in enumerate(ps):
        planar = bool(p.T.any())
        assert got.status[i] == 0 and got.n_poses[i] == (2 if planar else 1) and got.homog[i, 2] == 40 and got.inliers[40 * i:40 * i + 40].all()
        hc.check_poses(got, i)
        d = tk.truth_distances(got, i, tk.homog_truth_of(p))
        print(f"pair {i}: the candidates' distances from the truth {d}")
        assert min(d) <= tk.POSE_BOUND, (i, d)
        if planar:
            assert max(d) > 1e-3 and got.front[i, 0] == 40, (i, d)
        else:
            assert got.homog[i, 6] <= 1e-10 and not got.T[i].any() and not got.N[i].any() and not got.R[i, 1].any()
        dg = href.corner_distance(got.G[i], hc.true_homography(p), hc.F0)
        assert dg <= 1e-9, (i, dg)
        worst = [max(worst[0], min(d)), max(worst[1], dg)]
    _figure("homography", "truth", worst[0])
    _figure("homography", "truth_corner_pixels", worst[1])


@pytest.mark.parametrize("rounds", hc.ROUNDS)
@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("hypotheses", hc.HYPOTHESES)
def test_homog_against_the_yardstick(h, hypotheses, holes, rounds):
    b = tk.homog_ragged(holes)
    got = _homog(h, b, hypotheses=hypotheses, seed=tk.HOMOG_SAMPLER_SEED[(holes, hypotheses)], refine_rounds=rounds)
    worst = hc.agree(b, tk.homog_ragged_yardstick(holes, hypotheses, rounds), got, *hc.bounds())
    _figure("homography", f"yardstick_score_H_{hypotheses}_holes_{int(holes)}_rounds_{rounds}", worst[0])
    _figure("homography", f"yardstick_corner_pixels_H_{hypotheses}_holes_{int(holes)}_rounds_{rounds}", worst[1])


def test_homog_17_pairs(h):
    """the batch of 17 against the yardstick, and every pair alone with the bits it has in the batch"""
    b = tk.homog_many()
    got = _homog(h, b, hypotheses=tk.HOMOG_MANY_HYPOTHESES, seed=tk.HOMOG_MANY_SAMPLER_SEED)
    worst = hc.agree(b, tk.homog_many_yardstick(), got, *hc.bounds())
    _figure("homography", "yardstick_score_17_pairs", worst[0])
    _figure("homography", "yardstick_corner_pixels_17_pairs", worst[1])
    whole = _homog(h, b, hypotheses=65, seed=5)
    for i in range(b.n):
        one = hc.rows(b, [i])
        alone = _homog(h, one, hypotheses=65, seed=5)
        assert gpu_homog._same_bits(alone, gpu_homog._pair(whole, i)), i
        assert np.array_equal(alone.inliers, whole.inliers[int(b.row_ptr[i]):int(b.row_ptr[i + 1])]), i


def test_homog_shared_K_and_the_outputs_that_read_K(h):
    """One K_a and one K_b for all give the bits of their repeated per-pair arrays, right after a call of the same shapes with
    distinct K.  With the next pair's K_a, G, the counts, the winner, the rounds, the status and the inlier flags keep their bits
    (G lives in pixels) while H, R, T and N change on every pair with a model: K is read by the decomposition alone."""
    s, other = tk.homog_shared(), tk.homog_ragged(False)
    Ka, Kb = s.Ka[:1], s.Kb[:1]
    assert RL.relate_pair_args(s.row_ptr, s.uv_a, s.uv_b, s.q, Ka, Kb)[7] is True and s.n == other.n > 4 and not np.array_equal(Ka, Kb)
    for H in (5, 65):
        _homog(h, other, hypotheses=H)
        got = _homog(h, s, Ka=Ka, Kb=Kb, hypotheses=H)
        want = _homog(h, s, hypotheses=H)
        assert gpu_homog._same_bits(got, want) and np.array_equal(got.inliers, want.inliers) and np.count_nonzero(want.status == 0) >= 5
        wrong = _homog(h, s, Ka=tk.rolled(other.Ka), Kb=tk.rolled(other.Kb), hypotheses=H)   # the comparison can fail
        assert not any(np.array_equal(wrong.H[i], want.H[i]) for i in np.flatnonzero(want.status == 0))
    b = tk.homog_many()
    a, r = _homog(h, b, hypotheses=65, seed=5), _homog(h, b, Ka=tk.rolled(b.Ka), hypotheses=65, seed=5)
    assert gpu_homog._same_bits(a, r, ("G", "status")) and np.array_equal(gpu_homog._bits(a.homog[:, :6]), gpu_homog._bits(r.homog[:, :6]))
    assert np.array_equal(a.inliers, r.inliers)
    models = np.flatnonzero(a.status == 0)
    assert len(models) == 16
    for i in models:
        assert a.n_poses[i] == 2 and r.n_poses[i] == 2, i                     # half a pixel of noise: no pair is a rotation to 1e-10
        for name in ("H", "R", "T", "N"):
            assert not np.array_equal(getattr(a, name)[i], getattr(r, name)[i]), (i, name)


def test_homog_form_of_K(h):
    b = tk.homog_many()
    kw = dict(hypotheses=tk.HOMOG_MANY_HYPOTHESES, seed=tk.HOMOG_MANY_SAMPLER_SEED)
    a, m = _homog(h, b, **kw), _homog(h, tk.mixed_form(b, ("Ka", "Kb")), **kw)
    assert tk.homog_form_same(a, m)
    got, floor = tk.homog_form_units(a.status, a, m), tk.homog_form_change()
    _figure("homography", "form_change", got)
    assert got <= 10 * floor, (got, floor)


# ------------------------------------------------------------------ the decomposition over its range
def test_decomposition_over_its_range(h):
    """The table of tests/twoview_k_cases.py in one batch.  The estimated G is not exact, so the decomposition is isolated from the
    estimation: the device's own H of every pair is decomposed by the yardstick on the same rays, and every returned pose is one
    of the yardstick's within the case's bound (ten times the yardstick's own distance from the truth on the exact H, never below
    1e-13; both signs where exactly half the inliers are in front).  From |t| = 1e-3 on the nearer pose is at the truth within the
    same bound."""
    cases, ys, b = tk.decomposition_cases(), tk.decomposition_yardstick(), tk.decomposition_batch()
    got = _homog(h, b, hypotheses=64)
    assert not got.status.any() and got.inliers.all() and np.all(got.homog[:, 2] == tk.DECOMPOSITION_MATCHES)
    failed = []
    for i, (p, y) in enumerate(zip(cases, ys)):
        hc.check_poses(got, i)
        assert got.n_poses[i] == y.n_poses, (p.name, got.n_poses[i], got.homog[i, 6])
        _, gap, poses = href.decompose(got.H[i], p.xa, p.xb)
        assert len(poses) == y.n_poses and abs(got.homog[i, 6] - gap) <= 1e-12, (p.name, gap, got.homog[i, 6])
        other = max(tk.one_of(got.R[i, k], got.T[i, k], got.N[i, k], got.front[i, k], tk.DECOMPOSITION_MATCHES, poses) for k in range(y.n_poses))
        truth = min(tk.truth_distances(got, i, tk.decomposition_truth(p, y.n_poses)))
        checked = p.size >= tk.DECOMPOSITION_TRUTH_FROM
        print(f"twoview_k decomposition: {p.name:22s} gap {got.homog[i, 6]:.3e} poses {got.n_poses[i]} from the yardstick {other:.3e} "
              f"from the truth {truth:.3e}{'' if checked else ' (not asserted)'} bound {y.bound:.3e}")
        if other > y.bound or (checked and truth > y.bound):
            failed.append((p.name, other, truth, y.bound))
    assert not failed, failed
