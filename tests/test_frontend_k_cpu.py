"""The gate of the distinct-intrinsics cases of the front ends (tests/frontend_k_cases.py), without a GPU: the guards that the
existing CPU tests put on their own cases hold on these, the host walks agree with the yardsticks on them, the floors the GPU
bounds use are at rounding level, and -- the point of the cases -- the yardstick with a neighbour's K violates, item by item, the
bound tests/test_gpu_frontend_k.py applies to that item."""
import json
import os

import numpy as np
import pytest

import frontend_k_cases as fk
import locate_cases as lc
import relate_cases as rl
import resect_cases as rc
import resect_ref
import triangulate_cases as tc
import test_resect_cpu as resect_gate

FIGURES = os.path.join(lc.ROOT, "profiles", "frontend_intrinsics", "test_figures.json")


@pytest.fixture(scope="module", autouse=True)
def compiler():
    if lc.cxx() is None:
        pytest.skip("no host C++ compiler")


def _items(ys):
    return ys.items() if isinstance(ys, dict) else enumerate(ys)


# ------------------------------------------------------------------ the cases are what they claim to be
def test_every_entry_of_K_differs_from_item_to_item():
    entries = ((0, 0), (1, 1), (0, 2), (1, 2), (0, 1))
    batches = [fk.tri_big(), fk.tri_truth(), fk.resect_big(False), fk.resect_big(True), fk.resect_truth(), fk.locate_big(False),
               fk.locate_big(True), fk.locate_truth()]
    Ks = [b.K for b in batches]
    for b in (fk.relate_ragged(False), fk.relate_ragged(True), fk.relate_many(), fk.relate_truth()):
        Ks += [b.Ka, b.Kb, np.concatenate([b.Ka, b.Kb])]
    for K in Ks:
        for r, c in entries:
            assert len(np.unique(K[:, r, c])) == len(K)
        assert np.all(K[:, 2, 2] == 1.0) and np.all(K[:, 1, 0] == 0.0) and np.all(K[:, 2, :2] == 0.0)
    for b in (fk.tri_shared(), fk.resect_shared(), fk.locate_shared()):
        assert np.all(b.K == b.K[0]) and len(b.K) > 4
    s = fk.relate_shared()
    assert np.all(s.Ka == s.Ka[0]) and np.all(s.Kb == s.Kb[0]) and not np.array_equal(s.Ka[0], s.Kb[0]) and s.n > 4
    m = fk.mixed_form(fk.resect_small(False))
    assert np.count_nonzero(m.K[:, 2, 2] == rc.F0) == 3 and np.count_nonzero(m.K[:, 2, 2] == 1.0) == 6
    assert set(np.diff(fk.tri_big().row_ptr)[:-1]) == set(tc.RAGGED_LENGTHS) and tuple(tc.track(fk.tri_big(), 10)[0]) == fk.ALONE
    assert tuple(np.diff(fk.resect_small(False).row_ptr)) == fk.RESECT_LENGTHS and tuple(np.diff(fk.locate_small(False).row_ptr)) == lc.LENGTHS
    assert tuple(np.diff(fk.relate_ragged(False).row_ptr)) == rl.LENGTHS and fk.relate_many().n == 17
    for b in (fk.resect_truth(), fk.locate_truth(), fk.relate_truth()):
        assert np.all((np.diff(b.row_ptr) >= 40) & (np.diff(b.row_ptr) <= 64))
    assert np.all((np.diff(fk.tri_truth().row_ptr) >= 40) & (np.diff(fk.tri_truth().row_ptr) <= 64))


# ------------------------------------------------------------------ triangulation
def test_tri_host_walk_against_the_yardstick_and_the_truth():
    b = fk.tri_big()
    for q in (None, fk.tri_holes()):
        X, quality, status = fk.tri_host_walk(b, q)
        want = fk.tri_yardstick(b, q)
        assert np.array_equal(status, np.array([w[2] for w in want], np.uint32))
        assert np.array_equal(quality[:, 3], np.array([w[1][3] for w in want]))
        for i in np.flatnonzero(status == 0):
            assert np.linalg.norm(X[i] - want[i][0]) <= fk.tri_bound(b, i, want[i][0], q), i
            assert np.linalg.norm(X[i] - b.X_true[i]) <= fk.tri_bound(b, i, b.X_true[i], q), i
        assert np.count_nonzero(status == 0) >= b.n - 3
    t = fk.tri_truth()
    X, _, status = fk.tri_host_walk(t)
    assert not status.any()
    assert max(np.linalg.norm(X[i] - t.X_true[i]) / tc.cond_bound(t, i, t.X_true[i]) for i in range(t.n)) <= 1.0


def test_tri_a_neighbours_K_violates_the_bound_on_every_frame():
    ratio = fk.tri_wrong_K()
    print(f"triangulation: the error with K[j + 1] in frame j alone is at least {ratio.min():.3e} x 8 eps cond |X|")
    assert len(ratio) == 64 and np.all(np.isfinite(ratio)) and np.all(ratio > 1.0)


# ------------------------------------------------------------------ resection
def test_resect_cases_have_no_frame_at_a_threshold():
    for holes in (False, True):
        ys = list(fk.resect_yardstick(holes)) + (list(fk.resect_yardstick(holes, "big").values()) if not holes else [])
        for i, y in enumerate(ys):
            assert rc.margins_ok(y["log"], rc.RAGGED_OPTIONS[holes][1]), (holes, i)
        capped = sum(bool(y["status"] & resect_ref.NOT_CONVERGED) for y in ys)
        assert 0 < capped < sum(y["status"] != resect_ref.FEW_POINTS for y in ys)


def test_resect_host_walk_against_the_yardstick():
    worst = 0.0
    for holes in (False, True):
        b = fk.resect_small(holes)
        worst = max(worst, resect_gate._agree(fk.resect_host_walk(b, *rc.RAGGED_OPTIONS[holes]), fk.resect_yardstick(holes), b))
    b = fk.resect_big(False)
    got = fk.resect_host_walk(b, *rc.RAGGED_OPTIONS[False])
    ys = fk.resect_yardstick(False, "big")
    sub = rc.rows(b, fk.CHECKED)
    picked = [a[list(fk.CHECKED)] for a in got[:5]] + [[got[5][i] for i in fk.CHECKED], None]
    worst = max(worst, resect_gate._agree(picked, [ys[i] for i in fk.CHECKED], sub))
    print(f"host walk against the yardstick: {worst:.3e} Newton steps; resect_host_floor() {fk.resect_host_floor():.3e}")
    assert worst == fk.resect_host_floor()


def test_resect_truth_and_a_neighbours_K():
    b = fk.resect_truth()
    ys, floor = fk.resect_truth_yardstick()
    assert floor <= 1.0
    assert all(y["E"] <= 1e-22 for y in ys) and all(max(rc.pose_error(y["R"], y["T"], b.frames[i])) < 1e-13 for i, y in enumerate(ys))
    R, T = fk.resect_host_walk(b, 40, 0.0)[:2]
    assert max(rc.accuracy_units(R[i], T[i], b.frames[i], ys[i]["H"]) for i in range(b.n)) <= 10 * floor
    ratio = fk.resect_wrong_K()
    print(f"resection: the error with the next frame's K is at least {ratio.min():.3e} x the bound")
    assert len(ratio) == b.n and np.all(ratio > 1.0)


# ------------------------------------------------------------------ location
def _locate_cases():
    for holes in (False, True):
        yield fk.locate_small(holes), fk.locate_yardstick(holes), holes
    yield fk.locate_big(False), fk.locate_yardstick(False, "big"), "big"


def test_locate_cases_have_no_frame_at_a_threshold():
    located = 0
    for b, ys, name in _locate_cases():
        for i, y in _items(ys):
            assert not y["fragile"], (name, i)
            if y["status"]:
                continue
            located += 1
            assert lc.inliers_are_clear(b, i, y), (name, i)
            assert y["located"][1] <= 5 or lc.winner_is_clear(y), (name, i)
    assert located > 30


def test_locate_host_walk_against_the_yardstick():
    worst = 0.0
    for b, ys, name in _locate_cases():
        got = lc.host_walk(b, fk.LOCATE_HYPOTHESES, 1)
        worst = max(worst, lc.agree(b, ys, got, got.inliers))
    print(f"host walk against the yardstick: largest pose distance {worst:.3e}; locate_host_floor() {fk.locate_host_floor():.3e}")
    assert worst <= 1e-6 and fk.locate_host_floor() <= worst


def test_locate_truth_and_a_neighbours_K():
    b = fk.locate_truth()
    got = lc.host_walk(b, 64, 1)
    floor = fk.locate_truth_floor()
    assert np.all(got.status == 0) and got.located[:, 0].max() < 1e-6 and floor < 1e-6
    assert np.array_equal(got.located[:, 2], got.located[:, 1])
    ratio = fk.locate_wrong_K()
    print(f"location: truth floor {floor:.3e}; the error with the next frame's K is at least {ratio.min():.3e} x the bound")
    assert len(ratio) == b.n and np.all(ratio > 1.0)


# ------------------------------------------------------------------ relative pose
def test_relate_cases_have_no_pair_at_a_threshold():
    clear = 0
    for holes in (False, True):
        for H in fk.RELATE_HYPOTHESES:
            for i, y in enumerate(fk.relate_ragged_yardstick(holes, H)):
                assert y["status"] == 0 and not y["fragile"], (holes, H, i)
                assert y["margin"] > 1e-6 * rl.TAU ** 2, (holes, H, i, y["margin"])
                if y["related"][1] >= 8:
                    assert rl.winner_is_clear(y), (holes, H, i)
                    clear += 1
    assert clear == 2 * len(fk.RELATE_HYPOTHESES) * 5
    for i, y in enumerate(fk.relate_many_yardstick()):
        assert (y["status"] != 0) == (i == 2)
        if i != 2:
            assert not y["fragile"] and y["margin"] > 1e-6 * rl.TAU ** 2 and y["related"][1] >= 8 and rl.winner_is_clear(y), i


def test_relate_host_walk_against_the_yardstick():
    worst = 0.0
    for holes in (False, True):
        b = fk.relate_ragged(holes)
        for H in fk.RELATE_HYPOTHESES:
            worst = max(worst, rl.agree(b, fk.relate_ragged_yardstick(holes, H), rl.host_walk(b, H, 1), 1e-6))
    b = fk.relate_many()
    worst = max(worst, rl.agree(b, fk.relate_many_yardstick(), rl.host_walk(b, 65, 1), 1e-6))
    print(f"host walk against the yardstick: largest pose distance {worst:.3e}")


def test_relate_truth_and_a_neighbours_K():
    b = fk.relate_truth()
    got = rl.host_walk(b, 64, 1)
    assert np.all(got.status == 0)
    for i, y in enumerate(fk.relate_truth_yardstick()):
        assert y["status"] == 0 and max(rl.pose_error(y["R"], y["T"], b.R[i], b.T[i])) <= 1e-9
        exact = np.flatnonzero(y["scores"] < 1e-12)                 # every hypothesis that fits all matches is the truth: no twin pose
        assert len(exact) > 10 and all(max(rl.pose_error(y["at"](int(k))["R"], y["at"](int(k))["T"], b.R[i], b.T[i])) <= 1e-9 for k in exact), i
        assert max(rl.pose_error(got.R[i], got.T[i], b.R[i], b.T[i])) <= 1e-9 and got.related[i, 2] == got.related[i, 1] == got.related[i, 6]
    ratio = fk.relate_wrong_K()
    print(f"relative pose: the error with the next pair's K_a / K_b is at least {ratio[:, 0].min():.3e} / {ratio[:, 1].min():.3e} x the bound")
    assert ratio.shape == (b.n, 2) and np.all(ratio > 1.0)


# ------------------------------------------------------------------ the two forms of K, and the record
def test_the_form_of_K_changes_the_host_walks_by_rounding_only():
    """a third of the items stored as K f0: the same statuses, winners and inlier flags (asserted where the change is measured),
    the results apart by the figures the GPU test gives a factor of ten"""
    fig = fk.cpu_figures()
    print(json.dumps(fig, indent=1))
    assert fig["triangulate"]["form_change_in_cond_bounds"] <= 1.0
    assert fig["resect"]["form_change_newton_steps"] <= fig["resect"]["host_walk_floor_newton_steps"]
    assert fig["locate"]["form_change"] <= max(fig["locate"]["host_floor"], 1e-12)
    assert fig["relate"]["form_change"] <= 1e-9
    b, opts = fk.resect_small(False), rc.RAGGED_OPTIONS[False]
    a, m = fk.resect_host_walk(b, *opts), fk.resect_host_walk(fk.mixed_form(b), *opts)
    assert np.array_equal(a[4], m[4]) and all(np.array_equal(x, y) for x, y in zip(a[5], m[5]))       # status and the accept / reject logs
    t = fk.tri_big()
    assert np.array_equal(fk.tri_host_walk(t)[2], fk.tri_host_walk(fk.mixed_form(t))[2])
    # the record holds these figures as one run measured them; they are maxima of rounding errors, so only their kind is compared
    rec = json.load(open(FIGURES))["cpu"]
    assert {front: sorted(figures) for front, figures in rec.items()} == {front: sorted(figures) for front, figures in fig.items()}
