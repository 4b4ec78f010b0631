"""The front ends on the device (DESIGN.md sections 21 to 24) on batches whose items carry distinct intrinsics, one shared K, or
the same cameras stored as K f0 (tests/frontend_k_cases.py).  The host walks and the yardsticks take one K per item, so these are
the tests that see which K a kernel read: k_tri_pack, k_resect_pack, k_resect_frames, k_locate_score, k_locate_pick,
k_relate_solve and k_relate_pick.  tests/test_frontend_k_cpu.py shows that on the noise-free batches a neighbour's K misses every
bound used here by ten decades, and computes the floors."""
from types import SimpleNamespace

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import io as sio
from surikatoko_amd import locate as LC
from surikatoko_amd import relate as RL
from surikatoko_amd import resect as RS
from surikatoko_amd import triangulate as TR
import frontend_k_cases as fk
import locate_cases as lc
import relate_cases as rl
import resect_cases as rc
import test_gpu_resect as gpu_resect
import triangulate_cases as tc
import triangulate_ref as tref

pytestmark = pytest.mark.gpu
POSE_BOUND = 1e-9   # tests/test_gpu_relate.py


@pytest.fixture(scope="module")
def h():
    ba = sa.BundleAdjustmentKanatani(0)
    yield ba
    ba.close()


@pytest.fixture(scope="module", autouse=True)
def compiler():
    if lc.cxx() is None:
        pytest.skip("no host C++ compiler")


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1)


def _same_bits(a, b):
    a, b = list(a), list(b)
    return len(a) == len(b) and all((x is None and y is None) or np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _tri(h, b, q=None, K=None, **kw):
    return sa.triangulate_tracks(h, b.f0, b.row_ptr, b.frame, b.uv, b.R, b.T, b.K if K is None else K, q=q, **kw)


def _resect(h, b, K=None, **kw):
    return sa.resect_frames(h, b.f0, b.row_ptr, b.point, b.uv, b.X, b.K if K is None else K, b.R0, b.T0, q=b.q, **kw)


def _locate(h, b, K=None, **kw):
    return sa.locate_frames(h, b.f0, b.row_ptr, b.point, b.uv, b.X, b.K if K is None else K, q=b.q, **kw)


def _relate(h, b, Ka=None, Kb=None, **kw):
    return sa.relate_frames(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka if Ka is None else Ka, b.Kb if Kb is None else Kb, q=b.q, want_inliers=True,
                            inlier_pixels=rl.TAU, **kw)


def _located(res):
    return SimpleNamespace(R=res.R, T=res.T, located=res.located, status=res.located_status)


def _figure(front, what, value):
    print(f"frontend_k figure: {front} {what} {value:.3e}")


# ------------------------------------------------------------------ the truth, on noise-free batches
def test_tri_recovers_the_truth(h):
    """the bound of test_conditioning_stays_at_eps_cond: 8 eps cond_2(A) |X| to the truth and to the host function"""
    b = fk.tri_truth()
    X, quality, status = _tri(h, b)
    assert not status.any() and np.array_equal(quality[:, 3], np.diff(b.row_ptr).astype(np.float64))
    worst = 0.0
    for i in range(b.n):
        bound = tc.cond_bound(b, i, b.X_true[i])
        Xh = sio.triangulate_least_squares(tc.track(b, i)[1], tc.host_P(b, i), b.f0)
        worst = max(worst, np.linalg.norm(X[i] - b.X_true[i]) / bound, np.linalg.norm(X[i] - Xh) / bound)
    _figure("triangulate", "truth_in_cond_bounds", worst)
    assert worst <= 1.0


def test_resect_recovers_the_truth(h):
    """as test_noise_free_accuracy: ten times the yardstick's own maximum in eps sqrt(cond_2(H_s))"""
    b = fk.resect_truth()
    ys, floor = fk.resect_truth_yardstick()
    R, T, quality, info, status = _resect(h, b, attempts=40, rel_change=0.0)
    assert np.all(status == RS.RESECT_NOT_CONVERGED) and np.all(quality[:, 5] == 40)
    got = max(rc.accuracy_units(R[i], T[i], b.frames[i], ys[i]["H"]) for i in range(b.n))
    _figure("resect", "truth_eps_sqrt_cond", got)
    assert got <= 10 * floor
    assert np.all(quality[:, 0] < 1e-9)


def test_locate_recovers_the_truth(h):
    """as test_noise_free: ten times the host walk's distance from the truth on the same batch"""
    b = fk.locate_truth()
    res = _locate(h, b, hypotheses=64, want_inliers=True)
    bound = 10 * fk.locate_truth_floor()
    err = [max(lc.pose_error(res.R[i], res.T[i], f)) for i, f in enumerate(b.frames)]
    _figure("locate", "truth", max(err))
    assert not res.located_status.any()
    assert max(err) <= bound and res.located[:, 0].max() < 1e-6
    assert np.array_equal(res.located[:, 2], res.located[:, 1]) and res.inliers.all()


def test_relate_recovers_the_truth(h):
    """as test_noise_free: max(1e-13, 64 x the yardstick's own distance from the truth on the same pair)"""
    b = fk.relate_truth()
    res = _relate(h, b, hypotheses=64)
    assert np.all(res.status == 0)
    worst = 0.0
    for i, (br, bt) in enumerate(fk.relate_truth_bounds()):
        dr, dt = rl.pose_error(res.R[i], res.T[i], b.R[i], b.T[i])
        worst = max(worst, dr, dt)
        n = b.row_ptr[i + 1] - b.row_ptr[i]
        assert dr <= br and dt <= bt, (i, dr, br, dt, bt)
        assert res.related[i, 2] == n and res.related[i, 6] == n and res.inliers[b.row_ptr[i]:b.row_ptr[i + 1]].all() and res.related[i, 0] < 1e-6
    _figure("relate", "truth", worst)


# ------------------------------------------------------------------ the yardstick, on the ragged batches
@pytest.mark.parametrize("holes", [False, True])
def test_tri_against_the_yardstick(h, holes):
    """257 frames with their own K, every track length once; as test_ragged_batches_against_the_yardstick"""
    b = fk.tri_big()
    q = fk.tri_holes() if holes else None
    X, quality, status = _tri(h, b, q=q)
    want = fk.tri_yardstick(b, q)
    assert np.array_equal(status, np.array([w[2] for w in want], np.uint32))
    assert np.array_equal(quality[:, 3], np.array([w[1][3] for w in want]))
    few = quality[:, 3] < 2
    assert np.all(status[few] == TR.TRI_FEW_VIEWS) and np.all(np.isnan(X[few]))
    worst = 0.0
    for i in np.flatnonzero(~few):
        Xy, qy, _, _ = want[i]
        bound = fk.tri_bound(b, i, Xy, q)
        worst = max(worst, np.linalg.norm(X[i] - Xy) / bound)
        assert np.linalg.norm(X[i] - Xy) <= bound, i
        assert abs(quality[i, 1] - qy[1]) <= np.degrees(100 * tref.EPS), i
        qi = None if q is None else q[b.row_ptr[i]:b.row_ptr[i + 1]]
        A, _ = tc.system(b, i, qi)
        assert abs(quality[i, 2] - qy[2]) <= (100 * tref.EPS * tref.cond2(A) + 1e-12) * qy[2], i
    _figure("triangulate", f"yardstick_in_cond_bounds_holes_{int(holes)}", worst)


def test_tri_frames_at_the_block_edges_have_the_bits_of_a_call_of_their_own(h):
    """the track over frames 0, 3, 4, 5, 255 and 256, and the track of 100 views: the same cameras alone in a call"""
    b = fk.tri_big()
    whole = _tri(h, b)
    for i in (10, 9, 8):
        alone = _tri(h, fk.tri_alone(b, i))
        assert _same_bits(alone, [a[i:i + 1] for a in whole]), i


@pytest.mark.parametrize("holes", [False, True])
def test_resect_against_the_yardstick(h, holes):
    b = fk.resect_small(holes)
    attempts, rel_change = rc.RAGGED_OPTIONS[holes]
    floor = fk.resect_host_floor()
    worst = gpu_resect._agree(_resect(h, b, attempts=attempts, rel_change=rel_change), fk.resect_yardstick(holes), b, 10 * floor)
    _figure("resect", f"yardstick_newton_steps_holes_{int(holes)}", worst)


def test_resect_257_frames(h):
    """every eighth frame against the yardstick; frames 0, 3, 4, 5, 255 and 256 with the bits they have alone with their own K"""
    b = fk.resect_big(False)
    attempts, rel_change = rc.RAGGED_OPTIONS[False]
    whole = _resect(h, b, attempts=attempts, rel_change=rel_change)
    ys = fk.resect_yardstick(False, "big")
    idx = list(fk.CHECKED)
    worst = gpu_resect._agree([a[idx] for a in whole], [ys[i] for i in idx], rc.rows(b, idx), 10 * fk.resect_host_floor())
    _figure("resect", "yardstick_newton_steps_257", worst)
    for i in fk.ALONE:
        alone = _resect(h, rc.rows(b, [i]), attempts=attempts, rel_change=rel_change)
        assert _same_bits(alone, [a[i:i + 1] for a in whole]), i


@pytest.mark.parametrize("holes", [False, True])
def test_locate_against_the_yardstick(h, holes):
    b = fk.locate_small(holes)
    res = _locate(h, b, hypotheses=fk.LOCATE_HYPOTHESES, seed=1, want_inliers=True)
    worst = lc.agree(b, fk.locate_yardstick(holes), _located(res), res.inliers)
    _figure("locate", f"yardstick_holes_{int(holes)}", worst)
    assert worst <= 10 * fk.locate_host_floor()
    if holes:
        assert not res.inliers[b.q == 0].any()


def _locate_out(res):
    return (res.R, res.T, res.located, res.located_status)


def test_locate_257_frames(h):
    b = fk.locate_big(False)
    kw = dict(hypotheses=fk.LOCATE_HYPOTHESES, seed=1, want_inliers=True)
    whole = _locate(h, b, **kw)
    worst = lc.agree(b, fk.locate_yardstick(False, "big"), _located(whole), whole.inliers)
    _figure("locate", "yardstick_257", worst)
    assert worst <= 10 * fk.locate_host_floor()
    assert np.array_equal(whole.located_status, np.where(np.diff(b.row_ptr) < 4, LC.LOCATE_FEW_POINTS, 0))
    for i in fk.ALONE:
        alone = _locate(h, lc.rows(b, [i]), **kw)
        assert _same_bits(_locate_out(alone), [a[i:i + 1] for a in _locate_out(whole)]), i
        assert np.array_equal(alone.inliers, whole.inliers[b.row_ptr[i]:b.row_ptr[i + 1]]), i


@pytest.mark.parametrize("opts", [dict(attempts=10), dict(loss="cauchy", delta=2.0, attempts=20)])
def test_locate_chained_into_resect_is_resect_frames_from_the_located_poses(h, opts):
    b = lc.rows(fk.locate_big(True), range(40))
    plain = _locate(h, b, hypotheses=65, want_inliers=True)
    fine = _locate(h, b, hypotheses=65, refine=opts, want_inliers=True, want_weights=True)
    assert _same_bits((plain.located, plain.located_status, plain.inliers), (fine.located, fine.located_status, fine.inliers))
    own = sa.resect_frames(h, b.f0, b.row_ptr, b.point, b.uv, b.X, b.K, plain.R, plain.T, q=b.q, want_weights=True, **opts)
    assert _same_bits((fine.R, fine.T, fine.quality, fine.info, fine.status, fine.weights), own)
    assert np.count_nonzero(plain.located_status == 0) >= 30


@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("hypotheses", fk.RELATE_HYPOTHESES)
def test_relate_against_the_yardstick(h, hypotheses, holes):
    b = fk.relate_ragged(holes)
    worst = rl.agree(b, fk.relate_ragged_yardstick(holes, hypotheses), _relate(h, b, hypotheses=hypotheses), POSE_BOUND)
    _figure("relate", f"yardstick_H_{hypotheses}_holes_{int(holes)}", worst)


def _pair_bits(res, b, i):
    s = slice(int(b.row_ptr[i]), int(b.row_ptr[i + 1]))
    return np.concatenate([_bits(res.R[i]), _bits(res.T[i]), _bits(res.E[i]), _bits(res.related[i]), _bits(res.status[i:i + 1]), res.inliers[s]])


def test_relate_17_pairs(h):
    b = fk.relate_many()
    whole = _relate(h, b, hypotheses=65)
    worst = rl.agree(b, fk.relate_many_yardstick(), whole, POSE_BOUND)
    _figure("relate", "yardstick_17_pairs", worst)
    for i in (0, 3, 4, 5, 16):
        one = rl.rows(b, [i])
        assert np.array_equal(_pair_bits(_relate(h, one, hypotheses=65), one, 0), _pair_bits(whole, b, i)), i
    for H in (1, 3, 5):                      # three or four groups of one solve wave belong to different pairs
        few = _relate(h, b, hypotheses=H)
        for i in (0, 1, 3, 4, 5, 16):
            one = rl.rows(b, [i])
            assert np.array_equal(_pair_bits(_relate(h, one, hypotheses=H), one, 0), _pair_bits(few, b, i)), (H, i)


# ------------------------------------------------------------------ one K for all items: shared_k = 1
# The handle's K buffers only grow and a one-K call uploads nine doubles into their front, so what lies behind is what the last
# call left there.  Each one-K call below is therefore sent right after a call of the same shapes with distinct K, and before the
# call that repeats the K per item: a kernel that read K + 9 * i despite shared_k, or a launch that passed shared_k = 0, takes
# another camera for every item but the first and loses the bits.
def test_tri_shared_K(h):
    b = fk.tri_shared()
    other, one = fk.tri_big(), b.K[:1]
    assert one.shape == (1, 3, 3) and len(b.R) == len(other.R) > 4 and not np.array_equal(other.K[1], b.K[1])
    _tri(h, other)
    auto = _tri(h, b, K=one)
    _tri(h, other)
    told = _tri(h, b, K=one, shared_k=True)
    q = fk.tri_holes()
    _tri(h, other)
    fine = _tri(h, b, K=one, q=q, refine_attempts=3)
    want = _tri(h, b)
    assert _same_bits(auto, want) and _same_bits(told, want)
    assert not want[2][2:].any()
    assert _same_bits(fine, _tri(h, b, q=q, refine_attempts=3))


def test_resect_shared_K(h):
    b = fk.resect_shared()
    other, one = fk.resect_small(False), b.K[:1]
    assert RS.resect_frame_args(b.row_ptr, b.point, b.uv, b.q, one, b.R0, b.T0)[6] is True and b.n == other.n > 4
    assert RS.resect_frame_args(b.row_ptr, b.point, b.uv, b.q, b.K, b.R0, b.T0)[6] is False
    for kw in (dict(attempts=4, rel_change=1e-4), dict(attempts=6, loss="cauchy", delta=2.0, want_weights=True)):
        _resect(h, other)
        got = _resect(h, b, K=one, **kw)
        want = _resect(h, b, **kw)
        assert _same_bits(got, want)
        assert np.count_nonzero(want[4] & RS.RESECT_FEW_POINTS) == 2     # the frames of 0 and 2 points; the others were refined


def test_locate_shared_K(h):
    b = fk.locate_shared()
    other, one = fk.locate_small(False), b.K[:1]
    assert LC.locate_frame_args(b.row_ptr, b.point, b.uv, b.q, one)[6] is True and b.n == other.n > 4
    assert LC.locate_frame_args(b.row_ptr, b.point, b.uv, b.q, b.K)[6] is False
    for kw in (dict(hypotheses=65, want_inliers=True), dict(hypotheses=64, want_inliers=True, refine=dict(attempts=5), want_weights=True)):
        _locate(h, other, hypotheses=8)
        got = _locate(h, b, K=one, **kw)
        want = _locate(h, b, **kw)
        assert _same_bits(got, want)
        assert np.count_nonzero(want.located_status == 0) >= 5          # the call did locate frames


def test_relate_shared_K(h):
    b = fk.relate_shared()
    other, Ka, Kb = fk.relate_ragged(False), b.Ka[:1], b.Kb[:1]
    assert RL.relate_pair_args(b.row_ptr, b.uv_a, b.uv_b, b.q, Ka, Kb)[7] is True and b.n == other.n > 4 and not np.array_equal(Ka, Kb)
    assert RL.relate_pair_args(b.row_ptr, b.uv_a, b.uv_b, b.q, b.Ka, b.Kb)[7] is False
    for H in (3, 65):
        _relate(h, other, hypotheses=3)
        got = _relate(h, b, Ka=Ka, Kb=Kb, hypotheses=H)
        want = _relate(h, b, hypotheses=H)
        assert _same_bits(got, want)
        assert np.count_nonzero(want.status == 0) >= 5                  # the call did relate pairs


# ------------------------------------------------------------------ the same cameras stored as K f0
def test_tri_form_of_K(h):
    """a third of the frames with K(2,2) = f0: the same statuses; the points apart by at most ten times what the host walk shows"""
    b = fk.tri_big()
    a, m = _tri(h, b), _tri(h, fk.mixed_form(b))
    assert np.array_equal(a[2], m[2]) and np.array_equal(a[1][:, 3], m[1][:, 3])
    got, floor = fk.tri_form_units(b, a[0], m[0]), fk.tri_form_change()
    _figure("triangulate", "form_change_in_cond_bounds", got)
    assert got <= 10 * floor


def test_resect_form_of_K(h):
    b, opts = fk.resect_small(False), dict(zip(("attempts", "rel_change"), rc.RAGGED_OPTIONS[False]))
    a, m = _resect(h, b, **opts), _resect(h, fk.mixed_form(b), **opts)
    assert np.array_equal(a[4], m[4]) and np.array_equal(a[2][:, [1, 5]], m[2][:, [1, 5]])     # status, weighted observations, attempts used
    got, floor = fk.resect_form_units(b, fk.resect_yardstick(False), a, m), fk.resect_form_change()
    _figure("resect", "form_change_newton_steps", got)
    assert got <= 10 * floor


def test_locate_form_of_K(h):
    b = fk.locate_small(False)
    kw = dict(hypotheses=fk.LOCATE_HYPOTHESES, seed=1, want_inliers=True)
    a, m = _locate(h, b, **kw), _locate(h, fk.mixed_form(b), **kw)
    assert np.array_equal(a.located_status, m.located_status) and np.array_equal(a.located[:, 1:5], m.located[:, 1:5], equal_nan=True)
    assert np.array_equal(a.inliers, m.inliers)
    got, floor = fk.locate_form_units(a.located_status, (a.R, a.T), (m.R, m.T)), fk.locate_form_change()
    _figure("locate", "form_change", got)
    assert got <= 10 * floor


def test_relate_form_of_K(h):
    b = fk.relate_many()
    a, m = _relate(h, b, hypotheses=65), _relate(h, fk.mixed_form(b, ("Ka", "Kb")), hypotheses=65)
    assert np.array_equal(a.status, m.status) and np.array_equal(a.related[:, [1, 2, 3, 4, 6]], m.related[:, [1, 2, 3, 4, 6]], equal_nan=True)
    assert np.array_equal(a.inliers, m.inliers)
    got, floor = fk.relate_form_units(a.status, (a.R, a.T), (m.R, m.T)), fk.relate_form_change()
    _figure("relate", "form_change", got)
    assert got <= 10 * floor
