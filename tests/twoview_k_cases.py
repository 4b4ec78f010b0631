"""Cases in which every pair of a two-view batch carries its own two intrinsics matrices, for pair refinement
and the homography (section 27), and the table that walks the homography's decomposition over its range.  Shared by
tests/test_twoview_k_cpu.py (the gate: the guards of the existing cases hold on these, a neighbour's K misses every bound) and
tests/test_gpu_twoview_k.py (the kernels).  The sibling of tests/frontend_k_cases.py, whose helpers (own_K, mixed_form, rolled,
with_K, BIG, ALONE, CHECKED) are used as they are.  Built once per process and never modified.

Every pair of tests/pair_cases.py and tests/homography_cases.py carries relate_cases.K0 and K1, and the host walks and the numpy
yardsticks take one K per pair: the reads `shared_k ? K_a : K_a + 9 * j` of k_pair_pack, `kinv_all + SRK_PAIR_KINV * i` of
k_pair_refine and `K_a + (shared_k ? 0 : 9 * i)` of k_homog_pick exist in device and launch code alone.  Here K_a and K_b of every
pair are independent seeded draws and the pixels are projected with the pair's own matrices."""
import functools
from types import SimpleNamespace

import numpy as np

import frontend_k_cases as fk
import homography_cases as hc
import homography_ref as href
import pair_cases as pc
import pair_ref
import relate_cases as rl
import relate_ref as rlref
from frontend_k_cases import ALONE, BIG, CHECKED, mixed_form, own_K, rolled, with_K  # noqa: F401

POSE_BOUND = 1e-9                  # tests/test_gpu_relate.py, tests/test_gpu_homography.py: a noise-free pair against the truth
WRONG_K_FACTOR = 1e3               # a neighbour's K misses POSE_BOUND by at least this factor
# chosen on the CPU so that the guards of tests/test_twoview_k_cpu.py hold (no pair at a threshold, clear winners)
PAIR_SEED = {False: 2802, True: 2800}
PAIR_OPTIONS = pc.RAGGED_OPTIONS
PAIR_TRUTH_ATTEMPTS = 30           # from 3 and 5 degrees off, noise-free: E_pair reaches rounding well before
PAIR_BIG_OPTIONS = (4, 1e-4)
HOMOG_SEED = {False: 2900, True: 2901}
HOMOG_SAMPLER_SEED = {(False, 1): 2, (False, 63): 1, (False, 64): 1, (False, 65): 1, (False, 256): 23,
                      (True, 1): 1, (True, 63): 1, (True, 64): 1, (True, 65): 1, (True, 256): 8}
HOMOG_MANY_SEED, HOMOG_MANY_SAMPLER_SEED, HOMOG_MANY_HYPOTHESES = 2960, 2, 64
HOMOG_TRUTH_KINDS = ("planar", "planar", "rotation", "planar", "planar", "rotation")


def _pair(n, rng, **kw):
    return rl.pair(n, rng, Ka=own_K(rng, rl.K0), Kb=own_K(rng, rl.K1), **kw)


def _hpair(n, rng, kind, **kw):
    return hc.hpair(n, rng, kind, Ka=own_K(rng, rl.K0), Kb=own_K(rng, rl.K1), **kw)


def swapped(b):
    """the batch with K_a and K_b exchanged"""
    return with_K(b, Ka=b.Kb, Kb=b.Ka)


def wrong_K_views(b):
    """the batch with the next pair's K_a (K_b its own), with the next pair's K_b (K_a its own), and with K_a and K_b exchanged"""
    return dict(Ka_rolled=with_K(b, Ka=rolled(b.Ka)), Kb_rolled=with_K(b, Kb=rolled(b.Kb)), swapped=swapped(b))


# ------------------------------------------------------------------ pair refinement
@functools.lru_cache(maxsize=None)
def pair_ragged(holes=False):
    """pair_cases.ragged with K_a and K_b of every pair drawn independently"""
    rng = np.random.default_rng(PAIR_SEED[holes])
    ps, qs = [], []
    for n in pc.LENGTHS:
        extra = max(1, n // 5) if holes else 0
        p = _pair(n + extra, rng, planar=False, sigma=pc.SIGMA)
        w = rng.uniform(0.5, 2.0, n + extra)
        off = rng.choice(n + extra, extra, replace=False)
        w[off] = 0.0
        p.uv_b[off] = rng.uniform(0.0, 600.0, (extra, 2))
        ps.append(p)
        qs.append(w)
    return pc.with_starts(rl.batch(ps, np.concatenate(qs) if holes else None), rng)


@functools.lru_cache(maxsize=None)
def pair_ragged_yardstick(holes=False):
    b = pair_ragged(holes)
    attempts, rel_change = PAIR_OPTIONS[holes]
    return tuple(pc.yardstick(b, i, attempts=attempts, rel_change=rel_change) for i in range(b.n))


@functools.lru_cache(maxsize=None)
def pair_host_floor():
    """pair_cases.host_walk_floor on the batches here: the largest distance, in Newton-step units, between the yardstick and the
    host walk"""
    worst = 0.0
    for holes in (False, True):
        b = pair_ragged(holes)
        attempts, rel_change = PAIR_OPTIONS[holes]
        got, _, logs = pc.host_walk(b, attempts, rel_change)
        worst = max(worst, pc.agree(got, pc.tagged(pair_ragged_yardstick(holes), rel_change), b, logs=logs))
    return worst


@functools.lru_cache(maxsize=None)
def pair_truth():
    """six noise-free pairs of 40 .. 60 matches, general and forward motion, the starts 3 degrees and 5 degrees of direction off"""
    rng = np.random.default_rng(2810)
    return pc.with_starts(rl.batch([_pair(40 + 4 * i, rng, kind=kind) for i, kind in enumerate(fk.RELATE_TRUTH_KINDS)]), rng)


def pair_truth_yardstick(b):
    return [pc.yardstick(b, i, attempts=PAIR_TRUTH_ATTEMPTS, rel_change=0.0) for i in range(b.n)]


@functools.lru_cache(maxsize=None)
def pair_big():
    """257 pairs of 8 .. 20 matches with half a pixel of noise: 255 and 256 straddle k_pair_pack's block edge, 3, 4, 5 the
    four-waves-a-workgroup edge of k_pair_refine"""
    rng = np.random.default_rng(2820)
    return pc.with_starts(rl.batch([_pair(int(rng.integers(8, 21)), rng, sigma=pc.SIGMA) for _ in range(BIG)]), rng)


@functools.lru_cache(maxsize=None)
def pair_shared():
    """one pair of each length of pair_cases.LENGTHS, all with one K_a and one K_b (K_a != K_b)"""
    rng = np.random.default_rng(2830)
    Ka, Kb = own_K(rng, rl.K0), own_K(rng, rl.K1)
    return pc.with_starts(rl.batch([rl.pair(n, rng, sigma=pc.SIGMA, Ka=Ka, Kb=Kb) for n in pc.LENGTHS]), rng)


def pose_gap(R, T, Rt, Tt):
    """the larger of the rotation angle and the angle between the directions"""
    return max(rlref.rotation_angle(R, Rt), rlref.direction_angle(T, Tt))


def pair_form_units(status, a, m):
    """the largest pose_gap between two results (R, T each) over the pairs that were refined"""
    return max([0.0] + [pose_gap(a[0][i], a[1][i], m[0][i], m[1][i]) for i in np.flatnonzero((status & pair_ref.FEW_POINTS) == 0)])


@functools.lru_cache(maxsize=None)
def pair_form_change():
    """the host walk on pair_ragged(False) and on its copy with a third of the matrices stored as K f0: the same statuses,
    counters and accept / reject sequences; returns the largest distance between the poses"""
    b = pair_ragged(False)
    attempts, rel_change = PAIR_OPTIONS[False]
    (a, _, la), (m, _, lm) = pc.host_walk(b, attempts, rel_change), pc.host_walk(mixed_form(b, ("Ka", "Kb")), attempts, rel_change)
    assert np.array_equal(a.status, m.status) and np.array_equal(a.quality[:, [1, 4, 5]], m.quality[:, [1, 4, 5]], equal_nan=True)
    assert all(np.array_equal(x[:, 0], y[:, 0]) for x, y in zip(la, lm))
    return pair_form_units(a.status, (a.R, a.T), (m.R, m.T))


@functools.lru_cache(maxsize=None)
def pair_wrong_K():
    """per pair of pair_truth and per view of wrong_K_views: the yardstick's distance from the truth over POSE_BOUND"""
    b = pair_truth()
    out = {}
    for name, w in wrong_K_views(b).items():
        ys = pair_truth_yardstick(w)
        out[name] = np.array([pose_gap(y["R"], y["T"], b.R[i], b.T[i]) / POSE_BOUND for i, y in enumerate(ys)])
    return out


# ------------------------------------------------------------------ the homography
@functools.lru_cache(maxsize=None)
def homog_ragged(holes=False):
    """homography_cases.ragged with K_a and K_b of every pair drawn independently"""
    rng = np.random.default_rng(HOMOG_SEED[holes])
    ps, qs = [], []
    for k, n in enumerate(hc.LENGTHS):
        extra = (n + 4) // 5 if holes else 0
        ps.append(_hpair(n + extra, rng, "planar" if k % 2 == 0 else "rotation", sigma=0.5))
        w = rng.uniform(0.5, 2.0, n + extra)
        w[rng.choice(n + extra, extra, replace=False)] = 0.0
        qs.append(w)
    return hc.batch(ps, np.concatenate(qs) if holes else None)


def _homog_ragged_f():
    return homog_ragged(False)


def _homog_ragged_t():
    return homog_ragged(True)


def homog_ragged_scored(holes, hypotheses):
    return hc._scored(_homog_ragged_t if holes else _homog_ragged_f, hypotheses, HOMOG_SAMPLER_SEED[(holes, hypotheses)], hc.TAU)


def homog_ragged_yardstick(holes, hypotheses, rounds):
    return [href.pick(a, hypotheses, rounds) for a in homog_ragged_scored(holes, hypotheses)]


@functools.lru_cache(maxsize=None)
def homog_many():
    """homography_cases.many(17) with own K: 17 pairs of 8 .. 70 matches, pair 2 empty, half a pixel of noise"""
    rng = np.random.default_rng(HOMOG_MANY_SEED)
    ps = [_hpair(int(rng.integers(8, 71)), rng, "planar" if k % 2 == 0 else "rotation", sigma=0.5) for k in range(17)]
    ps[2] = _hpair(0, rng, "planar")
    return hc.batch(ps)


def homog_many_scored():
    return hc._scored(homog_many, HOMOG_MANY_HYPOTHESES, HOMOG_MANY_SAMPLER_SEED, hc.TAU)


@functools.lru_cache(maxsize=None)
def homog_many_yardstick(rounds=4):
    return [href.pick(a, HOMOG_MANY_HYPOTHESES, rounds) for a in homog_many_scored()]


@functools.lru_cache(maxsize=None)
def homog_truth():
    """six noise-free pairs of 40 matches: four on the plane, two pure rotations; the batch and its pairs"""
    rng = np.random.default_rng(2910)
    ps = [_hpair(40, rng, kind) for kind in HOMOG_TRUTH_KINDS]
    return hc.batch(ps), ps


@functools.lru_cache(maxsize=None)
def homog_shared():
    """one pair of each length of homography_cases.LENGTHS, all with one K_a and one K_b (K_a != K_b)"""
    rng = np.random.default_rng(2920)
    Ka, Kb = own_K(rng, rl.K0), own_K(rng, rl.K1)
    return hc.batch([hc.hpair(n, rng, "planar" if k % 2 == 0 else "rotation", sigma=0.5, Ka=Ka, Kb=Kb) for k, n in enumerate(hc.LENGTHS)])


def plane_distance(R, T, N, Rt, Tt, Nt):
    """the largest entry of (R, T, N) - (R_t, T_t, N_t)"""
    return max(np.abs(R - Rt).max(), np.abs(T - Tt).max(), np.abs(N - Nt).max())


def homog_truth_of(p):
    """(R, T / d, N) of a pair of homog_truth: a rotation has T = N = 0"""
    if not p.T.any():
        return p.R, np.zeros(3), np.zeros(3)
    return p.R, p.T / hc.PLANE_D, hc.PLANE_N


def truth_distances(got, i, truth):
    """the distances of pair i's candidates from the truth"""
    return [plane_distance(got.R[i, k], got.T[i, k], got.N[i, k], *truth) for k in range(int(got.n_poses[i]))]


def rays(p, Ka, Kb, f0=hc.F0):
    """the rays of a pair's pixels through the given matrices"""
    return href.homog(p.uv_a, f0) @ np.linalg.inv(Ka).T, href.homog(p.uv_b, f0) @ np.linalg.inv(Kb).T


@functools.lru_cache(maxsize=None)
def homog_wrong_K():
    """per pair of homog_truth and per view of wrong_K_views: the distance of the yardstick's nearer candidate from the truth over
    POSE_BOUND.  G lives in pixels and is the pair's true homography; only H = K_b^-1 G K_a and its decomposition read K"""
    b, ps = homog_truth()
    out = {}
    for name, w in dict(own=b, **wrong_K_views(b)).items():
        d = []
        for i, p in enumerate(ps):
            _, _, poses = href.decompose(np.linalg.inv(w.Kb[i]) @ hc.true_homography(p) @ w.Ka[i], *rays(p, w.Ka[i], w.Kb[i]))
            d.append(min(plane_distance(R, T, N, *homog_truth_of(p)) for R, T, N, _ in poses) / POSE_BOUND)
        out[name] = np.array(d)
    return out


def homog_form_units(status, a, m):
    """the largest distance between the poses of two results over the pairs with a model, candidate by candidate"""
    worst = 0.0
    for i in np.flatnonzero(status == 0):
        for k in range(int(a.n_poses[i])):
            worst = max(worst, plane_distance(a.R[i, k], a.T[i, k], a.N[i, k], m.R[i, k], m.T[i, k], m.N[i, k]))
    return worst


def homog_form_same(a, m):
    """what the form of K must not change: G, the counts, the winner, the rounds and the inlier flags, bit for bit"""
    return (np.array_equal(a.status, m.status) and np.array_equal(a.G.view(np.uint8), m.G.view(np.uint8)) and np.array_equal(a.n_poses, m.n_poses)
            and np.array_equal(a.homog[:, :6].view(np.uint8), m.homog[:, :6].view(np.uint8)) and np.array_equal(a.inliers, m.inliers)
            and np.array_equal(a.front, m.front))


@functools.lru_cache(maxsize=None)
def homog_form_change():
    b = homog_many()
    kw = dict(hypotheses=HOMOG_MANY_HYPOTHESES, seed=HOMOG_MANY_SAMPLER_SEED)
    a, m = hc.host_walk(b, **kw), hc.host_walk(mixed_form(b, ("Ka", "Kb")), **kw)
    assert homog_form_same(a, m)
    return homog_form_units(a.status, a, m)


# ------------------------------------------------------------------ the decomposition over its range
# One table for the CPU and the GPU, built from (R, t = T / d, N) directly: 40 noise-free matches on the plane N^T X = d, each case
# with its own K_a and K_b.  The baselines run from |t| = 1 down to 1e-11: w1 - w3 is about 2 |t|, so 1e-9 lies a factor 20 above
# SRK_HOMOG_GAP = 1e-10 and 1e-11 a factor 5 below.  (The gap itself is good to a few eps, six decades less than its distance from
# the bound in either case; the existing guard's factor of ten is for pairs with noise and would excuse |t| = 1e-11.)  The double
# singular values: t = s R N (the camera backs away along the normal, w2 = w3) and t = -s R N (it approaches, w1 = w2), where
# sqrt(1 - e3) or sqrt(e1 - 1) is the root of a rounding error and Jacobi's vectors of the repeated eigenvalue are arbitrary.  The
# rotations by 0, 0.3, pi - 1e-6 and pi about the optical axis (the scene stays in front) go through the nearest-rotation step.
DECOMPOSITION_BASELINES = (1.0, 1e-1, 1e-3, 1e-5, 1e-7, 1e-9, 1e-11)
DECOMPOSITION_DOUBLES = (0.3, 1e-3)
DECOMPOSITION_ANGLES = (("0", 0.0), ("0.3", 0.3), ("pi-1e-6", np.pi - 1e-6), ("pi", np.pi))
DECOMPOSITION_SCALES = (-3.0, 0.37, 2.5, -0.011, 1.0, 4e3, -1.0)     # the factors the exact H of every case is handed over with
DECOMPOSITION_MATCHES, DECOMPOSITION_DEPTH = 40, 6.0
DECOMPOSITION_FLOOR, DECOMPOSITION_FACTOR = 1e-13, 10.0
DECOMPOSITION_TRUTH_FROM = 1e-3    # the device's poses are compared with the truth from this |t| on


def _direction(rng):
    v = np.array([rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0), rng.uniform(0.3, 1.0)])
    return v / np.linalg.norm(v)


def _normal(rng):
    v = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 1.0])
    return v / np.linalg.norm(v)


def _general_rotation(rng):
    w = rng.normal(size=3)
    return rl.rotation(w / np.linalg.norm(w) * rng.uniform(0.1, 0.3))


def _plane_case(name, R, t, N, rng):
    d = DECOMPOSITION_DEPTH * N[2]                              # the plane meets the optical axis at the depth 6
    x, y = rng.uniform(-2.0, 2.0, DECOMPOSITION_MATCHES), rng.uniform(-1.5, 1.5, DECOMPOSITION_MATCHES)
    X = np.column_stack([x, y, (d - N[0] * x - N[1] * y) / N[2]])
    Xb = X @ R.T + d * t
    assert np.abs(X @ N - d).max() <= 1e-14 * d and X[:, 2].min() > 1.0 and Xb[:, 2].min() > 1.0, name    # in front of both cameras
    Ka, Kb = own_K(rng, rl.K0), own_K(rng, rl.K1)
    p = SimpleNamespace(name=name, R=R, T=d * t, t=t, N=N, d=d, X=X, Ka=Ka, Kb=Kb, uv_a=rl.pixels(Ka, X), uv_b=rl.pixels(Kb, Xb),
                        moved=np.zeros(0, int), H=R + np.outer(t, N), size=float(np.linalg.norm(t)))
    p.xa, p.xb = rays(p, Ka, Kb)
    return p


@functools.lru_cache(maxsize=None)
def decomposition_cases():
    rng = np.random.default_rng(2950)
    out = []

    def add(name, R, t, N):
        out.append(_plane_case(name, R, t, N, rng))
    for size in DECOMPOSITION_BASELINES:
        add(f"baseline_{size:.0e}", _general_rotation(rng), size * _direction(rng), _normal(rng))
    for s in DECOMPOSITION_DOUBLES:
        R, N = _general_rotation(rng), _normal(rng)
        add(f"double_upper_{s:g}", R, s * (R @ N), N)
        R, N = _general_rotation(rng), _normal(rng)
        add(f"double_lower_{s:g}", R, -s * (R @ N), N)
    for name, angle in DECOMPOSITION_ANGLES:
        add(f"rotation_{name}", rl.rotation(np.array([0.0, 0.0, angle])), 0.1 * _direction(rng), _normal(rng))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def decomposition_batch():
    return hc.batch(list(decomposition_cases()))


def decomposition_truth(p, n_poses):
    """(R, t, N) of a case; where the gap is below its bound the answer is the rotation alone, T = N = 0"""
    return (p.R, p.t, p.N) if n_poses == 2 else (p.R, np.zeros(3), np.zeros(3))


def nearest(poses, truth):
    return min(plane_distance(R, T, N, *truth) for R, T, N in poses)


@functools.lru_cache(maxsize=None)
def decomposition_yardstick():
    """Per case: the yardstick's decomposition of the exact H times every factor of DECOMPOSITION_SCALES (H normalised, gap,
    poses), the largest distance of its nearer candidate from the truth over the factors, and the bound that distance gives: ten
    times it, never below 1e-13.  The distance is taken over all factors because at a double singular value the number under the
    root is a rounding error of either sign: a negative one is clamped to zero and gives the truth exactly, so one factor alone may
    show no error where the next shows sqrt(eps / gap)."""
    out = []
    for p in decomposition_cases():
        runs = [href.decompose(s * p.H, p.xa, p.xb) for s in DECOMPOSITION_SCALES]
        n_poses = len(runs[0][2])
        assert all(len(r[2]) == n_poses for r in runs), p.name
        own = [nearest([c[:3] for c in r[2]], decomposition_truth(p, n_poses)) for r in runs]
        out.append(SimpleNamespace(runs=runs, gap=runs[0][1], n_poses=n_poses, distances=own, distance=max(own),
                                   bound=max(DECOMPOSITION_FLOOR, DECOMPOSITION_FACTOR * max(own))))
    return tuple(out)


def one_of(R, T, N, front, n_inliers, poses):
    """the distance of (R, T, N) from the nearest of the yardstick's `poses`; with exactly half the inliers in front both signs of
    (T, N) meet the rule, as in homography_cases.agree"""
    signs = (1.0, -1.0) if 2 * front == n_inliers else (1.0,)
    return min(plane_distance(R, T, N, Ry, sg * Ty, sg * Ny) for Ry, Ty, Ny, _ in poses for sg in signs)


def as_result(ds):
    """HomographyPoses of several cases as the fields homography_cases.check_poses reads"""
    return SimpleNamespace(H=np.array([d.H for d in ds]), n_poses=np.array([d.n_poses for d in ds]), R=np.array([d.R for d in ds]),
                           T=np.array([d.T for d in ds]), N=np.array([d.N for d in ds]), front=np.array([d.front for d in ds]))


# ------------------------------------------------------------------ the record
def cpu_figures():
    """what profiles/frontend_intrinsics/test_figures.json records of the CPU side under `pair` and `homography`"""
    pw, hw = pair_wrong_K(), homog_wrong_K()
    return dict(pair=dict(host_walk_floor_newton_steps=pair_host_floor(), form_change=pair_form_change(),
                          wrong_K_smallest_ratio={k: float(v.min()) for k, v in pw.items()}),
                homography=dict(form_change=homog_form_change(), own_K_largest_ratio=float(hw["own"].max()),
                                wrong_K_smallest_ratio={k: float(v.min()) for k, v in hw.items() if k != "own"}))
