"""The cases of map alignment, shared by tests/test_align_cpu.py (the yardstick and the host walk of a set,
no GPU) and tests/test_gpu_align.py (the kernels).  Built once per process and never modified; the yardstick's results are cached
per process."""
import functools
import os
from types import SimpleNamespace

import numpy as np

import align_ref as ref
from surikatoko_amd import align as AL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE, TAU = 0.01, 0.05
LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 300)   # weighted correspondences: the sample size, the edges of the ballot and of the lane-strided sums
HYPOTHESES = (1, 63, 64, 65, 256)                               # one lane, a wave short of one, a full wave, a wave and one lane, four waves
BATCH_SIZES = (1, 3, 5, 257)                                    # four waves a workgroup: a partly empty workgroup, many workgroups
ACCURACY_POINTS = (3, 4, 5, 63, 64, 65, 129, 300)
SCALES = (1e-3, 1.0, 1e3)
# the seed of the ragged batches (without / with q = 0 in between) and the sampler's seed per hypothesis count, chosen so that on
# every set of more than four correspondences the yardstick's winner is clear, no correspondence sits at the inlier threshold and
# no candidate's score at the score it has to beat (tests/test_align_cpu.py asserts it)
RAGGED_SEED = {False: 2524, True: 2517}
SAMPLER_SEED = {1: 1, 63: 1, 64: 1, 65: 1, 256: 1}
BIG_HYPOTHESES = 65                                             # the 257-set batch runs at this count only (the yardstick is a Python loop)
OUTLIER_SEED = {0.3: 2530, 0.5: 2550}


def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def similarity(rng, s=None):
    return (float(rng.uniform(0.5, 2.0)) if s is None else float(s), rotation(rng), rng.uniform(-3, 3, 3))


def apply(model, a):
    s, R, t = model
    return s * a @ R.T + t


def move_share(b, share, rng, tau=TAU):
    """`share` of the targets moved by 20 .. 200 tau in a random direction; returns their indices"""
    n = len(b)
    k = int(round(share * n))
    idx = np.sort(rng.choice(n, size=k, replace=False)) if k else np.zeros(0, np.int64)
    d = rng.normal(size=(k, 3))
    b[idx] += d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(20 * tau, 200 * tau, k)[:, None]
    return idx


def make_set(n, rng, sigma=0.0, share=0.0, s=None, with_scale=True, planar=False, centre=0.0, tau=TAU):
    """n points in a cube of side 4 (or on a plane in it) about `centre`, their images under a random similarity (scale s; 1
    without scale) plus sigma of noise, `share` of the targets moved"""
    a = rng.uniform(-2, 2, (n, 3))
    if planar:
        a[:, 2] = 0.3 * a[:, 0] - 0.2 * a[:, 1]
    a += centre
    truth = similarity(rng, s if with_scale else 1.0)
    if centre:
        truth = (truth[0], truth[1], truth[2] + centre)
    b = apply(truth, a) + sigma * rng.normal(size=(n, 3))
    moved = move_share(b, share, rng, tau) if n else np.zeros(0, np.int64)
    return SimpleNamespace(a=a, b=b, q=None, truth=truth, moved=moved)


def batch(sets):
    rp = np.concatenate([[0], np.cumsum([len(f.a) for f in sets])]).astype(np.int64)
    any_q = any(f.q is not None for f in sets)
    cat = lambda xs, w: np.concatenate(list(xs) + [np.zeros((0, w))]).reshape(-1, w)   # noqa: E731
    return SimpleNamespace(n=len(sets), row_ptr=rp, a=cat((f.a for f in sets), 3), b=cat((f.b for f in sets), 3),
                           q=np.concatenate([np.ones(len(f.a)) if f.q is None else f.q for f in sets] + [np.zeros(0)]) if any_q else None,
                           moved=np.concatenate([rp[i] + f.moved for i, f in enumerate(sets)] + [np.zeros(0, np.int64)]).astype(np.int64), sets=list(sets))


def rows(b, idx):
    return batch([b.sets[i] for i in idx])


def set_obs(b, i):
    o0, o1 = b.row_ptr[i], b.row_ptr[i + 1]
    return b.a[o0:o1], b.b[o0:o1], None if b.q is None else b.q[o0:o1]


def without_holes(b):
    """the batch with its q = 0 correspondences cut out"""
    keep = b.q > 0
    rp = np.concatenate([[0], np.cumsum([np.count_nonzero(keep[b.row_ptr[i]:b.row_ptr[i + 1]]) for i in range(b.n)])]).astype(np.int64)
    return SimpleNamespace(n=b.n, row_ptr=rp, a=b.a[keep], b=b.b[keep], q=b.q[keep], sets=b.sets), keep


@functools.lru_cache(maxsize=None)
def accuracy(with_scale, scale):
    """noise-free sets of 3 .. 300 points at one scale, then a coplanar set and a set whose centroids lie 1e6 from the origin"""
    rng = np.random.default_rng(25 + int(with_scale))
    sets = [make_set(n, rng, s=scale, with_scale=with_scale) for n in ACCURACY_POINTS]
    sets.append(make_set(100, rng, s=scale, with_scale=with_scale, planar=True))
    sets.append(make_set(100, rng, s=scale, with_scale=with_scale, centre=1e6))
    return batch(sets)


def accuracy_tau(b):
    """noise-free: a thousandth of the targets' extent"""
    return 1e-3 * float(np.ptp(b.sets[-2].b, axis=0).max())


@functools.lru_cache(maxsize=None)
def ragged(holes=False):
    """257 sets whose weighted lengths cycle through LENGTHS, 0.01 of noise, 30 % of the targets moved by 20 .. 200 tau.  With
    holes, every set also carries correspondences with q = 0 (about one in five, wrong targets) in between and the weighted ones
    carry q in 0.5 .. 2."""
    rng = np.random.default_rng(RAGGED_SEED[holes])
    sets = []
    for i in range(BATCH_SIZES[-1]):
        L = LENGTHS[i % len(LENGTHS)]
        f = make_set(L, rng, sigma=NOISE, share=0.3, planar=(i % 7 == 3 and L > 5))
        if holes:
            extra = max(1, L // 5)
            n = L + extra
            off = np.sort(rng.choice(n, size=extra, replace=False))
            on = np.setdiff1d(np.arange(n), off)
            a, b, q = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
            a[on], b[on], q[on] = f.a, f.b, rng.uniform(0.5, 2.0, L)
            a[off], b[off] = rng.uniform(-2, 2, (extra, 3)), rng.uniform(-5, 5, (extra, 3))
            f.a, f.b, f.q, f.moved = a, b, q, on[f.moved]
        sets.append(f)
    return batch(sets)


def small(holes=False):
    """the first len(LENGTHS) sets of the ragged batch, every length once: every hypothesis count runs on these"""
    return rows(ragged(holes), range(len(LENGTHS)))


BIG_CHECKED = tuple(range(0, BATCH_SIZES[-1], 8))   # the sets of the 257-set batch the yardstick walks: every length (8 and 13 are coprime)


@functools.lru_cache(maxsize=None)
def outliers(share):
    """eight sets of 200 correspondences, 0.01 of noise, `share` of the targets moved by 20 .. 200 tau"""
    rng = np.random.default_rng(OUTLIER_SEED[share])
    return batch([make_set(200, rng, sigma=NOISE, share=share) for _ in range(8)])


def outlier_hypotheses(share):
    """the reference's count for three-point samples at p = 0.999, rounded up to a wave"""
    return -(-AL.ransac_hypotheses(share, 0.999, 3) // 64) * 64


def yardstick(b, i, hypotheses, seed, tau=TAU, with_scale=True, refine_rounds=2):
    a, t, q = set_obs(b, i)
    return ref.align_set(a, t, q, hypotheses, tau, seed, with_scale, refine_rounds)


@functools.lru_cache(maxsize=None)
def small_yardstick(holes, hypotheses):
    b = small(holes)
    return tuple(yardstick(b, i, hypotheses, SAMPLER_SEED[hypotheses]) for i in range(b.n))


@functools.lru_cache(maxsize=None)
def big_yardstick(holes=False):
    """the yardstick on the sets BIG_CHECKED of the 257-set batch, as a dict by set"""
    b = ragged(holes)
    return {i: yardstick(b, i, BIG_HYPOTHESES, SAMPLER_SEED[BIG_HYPOTHESES]) for i in BIG_CHECKED}


@functools.lru_cache(maxsize=None)
def outlier_yardstick(share):
    b = outliers(share)
    return tuple(yardstick(b, i, outlier_hypotheses(share), 1) for i in range(b.n))


def near_ties(y):
    """the hypotheses whose score lies within 1e-9 (relative) of the yardstick's best"""
    s = y["scores"]
    return set(np.flatnonzero(s - s.min() <= 1e-9 * s.min()).tolist())


def winner_is_clear(y):
    """every score that differs from the yardstick's best lies more than 1e-9 (relative) above it"""
    s = y["scores"]
    best = s.min()
    return not np.isfinite(best) or not np.any((s != best) & (s - best <= 1e-9 * best))


def model_of(res, i=0):
    return float(res.s[i]), np.asarray(res.R[i]).reshape(3, 3), np.asarray(res.t[i]).reshape(3)


def host_walk(b, hypotheses, seed, tau=TAU, with_scale=True, refine_rounds=2):
    """every set of the batch walked on the host (srk_align_host_set): an AlignResult over the batch"""
    out = [AL.host_set(*set_obs(b, i)[:2], q=set_obs(b, i)[2], hypotheses=hypotheses, inlier_distance=tau, seed=seed, with_scale=with_scale,
                       refine_rounds=refine_rounds) for i in range(b.n)]
    return AL.AlignResult(*[np.concatenate([getattr(r, k) for r in out]) for k in AL.AlignResult._fields])


@functools.lru_cache(maxsize=None)
def host_floor():
    """The largest distance between the host walk and the yardstick over the aligned sets of the ragged cases (the small batches at
    every hypothesis count and the 257-set batch), refined and not: what the quaternion-Jacobi route and the SVD route, and two
    orders of summation, differ by in double precision.  The GPU tests allow ten times this."""
    cases = [(small(holes), small_yardstick(holes, H), H) for holes in (False, True) for H in HYPOTHESES]
    cases.append((ragged(False), big_yardstick(False), BIG_HYPOTHESES))
    worst = 0.0
    for b, ys, H in cases:
        for rounds in (0, 2):
            got = host_walk(b, H, SAMPLER_SEED[H], refine_rounds=rounds)
            for i, y in (ys.items() if isinstance(ys, dict) else enumerate(ys)):
                y = y if rounds else y["stage"]
                if y["status"] == 0 and int(got.aligned[i, 3]) == y["aligned"][3]:
                    worst = max(worst, ref.distance(model_of(got, i), (y["s"], y["R"], y["t"]), set_obs(b, i)[1]))
    return worst


@functools.lru_cache(maxsize=None)
def accuracy_floor(with_scale, scale):
    """the host walk's largest distance from the truth on the noise-free cases at 64 hypotheses (a CPU run)"""
    b = accuracy(with_scale, scale)
    got = host_walk(b, 64, 1, tau=accuracy_tau(b), with_scale=with_scale)
    return max(ref.distance(model_of(got, i), f.truth, f.b) for i, f in enumerate(b.sets))


def agree(b, ys, got, inliers=None, tau=TAU, stage=False):
    """A result (the host walk's or the device's AlignResult over the batch b) against the yardstick's on the sets ys (a sequence
    over all sets, or a dict by set; stage: against the yardstick's hypothesis stage).  Status, n and the number of hypotheses with
    a model always; the winning h must be one of the yardstick's near-ties (a single one where the winner is clear); the score to
    1e-12 against the yardstick's at the result's own model; where the winner is the yardstick's: the rounds accepted, the inlier
    count and the flags.  Returns the largest distance to the yardstick's model over those sets."""
    worst = 0.0
    for i, y in (ys.items() if isinstance(ys, dict) else enumerate(ys)):
        y = y["stage"] if stage else y
        al = got.aligned[i]
        assert got.status[i] == y["status"], i
        assert al[1] == y["aligned"][1] and al[4] == y["aligned"][4], (i, al, y["aligned"])
        if y["status"]:
            assert got.s[i] == 1.0 and np.array_equal(got.R[i], np.eye(3)) and np.array_equal(got.t[i], np.zeros(3)), i
            assert np.isnan(al[[0, 3, 6, 7]]).all() and al[2] == 0 and al[5] == 0, (i, al)
            continue
        h, n = int(al[3]), al[1]
        assert h in near_ties(y), (i, al, y["aligned"])
        a, t, q = set_obs(b, i)
        score, own = al[0] ** 2 * n, ref.score_at(model_of(got, i), a, t, q, tau)
        assert abs(score - own) <= 1e-12 * score, (i, score, own)
        R = np.asarray(got.R[i]).reshape(3, 3)
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-9 and abs(np.linalg.det(R) - 1) <= 1e-9, i
        if h != y["aligned"][3]:
            continue
        worst = max(worst, ref.distance(model_of(got, i), (y["s"], y["R"], y["t"]), t))
        assert al[5] == y["aligned"][5] and al[2] == y["aligned"][2], (i, al, y["aligned"])
        assert abs(al[7] - y["aligned"][7]) <= 1e-6 * al[7] + 1e-9 or (np.isnan(al[7]) and np.isnan(y["aligned"][7])), (i, al, y["aligned"])
        if al[5] > 0:
            assert abs(al[6] - y["aligned"][6]) <= 1e-9, (i, al, y["aligned"])
        else:
            assert np.isnan(al[6]), (i, al)
        if inliers is not None:
            assert np.array_equal(inliers[b.row_ptr[i]:b.row_ptr[i + 1]].astype(bool), y["inliers"]), i
    return worst
