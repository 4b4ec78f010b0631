"""Seeded cases for the two-view fundamental matrix (tests/test_fundamental_cpu.py, tests/test_gpu_fundamental.py) and their yardstick
results computed once per process (tests/fundamental_ref.py).  The pairs are relate_cases' (F0, K0, K1, general points, the plane
z = 6 + 0.2 x - 0.1 y, the pure rotation).  All shapes are small."""
import functools
import json
import os

import numpy as np

import fundamental_ref as ref
import relate_cases as rc
from relate_cases import ROOT, CSRC, F0, K0, K1, batch, rows, without_holes, pair_obs  # noqa: F401

TAU = 2.0
LENGTHS = (7, 8, 9, 63, 64, 65, 127, 128, 129, 200)   # weighted matches: below and at the sample size, at the wave boundaries
HYPOTHESES = (1, 63, 64, 65, 256)                     # a wave -1, 0, +1, four waves
ROUNDS = (0, 1, 8)
BATCH_SIZES = (1, 5, 17)                              # four waves a workgroup: a partly empty workgroup, more than one
RAGGED_SEED = {False: 2800, True: 2801}
SAMPLER_SEED = 3
OUTLIER_SEED = {0.3: 2831, 0.5: 2853}
OUTLIER_HYPOTHESES = {0.3: 256, 0.5: 1024}            # ransac_hypotheses(share, 0.999, 7) asks for 81 and 881
OUTLIER_ROUNDS = 8
MANY_SEED = 2860
WRONG_K_SEED = 2884                                   # of 2870 .. 2889 the host walks showed the effect on 16: this one clearly (139 against 160)
EXACT_FIT = ref.EXACT_FIT
BAND = 1e-9                                           # px^2 around tau^2 within which an inlier flag is rounding's


def true_fundamental(p):
    return ref.true_fundamental(p.R, p.T, p.Ka, p.Kb)


@functools.lru_cache(maxsize=None)
def ragged(holes=False):
    """one general pair of each length in LENGTHS with half a pixel of noise; with holes, a fifth more matches carry q = 0 and the
    rest weights between 0.5 and 2"""
    rng = np.random.default_rng(RAGGED_SEED[holes])
    ps, qs = [], []
    for n in LENGTHS:
        extra = (n + 4) // 5 if holes else 0
        ps.append(rc.pair(n + extra, rng, sigma=0.5))
        w = rng.uniform(0.5, 2.0, n + extra)
        w[rng.choice(n + extra, extra, replace=False)] = 0.0
        qs.append(w)
    return batch(ps, np.concatenate(qs) if holes else None)


@functools.lru_cache(maxsize=None)
def samples(count=400):
    """noise-free samples of eight matches from general scenes (seven and the eighth that chooses), K_a != K_b, with the truth"""
    rng = np.random.default_rng(2810)
    ps = [rc.pair(8, rng, hi=0.6) for _ in range(count)]
    return ps


@functools.lru_cache(maxsize=None)
def general_pairs():
    """noise-free general pairs of 40 matches, K_a != K_b"""
    rng = np.random.default_rng(2820)
    ps = [rc.pair(40, rng) for _ in range(3)]
    return batch(ps), ps


@functools.lru_cache(maxsize=None)
def degenerate_pairs():
    """noise-free pairs of 40 matches a homography explains: two planes, two pure rotations"""
    rng = np.random.default_rng(2821)
    ps = [rc.pair(40, rng, planar=True), rc.pair(40, rng, kind="rotation"), rc.pair(40, rng, planar=True), rc.pair(40, rng, kind="rotation")]
    return batch(ps), ps


@functools.lru_cache(maxsize=None)
def essential_pair():
    """a pair whose F is an essential matrix: K the identity in f0 units on both sides, half a pixel of noise; sigma = 1"""
    rng = np.random.default_rng(2822)
    p = rc.pair(120, rng, sigma=0.5, Ka=np.eye(3), Kb=np.eye(3))
    return batch([p]), p


@functools.lru_cache(maxsize=None)
def outliers(share):
    """two general pairs of 200 matches with half a pixel of noise, a share of the targets replaced by uniform points"""
    rng = np.random.default_rng(OUTLIER_SEED[share])
    ps = [rc.pair(200, rng, sigma=0.5, share=share) for _ in range(2)]
    return batch(ps), ps


@functools.lru_cache(maxsize=None)
def many(count, seed=MANY_SEED):
    """`count` general pairs of unequal length (8 .. 70 matches) with half a pixel of noise; the second has seven matches when
    count > 1 (FEW_POINTS) and the third none when count > 4"""
    rng = np.random.default_rng(seed)
    ps = [rc.pair(int(rng.integers(8, 71)), rng, sigma=0.5) for k in range(count)]
    if count > 1:
        ps[1] = rc.pair(7, rng, sigma=0.5)
    if count > 4:
        ps[2] = rc.pair(0, rng)
    return batch(ps)


@functools.lru_cache(maxsize=None)
def wrong_k():
    """one general pair of 200 matches with half a pixel of noise and a fifth of the targets replaced, and the intrinsics a user
    would guess: both focal lengths off by 20 %"""
    rng = np.random.default_rng(WRONG_K_SEED)
    p = rc.pair(200, rng, sigma=0.5, share=0.2)
    scale = np.diag([1.2, 1.2, 1.0])
    return batch([p]), p, scale @ p.Ka, scale @ p.Kb


# ------------------------------------------------------------------ the yardstick, once per process
@functools.lru_cache(maxsize=None)
def _scored_ragged(holes):
    b = ragged(holes)
    return [ref.score_all(b.f0, *pair_obs(b, i), max(HYPOTHESES), SAMPLER_SEED, TAU) for i in range(b.n)]


@functools.lru_cache(maxsize=None)
def ragged_yardstick(holes, hypotheses, rounds):
    return [ref.pick(a, hypotheses, rounds) for a in _scored_ragged(holes)]


def yardstick(b, hypotheses, seed, tau, rounds):
    return [ref.relate_uncalibrated(b.f0, *pair_obs(b, i), hypotheses, seed, tau, rounds) for i in range(b.n)]


@functools.lru_cache(maxsize=None)
def outlier_yardstick(share):
    return yardstick(outliers(share)[0], OUTLIER_HYPOTHESES[share], 1, TAU, OUTLIER_ROUNDS)


@functools.lru_cache(maxsize=None)
def many_yardstick(count, hypotheses=64, rounds=8):
    return yardstick(many(count), hypotheses, 1, TAU, rounds)


def near_ties(y, rel=1e-6):
    """the hypotheses whose score is within rel of the best, or, where the best fits exactly, below the score of residuals of 1e-6 px"""
    s = y["scores"]
    return set(np.flatnonzero(s <= s.min() * (1.0 + rel) + EXACT_FIT * y["fund"][1]).tolist())


# ------------------------------------------------------------------ the host walk (srk_fundamental_host_pair through the library)
def host_walk(b, hypotheses, seed, tau=TAU, rounds=8):
    """every pair of the batch walked on the host, as a FundamentalResult of the batch"""
    from surikatoko_amd import fundamental as FD
    outs = []
    for i in range(b.n):
        ua, ub, q = pair_obs(b, i)
        outs.append(FD.host_pair(b.f0, ua, ub, q=q, hypotheses=hypotheses, inlier_pixels=tau, seed=seed, refine_rounds=rounds))
    cat = lambda k: np.concatenate([o[k] for o in outs]) if outs else np.zeros(0)  # noqa: E731
    return FD.FundamentalResult(*[cat(k) for k in range(8)])


def check_model(got, i):
    """the properties of pair i's model: norm 1, the sign, rank 2 by construction, proper U and V, 0 <= sigma <= 1, the epipoles"""
    F, U, V, sg = got.F[i], got.U[i], got.V[i], got.sigma[i]
    assert abs(np.linalg.norm(F) - 1.0) <= 1e-14, i
    flat = F.reshape(-1)
    assert flat[int(np.argmax(np.abs(flat)))] > 0, i
    for M in (U, V):
        assert np.abs(M @ M.T - np.eye(3)).max() <= 1e-13 and abs(np.linalg.det(M) - 1.0) <= 1e-13, i
    assert 0.0 <= sg <= 1.0 and sg == got.fund[i, 9], i
    assert np.abs(ref.build(U, V, sg) - F).max() <= 1e-15, i
    assert np.abs(F @ V[:, 2]).max() <= 1e-15 and np.abs(F.T @ U[:, 2]).max() <= 1e-15, i


def agree(b, ys, got, score_bound, f_bound, figures=None):
    """The result `got` of the batch b against the yardstick's results ys: the same status, number of weighted matches, models and
    winner (one of the yardstick's near-ties), then the inlier flags outside a band of BAND px^2 around tau^2, the score within
    score_bound relative (for a model that fits exactly, relative to the score of residuals of 1e-6 px), F within f_bound entry by
    entry, the properties of the model, the RMS figures, the eighth-match error and the number of roots, and the information and
    its condition number against central differences at the returned representation.  Returns the largest (score, F) distances."""
    worst = [0.0, 0.0]
    for i, y in enumerate(ys):
        s = slice(int(b.row_ptr[i]), int(b.row_ptr[i + 1]))
        fd = got.fund[i]
        assert got.status[i] == y["status"], (i, got.status[i], y["status"])
        assert fd[1] == y["fund"][1], i
        assert fd[4] == y["fund"][4], (i, fd[4], y["fund"][4])
        if y["status"]:
            assert not got.F[i].any() and np.array_equal(got.U[i], np.eye(3)) and np.array_equal(got.V[i], np.eye(3)) and got.sigma[i] == 0, i
            assert not got.info[i].any() and not got.inliers[s].any(), i
            assert np.isnan(fd[[0, 3, 5, 8, 10]]).all() and not fd[[2, 6, 7, 9, 11]].any(), (i, fd)
            continue
        assert int(fd[3]) in near_ties(y), (i, fd[3], sorted(near_ties(y)))
        if int(fd[3]) != int(y["fund"][3]):           # a tie to rounding among orderings of the same sample: only the smallest pairs have one
            assert fd[1] <= 9, (i, fd[3], y["fund"][3])
            y = y["at"](int(fd[3]))
        check_model(got, i)
        ua, ub, q = pair_obs(b, i)
        keep = np.ones(len(ua), bool) if q is None else q > 0
        w = np.ones(int(keep.sum())) if q is None else q[keep]
        tau = TAU
        qs = w * ref.sampson(y["F"], ua[keep], ub[keep], b.f0)
        clear = np.abs(qs - tau * tau) > BAND
        assert np.array_equal(got.inliers[s][keep][clear], y["inliers"][keep][clear]), (i, np.flatnonzero(got.inliers[s] != y["inliers"]))
        assert not got.inliers[s][~keep].any(), i
        if clear.all():
            assert fd[2] == y["fund"][2], (i, fd, y["fund"])
        score, want = fd[0] ** 2 * fd[1], y["fund"][0] ** 2 * y["fund"][1]
        ds = abs(score - want) / max(want, EXACT_FIT * fd[1])
        df = float(np.abs(got.F[i] - y["F"]).max())
        if figures is not None:
            figures.append((ds, df))
        assert ds <= score_bound, (i, score, want, ds, y["trail"])
        assert df <= f_bound, (i, df, y["trail"])
        assert abs(fd[8] - y["fund"][8]) <= 1e-6 * y["fund"][8] + 1e-9, (i, fd[8], y["fund"][8])
        assert abs(fd[5] - y["fund"][5]) <= 1e-6 * y["fund"][5] + 1e-9, (i, fd[5], y["fund"][5])
        assert fd[11] == y["fund"][11] and fd[6] <= fd[7] <= 16, (i, fd, y["fund"])
        inl = got.inliers[s][keep].astype(bool)
        if inl.any():
            H, _ = ref.normal_equations(got.U[i], got.V[i], got.sigma[i], ua[keep][inl], ub[keep][inl], w[inl], b.f0)
            assert np.abs(got.info[i] - H).max() <= 1e-6 * np.abs(H).max(), (i, np.abs(got.info[i] - H).max(), np.abs(H).max())
            assert np.array_equal(got.info[i], got.info[i].T), i
            c = ref.cond1(got.info[i])
            assert (np.isnan(c) and np.isnan(fd[10])) or abs(fd[10] - c) <= 1e-6 * c, (i, fd[10], c)
        worst = [max(worst[0], ds), max(worst[1], df)]
    return worst


# ------------------------------------------------------------------ the measured figures (profiles/fundamental/test_figures.json)
FIGURES = os.path.join(ROOT, "profiles", "fundamental", "test_figures.json")


def committed_figures():
    with open(FIGURES) as f:
        return json.load(f)


def bounds():
    """the bounds of a result against the yardstick: ten times the largest distance the host walk showed over the committed cases
    (profiles/fundamental/test_figures.json), the factor for the device's different contraction of the same statements, and never
    looser than 1e-6 relative in the score and 1e-6 in an entry of F (the rule of the homography's tests)"""
    fig = committed_figures()["host_walk_against_yardstick"]
    return min(10.0 * fig["score_relative"], 1e-6), min(10.0 * fig["f_entry"], 1e-6)


def write_figures(key, values):
    """with SRK_WRITE_FIGURES set (to 1, or to the path of the copy to write), the measured figures of a test go into the file: how
    the committed ones were written"""
    where = os.environ.get("SRK_WRITE_FIGURES")
    if not where:
        return
    data = committed_figures() if os.path.exists(FIGURES) else {}
    data[key] = values
    path = where if where.endswith(".json") else FIGURES
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
