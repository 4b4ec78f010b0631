"""Seeded cases for the two-view homography (tests/test_homography_cpu.py, tests/test_gpu_homography.py) and their yardstick results
computed once per process (tests/homography_ref.py).  The pairs are relate_cases' (F0, K0, K1, the plane z = 6 + 0.2 x - 0.1 y, the
pure rotation over general points).  All shapes are small."""
import functools
import json
import os
from types import SimpleNamespace

import numpy as np

import homography_ref as ref
import relate_cases as rc
from relate_cases import ROOT, CSRC, F0, K0, K1, batch, rows, without_holes, pair_obs  # noqa: F401

TAU = 3.0                                      # half a pixel of noise: s is about 0.5 chi^2_4, tau^2 = 9 cuts where tau = 6 does at one pixel
OUTLIER_TAU = 6.0
LENGTHS = (4, 5, 8, 63, 64, 65, 129)           # weighted matches: at the sample size, at the wave boundaries
HYPOTHESES = (1, 63, 64, 65, 256)              # a wave -1, 0, +1, four waves
BATCH_SIZES = (1, 3, 4, 5, 17)                 # four waves a workgroup: a partly empty workgroup, more than one
ROUNDS = (0, 4)
RAGGED_SEED = {False: 2700, True: 2701}
# the sampler's seed per (holes, hypotheses), chosen so that every pair of at least eight matches has a clear winner and no pair
# sits at a threshold (test_homography_cpu.py asserts both)
SAMPLER_SEED = {(False, 1): 3, (False, 63): 17, (False, 64): 17, (False, 65): 17, (False, 256): 14,
                (True, 1): 3, (True, 63): 239, (True, 64): 239, (True, 65): 270, (True, 256): 29}
OUTLIER_SEED = {0.3: 2731, 0.5: 2753}          # chosen so that the yardstick meets the figures of the outlier test
OUTLIER_ROUNDS = 8
MANY_SEED = 2760
EXACT_FIT = ref.EXACT_FIT
PLANE_N = np.array([-0.2, 0.1, 1.0]) / np.linalg.norm([-0.2, 0.1, 1.0])
PLANE_D = 6.0 / np.linalg.norm([-0.2, 0.1, 1.0])


def true_homography(p):
    """the pixel homography of a planar pair (or of a pure rotation), norm 1 with (G p)_3 > 0"""
    H = p.R + np.outer(p.T, PLANE_N) / PLANE_D
    G = p.Kb @ H @ np.linalg.inv(p.Ka)
    return G / np.linalg.norm(G) * np.sign(G[2, 2])


def hpair(n, rng, kind, sigma=0.0, share=0.0, Ka=K0, Kb=K1):
    """a pair a homography explains: "planar" (the plane under a general motion) or "rotation" (general points, no baseline)"""
    return rc.pair(n, rng, planar=kind == "planar", sigma=sigma, share=share, kind="rotation" if kind == "rotation" else "general", Ka=Ka, Kb=Kb)


@functools.lru_cache(maxsize=None)
def ragged(holes=False):
    """one pair of each length in LENGTHS with half a pixel of noise, planar and rotation-only in turn; with holes, a fifth more
    matches carry q = 0 and the rest weights between 0.5 and 2"""
    rng = np.random.default_rng(RAGGED_SEED[holes])
    ps, qs = [], []
    for k, n in enumerate(LENGTHS):
        extra = (n + 4) // 5 if holes else 0
        ps.append(hpair(n + extra, rng, "planar" if k % 2 == 0 else "rotation", sigma=0.5))
        w = rng.uniform(0.5, 2.0, n + extra)
        w[rng.choice(n + extra, extra, replace=False)] = 0.0
        qs.append(w)
    return batch(ps, np.concatenate(qs) if holes else None)


@functools.lru_cache(maxsize=None)
def planar_pairs():
    """noise-free planar pairs of 40 matches, K_a != K_b"""
    rng = np.random.default_rng(2720)
    ps = [hpair(40, rng, "planar") for _ in range(3)]
    return batch(ps), ps


@functools.lru_cache(maxsize=None)
def rotation_pairs():
    """noise-free pure rotations over non-planar points"""
    rng = np.random.default_rng(2721)
    ps = [hpair(40, rng, "rotation") for _ in range(3)]
    return batch(ps), ps


@functools.lru_cache(maxsize=None)
def outliers(share):
    """two planar pairs of 200 matches with one pixel of noise, a share of the targets replaced by uniform points"""
    rng = np.random.default_rng(OUTLIER_SEED[share])
    ps = [hpair(200, rng, "planar", sigma=1.0, share=share) for _ in range(2)]
    return batch(ps), ps


def outlier_hypotheses(share):
    return ref.ransac_hypotheses(share, 0.999, 4)


@functools.lru_cache(maxsize=None)
def many(count, seed=MANY_SEED):
    """`count` pairs of unequal length (8 .. 70 matches, one of them empty when count > 4) with half a pixel of noise"""
    rng = np.random.default_rng(seed)
    ps = [hpair(int(rng.integers(8, 71)), rng, "planar" if k % 2 == 0 else "rotation", sigma=0.5) for k in range(count)]
    if count > 4:
        ps[2] = hpair(0, rng, "planar")
    return batch(ps)


def status_cases():
    """an empty pair, three matches, four collinear matches (in image a), and a good pair of eight"""
    rng = np.random.default_rng(2770)
    ps = [hpair(0, rng, "planar"), hpair(3, rng, "planar"), hpair(4, rng, "planar"), hpair(8, rng, "planar")]
    ps[2].uv_a = np.array([[100.0, 100.0], [200.0, 150.0], [300.0, 200.0], [400.0, 250.0]])
    return batch(ps)


# ------------------------------------------------------------------ the yardstick, once per process
@functools.lru_cache(maxsize=None)
def _scored(key, hypotheses, seed, tau):
    b = key() if callable(key) else key
    return [ref.score_all(b.f0, b.Ka[i], b.Kb[i], *pair_obs(b, i), hypotheses, seed, tau) for i in range(b.n)]


def _ragged_f():
    return ragged(False)


def _ragged_t():
    return ragged(True)


def ragged_yardstick(holes, hypotheses, rounds):
    scored = _scored(_ragged_t if holes else _ragged_f, hypotheses, SAMPLER_SEED[(holes, hypotheses)], TAU)
    return [ref.pick(a, hypotheses, rounds) for a in scored]


def yardstick(b, hypotheses, seed, tau, rounds):
    return [ref.relate_homography(b.f0, b.Ka[i], b.Kb[i], *pair_obs(b, i), hypotheses, seed, tau, rounds) for i in range(b.n)]


@functools.lru_cache(maxsize=None)
def outlier_yardstick(share):
    return yardstick(outliers(share)[0], outlier_hypotheses(share), 1, OUTLIER_TAU, OUTLIER_ROUNDS)


@functools.lru_cache(maxsize=None)
def many_yardstick(count, hypotheses=64, rounds=4):
    return yardstick(many(count), hypotheses, 1, TAU, rounds)


def near_ties(y, rel=1e-6):
    """the hypotheses whose score is within rel of the best, or, where the best fits exactly (four matches), below the score of residuals
    of 1e-6 px, the bound G itself is held to"""
    s = y["scores"]
    return set(np.flatnonzero(s <= s.min() * (1.0 + rel) + EXACT_FIT * y["homog"][1]).tolist())


def winner_is_clear(y, rel=1e-6):
    return len(near_ties(y, rel)) == 1


def at_a_threshold(A, y):
    """why the pair sits at a threshold, or None: a sample's determinant within 10x of the collinearity bound, a q s within 1e-6
    relative of tau^2 at a model whose inliers are taken, the gap within 10x of its bound, or a round decided neither clearly nor
    by rounding (homography_ref.TIE, CLEAR)"""
    if y["status"]:
        return None
    if A["collinear_margin"] < 1.0:
        return "a sample's triple within 10x of the collinearity bound"
    if y["edge"] < 1e-6:
        return "a match at the inlier threshold"
    if 0.1 * ref.GAP < y["gap"] < 10.0 * ref.GAP:
        return "the gap at its bound"
    if any(ref.TIE < abs(m) < ref.CLEAR for m in y["trail"]):
        return "a round between a tie and a clear decision"
    return None


# ------------------------------------------------------------------ the host walk (srk_homography_host_pair through the library)
def host_walk(b, hypotheses, seed, tau=TAU, rounds=4):
    """every pair of the batch walked on the host, as a HomographyResult of the batch"""
    from surikatoko_amd import homography as HG
    outs = []
    for i in range(b.n):
        ua, ub, q = pair_obs(b, i)
        outs.append(HG.host_pair(b.f0, ua, ub, b.Ka[i], b.Kb[i], q=q, hypotheses=hypotheses, inlier_pixels=tau, seed=seed, refine_rounds=rounds))
    cat = lambda k: np.concatenate([o[k] for o in outs]) if outs else np.zeros(0)  # noqa: E731
    return HG.HomographyResult(*[cat(k) for k in range(10)])


# ------------------------------------------------------------------ a result against the yardstick's
def agree(b, ys, got, score_bound, pixel_bound, figures=None):
    """The result `got` of the batch b against the yardstick's results ys: the same status, number of weighted matches and winner
    (for a pair of fewer than eight matches, one of the yardstick's near-ties: four to seven matches draw orderings of a few
    samples again and again), a number of rounds the yardstick allows (a round whose score ties with the one it has to beat to
    rounding may go either way), then at that winner and round count the same inlier flags and counts, the score within score_bound
    relative, G within pixel_bound at the corners of a 640 x 480 frame, H, the poses and the RMS figures.  Returns the largest
    (score distance, corner distance) seen."""
    worst = [0.0, 0.0]
    for i, y in enumerate(ys):
        s = slice(int(b.row_ptr[i]), int(b.row_ptr[i + 1]))
        hg = got.homog[i]
        assert got.status[i] == y["status"], (i, got.status[i], y["status"])
        assert hg[1] == y["homog"][1], i
        if y["status"]:
            assert np.array_equal(got.G[i], np.eye(3)) and np.array_equal(got.H[i], np.eye(3)) and got.n_poses[i] == 0, i
            assert not got.R[i].any() and not got.T[i].any() and not got.N[i].any() and not got.front[i].any() and not got.inliers[s].any(), i
            assert np.isnan(hg[[0, 3, 6, 7]]).all() and hg[2] == 0 and hg[5] == 0 and hg[4] == y["homog"][4], (i, hg)
            continue
        h, r = int(hg[3]), int(hg[5])
        if hg[1] >= 8:
            assert h == int(y["homog"][3]), (i, h, y["homog"][3])
            allowed = y["allowed"]
        else:
            assert h in near_ties(y), (i, h, sorted(near_ties(y)))
            allowed = y["walk"](h)[2]
        assert r in allowed, (i, r, allowed, y["trail"])
        z = y if (h == int(y["homog"][3]) and r == int(y["homog"][5])) else y["at"](h, r)
        assert hg[4] == z["homog"][4], (i, hg[4], z["homog"][4])
        assert np.array_equal(got.inliers[s], z["inliers"]), (i, np.flatnonzero(got.inliers[s] != z["inliers"]))
        assert hg[2] == z["homog"][2], (i, hg, z["homog"])
        score, want = hg[0] ** 2 * hg[1], z["homog"][0] ** 2 * z["homog"][1]
        # relative to the score, or for a model that fits exactly (four matches) to the score of residuals of 1e-6 px, the bound G
        # itself is held to: below it a score is rounding
        ds = abs(score - want) / max(want, EXACT_FIT * hg[1])
        dg = ref.corner_distance(got.G[i], z["G"], b.f0)
        if figures is not None:
            figures.append((ds, dg))
        assert ds <= score_bound, (i, score, want, ds)
        assert dg <= pixel_bound, (i, dg)
        assert abs(np.linalg.norm(got.G[i]) - 1.0) <= 1e-14, i
        assert abs(hg[7] - z["homog"][7]) <= 1e-6 * z["homog"][7] + 1e-9, (i, hg[7], z["homog"][7])
        # the decomposition: H to the same bound as G (relative), the gap, and every pose one of the yardstick's
        assert np.abs(got.H[i] - z["H"]).max() <= 1e-6, (i, np.abs(got.H[i] - z["H"]).max())
        assert abs(hg[6] - z["gap"]) <= 1e-6, (i, hg[6], z["gap"])
        assert got.n_poses[i] == z["n_poses"], (i, got.n_poses[i], z["n_poses"])
        check_poses(got, i)
        for k in range(got.n_poses[i]):
            # with exactly half of the inliers in front, (T, N) and (-T, -N) both meet the rule: the sign is the eigenvectors'
            signs = (1.0, -1.0) if 2 * got.front[i, k] == hg[2] else (1.0,)
            d = min(max(np.abs(got.R[i, k] - R).max(), np.abs(got.T[i, k] - sg * T).max(), np.abs(got.N[i, k] - sg * N).max())
                    for R, T, N, _ in z["poses"] for sg in signs)
            assert d <= 1e-5, (i, k, d)   # the poses amplify H's distance by 1 / gap at most ten on these pairs
        worst = [max(worst[0], ds), max(worst[1], dg)]
    return worst


def check_poses(got, i):
    """the properties of pair i's decomposition: H = R + (T/d) N^T, every R a proper rotation, |N| = 1, unused entries zero"""
    for k in range(2):
        R, T, N = got.R[i, k], got.T[i, k], got.N[i, k]
        if k >= got.n_poses[i]:
            assert not R.any() and not T.any() and not N.any() and got.front[i, k] == 0, (i, k)
            continue
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-13 and abs(np.linalg.det(R) - 1.0) <= 1e-13, (i, k)
        if got.n_poses[i] == 2:
            assert abs(np.linalg.norm(N) - 1.0) <= 1e-12, (i, k)
            assert np.abs(got.H[i] - (R + np.outer(T, N))).max() <= 1e-9, (i, k, np.abs(got.H[i] - (R + np.outer(T, N))).max())
        else:
            assert not T.any() and not N.any(), (i, k)
    if got.n_poses[i] == 2:
        assert got.front[i, 0] >= got.front[i, 1], i



# ------------------------------------------------------------------ the measured figures (profiles/homography/test_figures.json)
FIGURES = os.path.join(ROOT, "profiles", "homography", "test_figures.json")


def committed_figures():
    with open(FIGURES) as f:
        return json.load(f)


def bounds():
    """the bounds of a result against the yardstick: ten times the largest distance the host walk showed over the committed cases
    (profiles/homography/test_figures.json), the factor for the device's different contraction of the same statements, and never
    looser than 1e-6 relative / 1e-6 px"""
    fig = committed_figures()["host_walk_against_yardstick"]
    return min(10.0 * fig["score_relative"], 1e-6), min(10.0 * fig["corner_pixels"], 1e-6)


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


def outlier_conditions(b, ps, res):
    """at least 95 % of the unmoved matches flagged, at most 2 % of the moved, the corners within 3 px of the true homography"""
    out = []
    for i, p in enumerate(ps):
        flags = res["inliers"][i].astype(bool)
        moved = np.zeros(200, bool)
        moved[p.moved] = True
        out.append((flags[~moved].mean(), flags[moved].mean(), ref.corner_distance(res["G"][i], true_homography(p), F0)))
        assert out[-1][0] >= 0.95 and out[-1][1] <= 0.02 and out[-1][2] <= 3.0, (i, out[-1])
    return out
