"""Seeded cases for two-view relative pose (tests/test_relate_cpu.py, tests/test_gpu_relate.py), their yardstick results computed
once per process (tests/relate_ref.py), and the stand-alone host program (tests/cpp/test_relate_host.cpp).  All shapes are small."""
import functools
import os
import shutil
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np

import relate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surikatoko_amd", "csrc")
F0 = 600.0
K0 = np.array([[1.25, 0.0, 0.53], [0.0, 1.3, 0.4], [0.0, 0.0, 1.0]])   # pixels = f0 (K x)_xy / (K x)_z: 750 and 780 pixels of focal length
K1 = np.array([[1.1, 0.01, 0.5], [0.0, 1.15, 0.42], [0.0, 0.0, 1.0]])
TAU = 2.0
OUTLIER_TAU = 4.0                              # one pixel of noise in both images: four standard deviations of the Sampson distance
LENGTHS = (6, 7, 8, 63, 64, 65, 129)           # weighted matches: at the sample size, the wave boundaries
HYPOTHESES = (1, 3, 4, 5, 64, 65, 256)         # one solve group, a solve wave -1, 0, +1, a score wave 0, +1, four score waves
BATCH_SIZES = (1, 3, 4, 5, 17)                 # four waves a workgroup: a partly empty workgroup, more than one
SAMPLE_SEED = 2400
RAGGED_SEED = {False: 2424, True: 2469}     # chosen so that the pair of eight matches has a clear winner at every count
OUTLIER_SEED = {0.3: 2430, 0.5: 2453}          # chosen so that the yardstick meets the figures of the outlier test


def rotation(w):
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    k = ref.skew(w / th)
    return np.eye(3) + np.sin(th) * k + (1.0 - np.cos(th)) * (k @ k)


def pixels(K, x, f0=F0):
    p = x @ K.T
    return f0 * p[:, :2] / p[:, 2:3]


def motion(rng, kind="general", lo=0.01, hi=0.6):
    """(R, T) of frame b, |T| = 1 (0 for a pure rotation)"""
    w = rng.normal(size=3)
    R = rotation(w / np.linalg.norm(w) * rng.uniform(lo, hi))
    if kind == "rotation":
        return R, np.zeros(3)
    T = np.array([0.05, -0.03, 1.0]) + 0.02 * rng.normal(size=3) if kind == "forward" else rng.normal(size=3)
    return R, T / np.linalg.norm(T)


def points(n, rng, planar=False):
    X = np.column_stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4.0, 8.0, n)])
    if planar:
        X[:, 2] = 6.0 + 0.2 * X[:, 0] - 0.1 * X[:, 1]
    return X


def pair(n, rng, planar=False, sigma=0.0, share=0.0, kind="general", Ka=K0, Kb=K1, hi=0.3):
    """n matches of one pair: the truth, the pixels with noise sigma, and a share of them replaced by uniform points"""
    R, T = motion(rng, kind, hi=hi)
    X = points(n, rng, planar)
    ua, ub = pixels(Ka, X), pixels(Kb, X @ R.T + T)
    ua, ub = ua + sigma * rng.normal(size=ua.shape), ub + sigma * rng.normal(size=ub.shape)
    moved = np.sort(rng.choice(n, int(round(share * n)), replace=False))
    ub[moved] = np.column_stack([rng.uniform(-100.0, 700.0, len(moved)), rng.uniform(-150.0, 600.0, len(moved))])
    return SimpleNamespace(uv_a=ua, uv_b=ub, R=R, T=T, X=X, Ka=Ka, Kb=Kb, moved=moved)


def batch(pairs, q=None):
    row_ptr = np.concatenate([[0], np.cumsum([len(p.uv_a) for p in pairs])]).astype(np.int64)
    cat = lambda key, shape: np.concatenate([getattr(p, key) for p in pairs]).reshape(shape) if pairs else np.zeros(shape)  # noqa: E731
    moved = np.concatenate([p.moved + o for p, o in zip(pairs, row_ptr)]) if pairs else np.zeros(0, int)
    return SimpleNamespace(n=len(pairs), f0=F0, row_ptr=row_ptr, uv_a=cat("uv_a", (-1, 2)), uv_b=cat("uv_b", (-1, 2)), q=q,
                           Ka=np.array([p.Ka for p in pairs]).reshape(-1, 3, 3), Kb=np.array([p.Kb for p in pairs]).reshape(-1, 3, 3),
                           R=np.array([p.R for p in pairs]).reshape(-1, 3, 3), T=np.array([p.T for p in pairs]).reshape(-1, 3), moved=moved)


def rows(b, idx):
    """the batch of the pairs idx of b, in that order"""
    idx = list(idx)
    obs = np.concatenate([np.arange(b.row_ptr[i], b.row_ptr[i + 1]) for i in idx]).astype(int) if idx else np.zeros(0, int)
    row_ptr = np.concatenate([[0], np.cumsum([b.row_ptr[i + 1] - b.row_ptr[i] for i in idx])]).astype(np.int64)
    return SimpleNamespace(n=len(idx), f0=b.f0, row_ptr=row_ptr, uv_a=b.uv_a[obs], uv_b=b.uv_b[obs], q=None if b.q is None else b.q[obs],
                           Ka=b.Ka[idx], Kb=b.Kb[idx], R=b.R[idx], T=b.T[idx], moved=np.zeros(0, int))


def without_holes(b):
    """the batch without its matches of q = 0, and the mask of the matches kept"""
    keep = b.q > 0
    counts = [int(keep[b.row_ptr[i]:b.row_ptr[i + 1]].sum()) for i in range(b.n)]
    out = SimpleNamespace(**vars(b))
    out.row_ptr, out.uv_a, out.uv_b, out.q = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), b.uv_a[keep], b.uv_b[keep], b.q[keep]
    return out, keep


# ------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def samples(count=300):
    """noise-free samples of six matches for the five-point solve alone: a third planar, rotations from 0.01 to 0.6 rad"""
    rng = np.random.default_rng(SAMPLE_SEED)
    ps = [pair(6, rng, planar=i % 3 == 0, hi=0.6, Kb=K0) for i in range(count)]
    return SimpleNamespace(uv_a=np.array([p.uv_a for p in ps]), uv_b=np.array([p.uv_b for p in ps]), E=np.array([ref.skew(p.T) @ p.R for p in ps]))


@functools.lru_cache(maxsize=None)
def ragged(holes=False):
    """one pair of each length in LENGTHS with half a pixel of noise; with holes, a fifth more matches carry q = 0 and the rest
    weights between 0.5 and 2"""
    rng = np.random.default_rng(RAGGED_SEED[holes])
    ps, qs = [], []
    for k, n in enumerate(LENGTHS):
        extra = (n + 4) // 5 if holes else 0
        ps.append(pair(n + extra, rng, planar=k % 3 == 1, sigma=0.5))
        w = rng.uniform(0.5, 2.0, n + extra)
        w[rng.choice(n + extra, extra, replace=False)] = 0.0
        qs.append(w)
    return batch(ps, np.concatenate(qs) if holes else None)


@functools.lru_cache(maxsize=None)
def accuracy():
    """noise-free pairs of 40 matches: general, planar, forward motion and, last, a pure rotation"""
    rng = np.random.default_rng(2420)
    return batch([pair(40, rng), pair(40, rng), pair(40, rng, planar=True), pair(40, rng, planar=True), pair(40, rng, kind="forward"),
                  pair(40, rng, kind="rotation")])


ACCURACY_KINDS = ("general", "general", "planar", "planar", "forward", "rotation")


@functools.lru_cache(maxsize=None)
def outliers(share):
    """two pairs of 200 matches with one pixel of noise, a share of them replaced by uniform points"""
    rng = np.random.default_rng(OUTLIER_SEED[share])
    return batch([pair(200, rng, sigma=1.0, share=share) for _ in range(2)])


def outlier_hypotheses(share):
    return max(1, ref.ransac_hypotheses(share, 0.999, 5))


def many(count, seed=2460):
    """`count` pairs of unequal length (6 .. 70 matches, one of them empty when count > 4) with half a pixel of noise"""
    rng = np.random.default_rng(seed)
    ps = [pair(int(rng.integers(6, 71)), rng, sigma=0.5) for _ in range(count)]
    if count > 4:
        ps[2] = pair(0, rng)
    return batch(ps)


# ------------------------------------------------------------------ the yardstick, once per process
def pair_obs(b, i):
    s = slice(int(b.row_ptr[i]), int(b.row_ptr[i + 1]))
    return b.uv_a[s], b.uv_b[s], None if b.q is None else b.q[s]


@functools.lru_cache(maxsize=None)
def _all_ragged(holes):
    b = ragged(holes)
    return [ref.score_all(b.f0, b.Ka[i], b.Kb[i], *pair_obs(b, i), max(HYPOTHESES), 1, TAU) for i in range(b.n)]


def ragged_yardstick(holes, hypotheses):
    """the yardstick's results of the ragged pairs at a hypothesis count: a prefix of the same hypotheses"""
    return [ref.pick(a, hypotheses) for a in _all_ragged(holes)]


@functools.lru_cache(maxsize=None)
def batch_yardstick(key, hypotheses, seed=1):
    b = {"accuracy": accuracy, "out3": lambda: outliers(0.3), "out5": lambda: outliers(0.5)}[key]() if isinstance(key, str) else many(*key)
    tau = OUTLIER_TAU if isinstance(key, str) and key.startswith("out") else TAU
    return [ref.relate(b.f0, b.Ka[i], b.Kb[i], *pair_obs(b, i), hypotheses, seed, tau) for i in range(b.n)]


def near_ties(y, rel=1e-6):
    """the hypotheses whose score is within rel of the best"""
    s = y["scores"]
    return set(np.flatnonzero(s <= s.min() * (1.0 + rel) + 1e-300).tolist())


def winner_is_clear(y, rel=1e-6):
    return len(near_ties(y, rel)) == 1


def pose_error(R, T, Rt, Tt):
    """(rotation angle, angle between the translation directions) to the truth"""
    return ref.rotation_angle(R, Rt), (ref.direction_angle(T, Tt) if np.linalg.norm(Tt) > 0 else 0.0)


# ------------------------------------------------------------------ the host program (tests/cpp/test_relate_host.cpp)
def cxx():
    return shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def build_host_program(out, extra=()):
    return subprocess.run([cxx(), "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "test_relate_host.cpp"),
                           os.path.join(CSRC, "srk_relate.cpp"), "-o", str(out)], capture_output=True, text=True)


@functools.lru_cache(maxsize=None)
def host_program():
    """the stand-alone program, built once per process into a temporary directory; None without a host compiler"""
    if cxx() is None:
        return None
    exe = os.path.join(tempfile.mkdtemp(prefix="relate_bin"), "test_relate_host")
    r = build_host_program(exe)
    assert r.returncode == 0, r.stderr
    return exe


def _run(program, mode, write):
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            write(f)
        r = subprocess.run([program or host_program(), mode, src, dst], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return np.fromfile(dst, np.uint8)


def _taker(raw):
    pos = 0

    def take(dtype, count):
        nonlocal pos
        size = np.dtype(dtype).itemsize * count
        out = raw[pos:pos + size].view(dtype).copy()
        pos += size
        return out
    return take


def host_solve(uv_a, uv_b, Ka=K0, Kb=K0, f0=F0, program=None):
    """the five-point solve of samples [n][6][2]: E [n][10][3][3] (the first roots[i] are set), rec [n][20], roots [n]"""
    n = len(uv_a)

    def write(f):
        np.array([n], np.int64).tofile(f)
        np.array([f0]).tofile(f)
        np.ascontiguousarray(Ka).tofile(f)
        np.ascontiguousarray(Kb).tofile(f)
        np.ascontiguousarray(uv_a, np.float64).tofile(f)
        np.ascontiguousarray(uv_b, np.float64).tofile(f)
    take = _taker(_run(program, "solve", write))
    return take(np.float64, 90 * n).reshape(n, 10, 3, 3), take(np.float64, 20 * n).reshape(n, 20), take(np.int32, n)


def host_poses(E, program=None):
    n = len(E)

    def write(f):
        np.array([n], np.int64).tofile(f)
        np.ascontiguousarray(E, np.float64).tofile(f)
    take = _taker(_run(program, "poses", write))
    return take(np.float64, 36 * n).reshape(n, 4, 3, 3), take(np.float64, 12 * n).reshape(n, 4, 3)


def host_walk(b, hypotheses, seed, tau=TAU, program=None):
    """every pair of the batch walked on the host: R, T, E, related, scores [n][hypotheses], status, inliers"""
    def write(f):
        np.array([b.n, b.row_ptr[-1], int(b.q is not None), hypotheses, seed], np.int64).tofile(f)
        np.array([b.f0, tau], np.float64).tofile(f)
        b.row_ptr.astype(np.int64).tofile(f)
        np.ascontiguousarray(b.uv_a, np.float64).tofile(f)
        np.ascontiguousarray(b.uv_b, np.float64).tofile(f)
        if b.q is not None:
            np.ascontiguousarray(b.q, np.float64).tofile(f)
        np.ascontiguousarray(b.Ka, np.float64).tofile(f)
        np.ascontiguousarray(b.Kb, np.float64).tofile(f)
    take, n = _taker(_run(program, "pairs", write)), b.n
    return SimpleNamespace(R=take(np.float64, 9 * n).reshape(n, 3, 3), T=take(np.float64, 3 * n).reshape(n, 3), E=take(np.float64, 9 * n).reshape(n, 3, 3),
                           related=take(np.float64, 8 * n).reshape(n, 8), scores=take(np.float64, hypotheses * n).reshape(n, hypotheses),
                           status=take(np.uint32, n), inliers=take(np.uint8, int(b.row_ptr[-1])))


# ------------------------------------------------------------------ a result against the yardstick's
def agree(b, ys, got, pose_bound):
    """The result `got` of the batch b (R, T, E, related, status, inliers) against the yardstick's results ys: the same status,
    number of weighted matches and winner (for a pair of fewer than eight matches, one of the yardstick's near-ties: six or seven
    matches draw permutations of nearly one sample), then at that winner the same inlier flags and counts, the score to 1e-9
    relative, the sixth-match error, and the pose within pose_bound of the yardstick's.  Returns the largest pose distance seen."""
    worst = 0.0
    for i, y in enumerate(ys):
        s = slice(int(b.row_ptr[i]), int(b.row_ptr[i + 1]))
        rel = got.related[i]
        assert got.status[i] == y["status"], (i, got.status[i], y["status"])
        assert rel[1] == y["related"][1], i
        if y["status"]:
            assert np.array_equal(got.R[i], np.eye(3)) and not got.T[i].any() and not got.E[i].any() and not got.inliers[s].any(), i
            assert np.isnan(rel[[0, 3, 5, 7]]).all() and rel[2] == 0 and rel[6] == 0, (i, rel)
            continue
        h = int(rel[3])
        if rel[1] >= 8:
            assert h == int(y["related"][3]), (i, h, y["related"][3])
        else:
            assert h in near_ties(y), (i, h, sorted(near_ties(y)))
        z = y if h == int(y["related"][3]) else y["at"](h)
        # the solve loses the roots of a sample whose ten roots cluster in z: it never finds a model where
        # the yardstick has none, and a tenth of the yardstick's count is the allowance for the lost ones
        assert 0.9 * z["related"][4] <= rel[4] <= z["related"][4], (i, rel[4], z["related"][4])
        assert np.array_equal(got.inliers[s], z["inliers"]), (i, np.flatnonzero(got.inliers[s] != z["inliers"]))
        assert rel[2] == z["related"][2] and rel[6] == z["related"][6], (i, rel, z["related"])
        score, want = rel[0] ** 2 * rel[1], z["related"][0] ** 2 * z["related"][1]
        assert abs(score - want) <= 1e-9 * want, (i, score, want)
        assert abs(rel[5] - z["related"][5]) <= 1e-6 * z["related"][5] + 1e-9, (i, rel[5], z["related"][5])
        assert abs(rel[7] - z["related"][7]) <= 1e-9 + pose_bound, (i, rel[7], z["related"][7])
        d = max(ref.rotation_angle(got.R[i], z["R"]), ref.direction_angle(got.T[i], z["T"]), ref.essential_distance(got.E[i], z["E"]))
        assert abs(np.linalg.norm(got.T[i]) - 1.0) <= 1e-12 and np.abs(got.E[i] - ref.skew(got.T[i]) @ got.R[i]).max() <= 1e-15, i
        assert d <= pose_bound, (i, d, pose_bound)
        worst = max(worst, d)
    return worst
