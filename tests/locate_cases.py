"""The cases of resection without a start pose, shared by tests/test_locate_cpu.py (the yardstick and the
host walk of a frame, no GPU) and tests/test_gpu_locate.py (the kernels).  Built once per process and never modified.  The
geometry (landmarks at depth 6, poses, intrinsics) is that of the resection's cases."""
import functools
import os
import shutil
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np

import locate_ref as ref
import resect_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surikatoko_amd", "csrc")
F0, K0, DEPTH = rc.F0, rc.K0, rc.DEPTH
TAU = 4.0
LENGTHS = (0, 3, 4, 5, 63, 64, 65, 129, 300)     # weighted observations: below and at the sample size, the wave boundaries
HYPOTHESES = (1, 63, 64, 65, 256)                # one lane, a wave short of one, a full wave, a wave and one lane, four waves
BATCH_SIZES = (1, 3, 5, 257)                     # four waves a workgroup: a partly empty workgroup, many workgroups
ACCURACY_POINTS = (4, 5, 63, 64, 65, 129, 300)
# the seed of the ragged batches (without / with q = 0 in between) and the sampler's seed per hypothesis count, chosen so that on
# every frame the yardstick's winner is clear and no observation sits at the inlier threshold (tests/test_locate_cpu.py asserts it)
RAGGED_SEED = {False: 2300, True: 2301}
SAMPLER_SEED = {1: 1, 63: 1, 64: 1, 65: 1, 256: 1}
BIG_HYPOTHESES = 65                              # the 257-frame batch runs at this count only (the yardstick is a Python loop)
OUTLIER_SEED = {0.3: 2330, 0.5: 2350}
OUTLIER_REFINE = dict(loss="cauchy", delta=2.0, attempts=20)


def move_share(uv, share, rng):
    """`share` of the observations moved by 20 .. 60 px in a random direction; returns their indices"""
    n = len(uv)
    k = int(round(share * n))
    idx = np.sort(rng.choice(n, size=k, replace=False)) if k else np.zeros(0, np.int64)
    ang, mag = rng.uniform(0, 2 * np.pi, k), rng.uniform(20, 60, k)
    uv[idx] += np.column_stack([mag * np.cos(ang), mag * np.sin(ang)])
    return idx


def frame(n, rng, planar=False, sigma=0.0, share=0.0, K=K0):
    f = rc.frame(n, rng, planar=planar, sigma=sigma, K=K)
    f.moved = move_share(f.uv, share, rng) if n else np.zeros(0, np.int64)
    return f


def batch(frames, seed=0):
    b = rc.batch(frames, seed)
    b.moved = np.concatenate([b.row_ptr[i] + f.moved for i, f in enumerate(frames)] + [np.zeros(0, np.int64)]).astype(np.int64)
    return b


def rows(b, idx):
    return rc.rows(b, idx)


def without_holes(b):
    """the batch with its q = 0 observations cut out"""
    keep = b.q > 0
    rp = np.concatenate([[0], np.cumsum([np.count_nonzero(keep[b.row_ptr[i]:b.row_ptr[i + 1]]) for i in range(b.n)])]).astype(np.int64)
    return SimpleNamespace(f0=b.f0, n=b.n, row_ptr=rp, point=b.point[keep], uv=b.uv[keep], q=b.q[keep], X=b.X, K=b.K, frames=b.frames), keep


@functools.lru_cache(maxsize=None)
def p3p_triples(count=2000):
    """noise-free random triples at depth 6: X [count][3][3], uv [count][3][2] and the true poses"""
    rng = np.random.default_rng(2323)
    X, uv, R, T = np.zeros((count, 3, 3)), np.zeros((count, 3, 2)), np.zeros((count, 3, 3)), np.zeros((count, 3))
    for i in range(count):
        X[i] = rc.landmarks(3, rng)
        R[i], T[i] = rc.true_pose(rng)
        uv[i] = rc.project(K0, R[i], T[i], X[i])
    return SimpleNamespace(X=X, uv=uv, R=R, T=T)


def p3p_error(R, T, Rt, Tt):
    """the issue's measure: largest entry of R - R_true plus |T - T_true| over the depth"""
    return float(np.abs(R - Rt).max() + np.linalg.norm(T - Tt) / DEPTH)


@functools.lru_cache(maxsize=None)
def accuracy():
    """noise-free frames of 4 .. 300 points, volume and planar"""
    rng = np.random.default_rng(23)
    return batch([frame(n, rng, planar) for planar in (False, True) for n in ACCURACY_POINTS], seed=1)


@functools.lru_cache(maxsize=None)
def ragged(holes=False):
    """257 frames whose weighted lengths cycle through LENGTHS, 1 px of noise, 30 % of the observations moved by 20 .. 60 px,
    per-frame intrinsics.  With holes, every frame also carries observations with q = 0 (about one in five, wrong pixels) in between
    and the weighted ones carry q in 0.5 .. 2."""
    rng = np.random.default_rng(RAGGED_SEED[holes])
    frames = []
    for i in range(BATCH_SIZES[-1]):
        L = LENGTHS[i % len(LENGTHS)]
        K = K0.copy()
        K[0, 0] *= rng.uniform(0.9, 1.1)
        f = frame(L, rng, planar=(i % 7 == 3 and L > 5), sigma=1.0, share=0.3, K=K)
        if holes:
            extra = max(1, L // 5)
            n = L + extra
            off = np.sort(rng.choice(n, size=extra, replace=False))
            on = np.setdiff1d(np.arange(n), off)
            X, uv, q = np.zeros((n, 3)), np.zeros((n, 2)), np.zeros(n)
            X[on], uv[on], q[on] = f.X, f.uv, rng.uniform(0.5, 2.0, L)
            X[off], uv[off] = rc.landmarks(extra, rng), rng.uniform(0, 800, (extra, 2))
            f.X, f.uv, f.q, f.moved = X, uv, q, on[f.moved]
        frames.append(f)
    return batch(frames, seed=2)


def small(holes=False):
    """the first len(LENGTHS) frames of the ragged batch, every length once: every hypothesis count runs on these"""
    return rows(ragged(holes), range(len(LENGTHS)))


BIG_CHECKED = tuple(range(0, BATCH_SIZES[-1], 8))   # the frames of the 257-frame batch the yardstick walks: every length (8 and 9 are coprime)


@functools.lru_cache(maxsize=None)
def outliers(share):
    """eight frames of 200 points, 1 px of noise, `share` of the observations moved by 20 .. 60 px"""
    rng = np.random.default_rng(OUTLIER_SEED[share])
    return batch([frame(200, rng, sigma=1.0, share=share) for _ in range(8)], seed=3)


def outlier_hypotheses(share):
    """30 %: the reference's count for p = 0.999 rounded up to a wave; 50 %: 256"""
    return 256 if share == 0.5 else -(-ref.ransac_hypotheses(share, 0.999) // 64) * 64


def frame_obs(b, i):
    return rc.frame_obs(b, i)


def yardstick(b, i, hypotheses, seed, tau=TAU):
    uv, X, q = frame_obs(b, i)
    return ref.locate_frame(b.f0, uv, X, q, b.K[i], hypotheses, tau, seed)


@functools.lru_cache(maxsize=None)
def small_yardstick(holes, hypotheses):
    b = small(holes)
    return tuple(yardstick(b, i, hypotheses, SAMPLER_SEED[hypotheses]) for i in range(b.n))


@functools.lru_cache(maxsize=None)
def big_yardstick(holes=False):
    """the yardstick on the frames BIG_CHECKED of the 257-frame batch, as a dict by frame"""
    b = ragged(holes)
    return {i: yardstick(b, i, BIG_HYPOTHESES, SAMPLER_SEED[BIG_HYPOTHESES]) for i in BIG_CHECKED}


@functools.lru_cache(maxsize=None)
def outlier_yardstick(share):
    """the yardstick on the outlier frames, and the bound of the GPU test: twice its own largest pose error over these frames"""
    b = outliers(share)
    ys = tuple(yardstick(b, i, outlier_hypotheses(share), 1) for i in range(b.n))
    err = [pose_error(y["R"], y["T"], b.frames[i]) for i, y in enumerate(ys)]
    return ys, (2.0 * max(e[0] for e in err), 2.0 * max(e[1] for e in err))


def pose_error(R, T, f):
    """(rotation angle to the truth in radians, centre error over the depth)"""
    return ref.pose_distance(R, T, f.R_true, f.T_true, DEPTH)


def winner_is_clear(y):
    """the yardstick's best score at least 1e-6 (relative) below every different score"""
    s = y["scores"]
    best = s.min()
    other = s[s != best]
    return not np.isfinite(best) or other.size == 0 or other.min() - best >= 1e-6 * best


def inliers_are_clear(b, i, y, tau=TAU):
    """no weighted observation with q s within 1e-6 (relative) of tau^2 at the yardstick's pose"""
    uv, X, q = frame_obs(b, i)
    q = np.ones(len(uv)) if q is None else q
    _, _, z = ref.score_terms(b.f0, b.K[i], y["R"], y["T"], X, uv, q, tau)
    return not np.any((q > 0) & (np.abs(z - tau * tau) <= 1e-6 * tau * tau))


def score_at(b, i, R, T, tau=TAU):
    """the yardstick's score of frame i at the pose (R, T)"""
    uv, X, q = frame_obs(b, i)
    q = np.ones(len(uv)) if q is None else q
    on = q > 0
    return float(ref.score_terms(b.f0, b.K[i], R, T, X[on], uv[on], q[on], tau)[0].sum())


# ------------------------------------------------------------------ the host walk (tests/cpp/test_locate_host.cpp)
def cxx():
    return shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def build_host_program(out, extra=()):
    return subprocess.run([cxx(), "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "test_locate_host.cpp"),
                           os.path.join(CSRC, "srk_locate.cpp"), "-o", str(out)], capture_output=True, text=True)


@functools.lru_cache(maxsize=None)
def host_program():
    """the stand-alone program, built once per process into a temporary directory; None without a host compiler"""
    if cxx() is None:
        return None
    exe = os.path.join(tempfile.mkdtemp(prefix="locate_bin"), "test_locate_host")
    r = build_host_program(exe)
    assert r.returncode == 0, r.stderr
    return exe


def host_walk(b, hypotheses, seed, tau=TAU, program=None):
    """every frame of the batch walked on the host: R, T, located, scores [n][hypotheses], status, inliers"""
    program = program or host_program()
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            np.array([b.n, b.row_ptr[-1], len(b.X), int(b.q is not None), hypotheses, seed], np.int64).tofile(f)
            np.array([b.f0, tau], np.float64).tofile(f)
            b.row_ptr.astype(np.int64).tofile(f)
            b.point.astype(np.int32).tofile(f)
            np.ascontiguousarray(b.uv, np.float64).tofile(f)
            if b.q is not None:
                np.ascontiguousarray(b.q, np.float64).tofile(f)
            np.ascontiguousarray(b.X, np.float64).tofile(f)
            np.ascontiguousarray(b.K, np.float64).tofile(f)
        r = subprocess.run([program, "frames", src, dst], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        raw = np.fromfile(dst, np.uint8)
    n, pos = b.n, 0

    def take(dtype, count):
        nonlocal pos
        size = np.dtype(dtype).itemsize * count
        out = raw[pos:pos + size].view(dtype).copy()
        pos += size
        return out
    return SimpleNamespace(R=take(np.float64, 9 * n).reshape(n, 3, 3), T=take(np.float64, 3 * n).reshape(n, 3),
                           located=take(np.float64, 6 * n).reshape(n, 6), scores=take(np.float64, hypotheses * n).reshape(n, hypotheses),
                           status=take(np.uint32, n), inliers=take(np.uint8, int(b.row_ptr[-1])))


def pose_gap(R, T, y):
    """the larger of the two pose distances (radians, centre over depth) between a pose and the yardstick's result y"""
    return max(ref.pose_distance(R, T, y["R"], y["T"], DEPTH))


@functools.lru_cache(maxsize=None)
def _own_host_floor():
    return host_floor(tuple((small(holes), small_yardstick(holes, H), H, SAMPLER_SEED[H]) for holes in (False, True) for H in HYPOTHESES))


def host_floor(cases=None):
    """The largest pose distance between the host walk and the yardstick over the located frames of the small ragged batches at
    every hypothesis count: what the two implementations of the same formulas differ by in double precision (the closed-form
    roots against the companion matrix's, the triangle's frame against the SVD).  The GPU tests allow ten times this.
    cases: other batches, as (batch, its yardstick results, hypotheses, seed) each."""
    if cases is None:
        return _own_host_floor()
    worst = 0.0
    for b, ys, H, seed in cases:
        got = host_walk(b, H, seed)
        worst = max([worst] + [pose_gap(got.R[i], got.T[i], y) for i, y in (ys.items() if isinstance(ys, dict) else enumerate(ys))
                               if y["status"] == 0])
    return worst


@functools.lru_cache(maxsize=None)
def _own_accuracy_floor():
    return accuracy_floor(accuracy())


def accuracy_floor(b=None):
    """the host walk's largest distance from the truth on the noise-free cases (or on the batch b) at 64 hypotheses (a CPU run)"""
    if b is None:
        return _own_accuracy_floor()
    got = host_walk(b, 64, 1)
    return max(max(pose_error(got.R[i], got.T[i], f)) for i, f in enumerate(b.frames))


def agree(b, ys, got, inliers=None):
    """A result (the host walk's or the device's: R, T, located, status, and inliers [O] when given) against the yardstick's on the
    frames ys (a sequence over all frames, or a dict by frame).  Status, n and the number of hypotheses with a pose always; the
    winning h where the yardstick's winner is clear (else the chosen h must be one of the yardstick's near-ties: frames of four
    and five points draw permutations of one triple, whose scores differ by rounding only); the inlier count and the flags where
    no observation sits at the threshold; the score to 1e-12 against the yardstick's at the result's own pose.  Returns the
    largest pose distance to the yardstick over the frames with the same winner."""
    worst = 0.0
    for i, y in (ys.items() if isinstance(ys, dict) else enumerate(ys)):
        loc = got.located[i]
        assert got.status[i] == y["status"], i
        assert loc[1] == y["located"][1] and loc[4] == y["located"][4], (i, loc, y["located"])
        if y["status"]:
            assert np.array_equal(got.R[i], np.eye(3)) and np.array_equal(got.T[i], np.zeros(3)), i
            assert np.isnan(loc[0]) and np.isnan(loc[3]) and np.isnan(loc[5]) and loc[2] == 0, (i, loc)
            continue
        h, n, best = int(loc[3]), loc[1], y["scores"].min()
        if winner_is_clear(y):
            assert h == y["located"][3], (i, loc, y["located"])
        else:
            assert y["scores"][h] - best <= 1e-6 * best, (i, loc, y["located"])
        score = loc[0] ** 2 * n
        assert abs(score - score_at(b, i, got.R[i], got.T[i])) <= 1e-12 * score, (i, score, score_at(b, i, got.R[i], got.T[i]))
        assert abs(loc[0] - np.sqrt(y["scores"][h] / n)) <= 1e-6 * loc[0], i
        if h != y["located"][3]:
            continue
        worst = max(worst, pose_gap(got.R[i], got.T[i], y))
        assert abs(loc[5] - y["located"][5]) <= 1e-6 * max(1.0, loc[5]), i
        if inliers_are_clear(b, i, y):
            assert loc[2] == y["located"][2], (i, loc, y["located"])
            if inliers is not None:
                assert np.array_equal(inliers[b.row_ptr[i]:b.row_ptr[i + 1]].astype(bool), y["inliers"]), i
    return worst
