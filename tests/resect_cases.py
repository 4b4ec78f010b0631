"""The cases of batched camera resection, shared by tests/test_resect_cpu.py (the yardstick and the host
walk of a frame, no GPU) and tests/test_gpu_resect.py (the kernels).  Built once per process and never modified."""
import functools
from types import SimpleNamespace

import numpy as np

import resect_ref as ref

F0 = 600.0
K0 = np.diag([1 / F0, 1 / F0, 1.0]) @ np.array([[880.0, 0, 400], [0, 660, 300], [0, 0, 1]])
DEPTH = 6.0
LANES = 64   # SRK_RESECT_LANES
RAGGED_LENGTHS = (0, 2, 3, 4, LANES - 1, LANES, LANES + 1, 2 * LANES + 1, 300, 1000)   # weighted observations: the wave boundaries
BATCH_SIZES = (1, 3, 4, 5, 257)   # four frames a workgroup: the last workgroup partly empty, a wave past the end
ACCURACY_POINTS = (4, 6, 63, 64, 65, 129, 300)
# (attempts, rel_change) of the decision cases and of the two ragged batches (without / with q = 0 in between), chosen so that the
# yardstick's own decisions stay away from every threshold (tests/test_resect_cpu.py checks that): from these starts the fourth
# attempt already lowers E by a few 1e-16 of it only, and whether it is accepted is decided by rounding.  The defaults (10, 1e-9)
# would compare rounding, not code.
DECISION_PAIRS = ((1, 1e-3), (2, 0.3), (3, 2e-5), (3, 3e-6))
RAGGED_OPTIONS = {False: (4, 1e-4), True: (3, 5e-4)}
# ... and of the runs with a loss on the outlier case (delta 2 px).  The reweighted steps lower E by about a decade less each time,
# so with eight frames some stop test always falls within a factor 2 of any threshold: these runs end at their cap, where the
# poses have reached the accuracy the case is about (a numpy experiment: to four digits that of 30 attempts at 1e-9).
LOSS_DELTA = 2.0
LOSS_OPTIONS = {"huber": (4, 1e-7), "cauchy": (6, 1e-7)}


def rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    return ref.so3_exp(a / np.linalg.norm(a) * angle)


def landmarks(n, rng, planar=False):
    x, y = rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n)
    z = DEPTH + (0.3 * x - 0.2 * y if planar else rng.uniform(-2, 2, n))
    return np.column_stack([x, y, z])


def true_pose(rng):
    R = rot(rng.normal(size=3), rng.uniform(0.02, 0.2))
    C = rng.uniform(-0.3, 0.3, 3)
    return R, -R @ C


def off_pose(R, T, rng, angle, shift):
    """the pose turned by `angle` about a random axis and its centre moved by `shift` in a random direction"""
    t = rng.normal(size=3)
    return ref.move(R, T, np.concatenate([t / np.linalg.norm(t) * shift, rot(rng.normal(size=3), 1.0) @ np.array([angle, 0, 0])]))


def project(K, R, T, X):
    pqr = (X @ R.T + T) @ K.T
    return F0 * pqr[:, :2] / pqr[:, 2:3]


def frame(n, rng, planar=False, sigma=0.0, angle=np.radians(10), shift=0.5, K=K0):
    X = landmarks(n, rng, planar)
    R, T = true_pose(rng)
    uv = project(K, R, T, X) + sigma * rng.normal(size=(n, 2)) if n else np.zeros((0, 2))
    R0, T0 = off_pose(R, T, rng, angle, shift)
    return SimpleNamespace(X=X, uv=uv, K=K, R_true=R, T_true=T, R0=R0, T0=T0, q=None)


def batch(frames, seed=0):
    """frames -> the CSR arrays over one landmark array; the landmarks are stored in a shuffled order, so that the gather is one"""
    n = len(frames)
    row_ptr = np.zeros(n + 1, np.int64)
    row_ptr[1:] = np.cumsum([len(f.uv) for f in frames])
    N = int(row_ptr[-1])
    place = np.random.default_rng(seed).permutation(N).astype(np.int32)
    X = np.zeros((N, 3))
    uv = np.concatenate([f.uv for f in frames] + [np.zeros((0, 2))])
    if N:
        X[place] = np.concatenate([f.X for f in frames])
    has_q = any(f.q is not None for f in frames)
    q = np.concatenate([np.ones(len(f.uv)) if f.q is None else f.q for f in frames] + [np.zeros(0)]) if has_q else None
    return SimpleNamespace(f0=F0, n=n, row_ptr=row_ptr, point=place, uv=uv, q=q, X=X, K=np.stack([f.K for f in frames]),
                           R0=np.stack([f.R0 for f in frames]), T0=np.stack([f.T0 for f in frames]), frames=tuple(frames))


def rows(b, idx):
    """the frames idx of a batch, in that order, over the same landmark array"""
    idx = list(idx)
    obs = np.concatenate([np.arange(b.row_ptr[i], b.row_ptr[i + 1]) for i in idx] + [np.zeros(0, np.int64)]).astype(np.int64)
    rp = np.concatenate([[0], np.cumsum([b.row_ptr[i + 1] - b.row_ptr[i] for i in idx])]).astype(np.int64)
    return SimpleNamespace(f0=b.f0, n=len(idx), row_ptr=rp, point=b.point[obs], uv=b.uv[obs], q=None if b.q is None else b.q[obs], X=b.X,
                           K=b.K[idx], R0=b.R0[idx], T0=b.T0[idx], frames=tuple(b.frames[i] for i in idx))


def frame_obs(b, i):
    """(uv, X of its observations, q or None) of frame i"""
    o0, o1 = b.row_ptr[i], b.row_ptr[i + 1]
    return b.uv[o0:o1], b.X[b.point[o0:o1]], None if b.q is None else b.q[o0:o1]


def yardstick(b, i, **kw):
    uv, X, q = frame_obs(b, i)
    return ref.resect_frame(b.f0, uv, X, q, b.K[i], b.R0[i], b.T0[i], **kw)


@functools.lru_cache(maxsize=None)
def accuracy():
    """noise-free frames of 4 .. 300 points, volume and planar, the start off by 10 degrees and 0.5 units at depth 6"""
    rng = np.random.default_rng(22)
    return batch([frame(n, rng, planar) for planar in (False, True) for n in ACCURACY_POINTS], seed=1)


@functools.lru_cache(maxsize=None)
def ragged(holes=False):
    """257 frames whose weighted lengths cycle through RAGGED_LENGTHS, 1 px of noise, the start off by 3 degrees and 0.1 units, per-frame
    intrinsics.  With holes, every frame also carries observations with q = 0 (about one in five, wrong pixels) in between, so that
    the ranks among the weighted observations differ from the positions, and the weighted ones carry q in 0.5 .. 2."""
    rng = np.random.default_rng(2200 + int(holes))
    frames = []
    for i in range(BATCH_SIZES[-1]):
        L = RAGGED_LENGTHS[i % len(RAGGED_LENGTHS)]
        K = K0.copy()
        K[0, 0] *= rng.uniform(0.9, 1.1)
        f = frame(L, rng, planar=(i % 7 == 3), sigma=1.0, angle=np.radians(3), shift=0.1, K=K)
        if holes:
            extra = max(1, L // 5)
            n = L + extra
            off = np.sort(rng.choice(n, size=extra, replace=False))
            on = np.setdiff1d(np.arange(n), off)
            X, uv, q = np.zeros((n, 3)), np.zeros((n, 2)), np.zeros(n)
            X[on], uv[on], q[on] = f.X, f.uv, rng.uniform(0.5, 2.0, L)
            X[off], uv[off] = landmarks(extra, rng), rng.uniform(0, 800, (extra, 2))
            f.X, f.uv, f.q = X, uv, q
        frames.append(f)
    return batch(frames, seed=2)


@functools.lru_cache(maxsize=None)
def ragged_yardstick(holes=False):
    """the yardstick on every frame of ragged(holes) at RAGGED_OPTIONS[holes], computed once"""
    b = ragged(holes)
    attempts, rel_change = RAGGED_OPTIONS[holes]
    return tuple(yardstick(b, i, attempts=attempts, rel_change=rel_change) for i in range(b.n))


@functools.lru_cache(maxsize=None)
def outliers(n_frames=8):
    """200 points, 1 px of noise, 20 % of the observations moved by 20 .. 60 px, the start off by 3 degrees and 0.1 units"""
    rng = np.random.default_rng(2222)
    frames, moved = [], []
    for _ in range(n_frames):
        f = frame(200, rng, sigma=1.0, angle=np.radians(3), shift=0.1)
        idx = np.sort(rng.choice(200, size=40, replace=False))
        ang, mag = rng.uniform(0, 2 * np.pi, 40), rng.uniform(20, 60, 40)
        f.uv[idx] += np.column_stack([mag * np.cos(ang), mag * np.sin(ang)])
        frames.append(f)
        moved.append(idx)
    b = batch(frames, seed=3)
    b.moved = np.concatenate([b.row_ptr[i] + m for i, m in enumerate(moved)])
    return b


@functools.lru_cache(maxsize=None)
def decisions(n_frames=24):
    """frames of 20 .. 400 points with 1 px of noise, the start off by 2 .. 12 degrees and 0.05 .. 0.5 units: the loop's decisions"""
    rng = np.random.default_rng(2233)
    return batch([frame(int(rng.integers(20, 400)), rng, planar=bool(i % 5 == 0), sigma=1.0, angle=np.radians(rng.uniform(2, 12)),
                        shift=rng.uniform(0.05, 0.5)) for i in range(n_frames)], seed=4)


def margins_ok(log, rel_change):
    """no decision of a yardstick run at a threshold: every accept margin |E_cand - E_cur| above 1e-9 E, every stop test a factor 2
    away from rel_change E (an attempt whose factorisation failed has no E_cand: it is rejected whatever the rounding)"""
    for accepted, E_cur, E_cand in log:
        if np.isnan(E_cand):
            continue
        if not abs(E_cand - E_cur) > 1e-9 * E_cur:
            return False
        if accepted and rel_change > 0 and 0.5 * rel_change * E_cur <= E_cur - E_cand <= 2 * rel_change * E_cur:
            return False
    return True


def pose_delta(R, T, y):
    """d = [t; w] with (R, T) = the yardstick's result y moved by d: C = C_y + t, R^T = Exp(w) R_y^T (w from the skew part)"""
    D = R.T @ y["R"]
    w = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return np.concatenate([ref.centre(R, T) - ref.centre(y["R"], y["T"]), w])


def pose_units(R, T, y):
    """the distance of the pose (R, T) from the yardstick's result y in the Jacobi-scaled variables, in units of the Newton step
    |H_s^-1 g_s| that remains at the yardstick's result"""
    return float(np.linalg.norm(np.sqrt(np.diag(y["H"])) * pose_delta(R, T, y)) / ref.newton_step(y["H"], y["g"]))


def energy_tolerance(b, i, E, n):
    """The bound on a difference of two values of E: 1e-12 E, as long as the number format can deliver it.  A residual is a
    difference of pixel coordinates of size |uv|; the projection f0 p / r carries two roundings before the subtraction, so the
    residual is good to de = 2 eps max |uv| (3.6e-13 px at 800 px; times sqrt(q) with information), which moves E = sum q e^2 by
    2 sqrt(n E) de + n de^2.  That floor is the larger of the two only where E < n (2 de / 1e-12)^2 ~ 0.5 n px^2 (an rms residual
    below half a pixel): on the frames of three points, fitted exactly (E ~ 1e-20 at the end, ~ 1e-2 on the way).  On every frame
    with 1 px of noise E ~ 2 n, the floor is 5e-13 E and the bound is the plain 1e-12 E."""
    uv, _, q = frame_obs(b, i)
    de = 2 * ref.EPS * np.abs(uv).max() * (1.0 if q is None else np.sqrt(q.max()))
    return max(1e-12 * E, 2 * np.sqrt(n * E) * de + n * de * de)


def energy_floor(uv, E, n):
    """What the number format lets a loop see of E = sum of 2 n squares of residuals: each residual is a difference of pixel
    coordinates of size |uv|, good to a few eps |uv| (taken as 8), which moves E by 2 sqrt(n E) de + n de^2, and the sum itself
    carries up to 4 n eps E.  A loop that accepts an attempt iff E decreases cannot tell two poses apart whose E differ by less,
    so at rel_change 0 it comes to rest where the decrease a Newton step promises, g^T H^-1 g, is of this size."""
    de = 8 * ref.EPS * np.abs(uv).max()
    return 4 * n * ref.EPS * E + 2 * np.sqrt(n * E) * de + n * de * de


def newton_decrement(H, g):
    """g^T H^-1 g: the decrease of E that a full Newton step promises (in the Jacobi-scaled variables, the same number)"""
    d = 1.0 / np.sqrt(np.diag(H))
    return float((g * d) @ np.linalg.solve(ref.scaled(H), g * d))


def energy_at(b, i, R, T, kind=0, delta=None):
    """the yardstick's E of frame i at the pose (R, T)"""
    uv, X, q = frame_obs(b, i)
    return ref.terms(b.f0, uv, X, q, b.K[i], R, T, kind, delta)[0]


def pose_error(R, T, f):
    """(rotation angle to the truth in radians, centre error over the depth)"""
    return ref.angle_between(R, f.R_true), float(np.linalg.norm(ref.centre(R, T) - ref.centre(f.R_true, f.T_true)) / DEPTH)


def accuracy_units(R, T, f, H):
    """the larger of the two pose errors in units of eps sqrt(cond_2(H_s))"""
    return max(pose_error(R, T, f)) / (ref.EPS * np.sqrt(ref.cond2_scaled(H)))


@functools.lru_cache(maxsize=None)
def accuracy_yardstick():
    """the yardstick on the accuracy cases (40 attempts, rel_change 0) and its own maximum in that unit"""
    b = accuracy()
    ys = tuple(yardstick(b, i, attempts=40, rel_change=0.0) for i in range(b.n))
    return ys, max(accuracy_units(y["R"], y["T"], b.frames[i], y["H"]) for i, y in enumerate(ys))


@functools.lru_cache(maxsize=None)
def host_program():
    """tests/cpp/test_resect_host.cpp with csrc/srk_resect.cpp, built once per process into a temporary directory"""
    import os
    import shutil
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = os.path.join(tempfile.mkdtemp(prefix="resect_bin"), "test_resect_host")
    r = subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "test_resect_host.cpp"),
                        os.path.join(root, "surikatoko_amd", "csrc", "srk_resect.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def host_walk(b, attempts, rel_change):
    """every frame of the batch in the kernel's own order of operations on the host: R, T, quality, info, status, logs, w"""
    import os
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        write_host_input(src, b, attempts=attempts, rel_change=rel_change)
        r = subprocess.run([host_program(), "frames", src, dst], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return read_host_output(dst, b)


def host_walk_floor(cases=None):
    """The largest distance, in Newton-step units, between the yardstick and the kernel's order of operations walked on the host
    (host_walk), over the two ragged batches: computed on the CPU, the device is held to ten times this.  cases: other batches,
    as (batch, its yardstick results, attempts, rel_change) each."""
    if cases is None:
        cases = [(ragged(holes), ragged_yardstick(holes)) + RAGGED_OPTIONS[holes] for holes in (False, True)]
    worst = 0.0
    for b, ys, attempts, rel_change in cases:
        R, T = host_walk(b, attempts, rel_change)[:2]
        for i, y in (ys.items() if isinstance(ys, dict) else enumerate(ys)):
            if not y["status"] & ref.FEW_POINTS:
                worst = max(worst, pose_units(R[i], T[i], y))
    return worst


def write_host_input(path, b, attempts=10, rel_change=1e-9, kind=0, delta=0.0, want_weights=False):
    """the input file of tests/cpp/test_resect_host.cpp's `frames` mode"""
    with open(path, "wb") as f:
        np.array([b.n, b.row_ptr[-1], len(b.X), int(b.q is not None), attempts, kind, int(want_weights)], np.int64).tofile(f)
        np.array([b.f0, rel_change, delta], np.float64).tofile(f)
        b.row_ptr.astype(np.int64).tofile(f)
        b.point.astype(np.int32).tofile(f)
        np.ascontiguousarray(b.uv, np.float64).tofile(f)
        if b.q is not None:
            np.ascontiguousarray(b.q, np.float64).tofile(f)
        for a in (b.X, b.K, b.R0, b.T0):
            np.ascontiguousarray(a, np.float64).tofile(f)


def read_host_output(path, b, want_weights=False):
    """R, T, quality, info, status, the accept / reject log per frame, and w_out"""
    raw = np.fromfile(path, np.uint8)
    n, pos = b.n, 0

    def take(dtype, count):
        nonlocal pos
        size = np.dtype(dtype).itemsize * count
        out = raw[pos:pos + size].view(dtype).copy()
        pos += size
        return out
    R, T, quality, info = take(np.float64, 9 * n).reshape(n, 3, 3), take(np.float64, 3 * n).reshape(n, 3), take(np.float64, 6 * n).reshape(n, 6), \
        take(np.float64, 36 * n).reshape(n, 6, 6)
    status = take(np.uint32, n)
    counts = take(np.int32, n)
    flat = take(np.int32, int(counts.sum()))
    logs = np.split(flat, np.cumsum(counts)[:-1]) if n else []
    w = take(np.float64, int(b.row_ptr[-1])) if want_weights else None
    return R, T, quality, info, status, logs, w
