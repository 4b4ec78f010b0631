"""The cases of batched triangulation, shared by tests/test_triangulate_cpu.py (the host walk of a track and
the host function, no GPU) and tests/test_gpu_triangulate.py (the kernels).  Built once per process and never modified."""
import functools
from types import SimpleNamespace

import numpy as np

import triangulate_ref as ref

F0 = 600.0
GROUP = 8   # lanes that share a track (SRK_TRI_GROUP)
K0 = np.diag([1 / F0, 1 / F0, 1.0]) @ np.array([[880.0, 0, 400], [0, 660, 300], [0, 0, 1]])
VIEWS = (2, 3, 8, 32)
RATIOS = (1e-1, 1e-3, 1e-5)   # baseline / depth
RAGGED_LENGTHS = (0, 1, 2, 3, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP + 1, 33, 100)
RAGGED_SIZES = (1, 255, 257, 4099)   # the last three leave the last workgroup (32 tracks) partly empty


def rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def rig(n, baseline, rng, wobble=0.02):
    """n cameras spread over `baseline` along x (a little in y), looking down +z with a small random rotation: inverse poses"""
    R, T = np.empty((n, 3, 3)), np.empty((n, 3))
    for j in range(n):
        c = np.array([baseline * (j / max(n - 1, 1) - 0.5), 0.2 * baseline * rng.uniform(-1, 1), 0.05 * baseline * rng.uniform(-1, 1)])
        R[j] = rot(rng.normal(size=3), wobble * rng.uniform(0.2, 1))
        T[j] = -R[j] @ c
    return R, T


def pixels(R, T, K, frame, X):
    P = ref.proj_mats(R[frame], T[frame], K[frame] if K.ndim == 3 else K)
    return ref.project(F0, P, X)[0]


def batch(tracks, R, T, K, X_true=None):
    """tracks: list of (frame array, uv array) -> CSR arrays"""
    row_ptr = np.zeros(len(tracks) + 1, np.int64)
    row_ptr[1:] = np.cumsum([len(f) for f, _ in tracks])
    frame = np.concatenate([np.asarray(f, np.int32) for f, _ in tracks] + [np.zeros(0, np.int32)])
    uv = np.concatenate([np.asarray(m, np.float64).reshape(-1, 2) for _, m in tracks] + [np.zeros((0, 2))])
    return SimpleNamespace(f0=F0, R=R, T=T, K=K, row_ptr=row_ptr, frame=frame, uv=uv, X_true=X_true, n=len(tracks))


def track(b, i):
    o0, o1 = b.row_ptr[i], b.row_ptr[i + 1]
    return b.frame[o0:o1], b.uv[o0:o1]


@functools.lru_cache(maxsize=None)
def conditioning(n_views, ratio, n_tracks=200):
    """noise-free tracks of n_views at baseline / depth = ratio: the sliding window's new landmarks at low parallax"""
    rng = np.random.default_rng(1000 * n_views + int(round(-np.log10(ratio))))
    depth = 5.0
    R, T = rig(n_views, ratio * depth, rng)
    K = np.broadcast_to(K0, (n_views, 3, 3)).copy()
    X = np.column_stack([rng.uniform(-0.5, 0.5, n_tracks), rng.uniform(-0.5, 0.5, n_tracks), rng.uniform(0.8, 1.2, n_tracks) * depth])
    fr = np.arange(n_views)
    return batch([(fr, pixels(R, T, K, fr, x)) for x in X], R, T, K, X)


@functools.lru_cache(maxsize=None)
def ragged(n_tracks):
    """noise-free tracks whose lengths cycle through RAGGED_LENGTHS, over 100 frames on a wide rig"""
    rng = np.random.default_rng(77)
    M = 100
    R, T = rig(M, 3.0, rng, wobble=0.05)
    K = np.broadcast_to(K0, (M, 3, 3)).copy()
    K[:, 0, 0] *= rng.uniform(0.9, 1.1, M)   # per-frame intrinsics
    tracks, X = [], []
    for i in range(n_tracks):
        L = RAGGED_LENGTHS[i % len(RAGGED_LENGTHS)]
        x = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(4, 8)])
        fr = np.sort(rng.choice(M, size=L, replace=False)) if L else np.zeros(0, np.int64)
        tracks.append((fr, pixels(R, T, K, fr, x) if L else np.zeros((0, 2))))
        X.append(x)
    return batch(tracks, R, T, K, np.array(X))


@functools.lru_cache(maxsize=None)
def noisy(n_tracks=200, sigma=1.0):
    """tracks of 3 to 32 views with sigma pixels of noise, for the refinement"""
    rng = np.random.default_rng(2024)
    M = 40
    R, T = rig(M, 2.5, rng, wobble=0.05)
    K = np.broadcast_to(K0, (M, 3, 3)).copy()
    tracks, X = [], []
    for i in range(n_tracks):
        L = 3 + i % 30
        x = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(4, 8)])
        fr = np.sort(rng.choice(M, size=L, replace=False))
        tracks.append((fr, pixels(R, T, K, fr, x) + sigma * rng.normal(size=(L, 2))))
        X.append(x)
    return batch(tracks, R, T, K, np.array(X))


def system(b, i, q=None):
    """A, rhs of track i by the yardstick (weighted observations only)"""
    fr, uv = track(b, i)
    w = np.ones(len(fr)) if q is None else np.asarray(q, dtype=np.float64)
    keep = w > 0
    P = ref.proj_mats(b.R[fr[keep]], b.T[fr[keep]], b.K[fr[keep]])
    return ref.system_from_P(b.f0, uv[keep], P, w[keep])


def cond_bound(b, i, X, factor=8.0):
    """factor eps cond_2(A) |X|: the accuracy a backward-stable factorisation of the linear system delivers on consistent data"""
    A, _ = system(b, i)
    return factor * ref.EPS * ref.cond2(A) * np.linalg.norm(X)


def ls_bound(b, i, X, factor=8.0):
    """The same for data with noise: the perturbation bound of a least-squares solution under relative perturbations eps of A
    and b (Higham, Accuracy and Stability of Numerical Algorithms, theorem 20.1, first order):
    eps (cond + cond^2 |r| / (|A| |X|)) |X| with r the residual."""
    A, rhs = system(b, i)
    k = ref.cond2(A)
    r = np.linalg.norm(rhs - A @ X)
    return factor * ref.EPS * (k + k * k * r / (np.linalg.norm(A, 2) * np.linalg.norm(X))) * np.linalg.norm(X)


def host_P(b, i):
    fr, _ = track(b, i)
    return ref.proj_mats(b.R[fr], b.T[fr], b.K[fr]).reshape(-1, 12)


def write_host_input(path, b, q=None, refine_attempts=0, refine_rel_change=0.0, min_parallax_deg=0.0):
    """the input file of `test_tri_host tracks`"""
    with open(path, "wb") as f:
        np.array([b.n, len(b.frame), len(b.R), int(q is not None), 0, refine_attempts], np.int64).tofile(f)
        np.array([b.f0, refine_rel_change, min_parallax_deg], np.float64).tofile(f)
        b.row_ptr.astype(np.int64).tofile(f)
        b.frame.astype(np.int32).tofile(f)
        np.ascontiguousarray(b.uv, np.float64).tofile(f)
        if q is not None:
            np.ascontiguousarray(q, np.float64).tofile(f)
        for a in (b.R, b.T, b.K):
            np.ascontiguousarray(a, np.float64).tofile(f)


def read_host_output(path, n):
    raw = np.fromfile(path, np.uint8)
    X = raw[:24 * n].view(np.float64).reshape(n, 3)
    ql = raw[24 * n:56 * n].view(np.float64).reshape(n, 4)
    st = raw[56 * n:60 * n].view(np.uint32)
    return X, ql, st
