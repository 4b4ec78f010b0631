"""Cases in which every item of a front-end batch carries its own intrinsics (DESIGN.md sections 21 to 24), shared by
tests/test_frontend_k_cpu.py (the gate: the guards of the existing cases hold on these, and a neighbour's K violates every bound)
and tests/test_gpu_frontend_k.py (the kernels).  Built once per process and never modified.

The host walks and the yardsticks take one K per item, so the `K + 9 * i` reads and the `shared_k ? K : K + 9 * i` selections exist
in the kernels and their launch code alone.  The existing ragged cases vary K(0,0) only, and every pair of tests/relate_cases.py
carries the same two matrices: a kernel that took another item's fy, principal point or skew would pass on them.  Here fx, fy, u0,
v0 and the skew of every item (frame, pair side) are independent seeded draws, the pixels are projected with the item's own K, and
a third of the items of one batch per front end store the same camera as K f0 (K(2,2) = f0 instead of 1)."""
import functools
from types import SimpleNamespace

import numpy as np

import locate_cases as lc
import relate_cases as rl
import relate_ref as rlref
import resect_cases as rc
import triangulate_cases as tc
import triangulate_ref as tref

SPREAD = 0.15      # fx, fy times 1 +- SPREAD; u0, v0 shifted by up to +- SPREAD fx
SKEW = 0.02        # K(0,1) up to +- SKEW fx
BIG = 257          # items of the large batches: 255, 256 straddle the 256-thread block edge of the pack kernels
ALONE = (0, 3, 4, 5, 255, 256)   # ... and 3, 4, 5 the four-waves-a-workgroup edge of the others
CHECKED = tuple(range(0, BIG, 8))
RESECT_LENGTHS = rc.RAGGED_LENGTHS[:-1]         # 0 .. 300
RELATE_HYPOTHESES = (1, 3, 5, 65)               # the small counts put groups of different pairs into one solve wave
LOCATE_HYPOTHESES = lc.BIG_HYPOTHESES
# chosen on the CPU so that the guards of tests/test_frontend_k_cpu.py hold (clear winners, nothing at a threshold)
RESECT_SEED = {False: 2502, True: 2503}
LOCATE_SEED = {False: 2600, True: 2601}
RELATE_SEED = {False: 2702, True: 2705}
RELATE_MANY_SEED = 2760


def own_K(rng, base):
    """`base` (K(2,2) = 1) with fx, fy, u0, v0 and the skew drawn independently"""
    K = np.array(base, dtype=np.float64)
    fx = K[0, 0]
    d = rng.uniform(-1.0, 1.0, 5)
    K[0, 0] = fx * (1.0 + SPREAD * d[0])
    K[1, 1] *= 1.0 + SPREAD * d[1]
    K[0, 2] += SPREAD * fx * d[2]
    K[1, 2] += SPREAD * fx * d[3]
    K[0, 1] = SKEW * fx * d[4]
    return K


def k22_items(n, which=0):
    """the items stored as K f0 in the mixed-form batches; the second array of a batch (K_b) takes other items than the first, so
    that a kernel which scaled one side by the other's K(2,2) is seen"""
    return np.arange(n) % 3 == 1 + which


def with_K(b, **arrays):
    """the batch with other intrinsics arrays (K, or Ka and Kb)"""
    return SimpleNamespace(**{**vars(b), **arrays})


def mixed_form(b, keys=("K",)):
    """the same cameras, a third of them stored with K(2,2) = f0"""
    out = {}
    for which, k in enumerate(keys):
        K = getattr(b, k).copy()
        K[k22_items(len(K), which)] *= b.f0
        out[k] = K
    return with_K(b, **out)


def rolled(K):
    """every item with its successor's intrinsics"""
    return np.roll(K, -1, axis=0)


# ------------------------------------------------------------------ triangulation: the items are the frames
def _tri(M, frame_lists, seed, K=None):
    rng = np.random.default_rng(seed)
    R, T = tc.rig(M, 3.0, rng, wobble=0.05)
    K = np.stack([own_K(rng, tc.K0) for _ in range(M)]) if K is None else np.broadcast_to(K, (M, 3, 3)).copy()
    tracks, X = [], []
    for fr in frame_lists:
        fr = np.asarray(fr(rng) if callable(fr) else fr, np.int64)
        x = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(4, 8)])
        tracks.append((fr, tc.pixels(R, T, K, fr, x) if len(fr) else np.zeros((0, 2))))
        X.append(x)
    return tc.batch(tracks, R, T, K, np.array(X))


def _draw(M, L):
    return lambda rng: np.sort(rng.choice(M, size=L, replace=False))


@functools.lru_cache(maxsize=None)
def tri_big():
    """257 frames with their own K; one noise-free track of each length of RAGGED_LENGTHS, and a last one over the frames ALONE"""
    return _tri(BIG, [_draw(BIG, L) for L in tc.RAGGED_LENGTHS] + [ALONE], 2100)


@functools.lru_cache(maxsize=None)
def tri_holes():
    """information for tri_big: about one observation in five switched off, the others 0.5 .. 2"""
    b = tri_big()
    rng = np.random.default_rng(2101)
    q = rng.uniform(0.5, 2.0, len(b.frame))
    q[rng.uniform(size=len(q)) < 0.2] = 0.0
    return q


def tri_alone(b, i):
    """track i over its own frames only, renumbered 0 .. : the same cameras in a call of their own"""
    fr, uv = tc.track(b, i)
    return tc.batch([(np.arange(len(fr)), uv)], b.R[fr], b.T[fr], b.K[fr], b.X_true[i:i + 1])


@functools.lru_cache(maxsize=None)
def tri_truth():
    """64 frames, 24 noise-free tracks of 40 .. 63 views"""
    return _tri(64, [_draw(64, 40 + i) for i in range(24)], 2110)


@functools.lru_cache(maxsize=None)
def tri_shared():
    """tri_big's shapes with one K for all frames"""
    return _tri(BIG, [_draw(BIG, L) for L in tc.RAGGED_LENGTHS] + [ALONE], 2120, K=own_K(np.random.default_rng(2121), tc.K0))


def tri_yardstick(b, q=None):
    return [tref.triangulate_track(b.f0, *tc.track(b, i), b.R, b.T, b.K, q=None if q is None else q[b.row_ptr[i]:b.row_ptr[i + 1]])
            for i in range(b.n)]


def tri_bound(b, i, X, q=None):
    """8 eps cond_2(A) |X| of the (weighted) system of track i"""
    A, _ = tc.system(b, i, None if q is None else q[b.row_ptr[i]:b.row_ptr[i + 1]])
    return 8.0 * tref.EPS * tref.cond2(A) * np.linalg.norm(X)


# ------------------------------------------------------------------ resection and location: the items are the frames
def _holes(f, L, rng, landmarks):
    extra = max(1, L // 5)
    n = L + extra
    off = np.sort(rng.choice(n, size=extra, replace=False))
    on = np.setdiff1d(np.arange(n), off)
    X, uv, q = np.zeros((n, 3)), np.zeros((n, 2)), np.zeros(n)
    X[on], uv[on], q[on] = f.X, f.uv, rng.uniform(0.5, 2.0, L)
    X[off], uv[off] = landmarks(extra, rng), rng.uniform(0, 800, (extra, 2))
    f.X, f.uv, f.q = X, uv, q
    return on


@functools.lru_cache(maxsize=None)
def resect_big(holes=False):
    """resect_cases.ragged with every frame's K drawn in full, the lengths 0 .. 300"""
    rng = np.random.default_rng(RESECT_SEED[holes])
    frames = []
    for i in range(BIG):
        L = RESECT_LENGTHS[i % len(RESECT_LENGTHS)]
        f = rc.frame(L, rng, planar=(i % 7 == 3), sigma=1.0, angle=np.radians(3), shift=0.1, K=own_K(rng, rc.K0))
        if holes:
            _holes(f, L, rng, rc.landmarks)
        frames.append(f)
    return rc.batch(frames, seed=2)


def resect_small(holes=False):
    return rc.rows(resect_big(holes), range(len(RESECT_LENGTHS)))


@functools.lru_cache(maxsize=None)
def resect_yardstick(holes=False, which="small"):
    """the yardstick at RAGGED_OPTIONS[holes] on the small batch (a tuple) or on the frames CHECKED of the big one (a dict)"""
    attempts, rel_change = rc.RAGGED_OPTIONS[holes]
    if which == "small":
        b = resect_small(holes)
        return tuple(rc.yardstick(b, i, attempts=attempts, rel_change=rel_change) for i in range(b.n))
    b = resect_big(holes)
    return {i: rc.yardstick(b, i, attempts=attempts, rel_change=rel_change) for i in CHECKED}


@functools.lru_cache(maxsize=None)
def resect_truth():
    """twelve noise-free frames of 40 .. 62 points, every third planar, the start 10 degrees and 0.5 units off"""
    rng = np.random.default_rng(2510)
    return rc.batch([rc.frame(40 + 2 * i, rng, planar=(i % 3 == 2), K=own_K(rng, rc.K0)) for i in range(12)], seed=1)


@functools.lru_cache(maxsize=None)
def resect_truth_yardstick():
    """as resect_cases.accuracy_yardstick: 40 attempts at rel_change 0, and the yardstick's own maximum in eps sqrt(cond_2(H_s))"""
    b = resect_truth()
    ys = tuple(rc.yardstick(b, i, attempts=40, rel_change=0.0) for i in range(b.n))
    return ys, max(rc.accuracy_units(y["R"], y["T"], b.frames[i], y["H"]) for i, y in enumerate(ys))


@functools.lru_cache(maxsize=None)
def resect_shared():
    rng = np.random.default_rng(2520)
    K = own_K(rng, rc.K0)
    return rc.batch([rc.frame(L, rng, sigma=1.0, angle=np.radians(3), shift=0.1, K=K) for L in RESECT_LENGTHS], seed=5)


@functools.lru_cache(maxsize=None)
def locate_big(holes=False):
    """locate_cases.ragged with every frame's K drawn in full"""
    rng = np.random.default_rng(LOCATE_SEED[holes])
    frames = []
    for i in range(BIG):
        L = lc.LENGTHS[i % len(lc.LENGTHS)]
        f = lc.frame(L, rng, planar=(i % 7 == 3 and L > 5), sigma=1.0, share=0.3, K=own_K(rng, lc.K0))
        if holes:
            f.moved = _holes(f, L, rng, rc.landmarks)[f.moved]
        frames.append(f)
    return lc.batch(frames, seed=2)


def locate_small(holes=False):
    return lc.rows(locate_big(holes), range(len(lc.LENGTHS)))


@functools.lru_cache(maxsize=None)
def locate_yardstick(holes=False, which="small"):
    if which == "small":
        b = locate_small(holes)
        return tuple(lc.yardstick(b, i, LOCATE_HYPOTHESES, 1) for i in range(b.n))
    b = locate_big(holes)
    return {i: lc.yardstick(b, i, LOCATE_HYPOTHESES, 1) for i in CHECKED}


@functools.lru_cache(maxsize=None)
def locate_truth():
    """twelve noise-free frames of 40 .. 62 points, every third planar"""
    rng = np.random.default_rng(2610)
    return lc.batch([lc.frame(40 + 2 * i, rng, planar=(i % 3 == 2), K=own_K(rng, lc.K0)) for i in range(12)], seed=1)


@functools.lru_cache(maxsize=None)
def locate_truth_floor():
    """locate_cases.accuracy_floor on locate_truth: the host walk's largest distance from the truth at 64 hypotheses"""
    return lc.accuracy_floor(locate_truth())


@functools.lru_cache(maxsize=None)
def locate_host_floor():
    """locate_cases.host_floor on the batches here: the small ones with and without holes, and the frames CHECKED of the big one"""
    return lc.host_floor([(locate_small(holes), locate_yardstick(holes), LOCATE_HYPOTHESES, 1) for holes in (False, True)]
                         + [(locate_big(False), locate_yardstick(False, "big"), LOCATE_HYPOTHESES, 1)])


@functools.lru_cache(maxsize=None)
def locate_shared():
    rng = np.random.default_rng(2620)
    K = own_K(rng, lc.K0)
    return lc.batch([lc.frame(L, rng, sigma=1.0, share=0.3, K=K) for L in lc.LENGTHS], seed=5)


# ------------------------------------------------------------------ relative pose: the items are the pairs, two K each
def _pair(n, rng, **kw):
    return rl.pair(n, rng, Ka=own_K(rng, rl.K0), Kb=own_K(rng, rl.K1), **kw)


@functools.lru_cache(maxsize=None)
def relate_ragged(holes=False):
    """relate_cases.ragged with K_a and K_b of every pair drawn independently"""
    rng = np.random.default_rng(RELATE_SEED[holes])
    ps, qs = [], []
    for k, n in enumerate(rl.LENGTHS):
        extra = (n + 4) // 5 if holes else 0
        ps.append(_pair(n + extra, rng, planar=k % 3 == 1, sigma=0.5))
        w = rng.uniform(0.5, 2.0, n + extra)
        w[rng.choice(n + extra, extra, replace=False)] = 0.0
        qs.append(w)
    return rl.batch(ps, np.concatenate(qs) if holes else None)


@functools.lru_cache(maxsize=None)
def _relate_ragged_all(holes):
    b = relate_ragged(holes)
    return [rlref.score_all(b.f0, b.Ka[i], b.Kb[i], *rl.pair_obs(b, i), max(RELATE_HYPOTHESES), 1, rl.TAU) for i in range(b.n)]


def relate_ragged_yardstick(holes, hypotheses):
    return [rlref.pick(a, hypotheses) for a in _relate_ragged_all(holes)]


@functools.lru_cache(maxsize=None)
def relate_many():
    """17 pairs of 8 .. 70 matches (pair 2 empty) with half a pixel of noise"""
    rng = np.random.default_rng(RELATE_MANY_SEED)
    ps = [_pair(int(rng.integers(8, 71)), rng, sigma=0.5) for _ in range(17)]
    ps[2] = _pair(0, rng)
    return rl.batch(ps)


@functools.lru_cache(maxsize=None)
def relate_many_yardstick():
    b = relate_many()
    return [rlref.relate(b.f0, b.Ka[i], b.Kb[i], *rl.pair_obs(b, i), 65, 1, rl.TAU) for i in range(b.n)]


# No planar pair here: noise-free points on a plane seen from two calibrated cameras fit two essential matrices exactly (the
# twin pose of the plane's homography; here with every point in front of both cameras, 0.8 rad from the truth), so both score
# ~1e-24 and rounding picks one.  A yardstick run shows it on such a pair: hypotheses 60, 40, 20, ... carry the twin among equal
# scores.  The planar pairs of the ragged batches carry noise, which breaks the tie by a clear margin (the CPU gate checks it).
RELATE_TRUTH_KINDS = ("general", "general", "general", "general", "forward", "forward")


@functools.lru_cache(maxsize=None)
def relate_truth():
    """six noise-free pairs of 40 .. 60 matches: general and forward motion"""
    rng = np.random.default_rng(2710)
    return rl.batch([_pair(40 + 4 * i, rng, kind=kind) for i, kind in enumerate(RELATE_TRUTH_KINDS)])


@functools.lru_cache(maxsize=None)
def relate_truth_yardstick():
    b = relate_truth()
    return [rlref.relate(b.f0, b.Ka[i], b.Kb[i], *rl.pair_obs(b, i), 64, 1, rl.TAU) for i in range(b.n)]


@functools.lru_cache(maxsize=None)
def relate_shared():
    """seven pairs that all carry one K_a and one K_b (K_a != K_b)"""
    rng = np.random.default_rng(2720)
    Ka, Kb = own_K(rng, rl.K0), own_K(rng, rl.K1)
    return rl.batch([rl.pair(n, rng, sigma=0.5, Ka=Ka, Kb=Kb) for n in rl.LENGTHS])


def relate_pose_gap(R, T, y):
    return max(rlref.rotation_angle(R, y["R"]), rlref.direction_angle(T, y["T"]))


# ------------------------------------------------------------------ the host walks (triangulation's is built here; the others' by their cases)
@functools.lru_cache(maxsize=None)
def _workdir():
    import tempfile
    return tempfile.mkdtemp(prefix="frontend_k")


@functools.lru_cache(maxsize=None)
def _program(name):
    """tests/cpp/test_<name>_host.cpp with csrc/srk_<name>.cpp, built once per process"""
    import os
    import subprocess
    exe = os.path.join(_workdir(), f"test_{name}_host")
    r = subprocess.run([lc.cxx(), "-std=c++17", "-O1", os.path.join(lc.ROOT, "tests", "cpp", f"test_{name}_host.cpp"),
                        os.path.join(lc.CSRC, f"srk_{name}.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _walk(name, mode, write, read):
    import os
    import subprocess
    src, dst = os.path.join(_workdir(), f"{name}_in.bin"), os.path.join(_workdir(), f"{name}_out.bin")
    write(src)
    r = subprocess.run([_program(name), mode, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return read(dst)


def tri_host_walk(b, q=None):
    """X, quality, status of every track in the kernel's own order of operations"""
    return _walk("tri", "tracks", lambda p: tc.write_host_input(p, b, q=q), lambda p: tc.read_host_output(p, b.n))


resect_host_walk = rc.host_walk   # R, T, quality, info, status, logs, w


@functools.lru_cache(maxsize=None)
def resect_host_floor():
    """resect_cases.host_walk_floor on the batches here"""
    cases = [(resect_small(holes), resect_yardstick(holes)) + rc.RAGGED_OPTIONS[holes] for holes in (False, True)]
    cases.append((resect_big(False), resect_yardstick(False, "big")) + rc.RAGGED_OPTIONS[False])
    return rc.host_walk_floor(cases)


# ------------------------------------------------------------------ what the host walk changes between the two forms of K
def tri_form_units(b, X, Xm):
    """the largest distance between two results of the batch b, in units of each track's 8 eps cond_2(A) |X| (b in the K / f0 form)"""
    ok = np.flatnonzero(np.diff(b.row_ptr) >= 2)
    return max(np.linalg.norm(X[i] - Xm[i]) / tri_bound(b, i, b.X_true[i]) for i in ok)


@functools.lru_cache(maxsize=None)
def tri_form_change():
    b = tri_big()
    return tri_form_units(b, tri_host_walk(b)[0], tri_host_walk(mixed_form(b))[0])


def resect_form_units(b, ys, a, m):
    """the largest distance between the poses a and m (R, T each) in the Newton-step unit of the yardstick's results ys"""
    worst = 0.0
    for i, y in enumerate(ys):
        if not y["status"] & 1:
            d = np.linalg.norm(np.sqrt(np.diag(y["H"])) * rc.pose_delta(a[0][i], a[1][i], dict(R=m[0][i], T=m[1][i])))
            worst = max(worst, float(d / rc.ref.newton_step(y["H"], y["g"])))
    return worst


@functools.lru_cache(maxsize=None)
def resect_form_change():
    b, opts = resect_small(False), rc.RAGGED_OPTIONS[False]
    return resect_form_units(b, resect_yardstick(False), resect_host_walk(b, *opts), resect_host_walk(mixed_form(b), *opts))


def locate_form_units(status, a, m):
    return max([0.0] + [max(lc.ref.pose_distance(a[0][i], a[1][i], m[0][i], m[1][i], lc.DEPTH)) for i in np.flatnonzero(status == 0)])


@functools.lru_cache(maxsize=None)
def locate_form_change():
    b = locate_small(False)
    a, m = lc.host_walk(b, LOCATE_HYPOTHESES, 1), lc.host_walk(mixed_form(b), LOCATE_HYPOTHESES, 1)
    assert np.array_equal(a.status, m.status) and np.array_equal(a.located[:, 1:5], m.located[:, 1:5], equal_nan=True) and np.array_equal(a.inliers, m.inliers)
    return locate_form_units(a.status, (a.R, a.T), (m.R, m.T))


def relate_form_units(status, a, m):
    return max([0.0] + [max(rlref.rotation_angle(a[0][i], m[0][i]), rlref.direction_angle(a[1][i], m[1][i])) for i in np.flatnonzero(status == 0)])


@functools.lru_cache(maxsize=None)
def relate_form_change():
    b = relate_many()
    a, m = rl.host_walk(b, 65, 1), rl.host_walk(mixed_form(b, ("Ka", "Kb")), 65, 1)
    assert np.array_equal(a.status, m.status) and np.array_equal(a.related[:, 1:5], m.related[:, 1:5], equal_nan=True) and np.array_equal(a.inliers, m.inliers)
    return relate_form_units(a.status, (a.R, a.T), (m.R, m.T))


# ------------------------------------------------------------------ a neighbour's K on the noise-free batches
# Each function returns, per item, the yardstick's error with the next item's K over the bound the GPU test applies to that item
# with its own K.  tests/test_frontend_k_cpu.py asserts that every ratio is above one: no item sits where a wrong K goes unnoticed.
@functools.lru_cache(maxsize=None)
def tri_wrong_K():
    """per frame j: K[j] alone replaced by K[j + 1]; the smallest ratio over the tracks that observe j"""
    b = tri_truth()
    M = len(b.K)
    bounds = [tc.cond_bound(b, i, b.X_true[i]) for i in range(b.n)]
    out = np.full(M, np.inf)
    for j in range(M):
        K = b.K.copy()
        K[j] = b.K[(j + 1) % M]
        for i in range(b.n):
            fr, uv = tc.track(b, i)
            if j in fr:
                X = tref.triangulate_track(b.f0, fr, uv, b.R, b.T, K)[0]
                out[j] = min(out[j], np.linalg.norm(X - b.X_true[i]) / bounds[i])
    return out


@functools.lru_cache(maxsize=None)
def resect_wrong_K():
    b = resect_truth()
    ys, floor = resect_truth_yardstick()
    w = with_K(b, K=rolled(b.K))
    out = []
    for i in range(b.n):
        y = rc.yardstick(w, i, attempts=40, rel_change=0.0)
        out.append(rc.accuracy_units(y["R"], y["T"], b.frames[i], ys[i]["H"]) / (10.0 * floor))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def locate_wrong_K():
    b = locate_truth()
    w = with_K(b, K=rolled(b.K))
    bound = 10.0 * locate_truth_floor()
    out = []
    for i in range(b.n):
        y = lc.yardstick(w, i, 64, 1)
        out.append(max(lc.pose_error(y["R"], y["T"], b.frames[i])) / bound)
    return np.array(out)


def relate_truth_bounds():
    """(rotation, direction) bounds per pair: max(1e-13, 64 x the yardstick's own distance from the truth)"""
    b = relate_truth()
    return [tuple(max(1e-13, 64.0 * e) for e in rl.pose_error(y["R"], y["T"], b.R[i], b.T[i])) for i, y in enumerate(relate_truth_yardstick())]


@functools.lru_cache(maxsize=None)
def relate_wrong_K():
    """[n][2]: K_a rolled with K_b the pair's own, and the other way round; the larger of the rotation's and the direction's ratio"""
    b = relate_truth()
    bounds = relate_truth_bounds()
    out = np.zeros((b.n, 2))
    for side, w in enumerate((with_K(b, Ka=rolled(b.Ka)), with_K(b, Kb=rolled(b.Kb)))):
        for i in range(b.n):
            y = rlref.relate(b.f0, w.Ka[i], w.Kb[i], *rl.pair_obs(b, i), 64, 1, rl.TAU)
            dr, dt = rl.pose_error(y["R"], y["T"], b.R[i], b.T[i])
            out[i, side] = max(dr / bounds[i][0], dt / bounds[i][1])
    return out


def cpu_figures():
    """what profiles/frontend_intrinsics/test_figures.json records of the CPU side"""
    return dict(
        triangulate=dict(form_change_in_cond_bounds=tri_form_change(), wrong_K_smallest_ratio=float(tri_wrong_K().min())),
        resect=dict(host_walk_floor_newton_steps=resect_host_floor(), truth_floor_eps_sqrt_cond=resect_truth_yardstick()[1],
                    form_change_newton_steps=resect_form_change(), wrong_K_smallest_ratio=float(resect_wrong_K().min())),
        locate=dict(host_floor=locate_host_floor(), truth_floor=locate_truth_floor(), form_change=locate_form_change(),
                    wrong_K_smallest_ratio=float(locate_wrong_K().min())),
        relate=dict(truth_largest_bound=float(max(max(p) for p in relate_truth_bounds())), form_change=relate_form_change(),
                    wrong_K_smallest_ratio=float(relate_wrong_K().min())))
