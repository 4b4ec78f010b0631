"""The cases of two-view pose refinement, shared by tests/test_pair_cpu.py (the yardstick and the host walk
of a pair, no GPU) and tests/test_gpu_pair.py (the kernels).  Pairs, batches and rows are those of tests/relate_cases.py with start
poses added.  Built once per process and never modified."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import pair_ref as ref
import relate_cases as rc
import relate_ref

ROOT, CSRC, F0 = rc.ROOT, rc.CSRC, rc.F0
LANES = 64                                                    # SRK_PAIR_LANES
LENGTHS = (0, 4, 5, 6, 63, 64, 65, 128, 129, 200)             # weighted matches: below and at the five variables, the wave boundaries
BATCH_SIZES = (1, 3, 130)                                     # four pairs a workgroup: one wave, a partly empty workgroup, 33 workgroups
SIGMA = 0.5
START_ANGLE, START_DIRECTION = np.radians(3.0), np.radians(5.0)
# the seeds and (attempts, rel_change) of the two ragged batches (without / with q = 0 in between), chosen so that the yardstick's own
# decisions stay away from every threshold on every pair (tests/test_pair_cpu.py asserts that): some pairs stop by the test, the
# pairs of five and six matches (an exact fit: E_pair falls by decades per attempt) end at the cap
RAGGED_SEED = {False: 2601, True: 2601}
RAGGED_OPTIONS = {False: (4, 1e-2), True: (4, 1e-2)}
OUTLIER_SEED = 2630
OUTLIER_PAIRS, OUTLIER_MATCHES, OUTLIER_SHARE, OUTLIER_HYPOTHESES = 16, 200, 0.3, 256
OUTLIER_TAU = 2.0
OUTLIER_OPTIONS = (6, 1e-7)   # as the resection's runs with a loss: these end at their cap, where the poses have reached the accuracy the case is about


def off_pose(R, T, rng, angle=START_ANGLE, direction=START_DIRECTION):
    """the pose turned by `angle` about a random axis and its direction T turned by `direction` towards a random tangent"""
    a = rng.normal(size=3)
    B = ref.basis(T)
    ph = rng.uniform(0.0, 2.0 * np.pi)
    t = np.cos(direction) * T + np.sin(direction) * (B @ np.array([np.cos(ph), np.sin(ph)]))
    return R @ ref.so3_exp(a / np.linalg.norm(a) * angle).T, t / np.linalg.norm(t)


def with_starts(b, rng, **kw):
    starts = [off_pose(b.R[i], b.T[i], rng, **kw) for i in range(b.n)]
    b.R0 = np.array([s[0] for s in starts]).reshape(-1, 3, 3)
    b.T0 = np.array([s[1] for s in starts]).reshape(-1, 3)
    return b


def rows(b, idx):
    """the batch of the pairs idx of b, in that order, start poses included"""
    idx = list(idx)
    out = rc.rows(b, idx)
    out.R0, out.T0 = b.R0[idx], b.T0[idx]
    return out


def pair_obs(b, i):
    return rc.pair_obs(b, i)


def without_holes(b):
    return rc.without_holes(b)


@functools.lru_cache(maxsize=None)
def ragged(holes=False):
    """one pair of each length in LENGTHS with half a pixel of noise, the start 3 degrees and 5 degrees of direction off the truth;
    with holes, a fifth more matches carry q = 0 (and wrong pixels) and the rest weights between 0.5 and 2"""
    rng = np.random.default_rng(RAGGED_SEED[holes])
    ps, qs = [], []
    for k, n in enumerate(LENGTHS):
        extra = max(1, n // 5) if holes else 0
        p = rc.pair(n + extra, rng, planar=False, sigma=SIGMA)
        w = rng.uniform(0.5, 2.0, n + extra)
        off = rng.choice(n + extra, extra, replace=False)
        w[off] = 0.0
        p.uv_b[off] = rng.uniform(0.0, 600.0, (extra, 2))
        ps.append(p)
        qs.append(w)
    return with_starts(rc.batch(ps, np.concatenate(qs) if holes else None), rng)


def yardstick(b, i, **kw):
    uva, uvb, q = pair_obs(b, i)
    return ref.refine_pair(b.f0, uva, uvb, q, b.Ka[i], b.Kb[i], b.R0[i], b.T0[i], **kw)


@functools.lru_cache(maxsize=None)
def ragged_yardstick(holes=False):
    """the yardstick on every pair of ragged(holes) at RAGGED_OPTIONS[holes], computed once"""
    b = ragged(holes)
    attempts, rel_change = RAGGED_OPTIONS[holes]
    return tuple(yardstick(b, i, attempts=attempts, rel_change=rel_change) for i in range(b.n))


@functools.lru_cache(maxsize=None)
def many(count=BATCH_SIZES[-1], seed=2660):
    """`count` pairs of unequal length (5 .. 150 matches, one of them empty) with half a pixel of noise and off starts"""
    rng = np.random.default_rng(seed)
    ps = [rc.pair(int(rng.integers(5, 151)), rng, sigma=SIGMA) for _ in range(count)]
    ps[2] = rc.pair(0, rng)
    return with_starts(rc.batch(ps), rng)


@functools.lru_cache(maxsize=None)
def outliers():
    """16 pairs of 200 matches, half a pixel of noise, 30 % of the matches replaced by uniform points"""
    rng = np.random.default_rng(OUTLIER_SEED)
    return rc.batch([rc.pair(OUTLIER_MATCHES, rng, sigma=SIGMA, share=OUTLIER_SHARE) for _ in range(OUTLIER_PAIRS)])


@functools.lru_cache(maxsize=None)
def copies(count=8):
    """eight copies of one match: H has rank one"""
    rng = np.random.default_rng(2670)
    p = rc.pair(1, rng)
    p.uv_a, p.uv_b, p.moved = np.repeat(p.uv_a, count, axis=0), np.repeat(p.uv_b, count, axis=0), np.zeros(0, int)
    b = rc.batch([p])
    b.R0, b.T0 = b.R.copy(), b.T.copy()
    return b


# ------------------------------------------------------------------ a result against the yardstick's
def pose_delta(R, T, y):
    """d = [w; beta] with (R, T) = the yardstick's result y moved by d: R = R_y Exp(w)^T (w from the skew part of R^T R_y), beta
    the tangent part of T - T_y in the basis at T_y"""
    D = R.T @ y["R"]
    w = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return np.concatenate([w, y["basis"] @ (T - y["T"])])


def pose_units(R, T, y):
    """the distance of the pose (R, T) from the yardstick's result y in the Jacobi-scaled variables, in units of the Newton step
    |H_s^-1 g_s| that remains at the yardstick's result"""
    return float(np.linalg.norm(np.sqrt(np.diag(y["H"])) * pose_delta(R, T, y)) / ref.newton_step(y["H"], y["g"]))


def energy_tolerance(b, i, E, n):
    """The bound on a difference of two values of E_pair, argued as resect_cases.energy_tolerance: 1e-12 E, as long as the number
    format can deliver it.  The Sampson residual is r = (p_b . F p_a) / sqrt(den); the numerator is a sum of products of size
    |p| |F p| that cancel to r sqrt(den), and each term carries two roundings (the product, the sum), so r is good to
    de = 2 eps max |p| (p holds the pixel coordinates and f0; times sqrt(q) with information), which moves E = sum q r^2 by
    2 sqrt(n E) de + n de^2.  That floor is the larger of the two only where the rms residual is far below a pixel: on the pairs of
    five and six matches, fitted exactly."""
    uva, uvb, q = pair_obs(b, i)
    big = max(np.abs(uva).max(), np.abs(uvb).max(), abs(b.f0))
    de = 2 * ref.EPS * big * (1.0 if q is None else np.sqrt(q.max()))
    return max(1e-12 * E, 2 * np.sqrt(n * E) * de + n * de * de)


def energy_at(b, i, R, T, kind=ref.NONE, delta=None):
    """the yardstick's E_pair of pair i at the pose (R, T)"""
    uva, uvb, q = pair_obs(b, i)
    return ref.terms(b.f0, uva, uvb, q, b.Ka[i], b.Kb[i], R, T, kind, delta)[0]


def agree(got, ys, b, kind=ref.NONE, delta=None, logs=None, bound=None):
    """A result `got` (a PairResult over the batch b) against the yardstick's results ys, pair by pair, wherever the yardstick's
    log stays away from every threshold (resect_cases.margins_ok; the callers assert separately that no named case is excused):
    the same status, attempts and -- with logs -- accept / reject sequence; E_pair within energy_tolerance of the yardstick's E_pair
    at the result's own pose and, where the run ended by the stop test, of the yardstick's own; the pose within `bound` Newton-step
    units when given.  Returns the largest pose distance in those units."""
    import resect_cases
    worst = 0.0
    for i, y in enumerate(ys):
        if not resect_cases.margins_ok(y["log"], y["rel_change"]):
            continue
        q = got.quality[i]
        assert got.status[i] == y["status"], (i, got.status[i], y["status"])
        assert q[5] == y["quality"][5] and q[1] == y["quality"][1], (i, q, y["quality"])
        if logs is not None:
            assert [int(a) for a in logs[i][:, 0]] == [int(a) for a, _, _ in y["log"]], i
        if y["status"] & ref.FEW_POINTS:
            assert np.array_equal(got.R[i], b.R0[i]) and np.array_equal(got.T[i], b.T0[i]) and np.isnan(q[3]) and not np.any(got.info[i]), i
            continue
        assert q[4] == y["quality"][4], (i, q[4], y["quality"][4])
        assert abs(np.linalg.norm(got.T[i]) - 1.0) <= 4 * ref.EPS and np.abs(got.E[i] - ref.skew(got.T[i]) @ got.R[i]).max() <= 4 * ref.EPS, i
        E = q[0] ** 2 * q[1]
        tol = energy_tolerance(b, i, E, q[1])
        assert abs(E - energy_at(b, i, got.R[i], got.T[i], kind, delta)) <= tol, (i, E, tol)
        if not y["status"] & ref.NOT_CONVERGED:
            assert abs(E - y["E_pair"]) <= tol, (i, E, y["E_pair"], tol)
        units = pose_units(got.R[i], got.T[i], y)
        worst = max(worst, units)
        if bound is not None:
            assert units <= bound, (i, units, bound)
    return worst


def tagged(ys, rel_change):
    """the yardstick's results with the rel_change they ran at (agree reads it)"""
    for y in ys:
        y["rel_change"] = rel_change
    return ys


def host_walk(b, attempts=10, rel_change=1e-9, loss=None, delta=None, want_weights=False):
    """every pair of the batch walked on the host through the library (srk_pair_host_pair): a PairResult over the batch, g [n][5]
    and the logs"""
    from surikatoko_amd import pair as PR
    res, grads, logs = [], [], []
    for i in range(b.n):
        uva, uvb, q = pair_obs(b, i)
        r, g, log = PR.host_pair(b.f0, uva, uvb, b.Ka[i], b.Kb[i], b.R0[i], b.T0[i], q=q, attempts=attempts, rel_change=rel_change, loss=loss, delta=delta,
                                 want_weights=want_weights)
        res.append(r)
        grads.append(g)
        logs.append(log)
    cat = lambda k: np.concatenate([getattr(r, k) for r in res]) if res else None  # noqa: E731
    return PR.PairResult(cat("R"), cat("T"), cat("E"), cat("quality"), cat("info"), cat("basis"), cat("status"),
                         cat("weights") if want_weights else None), np.array(grads), logs


@functools.lru_cache(maxsize=None)
def host_walk_floor():
    """The largest distance, in Newton-step units, between the yardstick and the kernel's order of operations walked on the host,
    over the two ragged batches: computed on the CPU, the device is held to ten times this."""
    worst = 0.0
    for holes in (False, True):
        b = ragged(holes)
        attempts, rel_change = RAGGED_OPTIONS[holes]
        got, _, logs = host_walk(b, attempts, rel_change)
        worst = max(worst, agree(got, tagged(ragged_yardstick(holes), rel_change), b, logs=logs))
    return worst


def pose_error(R, T, Rt, Tt):
    """(rotation angle, angle between the translation directions) to the truth"""
    return relate_ref.rotation_angle(R, Rt), relate_ref.direction_angle(T, Tt)


# ------------------------------------------------------------------ the host program (tests/cpp/test_pair_host.cpp)
def build_host_program(out, extra=()):
    return subprocess.run([rc.cxx(), "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "test_pair_host.cpp"),
                           os.path.join(CSRC, "srk_pair.cpp"), "-o", str(out)], capture_output=True, text=True)


@functools.lru_cache(maxsize=None)
def host_program():
    """the stand-alone program, built once per process into a temporary directory; None without a host compiler"""
    if rc.cxx() is None:
        return None
    exe = os.path.join(tempfile.mkdtemp(prefix="pair_bin"), "test_pair_host")
    r = build_host_program(exe)
    assert r.returncode == 0, r.stderr
    return exe

