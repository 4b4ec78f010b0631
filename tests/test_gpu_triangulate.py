"""Batched landmark triangulation and refinement on the device (srk_triangulate_tracks, srk_ba_triangulate)
against the numpy yardstick (tests/triangulate_ref.py) on the cases of tests/triangulate_cases.py."""
import ctypes as C

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import _lib
from surikatoko_amd import ba as B
from surikatoko_amd import io as sio
from surikatoko_amd import triangulate as T
import hetero_cases
import triangulate_cases as tc
import triangulate_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def h():
    ba = sa.BundleAdjustmentKanatani(0)
    yield ba
    ba.close()


def _tri(h, b, q=None, rows=None, **kw):
    """the batch (or the tracks `rows` of it, in that order) through srk_triangulate_tracks"""
    if rows is None:
        return sa.triangulate_tracks(h, b.f0, b.row_ptr, b.frame, b.uv, b.R, b.T, b.K, q=q, **kw)
    obs = np.concatenate([np.arange(b.row_ptr[i], b.row_ptr[i + 1]) for i in rows] + [np.zeros(0, np.int64)])
    rp = np.concatenate([[0], np.cumsum([b.row_ptr[i + 1] - b.row_ptr[i] for i in rows])])
    return sa.triangulate_tracks(h, b.f0, rp, b.frame[obs], b.uv[obs], b.R, b.T, b.K, q=None if q is None else q[obs], **kw)


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.uint8).reshape(-1), y.view(np.uint8).reshape(-1)) for x, y in zip(a, b))


# ------------------------------------------------------------------ conditioning
@pytest.mark.parametrize("ratio", tc.RATIOS)
@pytest.mark.parametrize("n_views", tc.VIEWS)
def test_conditioning_stays_at_eps_cond(h, n_views, ratio):
    """noise-free tracks at baseline / depth 1e-1 .. 1e-5: every track within 8 eps cond_2(A) |X| of the truth and of the host
    function; a kernel that forms A^T A misses this by orders of magnitude at the two smaller ratios"""
    b = tc.conditioning(n_views, ratio)
    X, quality, status = _tri(h, b)
    assert not np.any(status & (T.TRI_FEW_VIEWS | T.TRI_DEGENERATE | T.TRI_BEHIND))
    worst = 0.0
    for i in range(b.n):
        bound = tc.cond_bound(b, i, b.X_true[i])
        Xh = sio.triangulate_least_squares(tc.track(b, i)[1], tc.host_P(b, i), b.f0)
        worst = max(worst, np.linalg.norm(X[i] - b.X_true[i]) / bound, np.linalg.norm(X[i] - Xh) / bound)
    print(f"views {n_views} ratio {ratio:g}: worst error / (8 eps cond |X|) = {worst:.3f}")
    assert worst <= 1.0
    assert np.all(quality[:, 3] == n_views)


# ------------------------------------------------------------------ ragged shapes
@pytest.fixture(scope="module")
def ragged_yardstick():
    """the yardstick on the 4099-track batch, computed once; the smaller batches are its leading tracks' shapes with other data"""
    out = {}

    def get(n):
        if n not in out:
            b = tc.ragged(n)
            out[n] = [ref.triangulate_track(b.f0, *tc.track(b, i), b.R, b.T, b.K) for i in range(b.n)]
        return out[n]
    return get


@pytest.mark.parametrize("n_tracks", tc.RAGGED_SIZES)
def test_ragged_batches_against_the_yardstick(h, ragged_yardstick, n_tracks):
    b = tc.ragged(n_tracks)
    X, quality, status = _tri(h, b)
    want = ragged_yardstick(n_tracks)
    lengths = np.diff(b.row_ptr)
    assert np.array_equal(quality[:, 3], lengths.astype(np.float64))
    few = lengths < 2
    assert np.all(status[few] == T.TRI_FEW_VIEWS) and np.all(np.isnan(X[few]))
    assert np.array_equal(status, np.array([w[2] for w in want], np.uint32))
    for i in np.flatnonzero(~few):
        Xy, qy, _, _ = want[i]
        assert np.linalg.norm(X[i] - Xy) <= tc.cond_bound(b, i, Xy), i
        # the angle of two rays that each carry a few roundings moves by a few eps (radians)
        assert abs(quality[i, 1] - qy[1]) <= np.degrees(100 * ref.EPS), i
        A, _ = tc.system(b, i)
        assert abs(quality[i, 2] - qy[2]) <= (100 * ref.EPS * ref.cond2(A) + 1e-12) * qy[2], i


# ------------------------------------------------------------------ independence and reproducibility
def test_a_tracks_bits_do_not_depend_on_the_batch(h):
    b = tc.ragged(4099)
    whole = _tri(h, b)
    assert _same_bits(whole, _tri(h, b))                       # two runs
    rev = _tri(h, b, rows=list(range(b.n))[::-1])              # reversed order: the outputs are permuted
    assert _same_bits([a[::-1].copy() for a in rev], whole)
    for i in (9, 4098, 2047, 33, 18):                          # alone: 100, 33, 17 views, ...
        alone = _tri(h, b, rows=[i])
        assert _same_bits(alone, [a[i:i + 1].copy() for a in whole]), i


# ------------------------------------------------------------------ weights
def test_weights(h):
    b = tc.noisy()
    plain = _tri(h, b, refine_attempts=5)
    assert _same_bits(plain, _tri(h, b, q=np.ones(len(b.frame)), refine_attempts=5))   # q = 1 is q = NULL
    # q_o = 0 is the track without that observation: switch off one observation per track (its first, middle or last)
    rng = np.random.default_rng(5)
    q = rng.uniform(0.5, 2.0, len(b.frame))
    off = np.array([b.row_ptr[i] + (0, (b.row_ptr[i + 1] - b.row_ptr[i]) // 2, b.row_ptr[i + 1] - b.row_ptr[i] - 1)[i % 3] for i in range(b.n)])
    q[off] = 0.0
    with_zero = _tri(h, b, q=q, refine_attempts=5)
    keep = np.ones(len(b.frame), bool)
    keep[off] = False
    rp = b.row_ptr - np.arange(b.n + 1)
    without = sa.triangulate_tracks(h, b.f0, rp, b.frame[keep], b.uv[keep], b.R, b.T, b.K, q=q[keep], refine_attempts=5)
    assert _same_bits(with_zero, without)
    assert np.array_equal(with_zero[1][:, 3], np.diff(rp).astype(np.float64))
    # and the weighted result is the yardstick's
    for i in range(0, b.n, 7):
        fr, uv = tc.track(b, i)
        Xy, qy, sy, _ = ref.triangulate_track(b.f0, fr, uv, b.R, b.T, b.K, q=q[b.row_ptr[i]:b.row_ptr[i + 1]])
        lin = _tri(h, b, q=q, rows=[i])
        A, rhs = tc.system(b, i, q[b.row_ptr[i]:b.row_ptr[i + 1]])
        k = ref.cond2(A)
        bound = 8 * ref.EPS * (k + k * k * np.linalg.norm(rhs - A @ Xy) / (np.linalg.norm(A, 2) * np.linalg.norm(Xy))) * np.linalg.norm(Xy)
        assert np.linalg.norm(lin[0][0] - Xy) <= bound and lin[2][0] == sy
        assert lin[1][0, 0] == pytest.approx(qy[0], rel=1e-9)
    # a track left with one weighted view
    q1 = np.ones(len(b.frame))
    q1[b.row_ptr[3] + 1:b.row_ptr[4]] = 0.0
    X, quality, status = _tri(h, b, q=q1)
    assert status[3] == T.TRI_FEW_VIEWS and np.all(np.isnan(X[3])) and quality[3, 3] == 1.0
    assert _same_bits([a[4:] for a in (X, quality, status)], [a[4:] for a in _tri(h, b)])


# ------------------------------------------------------------------ status bits
def test_status_bits(h):
    rng = np.random.default_rng(11)
    R, Tr = tc.rig(4, 1.0, rng)
    K = np.broadcast_to(tc.K0, (4, 3, 3)).copy()
    X0 = np.array([0.2, -0.1, 5.0])
    # two identical frames: zero baseline
    R2, T2 = np.stack([R[0], R[0]]), np.stack([Tr[0], Tr[0]])
    uv = tc.pixels(R2, T2, K[:2], np.array([0, 1]), X0)
    X, quality, status = sa.triangulate_tracks(h, tc.F0, [0, 2], [0, 1], uv, R2, T2, K[:2])
    assert (status[0] & T.TRI_DEGENERATE) or (np.all(np.isfinite(X[0])) and quality[0, 2] > 1e12)
    assert quality[0, 1] <= np.degrees(100 * ref.EPS)
    # a point behind the second camera (turned around): the linear system does not see the sign of the depth
    Rb, Tb = R.copy(), Tr.copy()
    flip = np.diag([-1.0, 1.0, -1.0])
    Rb[1], Tb[1] = flip @ R[1], flip @ Tr[1]
    fr = np.arange(4)
    uvb = tc.pixels(Rb, Tb, K, fr, X0)
    X, quality, status = sa.triangulate_tracks(h, tc.F0, [0, 4], fr, uvb, Rb, Tb, K)
    assert status[0] & T.TRI_BEHIND and np.linalg.norm(X[0] - X0) < 1e-9
    X, quality, status = sa.triangulate_tracks(h, tc.F0, [0, 4], fr, tc.pixels(R, Tr, K, fr, X0), R, Tr, K)
    assert status[0] == 0
    # the parallax gate: set above the reported angle, clear below
    angle = quality[0, 1]
    want = ref.triangulate_track(tc.F0, fr, tc.pixels(R, Tr, K, fr, X0), R, Tr, K)[1][1]
    assert angle == pytest.approx(want, abs=np.degrees(100 * ref.EPS)) and angle > 1.0
    for gate, bit in ((angle * 1.001, T.TRI_LOW_PARALLAX), (angle * 0.999, 0)):
        _, _, st = sa.triangulate_tracks(h, tc.F0, [0, 4], fr, tc.pixels(R, Tr, K, fr, X0), R, Tr, K, min_parallax_deg=gate)
        assert st[0] == bit
    assert T.tri_status_names(T.TRI_BEHIND | T.TRI_NOT_CONVERGED) == ["BEHIND", "NOT_CONVERGED"]


# ------------------------------------------------------------------ refinement
def _terms(b, i, X):
    fr, uv = tc.track(b, i)
    return ref.energy_terms(b.f0, uv, ref.proj_mats(b.R[fr], b.T[fr], b.K[fr]), np.ones(len(fr)), X)


def _newton_units(b, i, X):
    """|H^-1 g| at X in units of eps cond_2(H) |X|"""
    _, H, g = _terms(b, i, X)
    return np.linalg.norm(np.linalg.solve(H, g)) / (ref.EPS * np.linalg.cond(H, 2) * np.linalg.norm(X))


def test_refinement_never_raises_the_error_and_reaches_the_yardsticks_floor(h):
    """1 px of noise, 3 to 32 views, 20 attempts, refine_rel_change = 0.  Both loops run until no attempt can lower E any more, so
    the remaining Newton step |H^-1 g| is set by the rounding of E (about sqrt(eps E / |H|), hundreds of eps cond(H) |X| on the
    worst track, a hundredth on the median one).  Measured on the CPU for the yardstick's own converged points of this case:
    at most 1.14e3 eps cond_2(H) |X| (median 2.1e-2); the kernel's order of operations walked on the host: 9.2e2; the device:
    1.73e3.  The bound is 10 x the yardstick's maximum, computed here from the yardstick itself: 1.14e4."""
    b = tc.noisy()
    lin = _tri(h, b)
    X, quality, status = _tri(h, b, refine_attempts=20, refine_rel_change=0.0)
    # the loop's own E (quality[0] = sqrt(E / n), monotone in E): never above the linear point's, exactly
    assert np.all(quality[:, 0] <= lin[1][:, 0])
    assert np.all(status == T.TRI_NOT_CONVERGED)   # rel_change 0 never stops early: the yardstick's run hits the cap everywhere
    yard = [ref.triangulate_track(b.f0, *tc.track(b, i), b.R, b.T, b.K, refine_attempts=20, refine_rel_change=0.0) for i in range(b.n)]
    assert all(y[2] == ref.NOT_CONVERGED for y in yard)
    for i in range(b.n):   # the same statement with E recomputed by numpy: up to the rounding of a sum of 2 n squares
        assert _terms(b, i, X[i])[0] <= _terms(b, i, lin[0][i])[0] * (1 + 4 * len(tc.track(b, i)[0]) * ref.EPS), i
    floor = max(_newton_units(b, i, yard[i][0]) for i in range(b.n))
    got = max(_newton_units(b, i, X[i]) for i in range(b.n))
    print(f"Newton step in eps cond(H) |X|: yardstick {floor:.3e}, device {got:.3e}, bound {10 * floor:.3e}")
    assert got <= 10 * floor


def test_first_attempt_matches_the_yardstick(h):
    b = tc.noisy()
    lin = _tri(h, b)
    X, quality, status = _tri(h, b, refine_attempts=1, refine_rel_change=0.0)
    for i in range(b.n):
        Xy, qy, sy, log = ref.triangulate_track(b.f0, *tc.track(b, i), b.R, b.T, b.K, refine_attempts=1, refine_rel_change=0.0)
        accepted = not np.array_equal(X[i], lin[0][i])
        assert accepted == log[0][0] and status[i] == sy, i
        # the linear point within the least-squares perturbation bound, the step a 3 x 3 solve on top of it
        _, H, _ = _terms(b, i, Xy)
        step = 8 * ref.EPS * np.linalg.cond(H, 2) * np.linalg.norm(Xy - lin[0][i])
        assert np.linalg.norm(X[i] - Xy) <= tc.ls_bound(b, i, Xy) + step, i
        assert quality[i, 0] == pytest.approx(qy[0], rel=1e-9)


@pytest.mark.parametrize("attempts,rel_change", [(1, 2e-4), (2, 3e-11), (6, 1e-6)])
def test_not_converged_exactly_where_the_yardstick_hits_the_cap(h, attempts, rel_change):
    """(1, 2e-4) and (2, 3e-11) split the tracks: the first accepted attempt lowers E by 1e-5 .. 9e-4 of E, the second by
    3e-13 .. 7e-9 (tests/test_triangulate_cpu.py checks that no track sits at a threshold)"""
    b = tc.noisy()
    X, quality, status = _tri(h, b, refine_attempts=attempts, refine_rel_change=rel_change)
    yard = [ref.triangulate_track(b.f0, *tc.track(b, i), b.R, b.T, b.K, refine_attempts=attempts, refine_rel_change=rel_change) for i in range(b.n)]
    want = np.array([y[2] for y in yard], np.uint32)
    assert np.array_equal(status, want)
    if attempts < 6:
        assert 0 < np.count_nonzero(want & ref.NOT_CONVERGED) < b.n


# ------------------------------------------------------------------ the resident scene
SPEC = sa.SceneSpec(n_frames=10, grid_nx=12, grid_ny=9, vis_window=5)


def _resident(reorder, hetero=False):
    """hetero: every frame with its own fx, fy, u0 and v0 (zero skew: what the resident core takes), so that a resident K that did not
    travel with its renumbered frame would be seen"""
    sc = sa.generate_scene(SPEC)
    if hetero:
        sc = hetero_cases.per_frame_intrinsics(sc, SPEC.f0)
        assert min(hetero_cases.distinct_intrinsics(sc)) == sc.M
    if reorder:
        sc = sa.renumber_frames(sc, np.random.default_rng(3).permutation(sc.M))
    g = sa.BundleAdjustmentKanatani(0)
    if reorder:
        g.set_frame_reordering(1)
    assert g.upload(SPEC.f0, sc)
    g.optimize(max_iterations=3)
    return g, sc


@pytest.mark.parametrize("reorder", [False, True])
def test_resident_scene_equals_the_downloaded_poses(h, reorder):
    _resident_scene_equals_the_downloaded_poses(h, reorder, False)


@pytest.mark.parametrize("reorder", [False, True])
def test_resident_scene_with_per_frame_intrinsics_equals_the_downloaded_poses(h, reorder):
    """intrinsic corrections are never applied, so the scene's K is the resident K: triangulate_tracks gets the
    scene's per-frame K in the caller's frame order"""
    _resident_scene_equals_the_downloaded_poses(h, reorder, True)


def _resident_scene_equals_the_downloaded_poses(h, reorder, hetero):
    g, sc = _resident(reorder, hetero)
    try:
        before = [g.buffer(w).copy() for w in (B.BUF_POINTS, B.BUF_CAM_R, B.BUF_CAM_T)]
        X, quality, status = g.triangulate(sc.row_ptr, sc.obs_frame, sc.obs_uv, revert_normalization=True)
        assert all(np.array_equal(a.view(np.uint8), g.buffer(w).view(np.uint8)) for a, w in zip(before, (B.BUF_POINTS, B.BUF_CAM_R, B.BUF_CAM_T)))
        if reorder:
            order = g.frame_order()
            assert order is not None and not np.array_equal(order, np.arange(sc.M))
        got = sc.copy()
        g.download(got, revert_normalization=True)
        R, Tt = got.cam_R.reshape(-1, 3, 3), got.cam_T.reshape(-1, 3)
        K = np.asarray(sc.K, np.float64).reshape(-1, 3, 3)
        Xc, qc, sc_status = sa.triangulate_tracks(h, SPEC.f0, sc.row_ptr, sc.obs_frame, sc.obs_uv, R, Tt, K)
        assert np.array_equal(status, sc_status) and not np.any(status)
        b = tc.batch([(sc.obs_frame[sc.row_ptr[i]:sc.row_ptr[i + 1]], sc.obs_uv.reshape(-1, 2)[sc.row_ptr[i]:sc.row_ptr[i + 1]]) for i in range(sc.N)],
                     R, Tt, np.broadcast_to(K, R.shape))
        C0 = -sc.cam_R.reshape(-1, 3, 3)[0].T @ sc.cam_T.reshape(-1, 3)[0]   # the origin of the normalised coordinates
        for i in range(sc.N):
            # The two compute in different coordinates, each within the bound of its own system.  A rigid motion and a scale leave
            # cond(A) alone and move the origin: the resident result's |X| is the distance from frame 0's centre.  The
            # observations carry the scene's residual after three iterations, so the bound is the least-squares one.
            assert np.linalg.norm(X[i] - Xc[i]) <= tc.ls_bound(b, i, Xc[i]) * (1 + np.linalg.norm(Xc[i] - C0) / np.linalg.norm(Xc[i])), i
        assert np.allclose(quality[:, 0], qc[:, 0], rtol=1e-6, atol=1e-9) and np.array_equal(quality[:, 3], qc[:, 3])
        # in the normalised coordinates the result is the normalised point
        Xn, _, _ = g.triangulate(sc.row_ptr, sc.obs_frame, sc.obs_uv, revert_normalization=False)
        assert not np.array_equal(Xn, X)
    finally:
        g.close()


def test_resident_scene_refusals():
    sc = sa.generate_scene(SPEC)
    g = sa.BundleAdjustmentKanatani(0)
    try:
        with pytest.raises(RuntimeError):   # no scene
            g.triangulate(sc.row_ptr, sc.obs_frame, sc.obs_uv)
        g.set_intrinsic_groups(np.zeros(sc.M, np.int32))
        assert g.upload(SPEC.f0, sc)
        with pytest.raises(ValueError):
            g.triangulate(sc.row_ptr, sc.obs_frame, sc.obs_uv)
        assert "intrinsic groups" in g.last_error()
    finally:
        g.close()
    g = sa.BundleAdjustmentKanatani(0)
    try:
        hook = _lib.ALLREDUCE_FN(lambda *a: 0)
        assert g.upload(SPEC.f0, sc)
        g.set_allreduce(hook, 0, 2)
        with pytest.raises(ValueError):
            g.triangulate(sc.row_ptr, sc.obs_frame, sc.obs_uv)
        assert "more than one rank" in g.last_error()
    finally:
        g.close()


# ------------------------------------------------------------------ bad arguments
def test_bad_arguments_launch_nothing(h):
    """the checks only: nothing of these batches reaches a kernel"""
    b = tc.ragged(255)
    n_frames = len(b.R)
    out = [np.full((b.n, 3), 7.0), np.full((b.n, 4), 7.0), np.full(b.n, 7, np.uint32)]

    def call(rp, fr, uv, q=None):
        rp, fr, uv = np.asarray(rp, np.int64), np.asarray(fr, np.int32), np.ascontiguousarray(uv, np.float64)
        rc = sa.lib().srk_triangulate_tracks(C.c_void_p(h._h), C.c_double(b.f0), C.c_int64(len(rp) - 1), B._p(rp), B._p(fr), B._p(uv),
                                             None if q is None else B._p(q), C.c_int32(n_frames), B._p(b.R), B._p(b.T), B._p(b.K), C.c_int(0), None,
                                             B._p(out[0]), B._p(out[1]), B._p(out[2]))
        return rc, h.last_error()

    fr = b.frame.copy()
    fr[17] = n_frames
    rc, why = call(b.row_ptr, fr, b.uv)
    assert rc == -1 and "out of range" in why
    rp = b.row_ptr.copy()
    rp[5] = rp[4] - 1
    rc, why = call(rp, b.frame, b.uv)
    assert rc == -1 and "decreases" in why
    uv = b.uv.copy()
    uv[40, 1] = np.nan
    rc, why = call(b.row_ptr, b.frame, uv)
    assert rc == -1 and "not finite" in why
    q = np.ones(len(b.frame))
    q[3] = -1.0
    rc, why = call(b.row_ptr, b.frame, b.uv, q)
    assert rc == -1 and "q of observation 3" in why
    assert all(np.all(a == 7) for a in out)                    # nothing written
    with pytest.raises(ValueError):
        sa.triangulate_tracks(h, b.f0, b.row_ptr, b.frame, b.uv, b.R, b.T, b.K, refine_attempts=65)
    X, _, status = _tri(h, b)                                  # the handle works afterwards
    assert np.all(np.isfinite(X[np.diff(b.row_ptr) >= 2])) and np.all(status[np.diff(b.row_ptr) >= 2] == 0)


# ------------------------------------------------------------------ the C++ adapter
def test_cpp_adapter_triangulate(tmp_path):
    import os
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "triangulate_adapter"
    r = subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(root, "include"), "-I", os.path.join(root, "demos"),
                        os.path.join(here, "cpp", "test_triangulate_adapter.cpp"), "-o", str(exe),
                        "-L", os.path.join(root, "surikatoko_amd"), "-lsrk_ba",
                        "-Wl,-rpath," + os.path.join(root, "surikatoko_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "triangulate adapter ok" in r.stdout
