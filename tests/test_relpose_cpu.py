"""Relative-pose factors without a device: the yardstick's added terms against finite differences of the objective, the host
normalisation map, the setter's checks, the planner with pairs, and the conditioning of every case the GPU tests compare."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import ba as B
import constant_cases as cc
import constant_ref as kref
import prior_cases as pc
import relpose_cases as rc
import relpose_ref as rr
import weighted_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surikatoko_amd", "csrc")


def _orc_scene(orc, sc, normalise=True):
    so = orc.Scene(sc.points, sc.cam_R, sc.cam_T, sc.K, sc.shared_k, sc.row_ptr, sc.obs_frame, sc.obs_uv)
    nrm = None
    if normalise:
        ok, nrm = orc.normalize(so)
        assert ok
    return so, nrm


def _one_factor(so, a, b, angle, seed=1):
    """a factor on (a, b) whose rotation residual has the given angle and whose translation residual is 0.1 world units"""
    Z, z = rr.relative_pose(so, a, b)
    axis = np.array([0.3, -0.5, 0.8])
    axis /= np.linalg.norm(axis)
    A = np.random.RandomState(seed).uniform(-1, 1, size=(6, 6))
    L = A @ A.T + 0.5 * np.eye(6)
    return rr.Factors([a], [b], (Z @ pc.rodrigues(axis * angle))[None], (z + np.array([0.06, -0.08, 0.05]))[None], L[None])


def _central(f, eps):
    """central difference of f at 0 with step eps, the eps^2 term removed with the step 2 eps (Richardson): the factor energy is
    no quadratic in the rotation variables (unlike a position prior), and its plain central difference with eps = 1e-4 is off
    by 1.4e-6 of the gradient on the scene used here (measured: 1.4e-4, 1.4e-6, 1.4e-8 at 1e-3, 1e-4, 1e-5, so it is the third
    derivative and no error of the gradient), above the tolerance the test takes from tests/test_prior_cpu.py; what is left
    is of order eps^4"""
    d1 = (f(eps) - f(-eps)) / (2 * eps)
    d2 = (f(2 * eps) - f(-2 * eps)) / (4 * eps)
    return (4.0 * d1 - d2) / 3.0


def _moved(orc, so, j, v, step):
    s2 = so.copy()
    corr = np.zeros(3 * so.N + 10 * so.M)
    corr[3 * so.N + 10 * j + v] = step
    orc.apply_corrections(s2, corr)
    return s2


def _fd_gradient(orc, so, fac, frames, eps):
    """differences of the factor energy along the T and W variables of the given frames, through orc.apply_corrections"""
    return np.array([_central(lambda t: rr.energy(fac, _moved(orc, so, j, v, t)), eps) for j in frames for v in range(4, 10)])


@pytest.mark.parametrize("angle", [0.0, 1e-9, 0.05, 1.0])
def test_gradient_terms_agree_with_finite_differences(orc, angle):
    """2 J_a^T L e and 2 J_b^T L e against central differences of the factor energy for the T and W variables of both frames,
    full information matrix, rotation residuals of 0, 1e-9 (both in the series branch of Log and Jr^-1), 0.05 and 1 rad.
    Step 1e-4 and rel 1e-6 as tests/test_prior_cpu.py, the differences taken by _central.  The tolerance is relative to the
    largest gradient entry of the factor (an entry that is zero by symmetry has no scale of its own)."""
    sc, f0 = cc.scene("nf2_short_runs")
    so, _ = _orc_scene(orc, sc)
    a, b = 2, 4
    fac = _one_factor(so, a, b, angle)
    e, Ja, Jb = rr.jacobians(fac, so)
    assert np.linalg.norm(e[0, 3:]) == pytest.approx(angle, rel=1e-6, abs=1e-15)
    g = np.concatenate([2 * Ja[0].T @ fac.info[0] @ e[0], 2 * Jb[0].T @ fac.info[0] @ e[0]])
    fd = _fd_gradient(orc, so, fac, (a, b), 1e-4)
    print(f"angle {angle:g}: gradient vs finite differences {np.abs(fd - g).max() / np.abs(g).max():.3e}")
    assert np.all(np.isfinite(g)) and np.abs(g).max() > 0
    assert np.abs(fd - g).max() < 1e-6 * np.abs(g).max()
    # and through add_terms: the frame gradients of the oracle's layout, nothing in the intrinsics or the landmarks
    base = orc.derivatives(f0, so)
    gt, V, U, W = rr.add_terms(base, so, fac)
    d = (gt - base[0])[3 * so.N:].reshape(-1, 10)
    assert np.allclose(d[a, 4:], g[:6], rtol=0, atol=1e-12 * np.abs(g).max())
    assert np.allclose(d[b, 4:], g[6:], rtol=0, atol=1e-12 * np.abs(g).max())
    assert np.all(d[:, :4] == 0) and np.all((gt - base[0])[:3 * so.N] == 0)
    other = np.ones(so.M, dtype=bool)
    other[[a, b]] = False
    assert np.all(d[other] == 0) and np.array_equal(U[other], base[2][other]) and np.array_equal(V, base[1])
    assert np.all((U - base[2])[:, :4, :] == 0) and np.all((U - base[2])[:, :, :4] == 0)


def test_zero_residual_factor_gives_zero_gradient_finite_blocks_and_exact_gauss_newton(orc):
    """a factor whose measurement is the current relative pose: e = 0 exactly, zero gradient, finite blocks; and there
    Gauss-Newton is exact, so 2 J^T L J (both diagonal blocks and the coupling block) equals the finite-difference Jacobian of
    the gradient (step 1e-4, _central), to rel 1e-5 of the largest block entry, as tests/test_prior_cpu.py holds second
    differences."""
    sc, f0 = cc.scene("nf2_short_runs")
    so, _ = _orc_scene(orc, sc)
    a, b = 4, 2  # given backwards as well
    Z, z = rr.relative_pose(so, a, b)
    L = _one_factor(so, a, b, 0.0).info
    fac = rr.Factors([a], [b], Z[None], z[None], L)
    e, Ja, Jb = rr.jacobians(fac, so)
    assert np.all(e == 0)
    base = orc.derivatives(f0, so)
    g, V, U, W = rr.add_terms(base, so, fac)
    assert np.array_equal(g, base[0])
    Cb = rr.couplings(fac, so)[0]
    assert np.all(np.isfinite(U)) and np.all(np.isfinite(Cb)) and np.abs(Cb).max() > 0
    H = np.zeros((12, 12))  # finite-difference Jacobian of the factor's gradient over (a's pose, b's pose)
    eps = 1e-4
    def grad(s2):
        e2, Ja2, Jb2 = rr.jacobians(fac, s2)
        return np.concatenate([2 * Ja2[0].T @ L[0] @ e2[0], 2 * Jb2[0].T @ L[0] @ e2[0]])

    for col, (j, v) in enumerate([(a, v) for v in range(4, 10)] + [(b, v) for v in range(4, 10)]):
        H[:, col] = _central(lambda t: grad(_moved(orc, so, j, v, t)), eps)
    want = np.block([[(U - base[2])[a, 4:, 4:], Cb], [Cb.T, (U - base[2])[b, 4:, 4:]]])
    print(f"2 J^T L J vs finite differences of the gradient: {np.abs(H - want).max() / np.abs(want).max():.3e}")
    assert np.abs(H - want).max() < 1e-5 * np.abs(want).max()
    assert np.abs(H[:6, 6:] - Cb).max() < 1e-5 * np.abs(Cb).max()


def test_host_normalisation_map_leaves_the_factor_energy_unchanged(orc):
    """prior_cases.rotated: R0 != I and s = 2.5.  The library's host map equals the numpy map and the factor energy of the
    normalised scene against the mapped factors equals that of the scene as given, to 1e-12"""
    sc, f0, fac_w, _, _, _ = rc.case("nf2_gauge_frames_full_information_rotated_world")
    e_world = rr.energy(fac_w, sc)
    sn = sc.copy()
    ok, nrm = sa.normalize_scene_inplace(sn)
    assert ok
    R0 = np.array(list(nrm.R0)).reshape(3, 3)
    assert np.abs(R0 - np.eye(3)).max() > 0.1 and abs(nrm.world_scale - 1) > 0.1
    ref = rr.normalised(fac_w, nrm)
    zn, ln = B.normalize_relative_pose_factors(nrm, fac_w.z, rr.tri21(fac_w.info))
    assert np.abs(zn - ref.z).max() < 1e-13 * np.abs(ref.z).max()
    assert np.abs(ln - rr.tri21(ref.info)).max() < 1e-13 * np.abs(ref.info).max()
    lib = rr.Factors(fac_w.a, fac_w.b, fac_w.Z, zn, rr.full(ln))
    e_n = rr.energy(lib, sn)
    print(f"factor energy as given {e_world}, normalised {e_n}")
    assert e_world > 0 and e_n == pytest.approx(e_world, rel=1e-12)
    ident = B.Normalizer()
    ident.R0[0] = ident.R0[4] = ident.R0[8] = 1.0
    ident.world_scale = 1.0
    z2, l2 = B.normalize_relative_pose_factors(ident, fac_w.z, rr.tri21(fac_w.info))
    assert np.array_equal(z2, fac_w.z) and np.array_equal(l2, rr.tri21(fac_w.info))
    # relative_pose(): the library's helper is the yardstick's
    Z, z = B.relative_pose(sc, 1, 4)
    Zr, zr = rr.relative_pose(sc, 1, 4)
    assert np.abs(Z - Zr).max() < 1e-14 and np.abs(z - zr).max() < 1e-13 * max(1.0, np.abs(zr).max())


# ------------------------------------------------------------------ the setter's checks (host only)

def _check(a, b, Z, z, L):
    arrs = [np.ascontiguousarray(np.asarray(a, np.int32)), np.ascontiguousarray(np.asarray(b, np.int32)),
            np.ascontiguousarray(np.asarray(Z, np.float64)), np.ascontiguousarray(np.asarray(z, np.float64)),
            np.ascontiguousarray(np.asarray(L, np.float64))]
    why = C.c_char_p()
    r = sa.lib().srk_ba_check_relative_pose_factors(C.c_int32(arrs[0].size), *[x.ctypes.data_as(C.c_void_p) for x in arrs], C.byref(why))
    return r, (why.value or b"").decode()


def test_setter_checks():
    sc, f0 = cc.scene("nf2_short_runs")
    fac = rc.factors_for(sc, [(0, 1), (1, 2), (4, 5)], "full")
    good = (fac.a, fac.b, fac.Z.reshape(-1, 9), fac.z, rr.tri21(fac.info))
    assert _check(*good) == (0, "")

    def with_(i, val):
        out = [np.array(x, copy=True) for x in good]
        out[i] = np.asarray(val, dtype=out[i].dtype).reshape(out[i].shape)
        return out

    nan_t = good[3].copy(); nan_t[1, 2] = np.nan
    inf_R = good[2].copy(); inf_R[0, 0] = np.inf
    inf_L = good[4].copy(); inf_L[2, 5] = np.inf
    scaled = good[2].copy(); scaled[1] *= 1 + 1e-8        # not orthogonal to 1e-9
    mirror = good[2].copy(); mirror[2] = np.diag([1.0, 1.0, -1.0]).reshape(9)  # orthogonal, determinant -1
    indefinite = good[4].copy(); indefinite[0] = rr.tri21(np.diag([1.0, 1, 1, 1, 1, -1e-6])[None])[0]
    offdiag = good[4].copy(); Lm = np.eye(6); Lm[0, 5] = Lm[5, 0] = 2.0; offdiag[1] = rr.tri21(Lm[None])[0]  # eigenvalue -1
    bad = {
        "two different frames": (np.array([0, 1, 4]), np.array([1, 1, 5]), *good[2:]),
        "negative": (np.array([-1, 1, 4]), *good[1:]),
        "given twice": (np.array([0, 0, 1]), np.array([1, 1, 2]), *good[2:]),
        "sorted": (np.array([1, 0, 4]), np.array([2, 1, 5]), *good[2:]),
        "translation is not finite": with_(3, nan_t),
        "rotation is not finite": with_(2, inf_R),
        "information matrix is not finite": with_(4, inf_L),
        "not orthogonal": with_(2, scaled),
        "determinant": with_(2, mirror),
        "positive semi-definite": with_(4, indefinite),
        "positive semi-definite ": with_(4, offdiag),
    }
    for what, args in bad.items():
        r, why = _check(*args)
        assert r == -1 and what.strip() in why, (what, why)
    # (b, a) after (a, b) is the same unordered pair
    r, why = _check(np.array([0, 1]), np.array([1, 0]), good[2][:2], good[3][:2], good[4][:2])
    assert r == -1 and "given twice" in why
    # valid: pairs given backwards, an all-zero, a rotation-only and a rank-1 information matrix
    semi = good[4].copy()
    semi[0] = 0
    rot_only = np.zeros((6, 6)); rot_only[3:, 3:] = np.eye(3)
    semi[1] = rr.tri21(rot_only[None])[0]
    n = np.array([1.0, -2.0, 0.5, 0.0, 3.0, -1.0])
    semi[2] = rr.tri21(np.outer(n, n)[None])[0]
    assert _check(np.array([1, 2, 5]), np.array([0, 1, 4]), good[2], good[3], semi) == (0, "")
    assert _check([], [], np.zeros((0, 9)), np.zeros((0, 3)), np.zeros((0, 21)))[0] == 0


def test_relative_pose_information_conversions():
    f0, spx = 600.0, 0.3
    k = (spx / f0) ** 2
    a = B.relative_pose_information(2, sigma_t=0.02, sigma_r=0.001, sigma_pixels=spx, f0=f0)
    La = rr.full(a)
    assert a.shape == (2, 21) and np.allclose(np.diagonal(La, axis1=1, axis2=2), [[k / 4e-4] * 3 + [k / 1e-6] * 3] * 2, rtol=1e-12)
    assert np.count_nonzero(La[0]) == 6
    cov = np.diag([1.0, 2.0, 3.0, 0.1, 0.2, 0.3])
    cov[0, 4] = cov[4, 0] = 0.05
    c = B.relative_pose_information(3, covariance=cov, sigma_pixels=spx, f0=f0)
    assert c.shape == (3, 21) and np.allclose(rr.full(c)[2] @ cov, k * np.eye(6), atol=1e-15)
    d = B.relative_pose_information(2, info=np.eye(6) * 5.0)
    assert np.array_equal(rr.full(d)[1], np.eye(6) * 5.0)
    assert np.array_equal(B.relative_pose_information(2, info=a), a)
    for bad in (dict(n=1, sigma_t=0.02, sigma_r=0.01),                                  # no f0
                dict(n=1, sigma_t=0.02, f0=f0),                                         # sigma_r missing
                dict(n=1, sigma_t=0.0, sigma_r=0.01, f0=f0),                            # a zero sigma
                dict(n=2, info=np.zeros((3, 21))),                                      # three for two
                dict(n=1, covariance=np.diag([1.0, 1, 1, 1, 1, -1]), f0=f0),            # indefinite
                dict(n=1, info=np.zeros((6, 5)))):
        with pytest.raises(ValueError):
            B.relative_pose_information(**bad)


def test_symbols_are_exported_and_null_handles_are_refused():
    L = sa.lib()
    for name in ("srk_ba_set_relative_pose_factors", "srk_ba_check_relative_pose_factors", "srk_ba_relative_pose_factor_count",
                 "srk_ba_relative_pose_factors", "srk_ba_relative_pose_error", "srk_ba_relative_pose_residuals",
                 "srk_ba_normalize_relative_pose_factors", "srk_ba_relative_pose_pass_ms"):
        assert hasattr(L, name), name
    assert L.srk_ba_set_relative_pose_factors(None, C.c_int32(0), None, None, None, None, None) == -1
    assert L.srk_ba_relative_pose_factor_count(None, None) == -1
    assert L.srk_ba_relative_pose_factors(None, None, None, None, None, None) == -1
    assert L.srk_ba_relative_pose_error(None, None) == -3      # SRK_E_STATE
    assert L.srk_ba_relative_pose_residuals(None, None) == -3
    assert L.srk_ba_relative_pose_pass_ms(None, None, None, None) == -3
    x = np.zeros(3)
    assert L.srk_ba_normalize_relative_pose_factors(None, C.c_int32(1), x.ctypes.data_as(C.c_void_p), None, x.ctypes.data_as(C.c_void_p), None) == -1


# ------------------------------------------------------------------ the planner with pairs (host only)

@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("relpose_plan") / "test_relpose_plan"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_relpose_plan.cpp"),
                        os.path.join(CSRC, "srk_plan.cpp"), "-pthread", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr

    def run(M, window, mode, pairs=()):
        r = subprocess.run([str(exe), str(M), str(window), str(mode), *[str(x) for p in pairs for x in p]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = {}
        for line in r.stdout.splitlines():
            w = line.split()
            out[w[0]] = w[1] if w[0] == "digest" else [int(x) for x in w[1:]]
        out["min_cv"] = np.array(out["min_cv"])
        out["pairs"] = np.array(out.get("pairs", []), dtype=np.int64).reshape(-1, 2)
        out["fill"] = int(np.sum(np.arange(M) - out["min_cv"] + 1))  # block entries of the lower triangle inside the envelope
        return out
    return run


def test_planner_consecutive_pairs_inside_the_window_leave_the_plan_alone(plan):
    M, window = 40, 6
    none = plan(M, window, -1)
    chain = plan(M, window, -1, rc.chain(M) + [(3, 7), (20, 16)])
    assert np.array_equal(none["min_cv"], np.maximum(0, np.arange(M) - (window - 1)))
    assert np.array_equal(chain["min_cv"], none["min_cv"]) and chain["digest"] == none["digest"]
    assert chain["renumbered"] == none["renumbered"] == [0] and chain["fill"] == none["fill"]


def test_planner_far_pair_lowers_min_cv_and_keeps_every_other_table(plan):
    M, window = 40, 6
    none = plan(M, window, 0)
    for pair in ((2, 39), (39, 2)):  # either direction
        far = plan(M, window, 0, [pair])
        want = none["min_cv"].copy()
        want[39] = 2
        assert np.array_equal(far["min_cv"], want) and far["fill"] == none["fill"] + (39 - window + 1) - 2
        assert far["renumbered"] == [0] and far["digest"] == none["digest"]  # the pair touches the skyline alone
    two = plan(M, window, 0, [(2, 39), (10, 30)])
    want = none["min_cv"].copy()
    want[39], want[30] = 2, 10
    assert np.array_equal(two["min_cv"], want)


def test_planner_renumbering_sees_the_pairs(plan):
    """automatic mode: a loop closure between the ends of a banded sequence makes the caller's order far from banded, so the
    graph with the pair is renumbered (a ring: the band roughly doubles, instead of one row spanning everything) and min_cv
    covers the pair in the internal numbering; the same scene without the pair keeps the caller's order.  Mode 0 keeps the
    order with the pair as well."""
    M, window = 60, 6
    none = plan(M, window, -1)
    loop = plan(M, window, -1, [(0, 59)])
    assert none["renumbered"] == [0] and loop["renumbered"] == [1]
    a, b = loop["pairs"][0]
    hi, lo = max(a, b), min(a, b)
    assert loop["min_cv"][hi] <= lo
    band = lambda p: int(np.max(np.arange(M) - p["min_cv"]))
    print(f"band without the pair {band(none)}, with it renumbered {band(loop)}, kept {band(plan(M, window, 0, [(0, 59)]))}")
    assert band(none) == window - 1 and band(loop) <= 3 * window and band(plan(M, window, 0, [(0, 59)])) == 59


# ------------------------------------------------------------------ conditioning of every compared case

def _system(orc, name, c, weighted=False, with_factors=True):
    sc, f0, fac_w, fv, fconst, keep_gauge = rc.case(name)
    so, nrm = _orc_scene(orc, sc)
    fac = rr.normalised(fac_w, nrm) if with_factors else rr.Factors()
    base = wr.derivatives(f0, so, cc.information(sc), wr.HUBER, 1.0)[:4] if weighted else orc.derivatives(f0, so)
    pconst = np.zeros(so.N, dtype=bool)
    g, V, U, W = kref.restrict_all(so, rr.add_terms(base, so, fac), fconst, pconst, fv)
    S, _, _ = kref.schur(so, g, V, U, W, c)
    rr.add_couplings(S, fac, so)
    return S, kref.fixed_vars(so.M, fconst, keep_gauge, fv), V


@pytest.mark.parametrize("c", [1e-4, 1e-1])
@pytest.mark.parametrize("name", list(rc.CASES) + list(rc.SWEEP_CASES))
def test_every_gpu_case_is_positive_definite_and_well_conditioned(orc, name, c):
    """np.linalg.cholesky of the reference system's free part succeeds and its condition number after symmetric diagonal
    scaling is below 1e10, for every case the GPU tests use, the loss + information variant of the mode case and the cases
    over the whole range of residual angles (relpose_cases.SWEEP_CASES, half a turn among them) included"""
    for weighted in (False, True) if name == rc.MODE_CASE else (False,):
        S, fixed, V = _system(orc, name, c, weighted)
        cond = kref.system_check(S, fixed, 1e10)
        print(f"{name} c={c:g}{' (loss + information)' if weighted else ''}: cond {cond:.3e}")
        E = V.copy()
        E[:, np.arange(3), np.arange(3)] *= 1 + c
        assert np.all(np.linalg.det(E) > 0)


def _distance(s, pts_gt, R_gt, T_gt):
    return max(float(np.abs(s.cam_T - T_gt).max()), float(np.abs(s.cam_R - R_gt).max()), float(np.abs(s.points - pts_gt).max()))


METRIC_ITERATIONS = 12


def test_metric_scale_case_is_singular_in_scale_without_its_factors_and_the_python_loop_returns_to_ground_truth(orc):
    """Undamped (c = 0), frame 0 constant and the reference's gauge released: without the factors the system has the scale as
    a null vector (condition above 1e12 after diagonal scaling); with them it is positive definite, below 1e10 at both damping
    factors.  The reprojection sum is blind to the 2 % scale, the factor sum is not.  The Python loop's distance from the
    ground truth is computed and printed here: the GPU test recomputes it and takes ten times that value as its bound."""
    spec, sc, fac_w, fconst, pts_gt, R_gt, T_gt = rc.metric_scale()
    so, nrm = _orc_scene(orc, sc)
    fac = rr.normalised(fac_w, nrm)
    e_obs, e_fac = orc.reproj_error(spec.f0, so)[0], rr.energy(fac, so)
    print(f"metric scale: reprojection sum {e_obs:.3e}, factor sum {e_fac:.3e}, start {_distance(sc, pts_gt, R_gt, T_gt):.3e} from the ground truth")
    assert e_obs < 1e-20 and e_fac > 1e-6
    pconst = np.zeros(so.N, dtype=bool)
    fixed = kref.fixed_vars(so.M, fconst, 0, 6)
    base = orc.derivatives(spec.f0, so)
    g, V, U, W = kref.restrict_all(so, base, fconst, pconst, 6)
    S, _, _ = kref.schur(so, g, V, U, W, 0.0)
    free = np.flatnonzero(~fixed)
    A = S[np.ix_(free, free)]
    A = 0.5 * (A + A.T)
    d = np.sqrt(np.abs(np.diag(A)))
    cond0 = float(np.linalg.cond(A / d[:, None] / d[None, :]))
    g, V, U, W = kref.restrict_all(so, rr.add_terms(base, so, fac), fconst, pconst, 6)
    conds = []
    for c in (0.0, 1e-4, 1e-1):
        S, _, _ = kref.schur(so, g, V, U, W, c)
        rr.add_couplings(S, fac, so)
        conds.append(kref.system_check(S, fixed, 1e12 if c == 0 else 1e10))
    print(f"cond without factors {cond0:.3e}; with them {conds[0]:.3e} (c = 0), {conds[1]:.3e}, {conds[2]:.3e}")
    assert cond0 > 1e12
    so2 = orc.Scene(sc.points, sc.cam_R, sc.cam_T, sc.K, sc.shared_k, sc.row_ptr, sc.obs_frame, sc.obs_uv)
    rc_o, rep = rr.compute_inplace(orc, spec.f0, so2, fac_w, 0, 6, fconst=fconst, allowed_err_change=1e-30, max_hessian_factor=1e12,
                                   max_iterations=METRIC_ITERATIONS)
    d_cpu = _distance(so2, pts_gt, R_gt, T_gt)
    print(f"python loop: {rep.iterations} iterations, {rep.attempts} attempts, status {rep.status}, err {rep.err_initial:.3e} -> "
          f"{rep.err_final:.3e}, distance from the ground truth {d_cpu:.3e}")
    assert d_cpu < 1e-6, "the yardstick itself does not return to the ground truth"
