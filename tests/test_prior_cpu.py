"""Position priors without a device: the yardstick's added terms against finite differences of the objective, the host
normalisation map, the conditioning of every case the GPU tests compare, and the argument checks that need no GPU."""
import ctypes as C

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import ba as B
import constant_cases as cc
import constant_ref as kref
import prior_cases as pc
import prior_ref as pref
import weighted_ref as wr


def _orc_scene(orc, sc, normalise=True):
    so = orc.Scene(sc.points, sc.cam_R, sc.cam_T, sc.K, sc.shared_k, sc.row_ptr, sc.obs_frame, sc.obs_uv)
    nrm = None
    if normalise:
        ok, nrm = orc.normalize(so)
        assert ok
    return so, nrm


def _total(orc, f0, so, pri):
    return orc.reproj_error(f0, so)[0] + sum(pref.energy(pri, so))


def _fd(orc, f0, so, pri, var, eps):
    """central differences of E along one variable of the correction vector, through orc.apply_corrections: (E', E'')"""
    e = []
    for sgn in (1.0, 0.0, -1.0):
        s2 = so.copy()
        corr = np.zeros(3 * so.N + 10 * so.M)
        corr[var] = sgn * eps
        orc.apply_corrections(s2, corr)
        e.append(_total(orc, f0, s2, pri))
    return (e[0] - e[2]) / (2 * eps), (e[0] - 2 * e[1] + e[2]) / eps ** 2


def test_added_terms_agree_with_finite_differences(orc):
    """The prior's share of gradient and block diagonal, added terms minus the oracle's own, against the same difference of
    central finite differences of reproj_error + prior energy and of reproj_error alone -- so the oracle's Gauss-Newton
    approximation of the reprojection part drops out and what is compared is the prior's exact quadratic.  For a landmark,
    for a frame's T variables, and for a frame's W variables, where the centre prior must contribute nothing."""
    sc, f0, pri_w, _, _ = pc.case(pc.MODE_CASE)
    so, nrm = _orc_scene(orc, sc)
    pri = pref.normalised(pri_w, nrm)
    none = pref.Priors()
    base = orc.derivatives(f0, so)
    g, V, U, _ = pref.add_terms(base, so, pri)
    N = so.N
    i, j = int(pri.pidx[3]), int(pri.fidx[1])
    eps = 1e-4
    # the quadratic is exact in a landmark and in T; central differences of it carry rounding only: E ~ 1e-3, eps = 1e-4, so
    # the first difference is good to 1e-16 * 1e-3 / 1e-4 ~ 1e-15 absolute and the second to 1e-16 * 1e-3 / 1e-8 ~ 1e-11,
    # times the cancellation of two evaluations of the reprojection part that differ by its third derivatives: 1e-6 relative
    for what, var, gi, Hii in [("landmark", 3 * i + a, g[3 * i + a] - base[0][3 * i + a], V[i, a, a] - base[1][i, a, a]) for a in range(3)] + \
                              [("T", 3 * N + 10 * j + 4 + a, g[3 * N + 10 * j + 4 + a] - base[0][3 * N + 10 * j + 4 + a],
                                U[j, 4 + a, 4 + a] - base[2][j, 4 + a, 4 + a]) for a in range(3)]:
        d1, d2 = _fd(orc, f0, so, pri, var, eps)
        b1, b2 = _fd(orc, f0, so, none, var, eps)
        print(f"{what} var {var}: gradient term {gi:.6e} fd {d1 - b1:.6e}; block term {Hii:.6e} fd {d2 - b2:.6e}")
        assert gi != 0 and Hii > 0
        assert d1 - b1 == pytest.approx(gi, rel=1e-6)
        assert d2 - b2 == pytest.approx(Hii, rel=1e-5)  # E'' = 2 L_aa, the factor-2 convention of second_deriv
    for a in range(3):  # W: the rotation update leaves the centre alone
        var = 3 * N + 10 * j + 7 + a
        assert g[var] == base[0][var] and np.array_equal(U[j, 7:, :], base[2][j, 7:, :])
        s2 = so.copy()
        corr = np.zeros(3 * N + 10 * so.M)
        corr[var] = 1e-2
        orc.apply_corrections(s2, corr)
        assert np.abs(s2.cam_R[j] - so.cam_R[j]).max() > 1e-3
        assert np.abs(pref.centres(s2)[j] - pref.centres(so)[j]).max() < 1e-14
        assert pref.energy(pri, s2)[1] == pytest.approx(pref.energy(pri, so)[1], rel=1e-10)
    # off-diagonal entries of the added blocks: a full information matrix, mixed second differences of the prior energy
    sc, f0, pri_w, _, _ = pc.case("nf2_full_information_rotated_world")
    so, nrm = _orc_scene(orc, sc)
    pri = pref.normalised(pri_w, nrm)
    i = int(pri.pidx[2])
    k = 2
    h = 1e-3
    for a, b in ((0, 1), (0, 2), (1, 2)):
        e = {}
        for sa_, sb in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            s2 = so.copy()
            s2.points[i, a] += sa_ * h
            s2.points[i, b] += sb * h
            e[(sa_, sb)] = pref.energy(pri, s2)[0]
        mixed = (e[(1, 1)] - e[(1, -1)] - e[(-1, 1)] + e[(-1, -1)]) / (4 * h * h)
        assert mixed == pytest.approx(2 * pri.pinfo[k, a, b], rel=1e-6) and pri.pinfo[k, a, b] != 0


def test_host_normalisation_map_leaves_the_prior_energy_unchanged(orc):
    """on a scene whose frame 0 is not the identity and whose scale is not 1: the library's host map equals the numpy map, and
    the prior energy of the normalised scene against the mapped priors equals that of the scene as given, to 1e-12"""
    sc, f0, pri_w, _, _ = pc.case("nf16_full_information_rotated_world_free_gauge")
    e_world = pref.energy(pri_w, sc)
    sn = sc.copy()
    ok, nrm = sa.normalize_scene_inplace(sn)
    assert ok
    R0 = np.array(list(nrm.R0)).reshape(3, 3)
    assert np.abs(R0 - np.eye(3)).max() > 0.1 and abs(nrm.world_scale - 1) > 0.1
    ref = pref.normalised(pri_w, nrm)
    pp, pl = B.normalize_position_priors(nrm, pri_w.ppos, pref.six(pri_w.pinfo))
    fp, fl = B.normalize_position_priors(nrm, pri_w.fpos, pref.six(pri_w.finfo))
    assert np.abs(pp - ref.ppos).max() < 1e-13 * np.abs(ref.ppos).max()
    assert np.abs(pl - pref.six(ref.pinfo)).max() < 1e-13 * np.abs(ref.pinfo).max()
    assert np.abs(fp - ref.fpos).max() < 1e-13 * np.abs(ref.fpos).max()
    assert np.abs(fl - pref.six(ref.finfo)).max() < 1e-13 * np.abs(ref.finfo).max()
    lib = pref.Priors(pri_w.pidx, pp, pref.full(pl), pri_w.fidx, fp, pref.full(fl))
    e_n = pref.energy(lib, sn)
    print(f"prior energy as given {e_world}, normalised {e_n}")
    assert e_world[0] > 0 and e_world[1] > 0
    assert e_n[0] == pytest.approx(e_world[0], rel=1e-12) and e_n[1] == pytest.approx(e_world[1], rel=1e-12)
    # the identity normaliser is the identity map
    ident = B.Normalizer()
    ident.R0[0] = ident.R0[4] = ident.R0[8] = 1.0
    ident.world_scale = 1.0
    pp2, pl2 = B.normalize_position_priors(ident, pri_w.ppos, pref.six(pri_w.pinfo))
    assert np.array_equal(pp2, pri_w.ppos) and np.array_equal(pl2, pref.six(pri_w.pinfo))


def _system(orc, name, c, weighted=False, with_priors=True, fv=None):
    sc, f0, pri_w, keep_gauge, fv_case = pc.case(name)
    fv = fv or fv_case
    so, nrm = _orc_scene(orc, sc)
    pri = pref.normalised(pri_w, nrm) if with_priors else pref.Priors()
    base = wr.derivatives(f0, so, cc.information(sc), wr.HUBER, 1.0)[:4] if weighted else orc.derivatives(f0, so)
    none = np.zeros(so.M, dtype=bool), np.zeros(so.N, dtype=bool)
    g, V, U, W = kref.restrict_all(so, pref.add_terms(base, so, pri), *none, fv)
    S, _, _ = kref.schur(so, g, V, U, W, c)
    return S, kref.fixed_vars(so.M, none[0], keep_gauge, fv), V


@pytest.mark.parametrize("c", [1e-4, 1e-1])
@pytest.mark.parametrize("name", list(pc.CASES))
def test_every_gpu_case_is_positive_definite_and_well_conditioned(orc, name, c):
    """np.linalg.cholesky of the reference system's free part succeeds and its condition number after symmetric diagonal
    scaling is below 1e10 (the condition tests/test_constant_cpu.py imposes), for every case the GPU tests use, the loss +
    information variant of the mode case included"""
    for weighted, fv in ((False, None), (True, None)) if name == pc.MODE_CASE else ((False, None), (False, 6)) if name == pc.TWO_KERNEL_CASE else ((False, None),):
        S, fixed, V = _system(orc, name, c, weighted, fv=fv)
        cond = kref.system_check(S, fixed, 1e10)
        print(f"{name} c={c:g}{' (loss + information)' if weighted else ''}: cond {cond:.3e}")
        E = V.copy()
        E[:, np.arange(3), np.arange(3)] *= 1 + c
        assert np.all(np.linalg.det(E) > 0)


@pytest.mark.parametrize("c", [1e-4, 1e-1])
def test_constant_block_combination_is_positive_definite_and_well_conditioned(orc, c):
    """the same condition for the mode case together with the constant blocks of
    test_prior_on_a_constant_block_adds_a_constant_to_the_error_and_nothing_else"""
    sc, f0, pri_w, keep_gauge, fv = pc.case(pc.MODE_CASE)
    fconst, pconst = pc.constant_combination(sc, pri_w)
    so, nrm = _orc_scene(orc, sc)
    pri = pref.normalised(pri_w, nrm)
    g, V, U, W = kref.restrict_all(so, pref.add_terms(orc.derivatives(f0, so), so, pri), fconst, pconst, fv)
    S, _, _ = kref.schur(so, g, V, U, W, c)
    print(f"constant combination c={c:g}: cond {kref.system_check(S, kref.fixed_vars(so.M, fconst, keep_gauge, fv), 1e10):.3e}")


@pytest.mark.parametrize("name", pc.FREE_GAUGE_CASES)
def test_free_gauge_cases_are_singular_without_their_priors(orc, name):
    """keep_gauge = 0: without the priors the undamped system (c = 0; the damping c diag(H) alone would regularise it to about
    1 / c) has the seven gauge directions as null vectors, condition above 1e12 after diagonal scaling; with the priors it is
    positive definite with a condition below that, undamped as well"""
    S, fixed, _ = _system(orc, name, 0.0, with_priors=False)
    free = np.flatnonzero(~fixed)
    A = S[np.ix_(free, free)]
    A = 0.5 * (A + A.T)
    d = np.sqrt(np.abs(np.diag(A)))
    cond = float(np.linalg.cond(A / d[:, None] / d[None, :]))
    # (the undamped ten-variable system is poorly scaled in its intrinsics with any gauge; the bound of 1e10 is imposed at the
    # damping factors the GPU tests compare, in the test above.  Here: on the regular side of what counts as singular.)
    S2, fixed2, _ = _system(orc, name, 0.0)
    cond2 = kref.system_check(S2, fixed2, 1e12)
    print(f"{name}: cond without priors {cond:.3e}, with {cond2:.3e}")
    assert cond > 1e12


def test_georeferencing_case_is_regular_and_its_two_sums_start_within_a_factor_100(orc):
    spec, sc, pri_w = pc.georeferencing()[:3]
    so, nrm = _orc_scene(orc, sc)
    pri = pref.normalised(pri_w, nrm)
    e_obs, e_pri = orc.reproj_error(spec.f0, so)[0], sum(pref.energy(pri, so))
    print(f"georeferencing: reprojection sum {e_obs:.3e}, prior sum {e_pri:.3e} (L = {pc.L_GEOREF})")
    assert 0.01 < e_pri / e_obs < 100
    none = np.zeros(so.M, dtype=bool), np.zeros(so.N, dtype=bool)
    for c in (1e-4, 1e-1):
        g, V, U, W = kref.restrict_all(so, pref.add_terms(orc.derivatives(spec.f0, so), so, pri), *none, 6)
        S, _, _ = kref.schur(so, g, V, U, W, c)
        print(f"georeferencing c={c:g}: cond {kref.system_check(S, kref.fixed_vars(so.M, none[0], 0, 6), 1e10):.3e}")


# ------------------------------------------------------------------ the Python conversions, the C ABI without a device

def test_prior_information_conversions():
    f0, spx = 600.0, 0.3
    k = (spx / f0) ** 2
    a = B.prior_information(0.02, n=2, sigma_pixels=spx, f0=f0)
    assert a.shape == (2, 6) and np.allclose(a, [[k / 4e-4, 0, 0, k / 4e-4, 0, k / 4e-4]] * 2, rtol=1e-12)
    b = B.prior_information([[1.0, 1.0, 3.0]], n=1, sigma_pixels=spx, f0=f0)
    assert np.allclose(b, [[k, 0, 0, k, 0, k / 9]], rtol=1e-12)
    assert np.array_equal(B.prior_information([1.0, 1.0, 3.0], n=4, sigma_pixels=spx, f0=f0), np.repeat(b, 4, axis=0))
    # per-axis sigmas of THREE priors are [3][3]: sigmas, never one covariance for all
    sg = np.array([[1.0, 2.0, 3.0], [0.5, 0.25, 4.0], [2.0, 2.0, 1.0]])
    s3 = B.prior_information(sg, n=3, sigma_pixels=spx, f0=f0)
    assert s3.shape == (3, 6) and np.allclose(s3[:, [0, 3, 5]], k / sg ** 2, rtol=1e-12) and np.all(s3[:, [1, 2, 4]] == 0)
    cov = np.array([[[2.0, 0.5, 0.0], [0.5, 1.0, 0.2], [0.0, 0.2, 3.0]]])
    c = B.prior_information(cov, n=1, sigma_pixels=spx, f0=f0)
    assert np.allclose(pref.full(c)[0] @ cov[0], k * np.eye(3), atol=1e-15)
    c3 = B.prior_information(cov, n=3, sigma_pixels=spx, f0=f0)  # one covariance for all goes in as [1][3][3]
    assert c3.shape == (3, 6) and np.array_equal(c3, np.repeat(c, 3, axis=0))
    d = B.prior_information(n=3, info=np.eye(3)[None] * 5.0)
    assert d.shape == (3, 6) and np.array_equal(d[2], [5, 0, 0, 5, 0, 5])
    assert np.array_equal(B.prior_information(n=2, info=[[1, 0, 0, 2, 0, 3], [4, 0, 0, 5, 0, 6]]), [[1, 0, 0, 2, 0, 3], [4, 0, 0, 5, 0, 6]])
    for bad in (dict(spec=0.02, n=1),                                               # a sigma without sigma_pixels / f0
                dict(spec=sg, n=2, sigma_pixels=spx, f0=f0),                        # three rows for two priors
                dict(spec=np.array([[[1.0, 2.0, 0], [0, 1.0, 0], [0, 0, 1.0]]]), n=1, sigma_pixels=spx, f0=f0),  # not symmetric
                dict(spec=np.array([[[1.0, 2.0, 0], [2.0, 1.0, 0], [0, 0, 1.0]]]), n=1, sigma_pixels=spx, f0=f0),  # indefinite
                dict(spec=[1.0, 0.0, 1.0], n=1, sigma_pixels=spx, f0=f0),           # a zero sigma
                dict(n=3, info=np.eye(3))):                                         # a bare [3][3] is neither [n][6] nor [n][3][3]
        with pytest.raises(ValueError):
            B.prior_information(**bad)


def test_symbols_are_exported_and_null_handles_are_refused():
    L = sa.lib()
    for name in ("srk_ba_set_position_priors", "srk_ba_position_prior_counts", "srk_ba_position_priors", "srk_ba_prior_error",
                 "srk_ba_prior_residuals", "srk_ba_normalize_position_priors", "srk_ba_prior_pass_ms"):
        assert hasattr(L, name), name
    assert L.srk_ba_set_position_priors(None, C.c_int64(0), None, None, None, C.c_int32(0), None, None, None, C.c_int(1)) == -1
    assert L.srk_ba_position_prior_counts(None, None, None) == -1
    assert L.srk_ba_position_priors(None, None, None, None, None, None, None, None) == -1
    assert L.srk_ba_prior_error(None, None, None) == -3      # SRK_E_STATE
    assert L.srk_ba_prior_residuals(None, None, None) == -3
    assert L.srk_ba_prior_pass_ms(None, None, None) == -3
    x = np.zeros(3)
    assert L.srk_ba_normalize_position_priors(None, C.c_int64(1), x.ctypes.data_as(C.c_void_p), None, x.ctypes.data_as(C.c_void_p), None) == -1
