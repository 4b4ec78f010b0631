"""The covariance reference and the host-only entry points, without a GPU: the Schur route of tests/covariance_ref.py against the
inverse of the full Hessian, every case of tests/covariance_cases.py positive definite, the reference's two summation orders
within 16 eps cond of one another (the GPU comparison allows 64 eps cond), and srk_ba_revert_covariances against numpy and
against srk_ba_normalize_position_priors."""
import ctypes as C

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import ba as B
import covariance_cases as vc
import covariance_ref as vref
import prior_cases as pc
import prior_ref as pref

COMPARED = [(n, c) for n in vc.CASES for c in vc.dampings(n)]


@pytest.mark.parametrize("name", vc.DENSE_CASES)
def test_schur_route_equals_full_hessian_route(orc, name):
    for c in vc.dampings(name):
        a = vc.reference(orc, name, c)
        b = vc.reference(orc, name, c, dense=True)
        tol = 16 * vref.EPS * a["cond"]
        ef, ep = vref.block_err(a["FB"], b["FB"]), vref.block_err(a["PB"], b["PB"])
        print(f"\n{name} c={c:g}: cond {a['cond']:.3e}, frames {ef:.3e}, landmarks {ep:.3e} (16 eps cond = {tol:.3e})")
        assert ef < tol and ep < tol


@pytest.mark.parametrize("name,c", COMPARED)
def test_cases_positive_definite_and_summation_orders_agree(orc, name, c):
    a = vc.reference(orc, name, c)  # spd_inverse raises when the free part of S is not positive definite
    b = vc.reference(orc, name, c, reverse=True)
    k = vc.case(name)
    tol = 16 * vref.EPS * a["cond"]
    ef = vref.block_err(b["FB"][k.frames], a["FB"][k.frames])
    ep = vref.block_err(b["PB"][k.points], a["PB"][k.points])
    print(f"\n{name} c={c:g}: cond {a['cond']:.3e}, orders differ by {max(ef, ep) / (vref.EPS * a['cond']):.2f} eps cond")
    assert ef < tol and ep < tol
    # every selected block is positive semi-definite with zero rows exactly where a variable is fixed, and symmetric
    for blk in list(a["FB"][k.frames]) + list(a["PB"][k.points]):
        assert np.array_equal(blk, blk.T) or np.abs(blk - blk.T).max() <= 4 * vref.EPS * np.abs(blk).max()
        d = np.diag(blk)
        live = d > 0
        assert np.all(d >= 0) and np.all(blk[~live] == 0) and np.all(blk[:, ~live] == 0)
        if live.any():
            s = blk[np.ix_(live, live)] / np.sqrt(np.outer(d[live], d[live]))
            assert np.linalg.eigvalsh(0.5 * (s + s.T)).min() > -1e-9
    # the fixed variables of the gauge frames: frame 0 all zeros, frame 1 one zero row and column
    if k.keep_gauge and not k.fconst[:2].any():
        off = 10 - k.fv
        assert np.all(a["FB"][0][4 - off:, :] == 0) and np.all(a["FB"][0][:, 4 - off:] == 0)  # the pose part; intrinsics move
        z = np.flatnonzero(np.diag(a["FB"][1]) == 0)
        assert list(z) == [4 - off + 1]


def _normalizer(seed=3):
    rs = np.random.RandomState(seed)
    nrm = sa.ba.Normalizer()
    R0 = pc.rodrigues(rs.uniform(-1, 1, size=3))
    for i, v in enumerate(R0.reshape(-1)):
        nrm.R0[i] = float(v)
    for i, v in enumerate(rs.uniform(-2, 2, size=3)):
        nrm.T0[i] = float(v)
    nrm.world_scale = 1.7
    return nrm


def _spd(rs, n, m):
    A = rs.uniform(-1, 1, size=(n, m, m))
    return np.einsum("nab,ncb->nac", A, A) + 0.5 * np.eye(m)


@pytest.mark.parametrize("fv", [6, 10])
def test_revert_covariances_equals_numpy_map(fv):
    rs = np.random.RandomState(fv)
    nrm = _normalizer()
    FB, PB = _spd(rs, 5, fv), _spd(rs, 7, 3)
    fo, po = B.revert_covariances(nrm, FB, PB)
    fr, pr = vref.revert(nrm, FB, PB)
    assert np.abs(fo - fr).max() < 1e-14 * np.abs(fr).max() and np.abs(po - pr).max() < 1e-14 * np.abs(pr).max()
    assert np.array_equal(fo, fo.transpose(0, 2, 1)) and np.array_equal(po, po.transpose(0, 2, 1))
    if fv == 10:  # the intrinsic block itself is untouched
        assert np.abs(fo[:, :4, :4] - FB[:, :4, :4]).max() < 1e-15
    # either kind on its own
    f1, p1 = B.revert_covariances(nrm, FB, None)
    f2, p2 = B.revert_covariances(nrm, None, PB)
    assert p1 is None and f2 is None and np.array_equal(f1, fo) and np.array_equal(p2, po)


def test_revert_covariances_inverts_the_prior_map():
    """an information matrix L through srk_ba_normalize_position_priors gives L_n; the covariance L_n^-1 reverted is L^-1"""
    rs = np.random.RandomState(1)
    nrm = _normalizer(5)
    L = _spd(rs, 6, 3)
    _, Ln6 = B.normalize_position_priors(nrm, np.zeros((6, 3)), pref.six(L))
    _, Sig = B.revert_covariances(nrm, None, np.linalg.inv(pref.full(Ln6)))
    assert np.abs(np.einsum("nab,nbc->nac", Sig, L) - np.eye(3)).max() < 1e-13


def test_argument_errors_without_a_device():
    L = sa.lib()
    nrm = _normalizer()
    blk = np.zeros((1, 6, 6))
    p = blk.ctypes.data_as(C.c_void_p)
    assert L.srk_ba_revert_covariances(None, 6, 1, p, 0, None) == -1
    assert L.srk_ba_revert_covariances(C.byref(nrm), 7, 1, p, 0, None) == -1
    assert L.srk_ba_revert_covariances(C.byref(nrm), 6, 1, None, 0, None) == -1
    assert L.srk_ba_revert_covariances(C.byref(nrm), 6, 0, None, 2, None) == -1
    assert L.srk_ba_revert_covariances(C.byref(nrm), 6, -1, p, 0, None) == -1
    assert L.srk_ba_revert_covariances(C.byref(nrm), 6, 0, None, 0, None) == 0
    # without a handle there is no scene
    assert L.srk_ba_phase_covariance(None, 0, None, None, 0, None, None) == -3
    assert L.srk_ba_covariances(None, C.c_double(1.0), 0, None, None, 0, None, None, 1) == -3
    assert L.srk_ba_set_covariance_batch(None, 96) == -1
