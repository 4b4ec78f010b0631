"""Cross-covariances between blocks and relative-pose covariances on the GPU (srk_ba_phase_cross_covariance,
srk_ba_cross_covariances, srk_ba_relative_pose_covariances) against the numpy reference of tests/cross_covariance_ref.py on the
cases of tests/cross_covariance_cases.py (each checked by tests/test_cross_covariance_cpu.py).

Metric of a cross block: max |a - b| / sqrt(ref_pp,ii ref_qq,jj), the denominators being the reference's marginal diagonals of the
two blocks (|Sigma_ij| <= sqrt(Sigma_ii Sigma_jj)); an entry whose denominator is 0 must be an exact 0.  Bound: 64 eps
cond_scaled(S_free), section 16's, carried across blocks; the reference's own summation orders differ by at most 2.95 eps cond
(tests/test_cross_covariance_cpu.py allows 16).  Every compared case asserts that the reference's largest |correlation| among
the requested off-diagonal blocks exceeds 1e-3, so that a zero block cannot pass.

A relative-pose covariance is a sum of entries of the joint covariance S of the two frames' pose variables weighted by the
Jacobian J = [J_a J_b]; every entry of S is allowed 64 eps cond sqrt(S_kk S_ll), so entry (i, j) of J S J^T is allowed
64 eps cond g_i g_j with g = |J| sqrt(diag S).  The poses J is formed from are rounded themselves (an entry of J that is zero in
exact arithmetic, as between the gauge frames, is 0 in one computation and 1e-17 in another; the library forms J from the
resident scene, the reference from its own normalisation): with |J_ik| <= 1 + |d| that moves an entry by up to a few
eps G^2, G = (1 + |d|) sum_k sqrt(S_kk); 16 eps G^2 is allowed on top.  _relpose_err returns the largest difference as a
fraction of this allowance.

Three properties hold to the bit: a pair (p, p) returns what srk_ba_phase_covariance returns for p; block (q, p) is the transpose
of block (p, q); a pair's result does not depend on the batch cap or on the other pairs of the call.  The second is checked
inside one call in every staged case.  The first and the third compare two calls, i.e. two builds of the system, which have
the same bits in deterministic mode only -- and that mode exists with ten variables a frame only (fixed intrinsics refuse it):
they run on the ten-variable cases, shapes (10, 10), (3, 10) and (3, 3); the six-variable instantiations are the same template.
The measured errors are in DESIGN.md section 17."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import surikatoko_amd as sa
import cross_covariance_cases as xc
import covariance_ref as vref
import cross_covariance_ref as xref
import prior_cases as pc
import relpose_ref as rref
from gpu_common import handle as _handle

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

STAGED = [(n, c) for n in xc.CASES for c in xc.dampings(n)]


def _staged(gpu, k, c, ff=None, pf=None, pp=None):
    gpu.phase_derivatives()
    gpu.phase_schur(c)
    return gpu.phase_cross_covariance(k.ff if ff is None else ff, k.pf if pf is None else pf, k.pp if pp is None else pp)


def _transposes_and_repeats(k, got):
    """to the bit: block (q, p) is the transpose of block (p, q), a repeated pair repeats its block, (p, p) is symmetric"""
    FF, _, PP = got
    n = 0
    for pairs, blocks in ((k.ff, FF), (k.pp, PP)):
        first = {}
        for idx, (a, b) in enumerate(pairs.tolist()):
            if (a, b) in first:
                assert np.array_equal(blocks[idx], blocks[first[(a, b)]])
            first.setdefault((a, b), idx)
        for (a, b), idx in first.items():
            if (b, a) in first:
                assert np.array_equal(blocks[idx], blocks[first[(b, a)]].T), (a, b)
                n += 1
    assert n > 4
    return n


def _check(got, orc, name, c, k, what, scale=1.0, lim=None):
    ref, diags = xc.reference_blocks(orc, name, c)
    cond = xc.reference(orc, name, c)["cond"]
    corr = xc.assert_correlated(k, ref, diags)
    e = xc.errors(got, [scale * r for r in ref], [(scale * dp, scale * dq) for dp, dq in diags])  # (asserts the exact zeros)
    lim = xc.bound(cond) if lim is None else lim
    print(f"\n{what}: cond {cond:.3e}, frame x frame off by {e[0]:.3e}, landmark x frame by {e[1]:.3e}, landmark x landmark by "
          f"{e[2]:.3e} (bound {lim:.3e}; {max(e) / (xref.EPS * cond):.2f} eps cond; largest correlations "
          f"{corr[0]:.3f} / {corr[1]:.3f} / {corr[2]:.3f})")
    assert all(np.all(np.isfinite(g)) for g in got)
    assert max(e) < lim
    return e


@pytest.mark.parametrize("name,c", STAGED)
def test_phase_cross_covariance_vs_reference(orc, name, c):
    k = xc.case(name)
    h = _handle(k.fv)
    try:
        xc.configure(h, k)
        assert h.upload(k.f0, k.sc) and h.frame_vars() == k.fv
        got = _staged(h, k, c)
        assert got[0].shape == (len(k.ff), k.fv, k.fv) and got[1].shape == (len(k.pf), 3, k.fv) and got[2].shape == (len(k.pp), 3, 3)
        _check(got, orc, name, c, k, f"{name} c={c:g}")
        _transposes_and_repeats(k, got)
        # pairs with a constant landmark are zero blocks
        assert np.all(got[1][k.pconst[k.pf[:, 0]]] == 0) and np.all(got[2][k.pconst[k.pp[:, 0]] | k.pconst[k.pp[:, 1]]] == 0)
    finally:
        h.close()


@pytest.mark.parametrize("name", ["w8_edges_fv10", "nf16_edges_fv10", "ragged_constant_free_gauge_fv10"])
def test_pair_with_itself_has_the_bits_of_the_marginal_block(name):
    c = 1e-4
    k = xc.case(name)
    h = _handle(k.fv, deterministic=True)
    try:
        xc.configure(h, k)
        assert h.upload(k.f0, k.sc) and h.deterministic()
        h.phase_derivatives()
        h.phase_schur(c)
        FB, PB = h.phase_covariance(k.frames, k.points)
        FF, _, PP = _staged(h, k, c, np.stack([k.frames, k.frames], axis=1), [], np.stack([k.points, k.points], axis=1))
        assert np.array_equal(FF, FB) and np.array_equal(PP, PB) and np.abs(FB).max() > 0 and np.abs(PB).max() > 0
        assert np.array_equal(FF, FF.transpose(0, 2, 1)) and np.array_equal(PP, PP.transpose(0, 2, 1))
    finally:
        h.close()


@pytest.mark.parametrize("name", ["w8_edges_fv10", "ragged_constant_free_gauge_fv10"])
def test_a_pair_does_not_depend_on_the_batch_or_on_the_other_pairs(name):
    c = 1e-4
    k = xc.case(name)
    h = _handle(k.fv, deterministic=True)
    try:
        xc.configure(h, k)
        assert h.upload(k.f0, k.sc) and h.deterministic()
        full = _staged(h, k, c)
        for cap in (20, 96, 1):  # (1: the effective cap is 20 columns)
            h.set_covariance_batch(cap)
            other = _staged(h, k, c)
            assert all(np.array_equal(a, b) for a, b in zip(full, other)), cap
        h.set_covariance_batch(0)
        # every fifth pair alone, in reverse order; one pair alone
        sub = [np.arange(len(p))[::5][::-1] for p in (k.ff, k.pf, k.pp)]
        part = _staged(h, k, c, k.ff[sub[0]], k.pf[sub[1]], k.pp[sub[2]])
        assert all(np.array_equal(a[s], b) for a, s, b in zip(full, sub, part))
        one = _staged(h, k, c, k.ff[1:2], [], [])
        assert np.array_equal(one[0][0], full[0][1]) and one[1].shape == (0, 3, k.fv)
    finally:
        h.close()


@pytest.mark.parametrize("name", ["w8_every_frame_fv6", "nf16_shuffled_fv6", "nf16_factors_fv6"])
def test_cross_covariances_scaled_and_mapped(orc, name):
    """cross_covariances() = the c = 0 blocks times 2 (sigma / f0)^2, mapped by D_p Sigma D_q^T: on the scene in a rotated,
    shifted and scaled world, so that the normalisation has R0 != I and s != 1"""
    k = xc.case(name)
    ref, diags = xc.reference_blocks(orc, name, 0.0)
    cond = xc.reference(orc, name, 0.0)["cond"]
    rot = pc.rotated(k.sc)
    so = orc.Scene(rot.points, rot.cam_R, rot.cam_T, rot.K, rot.shared_k, rot.row_ptr, rot.obs_frame, rot.obs_uv)
    ok, nrm = orc.normalize(so)
    assert ok and abs(nrm.world_scale - 1) > 1e-3 and abs(nrm.R0[0] - 1) > 1e-3
    if k.fac is not None:  # the factors of the case, in the rotated world's units
        k.fac.z = 2.5 * k.fac.z
        D = np.diag([1 / 2.5] * 3 + [1.0] * 3)
        k.fac.info = np.einsum("ab,nbc,cd->nad", D, k.fac.info, D)
    sigma = 0.7
    kf = 2.0 * (sigma / k.f0) ** 2
    h = _handle(k.fv)
    try:
        xc.configure(h, k)
        assert h.upload(k.f0, rot)
        before = [b.copy() for b in (rot.points, rot.cam_R, rot.cam_T)]
        gn = h.cross_covariances(k.ff, k.pf, k.pp, sigma_pixels=sigma, caller_coordinates=False)
        _check(gn, orc, name, 0.0, k, name + " normalised", scale=kf)
        gc = h.cross_covariances(k.ff, k.pf, k.pp, sigma_pixels=sigma)
        e = xref.mapped_errors(gc, [kf * r for r in ref], [(kf * dp, kf * dq) for dp, dq in diags], nrm, k.fv)
        print(f"\n{name} caller's coordinates: off by {e[0]:.3e} / {e[1]:.3e} / {e[2]:.3e} (bound {xc.bound(cond):.3e})")
        assert max(e) < xc.bound(cond)
        assert np.abs(gc[0] - gn[0]).max() > 0 and np.abs(gc[1] - gn[1]).max() > 0 and np.abs(gc[2] - gn[2]).max() > 0  # the map did something
        _transposes_and_repeats(k, gc)  # to the bit in the caller's coordinates as well
        assert all(np.array_equal(a, b) for a, b in zip(before, (rot.points, rot.cam_R, rot.cam_T)))
        with pytest.raises(ValueError):
            h.cross_covariances(k.ff, k.pf, k.pp, sigma_pixels=0.0)
    finally:
        h.close()


def _relpose_err(got, inv, so, pairs, cond, scale=None):
    """the largest |got - ref|_ij as a fraction of its allowance 64 eps cond g_i g_j + 16 eps G^2 (module docstring) over the
    pairs; scale [6]: the units of got relative to the normalised scene's (None = the same)"""
    worst, where = 0.0, None
    o = inv.fv - 6
    _, Cn = rref.poses(so)
    for blk, (a, b) in zip(got, np.asarray(pairs).tolist()):
        ref = xref.relative_pose_covariance(inv, so, a, b)
        Ja, Jb = xref.relative_pose_jacobians(so, a, b)
        d = np.sqrt(np.concatenate([inv.frame_diag(a)[o:], inv.frame_diag(b)[o:]]))
        g = np.abs(np.concatenate([Ja, Jb], axis=1)) @ d
        G = np.full(6, (1 + np.linalg.norm(Cn[b] - Cn[a])) * d.sum())
        if scale is not None:
            ref, g, G = ref * np.outer(scale, scale), g * scale, G * scale
        assert np.array_equal(blk, blk.T) and np.all(np.isfinite(blk))
        e = float((np.abs(blk - ref) / (xc.bound(cond) * np.outer(g, g) + 16 * xref.EPS * np.outer(G, G))).max())
        if not e <= worst:
            worst, where = e, (a, b)
    print(f"\n(worst relative pose: pair {where}, {worst:.3e} of its allowance)")
    return worst


@pytest.mark.parametrize("name", ["w8_every_frame_fv6", "nf16_factors_fv6", "nf16_shuffled_fv6"])
def test_relative_pose_covariances_vs_reference(orc, name):
    k = xc.case(name)
    r = xc.reference(orc, name, 0.0)
    sigma = 0.5
    kf = 2.0 * (sigma / k.f0) ** 2
    pairs = np.concatenate([k.rel, np.stack([np.arange(k.sc.M - 1), np.arange(1, k.sc.M)], axis=1).astype(np.int32)])
    h = _handle(k.fv)
    try:
        xc.configure(h, k)
        assert h.upload(k.f0, k.sc)
        got = h.relative_pose_covariances(pairs, sigma_pixels=sigma)
        s = float(r["nrm"].world_scale)
        unit = np.sqrt(kf) * np.array([1 / s] * 3 + [1.0] * 3)
        e = _relpose_err(got, r["inv"], r["so"], pairs, r["cond"], unit)
        print(f"\n{name}: {len(pairs)} relative poses off by {e:.3e} of the allowance ({64 * e:.2f} eps cond)")
        assert e < 1
        with pytest.raises(ValueError):
            h.relative_pose_covariances([(3, 3)])
        assert h.relative_pose_covariances(np.zeros((0, 2), dtype=np.int32)).shape == (0, 6, 6)
    finally:
        h.close()


def test_relative_pose_covariance_from_a_constant_frame_is_the_marginal_of_the_other(orc):
    """frame a constant, the gauge not kept, relative-pose factors give the scale: S_aa = S_ab = 0 and Sigma_rel = J_b S_bb J_b^T,
    with S_bb from the marginal call, in the caller's coordinates (J_b = diag(R_a, R_b) with the uploaded rotations)"""
    k = xc.case("nf16_factors_fv6")
    a, b = 3, 12
    k.fconst[a] = True
    k.keep_gauge = 0
    r = xc.build_reference(orc, k, 0.0)
    sc = pc.rotated(k.sc)
    k.fac.z = 2.5 * k.fac.z
    D = np.diag([1 / 2.5] * 3 + [1.0] * 3)
    k.fac.info = np.einsum("ab,nbc,cd->nad", D, k.fac.info, D)
    h = _handle(k.fv)
    try:
        xc.configure(h, k)
        assert h.upload(k.f0, sc)
        got = h.relative_pose_covariances([(a, b), (b, a)], sigma_pixels=0.8)
        FB, _ = h.covariances([a, b], [], sigma_pixels=0.8)
        assert np.all(FB[0] == 0) and np.all(np.diag(FB[1]) > 0)
        R = sc.cam_R.reshape(-1, 3, 3)
        for blk, (x, y, sb) in zip(got, ((a, b, FB[1]), (b, a, FB[1]))):
            # the moving frame is b in both orders; as the second frame its Jacobian is diag(R_x, R_y), as the first
            # [[-R_x, R_x [d]x], [0, -R_y]]
            if y == b:
                J = np.zeros((6, 6))
                J[:3, :3], J[3:, 3:] = R[x], R[y]
            else:
                Cx, Cy = -R[x].T @ sc.cam_T[x], -R[y].T @ sc.cam_T[y]
                J = np.zeros((6, 6))
                J[:3, :3], J[:3, 3:], J[3:, 3:] = -R[x], R[x] @ np.array([[0, -(Cy - Cx)[2], (Cy - Cx)[1]], [(Cy - Cx)[2], 0, -(Cy - Cx)[0]],
                                                                            [-(Cy - Cx)[1], (Cy - Cx)[0], 0]]), -R[y]
            ref = J @ sb @ J.T
            g = np.abs(J) @ np.sqrt(np.diag(sb))
            e = float((np.abs(blk - ref) / np.outer(g, g)).max())
            print(f"\nconstant frame {a}, pair ({x}, {y}): off by {e:.3e} (bound {xc.bound(r['cond']):.3e})")
            assert np.array_equal(blk, blk.T) and e < xc.bound(r["cond"])
    finally:
        h.close()


def test_relative_pose_covariance_in_a_rotated_and_scaled_world(orc):
    """the same scene uploaded in a rotated, shifted and scaled world (X' = 2.5 (Q X + t)): the rotation block is unchanged,
    the translation block scaled by the square of the ratio of the world scales, the mixed block by the ratio"""
    name = "w8_every_frame_fv6"
    k = xc.case(name)
    r = xc.reference(orc, name, 0.0)
    pairs = [(40, 41), (10, 60), (69, 2)]
    out = []
    for sc in (k.sc, pc.rotated(k.sc)):
        h = _handle(k.fv)
        try:
            xc.configure(h, k)
            assert h.upload(k.f0, sc)
            out.append(h.relative_pose_covariances(pairs))
        finally:
            h.close()
    # far from the gauge frames the cross term is what matters: the marginal-only figure is several times too large
    h = _handle(k.fv)
    try:
        xc.configure(h, k)
        assert h.upload(k.f0, k.sc)
        FB, _ = h.covariances([40, 41], [], caller_coordinates=False)
    finally:
        h.close()
    Ja, Jb = xref.relative_pose_jacobians(r["so"], 40, 41)
    marg = Ja @ FB[0] @ Ja.T + Jb @ FB[1] @ Jb.T
    assert np.trace(marg[:3, :3]) / float(r["nrm"].world_scale) ** 2 > 4 * np.trace(out[0][0][:3, :3])
    q = np.array([2.5] * 3 + [1.0] * 3)
    s = float(r["nrm"].world_scale)
    unit = np.sqrt(2.0) / k.f0 * np.array([1 / s] * 3 + [1.0] * 3)
    e0 = _relpose_err(out[0], r["inv"], r["so"], pairs, r["cond"], unit)
    e1 = _relpose_err(out[1], r["inv"], r["so"], pairs, r["cond"], unit * q)
    print(f"\nrelative poses: off by {e0:.3e} of the allowance as given, {e1:.3e} in the rotated and scaled world")
    assert e0 < 1 and e1 < 1
    assert np.abs(out[1][:, :3, :3] / out[0][:, :3, :3] / 6.25 - 1).max() < 1e-2  # (entries of either sign, none near zero)


def _joint_selection(k):
    frames = [int(f) for f in dict.fromkeys(k.frames.tolist())][-8:] + [0, 1]
    return frames, [int(i) for i in dict.fromkeys(k.points.tolist())]


def _joint_layout(J, fv, nf, npt):
    """the diagonal blocks of the joint matrix over [frames..., points...]"""
    assert J.shape == (fv * nf + 3 * npt,) * 2 and np.array_equal(J, J.T)
    return (np.array([J[fv * x:fv * x + fv, fv * x:fv * x + fv] for x in range(nf)]),
            np.array([J[fv * nf + 3 * x:fv * nf + 3 * x + 3, fv * nf + 3 * x:fv * nf + 3 * x + 3] for x in range(npt)]))


@pytest.mark.parametrize("name", ["w8_every_frame_fv6", "nf16_constant_frames_and_landmarks_fv6"])
def test_joint_covariance(orc, name):
    """exactly symmetric, positive semi-definite on its free part to the bound, its diagonal blocks those of covariances()
    (another build of the system: to the bound here, to the bit in the next test)"""
    k = xc.case(name)
    r = xc.reference(orc, name, 0.0)
    frames, points = _joint_selection(k)
    h = _handle(k.fv)
    try:
        xc.configure(h, k)
        assert h.upload(k.f0, k.sc)
        J = h.joint_covariance(frames, points, sigma_pixels=0.6)
        JF, JP = _joint_layout(J, k.fv, len(frames), len(points))
        FB, PB = h.covariances(frames, points, sigma_pixels=0.6)
        assert vref.block_err(JF, FB) < xc.bound(r["cond"]) and vref.block_err(JP, PB) < xc.bound(r["cond"])
        d = np.diag(J)
        live = d > 0
        assert np.all(J[~live] == 0) and np.all(J[:, ~live] == 0) and live.sum() >= 6 * 7
        lo = np.linalg.eigvalsh(J[np.ix_(live, live)] / np.sqrt(np.outer(d[live], d[live]))).min()
        print(f"\n{name}: joint covariance of {len(frames)} frames and {len(points)} landmarks, {live.sum()} free variables, smallest "
              f"eigenvalue of the correlation matrix {lo:.3e} (allowed {-xc.bound(r['cond']):.3e})")
        assert lo > -xc.bound(r["cond"])
        # the normalised scene's variables: the same matrix from the staged blocks' convention
        Jn = h.joint_covariance(frames, points, sigma_pixels=0.6, caller_coordinates=False)
        assert np.array_equal(Jn, Jn.T) and (np.abs(Jn - J).max() > 0 or float(r["nrm"].world_scale) == 1.0)
    finally:
        h.close()


def test_joint_covariance_diagonal_blocks_have_the_bits_of_covariances():
    """deterministic mode (ten variables a frame): the diagonal blocks of the joint matrix are covariances()' to the bit"""
    k = xc.case("w8_edges_fv10")
    frames, points = _joint_selection(k)
    h = _handle(k.fv, deterministic=True)
    try:
        xc.configure(h, k)
        assert h.upload(k.f0, k.sc) and h.deterministic()
        J = h.joint_covariance(frames, points, sigma_pixels=0.6)
        JF, JP = _joint_layout(J, k.fv, len(frames), len(points))
        FB, PB = h.covariances(frames, points, sigma_pixels=0.6)
        assert np.array_equal(JF, FB) and np.array_equal(JP, PB) and np.abs(FB).max() > 0
    finally:
        h.close()


def test_rcs_modes_give_the_same_blocks(orc):
    name, c = "w8_every_frame_fv6", 1e-4
    k = xc.case(name)
    cond = xc.reference(orc, name, c)["cond"]
    _, diags = xc.reference_blocks(orc, name, c)
    out = {}
    for mode in (2, 1, 0):
        h = _handle(k.fv)
        try:
            xc.configure(h, k)
            h.set_rcs_mode(mode)
            assert h.upload(k.f0, k.sc)
            out[mode] = _staged(h, k, c)
            _check(out[mode], orc, name, c, k, f"rcs mode {mode}")
        finally:
            h.close()
    for mode in (1, 0):
        assert max(xc.errors(out[mode], out[2], diags)) < xc.bound(cond)


def test_deterministic_mode_same_bits(orc):
    name, c = "nf16_edges_fv10", 1e-4
    k = xc.case(name)
    h = _handle(k.fv, deterministic=True)
    try:
        xc.configure(h, k)
        assert h.upload(k.f0, k.sc) and h.deterministic()
        a = _staged(h, k, c)
        b = _staged(h, k, c)
        _check(a, orc, name, c, k, name + " deterministic")
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    finally:
        h.close()


def test_f32_storage(orc):
    """f32 storage of the point-frame blocks: the blocks move by the storage's rounding (2^-24 relative in W) times the
    conditioning; section 16's bound 2^-23 cond"""
    name, c = "nf16_edges_fv10", 1e-4
    k = xc.case(name)
    cond = xc.reference(orc, name, c)["cond"]
    h = _handle(k.fv, storage_precision=True)
    try:
        xc.configure(h, k)
        assert h.upload(k.f0, k.sc)
        got = _staged(h, k, c)
        _check(got, orc, name, c, k, "f32 storage", lim=2.0 ** -23 * cond)
        _transposes_and_repeats(k, got)
    finally:
        h.close()


def test_after_compute_inplace(orc):
    """after ComputeInplace the result is resident: the calls answer for it and leave the downloaded scene untouched"""
    k = xc.case("w8_every_frame_fv6")
    h = _handle(k.fv)
    try:
        crit = sa.BundleAdjustmentKanataniTermCriteria()
        crit.AllowedReprojErrRelativeChange(1e-10)
        crit.MaxHessianFactor(1e6)
        sg = k.sc.copy()
        h.ComputeInplace(k.f0, sg, crit, 20)
        assert h.report.iterations >= 1 and h.OptimizationStatusString() != "device error"
        kept = [a.copy() for a in (sg.points, sg.cam_R, sg.cam_T)]
        got = h.cross_covariances(k.ff, k.pf, k.pp, sigma_pixels=0.3)
        rel = h.relative_pose_covariances(k.rel, sigma_pixels=0.3)
        assert all(np.array_equal(a, b) for a, b in zip(kept, (sg.points, sg.cam_R, sg.cam_T)))
        # the reference at the optimised scene
        k2 = xc.case("w8_every_frame_fv6")
        k2.sc = sg
        r = xc.build_reference(orc, k2, 0.0)
        kf = 2.0 * (0.3 / k.f0) ** 2
        ref, diags = xref.blocks(r["inv"], k.ff, k.pf, k.pp), xref.diagonals(r["inv"], k.ff, k.pf, k.pp)
        e = xref.mapped_errors(got, [kf * x for x in ref], [(kf * dp, kf * dq) for dp, dq in diags], r["nrm"], k.fv)
        print(f"\nafter ComputeInplace: cross blocks off by {max(e):.3e} (bound {xc.bound(r['cond']):.3e})")
        assert max(e) < xc.bound(r["cond"])
        s = float(r["nrm"].world_scale)
        e = _relpose_err(rel, r["inv"], r["so"], k.rel, r["cond"], np.sqrt(kf) * np.array([1 / s] * 3 + [1.0] * 3))
        print(f"\nafter ComputeInplace: relative poses off by {e:.3e} of the allowance")
        assert e < 1
        assert h.optimize(crit, 2) in (True, False)
    finally:
        h.close()


def test_refusals_leave_the_handle_usable():
    k = xc.case("nf16_edges_fv6")
    h = _handle(k.fv)
    try:
        with pytest.raises(RuntimeError):
            h._raise(h._lib.srk_ba_phase_cross_covariance(h._h, *([0, None, None, None] * 3)))  # no scene
        with pytest.raises(RuntimeError):
            h._raise(h._lib.srk_ba_relative_pose_covariances(h._h, 1.0, 0, None, None, None))
        assert h.upload(k.f0, k.sc)
        h.phase_derivatives()
        h.phase_schur(1e-4)
        M, N = k.sc.M, k.sc.N
        for ff, pf, pp in (([(M, 0)], [], []), ([(0, -1)], [], []), ([], [(N, 0)], []), ([], [(0, M)], []), ([], [], [(0, N)]), ([], [], [(-1, 0)])):
            with pytest.raises(ValueError):
                h.phase_cross_covariance(ff, pf, pp)
            assert "out of range" in h.last_error()
        blk = np.zeros((1, 6, 6))
        assert h._lib.srk_ba_phase_cross_covariance(h._h, 1, None, None, blk.ctypes.data, 0, None, None, None, 0, None, None, None) == -1
        for s in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                h.cross_covariances([(1, 2)], sigma_pixels=s)
            with pytest.raises(ValueError):
                h.relative_pose_covariances([(1, 2)], sigma_pixels=s)
        with pytest.raises(ValueError):
            h.relative_pose_covariances([(1, M)])
        # the refused calls left the system alone
        FF, PF, PP = h.phase_cross_covariance([(2, 3)], [(0, 2)], [(0, 1)])
        assert np.abs(FF).max() > 0 and np.abs(PF).max() > 0 and np.abs(PP).max() > 0
        assert h.relative_pose_covariances([(2, 3)])[0, 0, 0] > 0
        # no pairs at all: the system is factorised, nothing else happens
        h.phase_derivatives()
        h.phase_schur(1e-4)
        assert [len(x) for x in h.phase_cross_covariance()] == [0, 0, 0]
    finally:
        h.close()
    g = _handle(10)
    try:
        g.set_intrinsic_groups(np.zeros(k.sc.M, dtype=np.int32))
        assert g.upload(k.f0, k.sc)
        with pytest.raises(ValueError):
            g.cross_covariances([(0, 1)])
        assert "intrinsic groups" in g.last_error()
        with pytest.raises(ValueError):
            g.relative_pose_covariances([(0, 1)])
    finally:
        g.close()


def test_cpp_adapter_cross_covariances(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "cross_covariance_adapter"
    r = subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "demos"),
                        os.path.join(HERE, "cpp", "test_cross_covariance_adapter.cpp"), "-o", str(exe),
                        "-L", os.path.join(ROOT, "surikatoko_amd"), "-lsrk_ba",
                        "-Wl,-rpath," + os.path.join(ROOT, "surikatoko_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cross-covariance adapter ok" in r.stdout
