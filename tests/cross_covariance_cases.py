"""The cases of the cross-covariance tests, shared by tests/test_gpu_cross_covariance.py and tests/test_cross_covariance_cpu.py.

Scenes and settings are those of tests/covariance_cases.py (largest: w8_m70, n = 420 with six variables a frame, 700 with
ten).  The pairs sit where k_cov_cross and the batch builder can go wrong:

- frames: two in the same 64-row tile (2, 3); in different tiles and, on w8_m70, further apart than the band and sharing no
  landmark (2, M - 1); every pair, in both orders and with itself, of the frames whose variables straddle a tile boundary
  (10, 21, 42 with six variables, 6, 12, 25 with ten), the gauge frames 0 and 1 and the last frame -- so a gauge frame with a
  free one, frame 1 with itself, (p, q) beside (q, p), (p, p), and blocks used by many pairs; a repeated pair; the constant
  frames of a case with a free one; the two frames a relative-pose factor couples directly;
- landmark x frame: every landmark of the covariance case (the first, the last, the longest track, one seen from two tiles;
  constant ones; the one with a q = 0 observation) with the frame before its first frame, its first, a middle and its last
  frame and the frame after its last, and with the last frame of the scene;
- landmark x landmark: every pair of those landmarks in both orders and with itself (landmarks 0 and N - 1 share no frame).

A case may cap the batch (20 columns: one pair of ten-variable frames a batch; 96).  Dampings follow covariance_cases.dampings."""
import numpy as np

import covariance_cases as vc
import covariance_ref as vref
import cross_covariance_ref as xref
import prior_ref as pref
import relpose_ref as rref
import weighted_ref as wr

# name -> (the case of covariance_cases whose scene, settings and landmarks are used, batch cap or None = the case's own)
CASES = {
    "nf2_all_fv6": ("nf2_all_fv6", None),
    "nf2_all_fv10": ("nf2_all_fv10", None),
    "nf16_edges_fv6": ("nf16_edges_fv6", None),
    "nf16_edges_fv10": ("nf16_edges_fv10", None),
    "w8_every_frame_fv6": ("w8_every_frame_fv6", None),
    "w8_every_frame_fv6_batch20": ("w8_every_frame_fv6", 20),
    "w8_every_frame_fv6_batch96": ("w8_every_frame_fv6", 96),
    "w8_edges_fv10": ("w8_edges_fv10", None),
    "w8_edges_fv10_batch20": ("w8_edges_fv10", 20),
    "nf16_constant_frames_and_landmarks_fv6": ("nf16_constant_frames_and_landmarks_fv6", None),
    "ragged_constant_free_gauge_fv10": ("ragged_constant_free_gauge_fv10", 96),
    "nf16_q0_fv6": ("nf16_q0_fv6", None),
    "nf16_priors_fv6": ("nf16_priors_fv6", None),
    "nf16_factors_fv6": ("nf16_factors_fv6", None),
    "nf16_shuffled_fv6": ("nf16_shuffled_fv6", None),
}
DENSE_CASES = ("nf2_all_fv6", "nf2_all_fv10")


def dampings(name):
    return vc.dampings(CASES[name][0])


def _frames_of(sc, i):
    rp, fr = np.asarray(sc.row_ptr), np.asarray(sc.obs_frame)
    return np.sort(fr[rp[i]:rp[i + 1]]).astype(np.int64)


def _pairs(k):
    sc, M = k.sc, k.sc.M
    edge = [f for f in vc._edge_frames(sc, k.fv) if f < M]
    edge = list(dict.fromkeys(edge))
    ff = [(2, 3), (2, M - 1), (M - 1, 2), (2, 3)]
    ff += [(a, b) for a in edge for b in edge]
    for j in np.flatnonzero(k.fconst)[:2]:
        free = int(np.flatnonzero(~k.fconst)[-1])
        ff += [(int(j), free), (free, int(j)), (int(j), int(j))]
    if k.fac is not None:
        ff += [(int(k.fac.a[0]), int(k.fac.b[0])), (int(k.fac.b[0]), int(k.fac.a[0]))]
    lm = list(dict.fromkeys(int(i) for i in k.points))
    pf = []
    for i in lm:
        f = _frames_of(sc, i)
        for j in (int(f[0]) - 1, int(f[0]), int(f[len(f) // 2]), int(f[-1]), int(f[-1]) + 1, M - 1):
            if 0 <= j < M:
                pf.append((i, j))
    pp = [(a, b) for a in lm for b in lm]
    return (np.asarray(ff, dtype=np.int32).reshape(-1, 2), np.asarray(pf, dtype=np.int64).reshape(-1, 2),
            np.asarray(pp, dtype=np.int64).reshape(-1, 2))


def case(name):
    """the covariance case (covariance_cases.case) with ff, pf, pp (pairs in the caller's numbering), rel (frame pairs a != b for
    the relative-pose covariance) and the batch cap of this case"""
    base, batch = CASES[name]
    k = vc.case(base)
    k.name = name
    if batch is not None:
        k.batch = batch
    k.ff, k.pf, k.pp = _pairs(k)
    k.rel = np.asarray([(a, b) for a, b in k.ff if a != b], dtype=np.int32).reshape(-1, 2)
    return k


configure = vc.configure
bound = vc.bound


def build_reference(orc, k, c, reverse=False, dense=False):
    """dict(inv = the cross_covariance_ref.Inverse of the case object k at damping c in the normalised scene, cond, nrm, so)"""
    so = orc.Scene(k.sc.points, k.sc.cam_R, k.sc.cam_T, k.sc.K, k.sc.shared_k, k.sc.row_ptr, k.sc.obs_frame, k.sc.obs_uv)
    ok, nrm = orc.normalize(so)
    assert ok
    pri = None if k.pri is None else pref.normalised(k.pri, nrm)
    fac = None if k.fac is None else rref.normalised(k.fac, nrm)
    der = None if k.q is None else (lambda s: wr.derivatives(k.f0, s, k.q))
    restricted = vref.blocks_of(orc, k.f0, so, k.fv, k.fconst, k.pconst, pri, fac, der)
    if dense:
        inv = xref.DenseInverse(so, restricted, c, k.fv, k.fconst, k.pconst, k.keep_gauge, fac)
    else:
        inv = xref.SchurInverse(so, restricted, c, k.fv, k.fconst, k.pconst, k.keep_gauge, fac, reverse)
    return dict(inv=inv, cond=inv.cond, nrm=nrm, so=so)


_refs = {}


def reference(orc, name, c, reverse=False, dense=False):
    """build_reference of the named case, computed once per (scene and settings, damping, route): cases that differ in the
    batch cap alone share it"""
    key = (CASES[name][0], float(c), bool(reverse), bool(dense))
    if key not in _refs:
        _refs[key] = build_reference(orc, vc.case(CASES[name][0]), c, reverse, dense)
    return _refs[key]


_blocks = {}


def reference_blocks(orc, name, c, reverse=False, dense=False):
    """(the reference's three block arrays for the case's pairs, the marginal diagonals of every pair) -- computed once"""
    key = (CASES[name][0], float(c), bool(reverse), bool(dense))
    if key not in _blocks:
        k = case(name)
        inv = reference(orc, name, c, reverse, dense)["inv"]
        main = reference(orc, name, c)["inv"]  # the denominators are always those of the reference proper
        _blocks[key] = (xref.blocks(inv, k.ff, k.pf, k.pp), xref.diagonals(main, k.ff, k.pf, k.pp))
    return _blocks[key]


def errors(got, ref_blocks, diags):
    """the three cross_err of (FF, PF, PP) against the reference (asserting the exact zeros)"""
    return tuple(xref.cross_err(g, r, dp, dq) for g, r, (dp, dq) in zip(got, ref_blocks, diags))


def assert_correlated(k, ref_blocks, diags):
    """the reference's largest |correlation| among the requested off-diagonal blocks exceeds 1e-3: a zero block would not pass"""
    off = (k.ff[:, 0] != k.ff[:, 1], np.ones(len(k.pf), dtype=bool), k.pp[:, 0] != k.pp[:, 1])
    r = [xref.max_offdiagonal_correlation(b, dp, dq, o) for b, (dp, dq), o in zip(ref_blocks, diags, off)]
    assert min(r) > 1e-3, r
    return r
