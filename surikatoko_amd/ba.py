"""Host-side mirror of the reference's BA operator interface over the C ABI (include/srk_ba.h).

Same names, argument meaning and error behaviour as suriko's
  BundleAdjustmentKanatani            cpp_impl/suriko-engine/include/suriko/bundle-adj-kanatani.h:96-261
  BundleAdjustmentKanataniTermCriteria                                             .h:68-92
  NormalizeSceneInplace / CheckWorldIsNormalized                                   .h:61-65
so that tests/ read like the reference's own tests.  Scenes are flat arrays (class Scene) instead of
FragmentMap / CornerTrackRepository / std::vector<SE3Transform>; the C++ adapter that converts those
containers is include/suriko_amd/bundle-adj-kanatani.hpp.

Everything computes on the GPU through libsrk_ba.so.  Nothing here imports oracle/.
"""
import ctypes as C
import math

import numpy as np

from ._lib import MargCounts, MargReport, Normalizer, Report, lib

BUF_GRAD, BUF_POINT_BLOCKS, BUF_FRAME_BLOCKS, BUF_POINT_FRAME, BUF_RCS, BUF_RCS_RHS, BUF_CORRECTIONS, BUF_POINTS, \
    BUF_CAM_R, BUF_CAM_T = range(10)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def status_string(status):
    return lib().srk_ba_status_string(int(status)).decode()


def device_count():
    return int(lib().srk_ba_device_count())


class Scene:
    """Flat scene arrays in the C-ABI layout (include/srk_ba.h); arrays are owned copies, mutated in place by BA."""

    def __init__(self, points, cam_R, cam_T, K, shared_k, row_ptr, obs_frame, obs_uv):
        self.points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3).copy()
        self.cam_R = np.ascontiguousarray(cam_R, dtype=np.float64).reshape(-1, 9).copy()
        self.cam_T = np.ascontiguousarray(cam_T, dtype=np.float64).reshape(-1, 3).copy()
        self.K = np.ascontiguousarray(K, dtype=np.float64).reshape(-1, 9).copy()
        self.shared_k = int(bool(shared_k))
        self.row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64).copy()
        self.obs_frame = np.ascontiguousarray(obs_frame, dtype=np.int32).copy()
        self.obs_uv = np.ascontiguousarray(obs_uv, dtype=np.float64).reshape(-1, 2).copy()

    N = property(lambda self: self.points.shape[0])
    M = property(lambda self: self.cam_R.shape[0])
    O = property(lambda self: int(self.row_ptr[-1]))

    def copy(self):
        return Scene(self.points, self.cam_R, self.cam_T, self.K, self.shared_k, self.row_ptr, self.obs_frame,
                     self.obs_uv)

    def shard(self, rank, world):
        """Landmark shard of this scene for `rank` of `world` (contiguous pnt_ind range balanced by observation
        count, cameras replicated) -- SURVEY 8e partitioning."""
        lo, hi = shard_bounds(self.row_ptr, rank, world)
        o0, o1 = int(self.row_ptr[lo]), int(self.row_ptr[hi])
        return Scene(self.points[lo:hi], self.cam_R, self.cam_T, self.K, self.shared_k,
                     self.row_ptr[lo:hi + 1] - o0, self.obs_frame[o0:o1], self.obs_uv[o0:o1]), (lo, hi)

    def scene_args(self):
        return (C.c_int64(self.N), _p(self.points), C.c_int32(self.M), _p(self.cam_R), _p(self.cam_T), _p(self.K),
                C.c_int(self.shared_k), _p(self.row_ptr), _p(self.obs_frame), _p(self.obs_uv))


def covisibility(scene, to_internal=None):
    """min_cv[j] = smallest frame index that shares a landmark with frame j (the skyline of the reduced camera
    system); computed on the WHOLE scene before sharding.  to_internal: the frame numbering given to
    set_frame_order() -- the result is then in that numbering, as srk_ba_set_covisibility wants it."""
    M = scene.M
    f = scene.obs_frame if to_internal is None else np.asarray(to_internal, np.int32)[scene.obs_frame]
    counts = np.diff(scene.row_ptr)
    first = np.minimum.reduceat(f, scene.row_ptr[:-1][counts > 0]) if scene.O else np.zeros(0, np.int32)
    first_per_obs = np.repeat(first, counts[counts > 0])
    min_cv = np.arange(M, dtype=np.int64)
    np.minimum.at(min_cv, f, first_per_obs)
    return min_cv.astype(np.int32)


def frame_order(scene, mode=-1):
    """srk_frame_order on the host: to_internal[frame] when renumbering the frames pays (mode -1) / differs (mode 1), else
    None.  For landmark shards: find it on the whole scene, give it to every rank's set_frame_order()."""
    to_int = np.zeros(scene.M, np.int32)
    rc = lib().srk_frame_order(C.c_int(mode), C.c_int64(scene.N), C.c_int32(scene.M), _p(scene.row_ptr), _p(scene.obs_frame), _p(to_int))
    if rc < 0:
        raise ValueError("srk_frame_order: bad arguments")
    return to_int if rc == 1 else None


def shard_bounds(row_ptr, rank, world):
    """Contiguous pnt_ind range [lo, hi) of `rank`: cut points chosen so every rank gets ~O/world observations."""
    row_ptr = np.asarray(row_ptr)
    N = len(row_ptr) - 1
    O = int(row_ptr[-1])
    cuts = [0]
    for r in range(1, world):
        target = O * r // world
        cuts.append(int(np.searchsorted(row_ptr, target, side="left")))
    cuts.append(N)
    cuts = [min(max(c, 0), N) for c in cuts]
    for i in range(1, len(cuts)):
        cuts[i] = max(cuts[i], cuts[i - 1])
    return cuts[rank], cuts[rank + 1]


class BundleAdjustmentKanataniTermCriteria:
    """bundle-adj-kanatani.h:68-92 -- two optionals; None = unset ('potentially optimize forever')."""

    def __init__(self):
        self._allowed_reproj_err_rel_change = None
        self._max_hessian_factor = None

    def AllowedReprojErrRelativeChange(self, value="__get__"):
        if value == "__get__":
            return self._allowed_reproj_err_rel_change
        self._allowed_reproj_err_rel_change = value

    def MaxHessianFactor(self, value="__get__"):
        if value == "__get__":
            return self._max_hessian_factor
        self._max_hessian_factor = value


def normalize_scene_inplace(scene, t1y_dist=1.0, unity_comp_ind=1):
    """NormalizeSceneInplace (bundle-adj-kanatani.h:61-62, .cpp:277-286).  Returns (success, normalizer)."""
    if not (0 <= unity_comp_ind < 3):
        raise ValueError("Can normalize only one of [T1x, T1y, Tz] components")  # CHECK at .cpp:129
    nrm = Normalizer()
    ok = lib().srk_ba_normalize_scene(C.c_int64(scene.N), _p(scene.points), C.c_int32(scene.M), _p(scene.cam_R),
                                      _p(scene.cam_T), C.c_double(t1y_dist), C.c_int32(unity_comp_ind), C.byref(nrm))
    return bool(ok), nrm


def revert_normalization(scene, nrm):
    """SceneNormalizer::RevertNormalization (.cpp:249-270)."""
    lib().srk_ba_revert_normalization(C.c_int64(scene.N), _p(scene.points), C.c_int32(scene.M), _p(scene.cam_R),
                                      _p(scene.cam_T), C.byref(nrm))


def prior_information(spec=None, n=None, info=None, sigma_pixels=None, f0=None):
    """[n][6] information matrices (xx xy xz yy yz zz) of n position priors.  info= gives them directly: [n][6] or [n][3][3]
    (or one [6] / [1][3][3] for all).  Otherwise spec is read by its number of dimensions alone: a scalar is one sigma for all,
    1-D [3] per-axis sigmas for all, 2-D [n][3] per-axis sigmas, 3-D [n][3][3] (or [1][3][3] for all) covariances -- a single
    covariance goes in as [1][3][3], so that per-axis sigmas of three priors are never taken for one.  World units; they become
    L = (sigma_pixels / f0)^2 Sigma^-1, the prior beside observations of pixel noise sigma_pixels, in the units of the error,
    (pix / f0)^2.  A covariance must be symmetric positive definite."""
    def rows(a, what):
        if n is not None and a.shape[0] == 1 and n != 1:
            a = np.repeat(a, n, axis=0)
        if n is not None and a.shape[0] != n:
            raise ValueError(f"position priors: {a.shape[0]} {what} for {n} priors")
        return a

    def six(L):
        return np.ascontiguousarray(np.stack([L[:, 0, 0], L[:, 0, 1], L[:, 0, 2], L[:, 1, 1], L[:, 1, 2], L[:, 2, 2]], axis=1))

    if info is not None:
        a = np.asarray(info, dtype=np.float64)
        if a.ndim == 3 and a.shape[1:] == (3, 3):
            return six(rows(a, "information matrices"))
        if (a.ndim == 1 and a.size == 6) or (a.ndim == 2 and a.shape[1] == 6):
            return np.ascontiguousarray(rows(a.reshape(-1, 6), "information matrices"))
        raise ValueError("position priors: info= is [n][6] (xx xy xz yy yz zz) or [n][3][3]")
    if spec is None:
        raise ValueError("position priors: give a sigma, per-axis sigmas, covariances or info=")
    if sigma_pixels is None or not f0:
        raise ValueError("position priors: sigmas and covariances need sigma_pixels and the scene's f0 (or pass info=)")
    a = np.asarray(spec, dtype=np.float64)
    if a.ndim == 0:
        cov = np.eye(3)[None] * float(a) ** 2
    elif (a.ndim == 1 and a.size == 3) or (a.ndim == 2 and a.shape[1] == 3):
        sg = a.reshape(-1, 3)
        cov = np.zeros((sg.shape[0], 3, 3))
        cov[:, np.arange(3), np.arange(3)] = sg ** 2
    elif a.ndim == 3 and a.shape[1:] == (3, 3):
        cov = a
        if np.abs(cov - cov.transpose(0, 2, 1)).max() > 1e-12 * np.abs(cov).max():
            raise ValueError("position priors: a covariance is not symmetric")
    else:
        raise ValueError("position priors: spec is a sigma, per-axis sigmas [n][3] or covariances [n][3][3]")
    cov = rows(cov, "sigmas / covariances")
    if not np.all(np.isfinite(cov)) or np.any(np.linalg.eigvalsh(0.5 * (cov + cov.transpose(0, 2, 1))) <= 0):
        raise ValueError("position priors: sigmas must be positive and covariances positive definite")
    L = np.linalg.inv(cov) * (float(sigma_pixels) / float(f0)) ** 2
    return six(0.5 * (L + L.transpose(0, 2, 1)))


def normalize_position_priors(nrm, pos, info):
    """positions [n][3] and information matrices [n][6] through a Normalizer, as the upload maps them
    (srk_ba_normalize_position_priors; host only).  Returns (pos_n, info_n)."""
    pos = np.ascontiguousarray(np.asarray(pos, dtype=np.float64).reshape(-1, 3))
    info = np.ascontiguousarray(np.asarray(info, dtype=np.float64).reshape(-1, 6))
    if pos.shape[0] != info.shape[0]:
        raise ValueError("normalize_position_priors: one information matrix per position")
    po, io = np.zeros_like(pos), np.zeros_like(info)
    rc = lib().srk_ba_normalize_position_priors(C.byref(nrm), C.c_int64(pos.shape[0]), _p(pos), _p(info), _p(po), _p(io))
    if rc != 0:
        raise ValueError("srk_ba_normalize_position_priors: bad argument")
    return po, io


def revert_covariances(nrm, frame_cov=None, point_cov=None):
    """covariance blocks of the normalised scene's variables in the caller's coordinates (srk_ba_revert_covariances; host only):
    frame_cov [n][fv][fv] (fv 6 or 10), point_cov [n][3][3]; either may be None.  Returns copies (frame_cov, point_cov)."""
    fc = None if frame_cov is None else np.array(frame_cov, dtype=np.float64, order="C")
    pc = None if point_cov is None else np.array(point_cov, dtype=np.float64, order="C").reshape(-1, 3, 3)
    fv = 6 if fc is None else fc.shape[-1]
    if fc is not None:
        fc = fc.reshape(-1, fv, fv)
    rc = lib().srk_ba_revert_covariances(C.byref(nrm), C.c_int(fv), C.c_int32(0 if fc is None else len(fc)),
                                         _p(fc) if fc is not None and len(fc) else None, C.c_int64(0 if pc is None else len(pc)),
                                         _p(pc) if pc is not None and len(pc) else None)
    if rc != 0:
        raise ValueError("srk_ba_revert_covariances: bad argument")
    return fc, pc


def revert_cross_covariances(nrm, frame_frame=None, point_frame=None, point_point=None):
    """cross-covariance blocks of the normalised scene's variables in the caller's coordinates (srk_ba_revert_cross_covariances;
    host only): frame_frame [n][fv][fv], point_frame [n][3][fv] (fv 6 or 10), point_point [n][3][3]; any may be None.  A block
    between p and q maps as D_p Sigma D_q^T.  Returns copies (frame_frame, point_frame, point_point)."""
    ff = None if frame_frame is None else np.array(frame_frame, dtype=np.float64, order="C")
    pf = None if point_frame is None else np.array(point_frame, dtype=np.float64, order="C")
    pp = None if point_point is None else np.array(point_point, dtype=np.float64, order="C").reshape(-1, 3, 3)
    fv = ff.shape[-1] if ff is not None else (pf.shape[-1] if pf is not None else 6)
    if ff is not None:
        ff = ff.reshape(-1, fv, fv)
    if pf is not None:
        pf = pf.reshape(-1, 3, fv)
    args = []
    for a in (ff, pf, pp):
        args += [C.c_int64(0 if a is None else len(a)), _p(a) if a is not None and len(a) else None]
    if lib().srk_ba_revert_cross_covariances(C.byref(nrm), C.c_int(fv), *args) != 0:
        raise ValueError("srk_ba_revert_cross_covariances: bad argument")
    return ff, pf, pp


_RP_TRI = [(r, c) for r in range(6) for c in range(r, 6)]  # the 21 entries of the upper triangle of a 6 x 6, row by row


def relative_pose_information(n, info=None, sigma_t=None, sigma_r=None, covariance=None, sigma_pixels=1.0, f0=None):
    """[n][21] information matrices of n relative-pose factors: the upper triangle row by row, order [t; r].  info= gives them
    directly: [n][21] or [n][6][6] (or one for all).  Otherwise sigma_t (world units) and sigma_r (radians), scalars or [n], or
    covariance= [n][6][6] (or one [6][6] for all), become L = (sigma_pixels / f0)^2 Sigma^-1: the factor beside observations of
    pixel noise sigma_pixels, in the units of the error, (pix / f0)^2."""
    def rows(a):
        if a.shape[0] == 1 and n != 1:
            a = np.repeat(a, n, axis=0)
        if a.shape[0] != n:
            raise ValueError(f"relative-pose factors: {a.shape[0]} information matrices / sigmas / covariances for {n} factors")
        return a

    def tri(L):
        return np.ascontiguousarray(np.stack([L[:, r, c] for r, c in _RP_TRI], axis=1))

    if info is not None:
        a = np.asarray(info, dtype=np.float64)
        if a.shape[-2:] == (6, 6) and a.ndim in (2, 3):
            return tri(rows(a.reshape(-1, 6, 6)))
        if a.shape[-1] == 21 and a.ndim in (1, 2):
            return np.ascontiguousarray(rows(a.reshape(-1, 21)))
        raise ValueError("relative-pose factors: info= is [n][21] (upper triangle, row by row) or [n][6][6]")
    if not f0:
        raise ValueError("relative-pose factors: sigmas and covariances need the scene's f0 (or pass info=)")
    if covariance is not None:
        cov = np.asarray(covariance, dtype=np.float64)
        if cov.shape[-2:] != (6, 6) or cov.ndim not in (2, 3):
            raise ValueError("relative-pose factors: covariance= is [n][6][6] or [6][6]")
        cov = rows(cov.reshape(-1, 6, 6))
        if np.abs(cov - cov.transpose(0, 2, 1)).max() > 1e-12 * np.abs(cov).max():
            raise ValueError("relative-pose factors: a covariance is not symmetric")
    else:
        if sigma_t is None or sigma_r is None:
            raise ValueError("relative-pose factors: give info=, sigma_t= and sigma_r=, or covariance=")
        st = rows(np.asarray(sigma_t, dtype=np.float64).reshape(-1))
        sr = rows(np.asarray(sigma_r, dtype=np.float64).reshape(-1))
        cov = np.zeros((n, 6, 6))
        for e in range(3):
            cov[:, e, e] = st ** 2
            cov[:, 3 + e, 3 + e] = sr ** 2
    if not np.all(np.isfinite(cov)) or np.any(np.linalg.eigvalsh(0.5 * (cov + cov.transpose(0, 2, 1))) <= 0):
        raise ValueError("relative-pose factors: sigmas must be positive and covariances positive definite")
    L = np.linalg.inv(cov) * (float(sigma_pixels) / float(f0)) ** 2
    return tri(0.5 * (L + L.transpose(0, 2, 1)))


def relative_pose(scene, a, b):
    """(Z, z) of the pair (a, b) as the scene's poses have it: Z = R_a R_b^T, the orientation of camera b in camera a's frame,
    and z = R_a (C_b - C_a), the centre of b in a's frame -- the measurement a factor with zero residual carries"""
    R = np.asarray(scene.cam_R, dtype=np.float64).reshape(-1, 3, 3)
    T = np.asarray(scene.cam_T, dtype=np.float64).reshape(-1, 3)
    return R[a] @ R[b].T, R[a] @ (R[a].T @ T[a] - R[b].T @ T[b])


def normalize_relative_pose_factors(nrm, rel_t, info):
    """measured translations [n][3] and information matrices [n][21] through a Normalizer, as the upload maps them
    (srk_ba_normalize_relative_pose_factors; host only).  Returns (rel_t_n, info_n)."""
    rel_t = np.ascontiguousarray(np.asarray(rel_t, dtype=np.float64).reshape(-1, 3))
    info = np.ascontiguousarray(np.asarray(info, dtype=np.float64).reshape(-1, 21))
    if rel_t.shape[0] != info.shape[0]:
        raise ValueError("normalize_relative_pose_factors: one information matrix per translation")
    to, io = np.zeros_like(rel_t), np.zeros_like(info)
    rc = lib().srk_ba_normalize_relative_pose_factors(C.byref(nrm), C.c_int32(rel_t.shape[0]), _p(rel_t), _p(info), _p(to), _p(io))
    if rc != 0:
        raise ValueError("srk_ba_normalize_relative_pose_factors: bad argument")
    return to, io


def _joint_pose_prior_arrays(sets, sigma_pixels=None, f0=None):
    """the flat arrays of the C ABI from a list of sets.  A set is a dict with frames (k, strictly ascending), R [k][3][3] and
    C [k][3] (or poses=(R, C)): the linearisation poses, info= [6k][6k] or covariance= [6k][6k] (variable order frame by frame,
    [t; r] inside a frame), and optionally mean= [6k]; or a tuple (frames, R, C, info[, mean]).  A covariance becomes
    L = (sigma_pixels / f0)^2 Sigma^-1, as in relative_pose_information."""
    ptr, frames, Rs, Cs, means, infos = [0], [], [], [], [], []
    for st in sets:
        if not isinstance(st, dict):
            st = dict(zip(("frames", "R", "C", "info", "mean"), st))
        fr = np.asarray(st["frames"]).astype(np.int32).reshape(-1)
        k = fr.size
        R, Cc = st["poses"] if "poses" in st else (st["R"], st["C"])
        R = np.asarray(R, dtype=np.float64).reshape(-1, 9)
        Cc = np.asarray(Cc, dtype=np.float64).reshape(-1, 3)
        if R.shape[0] != k or Cc.shape[0] != k:
            raise ValueError("joint pose priors: one linearisation pose (R, C) per frame of a set")
        if st.get("info") is not None:
            L = np.asarray(st["info"], dtype=np.float64)
        elif st.get("covariance") is not None:
            if not f0:
                raise ValueError("joint pose priors: a covariance needs the scene's f0 (or pass info=)")
            cov = np.asarray(st["covariance"], dtype=np.float64)
            if cov.shape != (6 * k, 6 * k) or np.abs(cov - cov.T).max() > 1e-12 * np.abs(cov).max():
                raise ValueError("joint pose priors: covariance= is a symmetric [6k][6k]")
            cov = 0.5 * (cov + cov.T)
            if not np.all(np.isfinite(cov)) or np.any(np.linalg.eigvalsh(cov) <= 0):
                raise ValueError("joint pose priors: a covariance must be positive definite")
            L = np.linalg.inv(cov) * (float(1.0 if sigma_pixels is None else sigma_pixels) / float(f0)) ** 2
            L = 0.5 * (L + L.T)
        else:
            raise ValueError("joint pose priors: give info= or covariance= for every set")
        if L.shape != (6 * k, 6 * k):
            raise ValueError("joint pose priors: the information matrix of a set of k frames is [6k][6k]")
        m = np.zeros(6 * k) if st.get("mean") is None else np.asarray(st["mean"], dtype=np.float64).reshape(-1)
        if m.size != 6 * k:
            raise ValueError("joint pose priors: the mean of a set of k frames has 6k values")
        ptr.append(ptr[-1] + k)
        frames.append(fr); Rs.append(R); Cs.append(Cc); means.append(m); infos.append(L.reshape(-1))
    cat = lambda v, dt: np.ascontiguousarray(np.concatenate(v), dtype=dt)  # noqa: E731
    return (np.asarray(ptr, dtype=np.int32), cat(frames, np.int32), cat(Rs, np.float64), cat(Cs, np.float64), cat(means, np.float64),
            cat(infos, np.float64))


def _joint_pose_prior_sets(ptr, fr, R, Cc, m, L):
    """the inverse of _joint_pose_prior_arrays: a list of dicts frames, R, C, mean, info"""
    out, at = [], 0
    for g in range(len(ptr) - 1):
        a, b = int(ptr[g]), int(ptr[g + 1])
        n = 6 * (b - a)
        out.append(dict(frames=fr[a:b].copy(), R=R.reshape(-1, 3, 3)[a:b].copy(), C=Cc.reshape(-1, 3)[a:b].copy(),
                        mean=m.reshape(-1)[6 * a:6 * b].copy(), info=L[at:at + n * n].reshape(n, n).copy()))
        at += n * n
    return out


def check_joint_pose_priors(sets, keep_gauge=True):
    """the setter's checks on their own (srk_ba_check_joint_pose_priors; host only): None, or the text of the refusal"""
    if len(sets) == 0:
        return None
    ptr, fr, R, Cc, m, L = _joint_pose_prior_arrays(sets)
    why = C.c_char_p()
    lib().srk_ba_check_joint_pose_priors(C.c_int32(len(ptr) - 1), _p(ptr), _p(fr), _p(R), _p(Cc), _p(m), _p(L), C.c_int(int(keep_gauge)),
                                         C.byref(why))
    return why.value.decode() if why.value else None


def normalize_joint_pose_priors(nrm, sets):
    """a list of sets through a Normalizer, as the upload maps them (srk_ba_normalize_joint_pose_priors; host only): with
    X_n = s (R0 X + T0), Cbar_n = s (R0 Cbar + T0), Rbar_n = Rbar R0^T, m_n = D m, L_n = D^-T L D^-1, D = diag(s R0, R0)"""
    ptr, fr, R, Cc, m, L = _joint_pose_prior_arrays(sets)
    Ro, Co, mo, Lo = np.zeros_like(R), np.zeros_like(Cc), np.zeros_like(m), np.zeros_like(L)
    rc = lib().srk_ba_normalize_joint_pose_priors(C.byref(nrm), C.c_int32(len(ptr) - 1), _p(ptr), _p(R), _p(Cc), _p(m), _p(L), _p(Ro), _p(Co),
                                                  _p(mo), _p(Lo))
    if rc != 0:
        raise ValueError("srk_ba_normalize_joint_pose_priors: bad argument")
    return _joint_pose_prior_sets(ptr, fr, Ro, Co, mo, Lo)


def joint_pose_prior_from_covariance(frames, scene, joint_cov, frame_vars, sigma_pixels, f0):
    """A ready set for set_joint_pose_priors from a joint_covariance(frames, []) result (computed at pixel noise sigma_pixels) and
    the scene's current poses: the pose rows and columns of every frame are selected (which marginalises the intrinsics of
    the ten-variable layout), then L = (sigma_pixels / f0)^2 Sigma^-1; mean zero, linearised at the scene's poses.  frames
    must be strictly ascending, as joint_covariance was called."""
    fr = np.asarray(frames).astype(np.int32).reshape(-1)
    fv, k = int(frame_vars), fr.size
    off = fv - 6
    sel = np.concatenate([fv * i + off + np.arange(6) for i in range(k)])
    cov = np.asarray(joint_cov, dtype=np.float64)[np.ix_(sel, sel)]
    cov = 0.5 * (cov + cov.T)
    L = np.linalg.inv(cov) * (float(sigma_pixels) / float(f0)) ** 2
    R = np.asarray(scene.cam_R, dtype=np.float64).reshape(-1, 3, 3)[fr]
    T = np.asarray(scene.cam_T, dtype=np.float64).reshape(-1, 3)[fr]
    return dict(frames=fr, R=R.copy(), C=-np.einsum("kba,kb->ka", R, T), info=0.5 * (L + L.T), mean=np.zeros(6 * k))


def marginalize_dense(A, b, d, k):
    """the dense elimination of a marginalisation prior on caller-given A [6(d+k)][6(d+k)] and b, dropped slots first
    (srk_ba_marginalize_dense; host only): (info, eta, mean, defect).  Raises numpy.linalg.LinAlgError when A_DD is not positive
    definite."""
    n = 6 * (int(d) + int(k))
    A = np.ascontiguousarray(np.asarray(A, dtype=np.float64).reshape(n, n))
    b = np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(n))
    L, eta, m = np.zeros((6 * k, 6 * k)), np.zeros(6 * k), np.zeros(6 * k)
    defect = C.c_double(0)
    rc = lib().srk_ba_marginalize_dense(_p(A), _p(b), C.c_int32(int(d)), C.c_int32(int(k)), _p(L), _p(eta), _p(m), C.byref(defect))
    if rc < 0:
        raise ValueError("srk_ba_marginalize_dense: bad argument")
    if rc != 0:
        raise np.linalg.LinAlgError("srk_ba_marginalize_dense: the block of the dropped frames is not positive definite")
    return L, eta, m, defect.value


def revert_marginalization_prior(nrm, R=None, C_=None, info=None, eta=None, mean=None):
    """a marginalisation prior in the normalised variables back into the caller's coordinates
    (srk_ba_revert_marginalization_prior; host only): copies of the arrays given, None where None was given"""
    cp = lambda a, shape: None if a is None else np.ascontiguousarray(np.array(a, dtype=np.float64).reshape(shape))  # noqa: E731
    sizes = [np.asarray(a).size // s for a, s in ((R, 9), (C_, 3), (eta, 6), (mean, 6)) if a is not None]
    if info is not None:
        sizes.append(int(round(math.sqrt(np.asarray(info).size))) // 6)
    if not sizes or len(set(sizes)) != 1:
        raise ValueError("revert_marginalization_prior: arrays over one and the same number of frames")
    k = sizes[0]
    out = [cp(R, (k, 3, 3)), cp(C_, (k, 3)), cp(info, (6 * k, 6 * k)), cp(eta, 6 * k), cp(mean, 6 * k)]
    rc = lib().srk_ba_revert_marginalization_prior(C.byref(nrm), C.c_int32(k), *[None if a is None else _p(a) for a in out])
    if rc != 0:
        raise ValueError("srk_ba_revert_marginalization_prior: bad argument")
    return tuple(out)


def marginalization_landmarks(scene, frames, max_kept=16, q=None):
    """Which landmarks to marginalise with the frames dropped, so that the prior ties at most max_kept frames: the landmarks seen
    from a dropped frame are taken in the order of their track length as long as the union of their other frames stays within
    max_kept.  Returns (points, q): the chosen landmarks (ascending) and the observation information that switches off the
    dropped frames' observations of the others (the given q, or ones, with zeros there) -- what set_observation_information
    takes before marginalization_prior."""
    rp = np.asarray(scene.row_ptr)
    fr = np.asarray(scene.obs_frame)
    O = int(rp[-1])
    q = np.ones(O) if q is None else np.array(q, dtype=np.float64).reshape(O)
    drop = np.zeros(scene.M, dtype=bool)
    drop[np.asarray(frames, dtype=np.int64)] = True
    pt = np.repeat(np.arange(scene.N), np.diff(rp))
    hit = np.zeros(scene.N, dtype=bool)
    hit[pt[drop[fr] & (q > 0)]] = True
    cand = np.flatnonzero(hit)
    cand = cand[np.argsort(np.diff(rp)[cand], kind="stable")]
    kept = np.zeros(scene.M, dtype=bool)
    chosen = []
    for i in cand:
        f = fr[rp[i]:rp[i + 1]][q[rp[i]:rp[i + 1]] > 0]
        new = kept.copy()
        new[f[~drop[f]]] = True
        if new.sum() <= max_kept:
            kept = new
            chosen.append(int(i))
    take = np.zeros(scene.N, dtype=bool)
    take[chosen] = True
    q[drop[fr] & ~take[pt]] = 0.0
    return np.asarray(sorted(chosen), dtype=np.int64), q


def check_world_is_normalized(scene, t1y=1.0, unity_comp_ind=1):
    """CheckWorldIsNormalized (.cpp:288-333)."""
    return bool(lib().srk_ba_check_world_is_normalized(C.c_int32(scene.M), _p(scene.cam_R), _p(scene.cam_T),
                                                        C.c_double(t1y), C.c_int32(unity_comp_ind)))


class BundleAdjustmentKanatani:
    """Mirror of suriko::BundleAdjustmentKanatani on top of one srk_ba handle (one GPU)."""

    kPointVarsCount = 3
    kIntrinsicVarsCount = 4
    kTVarsCount = 3
    kWVarsCount = 3
    kMaxFrameVarsCount = 10

    def __init__(self, device=0):
        self._lib = lib()
        self._h = self._lib.srk_ba_create(int(device))
        if not self._h:
            raise RuntimeError("srk_ba_create failed: no usable HIP device (there is no CPU fallback)")
        self._f0 = 0.0
        self._scene = None
        self._status = ""
        self.report = Report()
        self._hook = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.srk_ba_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference API
    def ComputeInplace(self, f0, scene, term_crit=None, max_iterations=0):
        """bool ComputeInplace(f0, map, inverse_orient_cams, track_rep, shared_K | Ks, term_crit)
        (bundle-adj-kanatani.h:179-184).  `scene` is updated in place.  Raises ValueError where the reference
        CHECK-aborts (f0 ~ 0; fewer than two frames)."""
        a, m = self._criteria(term_crit)
        self._f0 = float(f0)
        self._scene = scene
        self.report = Report()
        rc = self._lib.srk_ba_compute_inplace(C.c_void_p(self._h), C.c_double(f0), *scene.scene_args(), a, m,
                                              C.c_int64(max_iterations), C.byref(self.report))
        self._raise(rc)
        self._status = status_string(self.report.status)
        return rc == 0

    def ComputeInplaceF32(self, f0, points, cam_R, cam_T, K, shared_k, row_ptr, obs_frame, obs_uv, term_crit=None,
                          max_iterations=0):
        """The call of a reference built with Scalar = float: float32 arrays (updated in place) at the boundary, the
        fp64 pipeline inside (srk_ba_compute_inplace_f32)."""
        for arr in (points, cam_R, cam_T, K, obs_uv):
            if arr.dtype != np.float32 or not arr.flags["C_CONTIGUOUS"]:
                raise ValueError("ComputeInplaceF32 takes C-contiguous float32 arrays")
        rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
        fr = np.ascontiguousarray(obs_frame, dtype=np.int32)
        a64, m64 = self._criteria(term_crit)
        a32 = C.c_float(term_crit.AllowedReprojErrRelativeChange()) if a64 is not None else None
        m32 = C.c_float(term_crit.MaxHessianFactor()) if m64 is not None else None
        self._f0 = float(f0)
        self.report = Report()
        rc = self._lib.srk_ba_compute_inplace_f32(
            C.c_void_p(self._h), C.c_float(f0), C.c_int64(points.shape[0]), _p(points), C.c_int32(cam_R.shape[0]), _p(cam_R),
            _p(cam_T), _p(K), C.c_int(int(bool(shared_k))), _p(rp), _p(fr), _p(obs_uv),
            C.byref(a32) if a32 is not None else None, C.byref(m32) if m32 is not None else None,
            C.c_int64(max_iterations), C.byref(self.report))
        self._raise(rc)
        self._status = status_string(self.report.status)
        return rc == 0

    def ReprojError(self, f0, scene):
        """static Scalar ReprojError(...) (.h:167-172, .cpp:410-490) -> (err, seen_points_count)."""
        seen = C.c_int64(0)
        e = self._lib.srk_ba_reproj_error(C.c_void_p(self._h), C.c_double(f0), *scene.scene_args(), C.byref(seen))
        if math.isnan(e):
            msg = self.last_error()
            if "hip" in msg.lower():
                raise RuntimeError("srk_ba_reproj_error: " + msg)
            raise ValueError("srk_ba_reproj_error: " + msg)  # the reference CHECK-aborts on bad arguments (:420-421)
        self._f0 = float(f0)
        return float(e), int(seen.value)

    def ReprojErrorMvf(self, f0, scene, z_tol=1e-5):
        """MultiViewIterativeFactorizer::ReprojError (multi-view-factorization.cpp:415-475) -> (ok, err, summands):
        the score the MVF driver takes before deciding to run BA; observations with |z| <= z_tol are skipped and
        ok is False when nothing was summed."""
        e, n = C.c_double(0), C.c_int64(0)
        rc = self._lib.srk_ba_reproj_error_mvf(C.c_void_p(self._h), C.c_double(f0), *scene.scene_args(), C.c_double(z_tol),
                                               C.byref(e), C.byref(n))
        if rc < 0:
            msg = self.last_error()
            if "hip" in msg.lower():
                raise RuntimeError("srk_ba_reproj_error_mvf: " + msg)
            raise ValueError("srk_ba_reproj_error_mvf: " + msg)
        return rc == 1, float(e.value), int(n.value)

    def ReprojErrorPixPerPoint(self, reproj_err, seen_points_count):
        """f0 * sqrt(err / seen) (.cpp:602-615)."""
        return self._f0 * math.sqrt(reproj_err / float(seen_points_count))

    def OptimizationStatusString(self):
        return self._status

    def PointsCount(self):
        return self._scene.N

    def FramesCount(self):
        return self._scene.M

    def VarsCount(self):
        return 3 * self._scene.N + self.frame_vars() * self._scene.M + 4 * self.intrinsic_groups()

    def NormalizedVarsCount(self):
        return self.VarsCount() - 7

    # ---- staged API (resident scene)
    def upload(self, f0, scene, already_normalized=False):
        self._f0 = float(f0)
        self._scene = scene
        rc = self._lib.srk_ba_upload_scene(C.c_void_p(self._h), C.c_double(f0), *scene.scene_args(),
                                           C.c_int(int(already_normalized)))
        if rc == 1:
            return False
        self._raise(rc)
        return True

    def optimize(self, term_crit=None, max_iterations=0):
        a, m = self._criteria(term_crit)
        self.report = Report()
        rc = self._lib.srk_ba_optimize(C.c_void_p(self._h), a, m, C.c_int64(max_iterations), C.byref(self.report))
        self._raise(rc)
        self._status = status_string(self.report.status)
        return rc == 0

    def download(self, scene=None, revert_normalization=True):
        scene = scene or self._scene
        self._raise(self._lib.srk_ba_download_scene(C.c_void_p(self._h), _p(scene.points), _p(scene.cam_R),
                                                    _p(scene.cam_T), C.c_int(int(revert_normalization))))
        return scene

    def reset(self):
        self._raise(self._lib.srk_ba_reset_scene(C.c_void_p(self._h)))

    def set_speculation(self, on=True):
        """Run the next damping factor beside the current attempt (one rank, instrumentation off); next upload."""
        self._raise(self._lib.srk_ba_set_speculation(C.c_void_p(self._h), C.c_int(int(bool(on)))))

    def set_deterministic(self, on=True):
        """ordered sums instead of fp64 atomics (srk_ba_set_deterministic); takes effect at the next upload"""
        self._raise(self._lib.srk_ba_set_deterministic(C.c_void_p(self._h), C.c_int(int(bool(on)))))

    def deterministic(self):
        """True when the uploaded scene runs in deterministic mode (srk_ba_deterministic)"""
        return int(self._lib.srk_ba_deterministic(C.c_void_p(self._h))) == 1

    MULTI_SCHEDULES = {"allreduce": 0, "dp": 1, "dp_force": 2}

    def set_multi_schedule(self, schedule="dp"):
        """exchange schedule with several ranks (srk_ba_set_multi_schedule): "dp" (default), "allreduce", "dp_force"; before upload"""
        self._raise(self._lib.srk_ba_set_multi_schedule(C.c_void_p(self._h), C.c_int(self.MULTI_SCHEDULES[schedule])))

    def multi_schedule(self):
        """schedule in effect (srk_ba_multi_schedule): 'allreduce', 'dp', 'dp (self-check passed)', 'allreduce (dp self-check failed)'"""
        return {0: "allreduce", 1: "dp", 2: "dp (self-check passed)", 3: "allreduce (dp self-check failed)"}[
            int(self._lib.srk_ba_multi_schedule(C.c_void_p(self._h)))]

    def set_frame_reordering(self, mode=-1):
        """-1 automatic, 0 = keep the caller's frame order, 1 = renumber whenever the ordering differs (next upload)"""
        self._raise(self._lib.srk_ba_set_frame_reordering(C.c_void_p(self._h), C.c_int(mode)))

    def set_frame_order(self, to_internal=None):
        """The frame numbering to use at the next upload (None: automatic); landmark shards: the same on every rank, found on
        the whole scene with surikatoko_amd.frame_order()."""
        if to_internal is None:
            self._raise(self._lib.srk_ba_set_frame_order(C.c_void_p(self._h), None, C.c_int32(0)))
        else:
            a = np.ascontiguousarray(to_internal, dtype=np.int32)
            self._raise(self._lib.srk_ba_set_frame_order(C.c_void_p(self._h), _p(a), C.c_int32(a.size)))

    def frame_order(self):
        """None when the frames are stored in the caller's order, else to_internal[caller's frame]"""
        to_int = np.zeros(self._scene.M if self._scene is not None else 0, np.int32)
        rc = self._lib.srk_ba_frame_order(C.c_void_p(self._h), _p(to_int))
        if rc < 0:
            self._raise(rc)
        return to_int if rc == 1 else None

    def set_solver_fusion(self, on=True):
        """Outer steps of the blocked Cholesky as one launch each (default) or as the panel / update launch sequence."""
        self._raise(self._lib.srk_ba_set_solver_fusion(C.c_void_p(self._h), C.c_int(int(bool(on)))))

    def solver_fusion(self):
        """True while the fused outer step is in use (False after a hand-off timeout, until the next upload / optimise call)"""
        return bool(self._lib.srk_ba_solver_fusion(C.c_void_p(self._h)))

    def solver_sync_timeouts(self):
        self._lib.srk_ba_solver_sync_timeouts.restype = C.c_int64
        return int(self._lib.srk_ba_solver_sync_timeouts(C.c_void_p(self._h)))

    def iteration_log(self):
        """accepted iterations of the last optimise / ComputeInplace call: dict of arrays attempts, ms (host time since the
        call began), err, hessian_factor (srk_ba_iteration_log)"""
        fn = self._lib.srk_ba_iteration_log
        fn.restype = C.c_int64
        n = int(fn(C.c_void_p(self._h), C.c_int64(0), None, None, None, None))
        att = np.zeros(max(n, 1), dtype=np.int32)
        ms = np.zeros(max(n, 1))
        err = np.zeros(max(n, 1))
        fac = np.zeros(max(n, 1))
        fn(C.c_void_p(self._h), C.c_int64(n), att.ctypes.data_as(C.c_void_p), ms.ctypes.data_as(C.c_void_p),
           err.ctypes.data_as(C.c_void_p), fac.ctypes.data_as(C.c_void_p))
        return {"attempts": att[:n], "ms": ms[:n], "err": err[:n], "hessian_factor": fac[:n]}

    def set_jacobian_mode(self, mode=-1):
        """-1 automatic, 0 = per-observation kernels only, 1 = run-based (uniform runs) whenever possible, 2 = run-based over
        frame unions (ragged tracks) whenever possible (next upload)"""
        self._raise(self._lib.srk_ba_set_jacobian_mode(C.c_void_p(self._h), C.c_int(mode)))

    def jacobian_kernel(self):
        return int(self._lib.srk_ba_jacobian_kernel(C.c_void_p(self._h)))

    def set_storage_precision(self, f32=False):
        """W stored as float (next upload); arithmetic stays fp64 -- see include/srk_ba.h"""
        self._raise(self._lib.srk_ba_set_storage_precision(C.c_void_p(self._h), C.c_int(int(bool(f32)))))

    def set_fixed_intrinsics(self, on=True):
        """Calibrated BA (next upload): the intrinsics are constants, each frame has the 6 pose variables [Tx Ty Tz Wx Wy Wz]
        and the reduced camera system is 6M wide -- see include/srk_ba.h.  Not with deterministic mode, f32 storage, fp32
        Schur sums or more than one rank (ValueError)."""
        self._raise(self._lib.srk_ba_set_fixed_intrinsics(C.c_void_p(self._h), C.c_int(int(bool(on)))))

    def frame_vars(self):
        """variables per frame of the uploaded scene (before an upload: of the next one): 10, or 6 with fixed intrinsics"""
        n = int(self._lib.srk_ba_frame_vars(C.c_void_p(self._h)))
        self._raise(n)
        return n

    def set_intrinsic_groups(self, groups):
        """Shared intrinsics (next upload): groups[frame] = its camera group 0..G-1 (G <= 32, every
        group used), or None (off).  Each group's [fx fy u0 v0] is solved with the poses and points; frames of a group must
        carry the same K.  Not with fixed intrinsics, f32 storage, fp32 Schur sums or more than one rank (ValueError)."""
        if groups is None:
            self._raise(self._lib.srk_ba_set_intrinsic_groups(C.c_void_p(self._h), None, C.c_int32(0), C.c_int32(0)))
            return
        g = np.ascontiguousarray(groups, dtype=np.int32)
        n_groups = int(g.max()) + 1 if g.size else 0
        self._raise(self._lib.srk_ba_set_intrinsic_groups(C.c_void_p(self._h), g.ctypes.data_as(C.c_void_p),
                                                          C.c_int32(g.size), C.c_int32(n_groups)))

    def intrinsic_groups(self):
        """number of intrinsic groups of the uploaded scene (before an upload: of the next one); 0 = off"""
        n = int(self._lib.srk_ba_intrinsic_groups(C.c_void_p(self._h)))
        self._raise(n)
        return n

    def download_intrinsics(self):
        """the current K of every group, [G][3][3]"""
        G = self.intrinsic_groups()
        K = np.zeros((max(G, 0), 3, 3))
        self._raise(self._lib.srk_ba_download_intrinsics(C.c_void_p(self._h), K.ctypes.data_as(C.POINTER(C.c_double)),
                                                         C.c_int32(G)))
        return K

    _LOSSES = {None: 0, "none": 0, "huber": 1, "cauchy": 2}

    def set_robust_loss(self, kind=None, delta=1.0):
        """Robust bundle adjustment: kind "huber", "cauchy" or None (plain least squares, the
        default) with the scale delta in pixels.  Takes effect at the next optimise / phase call; ValueError for an unknown
        kind or a delta that is not finite and positive."""
        k = kind.lower() if isinstance(kind, str) else kind
        if k not in self._LOSSES:
            raise ValueError(f"unknown robust loss {kind!r}: 'huber', 'cauchy' or None")
        code = self._LOSSES[k]
        self._raise(self._lib.srk_ba_set_robust_loss(C.c_void_p(self._h), C.c_int(code), C.c_double(delta if code else 0.0)))

    def robust_loss(self):
        """(kind, delta_pixels): kind "huber", "cauchy" or None"""
        k, dl = C.c_int(0), C.c_double(0)
        self._raise(self._lib.srk_ba_robust_loss(C.c_void_p(self._h), C.byref(k), C.byref(dl)))
        return {0: None, 1: "huber", 2: "cauchy"}[k.value], dl.value

    def observation_weights(self):
        """IRLS weights w = rho'(s) of the resident scene's observations, in the caller's observation order (all 1 without
        a loss); outliers of a robust solve have w < 1"""
        size = int(self._lib.srk_ba_buffer_size(C.c_void_p(self._h), C.c_int(BUF_POINT_FRAME)))
        self._raise(size)
        fv = 10 if self.intrinsic_groups() else self.frame_vars()  # (the point-frame blocks stay 10 wide with groups)
        n = size // (3 * fv)  # observations of the resident scene (of this rank's shard)
        w = np.empty(n, dtype=np.float64)
        self._raise(self._lib.srk_ba_observation_weights(C.c_void_p(self._h), w.ctypes.data_as(C.POINTER(C.c_double)),
                                                         C.c_int64(n)))
        return w

    def _n_observations(self):
        size = int(self._lib.srk_ba_buffer_size(C.c_void_p(self._h), C.c_int(BUF_POINT_FRAME)))
        self._raise(size)
        fv = 10 if self.intrinsic_groups() else self.frame_vars()
        return size // (3 * fv)

    def set_observation_information(self, q=None):
        """Per-observation information: q[o] >= 0 multiplies observation o's squared residual,
        E = sum rho(q s); q in the caller's observation order, None clears it (the default).  Kept across uploads and
        reset_scene; with a scene resident it takes effect at the next optimise / phase call without another upload.
        ValueError (the previous setting stays) for a negative or non-finite value, a wrong count, or a landmark left with
        fewer than two observations of positive information."""
        if q is None:
            self._raise(self._lib.srk_ba_set_observation_information(C.c_void_p(self._h), None, C.c_int64(0)))
            self._info_n = None
            return
        q = np.ascontiguousarray(q, dtype=np.float64).ravel()
        self._raise(self._lib.srk_ba_set_observation_information(C.c_void_p(self._h), q.ctypes.data_as(C.POINTER(C.c_double)),
                                                                 C.c_int64(q.size)))
        self._info_n = int(q.size)

    def observation_information(self):
        """the information set on the handle in the caller's observation order; all 1 (one per observation of the resident
        scene) when none is set"""
        n = getattr(self, "_info_n", None)
        if n is None:
            n = self._n_observations()
        q = np.empty(n, dtype=np.float64)
        self._raise(self._lib.srk_ba_observation_information(C.c_void_p(self._h), q.ctypes.data_as(C.POINTER(C.c_double)),
                                                             C.c_int64(n)))
        return q

    def observation_residuals(self):
        """raw (unwhitened) residuals of the resident scene in pixels, [O, 2] in the caller's observation order: after an
        optimise call those of the result.  Neither information nor a loss changes them."""
        n = self._n_observations()
        e = np.empty((n, 2), dtype=np.float64)
        self._raise(self._lib.srk_ba_observation_residuals(C.c_void_p(self._h), e.ctypes.data_as(C.POINTER(C.c_double)),
                                                           C.c_int64(n)))
        return e

    def _const_flags(self, sel, n, what):
        """index list or boolean mask -> uint8 flags of length n (None stays None)"""
        if sel is None:
            return None
        a = np.asarray(sel)
        if a.dtype == np.bool_:
            if n is not None and a.size != n:
                raise ValueError(f"set_constant_blocks: the {what} mask has {a.size} entries, expected {n}")
            return np.ascontiguousarray(a.ravel(), dtype=np.uint8)
        if n is None:
            raise ValueError(f"set_constant_blocks: an index list of {what} needs the count (n_{what}=..., or an uploaded scene)")
        idx = a.astype(np.int64).ravel()
        if idx.size and (idx.min() < 0 or idx.max() >= n):
            raise ValueError(f"set_constant_blocks: a {what} index is out of range")
        flags = np.zeros(n, dtype=np.uint8)
        flags[idx] = 1
        return flags

    def set_constant_blocks(self, frames=None, points=None, keep_gauge=True, n_frames=None, n_points=None):
        """Constant parameter blocks (next upload): frames / points are index lists or boolean masks in
        the caller's numbering, None = none of that kind; both None clears the setting (the default).  A constant frame or
        landmark keeps its values bit for bit; its observations still count.  keep_gauge=True keeps the reference's seven
        gauge variables constant as well; with False the constant set alone must fix the similarity.  Index lists take the
        counts from n_frames / n_points or from the scene last passed to this object.  Not with intrinsic groups or more
        than one rank, and not with everything constant (ValueError)."""
        if frames is None and points is None:
            self._raise(self._lib.srk_ba_set_constant_blocks(C.c_void_p(self._h), None, C.c_int32(0), None, C.c_int64(0), C.c_int(1)))
            return
        if n_frames is None and self._scene is not None:
            n_frames = self._scene.M
        if n_points is None and self._scene is not None:
            n_points = self._scene.N
        ff = self._const_flags(frames, n_frames, "frames")
        pf = self._const_flags(points, n_points, "points")
        self._raise(self._lib.srk_ba_set_constant_blocks(
            C.c_void_p(self._h), _p(ff) if ff is not None else None, C.c_int32(ff.size if ff is not None else 0),
            _p(pf) if pf is not None else None, C.c_int64(pf.size if pf is not None else 0), C.c_int(int(bool(keep_gauge)))))

    def constant_blocks(self):
        """None when no constant blocks are set, else (frame_mask, point_mask, keep_gauge): boolean masks in the caller's
        numbering, None for a kind that was not given"""
        nf, npt, kg = C.c_int32(0), C.c_int64(0), C.c_int(1)
        rc = self._lib.srk_ba_constant_counts(C.c_void_p(self._h), C.byref(nf), C.byref(npt))
        self._raise(rc)
        if rc == 0:
            return None
        ff = np.zeros(nf.value, dtype=np.uint8)
        pf = np.zeros(npt.value, dtype=np.uint8)
        self._raise(self._lib.srk_ba_constant_blocks(C.c_void_p(self._h), _p(ff) if nf.value else None,
                                                     _p(pf) if npt.value else None, C.byref(kg)))
        return (ff.astype(bool) if nf.value else None, pf.astype(bool) if npt.value else None, bool(kg.value))

    def constant_pass_ms(self):
        """(landmark pass, frame pass): device ms of the last launch of the two masking passes, with set_profile >= 1"""
        a, b = C.c_double(0), C.c_double(0)
        self._raise(self._lib.srk_ba_constant_pass_ms(C.c_void_p(self._h), C.byref(a), C.byref(b)))
        return a.value, b.value

    def _prior_arrays(self, arg, what, sigma_pixels, itype):
        """(index, position, spec) or (index, position) with the information in a dict {'info': ...} -> sorted arrays"""
        if arg is None:
            return np.zeros(0, itype), np.zeros((0, 3)), np.zeros((0, 6))
        if len(arg) != 3:
            raise ValueError(f"set_position_priors: {what} = (index, position, spec)")
        idx, pos, spec = arg
        idx = np.asarray(idx).astype(itype).ravel()
        pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
        if pos.shape[0] != idx.size:
            raise ValueError(f"set_position_priors: {what}: one position per index")
        if isinstance(spec, dict):
            info = prior_information(n=idx.size, info=spec["info"])
        else:
            info = prior_information(spec, n=idx.size, sigma_pixels=sigma_pixels, f0=self._f0)
        if info.shape[0] != idx.size:
            raise ValueError(f"set_position_priors: {what}: one sigma / covariance / information matrix per index")
        order = np.argsort(idx, kind="stable")
        return np.ascontiguousarray(idx[order]), np.ascontiguousarray(pos[order]), np.ascontiguousarray(info[order])

    def set_position_priors(self, points=None, frames=None, keep_gauge=True, sigma_pixels=None):
        """Gaussian position priors (next upload): points / frames are (index, position, spec) in the
        caller's numbering and world coordinates -- landmark positions, camera centres C = -R^T T.  spec is a scalar sigma,
        per-axis sigmas [n][3], covariances [n][3][3] (world units; they need sigma_pixels, the pixel noise of the
        observations, and the f0 of the scene last passed to this object -- before the first scene, convert with
        prior_information(..., f0=...)), or {'info': L} with the information matrices [n][6] (xx xy xz yy yz zz) or [n][3][3]
        in units of the error per squared world unit.  The shapes are read as prior_information reads them.  Both None
        clears the setting (the default).  keep_gauge=True keeps the reference's seven gauge variables constant; with False
        the priors alone must fix the similarity.  Not with intrinsic groups or more than one rank (ValueError)."""
        pi, pp, pl = self._prior_arrays(points, "points", sigma_pixels, np.int64)
        fi, fp, fl = self._prior_arrays(frames, "frames", sigma_pixels, np.int32)
        self._raise(self._lib.srk_ba_set_position_priors(
            C.c_void_p(self._h), C.c_int64(pi.size), _p(pi) if pi.size else None, _p(pp) if pi.size else None,
            _p(pl) if pi.size else None, C.c_int32(fi.size), _p(fi) if fi.size else None, _p(fp) if fi.size else None,
            _p(fl) if fi.size else None, C.c_int(int(bool(keep_gauge)))))

    def position_priors(self):
        """None when no priors are set, else a dict: point_index, point_pos, point_info, frame_index, frame_centre, frame_info
        (information matrices as [n][6]: xx xy xz yy yz zz), keep_gauge -- the stored setting in the caller's coordinates"""
        n, m, kg = C.c_int64(0), C.c_int32(0), C.c_int(1)
        rc = self._lib.srk_ba_position_prior_counts(C.c_void_p(self._h), C.byref(n), C.byref(m))
        self._raise(rc)
        if rc == 0:
            return None
        pi, pp, pl = np.zeros(n.value, np.int64), np.zeros((n.value, 3)), np.zeros((n.value, 6))
        fi, fp, fl = np.zeros(m.value, np.int32), np.zeros((m.value, 3)), np.zeros((m.value, 6))
        q = lambda a: _p(a) if a.size else None
        self._raise(self._lib.srk_ba_position_priors(C.c_void_p(self._h), q(pi), q(pp), q(pl), q(fi), q(fp), q(fl), C.byref(kg)))
        return dict(point_index=pi, point_pos=pp, point_info=pl, frame_index=fi, frame_centre=fp, frame_info=fl,
                    keep_gauge=bool(kg.value))

    def prior_error(self):
        """(landmark prior sum, frame prior sum) of the resident scene's current state; phase_error() minus both is the
        observation part"""
        a, b = C.c_double(0), C.c_double(0)
        self._raise(self._lib.srk_ba_prior_error(C.c_void_p(self._h), C.byref(a), C.byref(b)))
        return a.value, b.value

    def prior_residuals(self):
        """(X - Xbar [n][3], C - Cbar [n][3]) of the resident scene's current state in the caller's world coordinates, in the
        order of position_priors()"""
        n, m = C.c_int64(0), C.c_int32(0)
        self._raise(self._lib.srk_ba_position_prior_counts(C.c_void_p(self._h), C.byref(n), C.byref(m)))
        dp, df = np.zeros((n.value, 3)), np.zeros((m.value, 3))
        self._raise(self._lib.srk_ba_prior_residuals(C.c_void_p(self._h), _p(dp) if n.value else None, _p(df) if m.value else None))
        return dp, df

    def prior_pass_ms(self):
        """(derivative-side pass, error-side pass): device ms of the last launch of the two prior passes, with set_profile >= 1"""
        a, b = C.c_double(0), C.c_double(0)
        self._raise(self._lib.srk_ba_prior_pass_ms(C.c_void_p(self._h), C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_relative_pose_factors(self, pairs=None, rel_R=None, rel_t=None, info=None, sigma_t=None, sigma_r=None, covariance=None,
                                  sigma_pixels=1.0):
        """Relative-pose factors between frames (next upload).  pairs [n][2] = (a, b) in the caller's
        numbering, sorted by (min, max); rel_R [n][3][3] measures R_a R_b^T, rel_t [n][3] measures R_a (C_b - C_a) in world
        units (relative_pose(scene, a, b) gives both for a scene's poses).  The information comes as info= ([n][21] upper
        triangle row by row in the order [t; r], or [n][6][6], in units of the error), as sigma_t= / sigma_r= (world units,
        radians) or as covariance= ([n][6][6]); the last two become L = (sigma_pixels / f0)^2 Sigma^-1 with the f0 of the
        scene last passed to this object.  pairs None or empty clears the setting.  There is no keep_gauge: the gauge is what
        set_constant_blocks / set_position_priors say.  Not with intrinsic groups or more than one rank (ValueError)."""
        if pairs is None or len(pairs) == 0:
            self._raise(self._lib.srk_ba_set_relative_pose_factors(C.c_void_p(self._h), C.c_int32(0), None, None, None, None, None))
            return
        pr = np.asarray(pairs).astype(np.int32).reshape(-1, 2)
        n = pr.shape[0]
        fa, fb = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        Z = np.ascontiguousarray(np.asarray(rel_R, dtype=np.float64).reshape(-1, 9))
        z = np.ascontiguousarray(np.asarray(rel_t, dtype=np.float64).reshape(-1, 3))
        if Z.shape[0] != n or z.shape[0] != n:
            raise ValueError("set_relative_pose_factors: one rotation and one translation per pair")
        L = relative_pose_information(n, info=info, sigma_t=sigma_t, sigma_r=sigma_r, covariance=covariance,
                                      sigma_pixels=sigma_pixels, f0=self._f0)
        self._raise(self._lib.srk_ba_set_relative_pose_factors(C.c_void_p(self._h), C.c_int32(n), _p(fa), _p(fb), _p(Z), _p(z), _p(L)))

    def relative_pose_factors(self):
        """None when no factors are set, else a dict: pairs [n][2], rel_R [n][3][3], rel_t [n][3], info [n][21] -- the stored
        setting in the caller's numbering and coordinates"""
        n = C.c_int32(0)
        rc = self._lib.srk_ba_relative_pose_factor_count(C.c_void_p(self._h), C.byref(n))
        self._raise(rc)
        if rc == 0:
            return None
        fa, fb = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
        Z, z, L = np.zeros((n.value, 9)), np.zeros((n.value, 3)), np.zeros((n.value, 21))
        self._raise(self._lib.srk_ba_relative_pose_factors(C.c_void_p(self._h), _p(fa), _p(fb), _p(Z), _p(z), _p(L)))
        return dict(pairs=np.stack([fa, fb], axis=1), rel_R=Z.reshape(-1, 3, 3), rel_t=z, info=L)

    def relative_pose_error(self):
        """the factor sum of the resident scene's current state; phase_error() minus this (and the prior sums) is the
        observation part"""
        e = C.c_double(0)
        self._raise(self._lib.srk_ba_relative_pose_error(C.c_void_p(self._h), C.byref(e)))
        return e.value

    def relative_pose_residuals(self):
        """[e_t; e_r] [n][6] of the resident scene's current state in the caller's world units and radians, in the order of
        relative_pose_factors()"""
        n = C.c_int32(0)
        self._raise(self._lib.srk_ba_relative_pose_factor_count(C.c_void_p(self._h), C.byref(n)))
        r = np.zeros((n.value, 6))
        self._raise(self._lib.srk_ba_relative_pose_residuals(C.c_void_p(self._h), _p(r) if n.value else None))
        return r

    def relative_pose_pass_ms(self):
        """(derivative-side pass, coupling pass, error-side pass): device ms of the last launch, with set_profile >= 1"""
        a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
        self._raise(self._lib.srk_ba_relative_pose_pass_ms(C.c_void_p(self._h), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def set_joint_pose_priors(self, sets=None, keep_gauge=True, sigma_pixels=None):
        """Joint Gaussian pose priors over sets of frames (next upload).  sets: a list of dicts with
        frames (k <= 16, caller's numbering, strictly ascending), R [k][3][3] and C [k][3] (or poses=(R, C)): the
        linearisation poses in the caller's world, info= [6k][6k] in units of the error or covariance= [6k][6k] (becomes
        L = (sigma_pixels / f0)^2 Sigma^-1 with the f0 of the scene last passed to this object), and optionally mean= [6k];
        joint_pose_prior_from_covariance builds one from a joint_covariance result.  The residual of a frame is
        [C - Cbar; Log(R^T Rbar)].  keep_gauge False releases the reference's gauge: the priors must then fix the seven
        freedoms.  None or empty clears the setting.  Not with intrinsic groups or more than one rank (ValueError)."""
        if sets is None or len(sets) == 0:
            self._raise(self._lib.srk_ba_set_joint_pose_priors(C.c_void_p(self._h), C.c_int32(0), None, None, None, None, None, None, C.c_int(1)))
            return
        ptr, fr, R, Cc, m, L = _joint_pose_prior_arrays(sets, sigma_pixels, self._f0)
        self._raise(self._lib.srk_ba_set_joint_pose_priors(C.c_void_p(self._h), C.c_int32(len(ptr) - 1), _p(ptr), _p(fr), _p(R), _p(Cc), _p(m),
                                                           _p(L), C.c_int(int(keep_gauge))))

    def joint_pose_priors(self):
        """None when no priors are set, else (sets, keep_gauge): the stored setting as a list of dicts frames, R, C, mean, info
        in the caller's numbering and coordinates"""
        ns, nq, ni = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        rc = self._lib.srk_ba_joint_pose_prior_counts(C.c_void_p(self._h), C.byref(ns), C.byref(nq), C.byref(ni))
        self._raise(rc)
        if rc == 0:
            return None
        ptr, fr = np.zeros(ns.value + 1, np.int32), np.zeros(nq.value, np.int32)
        R, Cc, m, L = np.zeros((nq.value, 9)), np.zeros((nq.value, 3)), np.zeros(6 * nq.value), np.zeros(ni.value)
        kg = C.c_int(1)
        self._raise(self._lib.srk_ba_joint_pose_priors(C.c_void_p(self._h), _p(ptr), _p(fr), _p(R), _p(Cc), _p(m), _p(L), C.byref(kg)))
        return _joint_pose_prior_sets(ptr, fr, R, Cc, m, L), bool(kg.value)

    def joint_pose_prior_error(self):
        """the priors' sum of the resident scene's current state"""
        e = C.c_double(0)
        self._raise(self._lib.srk_ba_joint_pose_prior_error(C.c_void_p(self._h), C.byref(e)))
        return e.value

    def joint_pose_prior_residuals(self):
        """r - m per set (a list of [6k] arrays) of the resident scene's current state in the caller's world units and
        radians, in the order of joint_pose_priors()"""
        ns, nq, ni = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        self._raise(self._lib.srk_ba_joint_pose_prior_counts(C.c_void_p(self._h), C.byref(ns), C.byref(nq), C.byref(ni)))
        ptr, r = np.zeros(ns.value + 1, np.int32), np.zeros(6 * nq.value)
        self._raise(self._lib.srk_ba_joint_pose_priors(C.c_void_p(self._h), _p(ptr), None, None, None, None, None, None))
        self._raise(self._lib.srk_ba_joint_pose_prior_residuals(C.c_void_p(self._h), _p(r) if nq.value else None))
        return [r[6 * int(ptr[g]):6 * int(ptr[g + 1])].copy() for g in range(ns.value)]

    def joint_pose_prior_pass_ms(self):
        """(derivative-side passes, coupling pass, error-side pass): device ms of the last launch, with set_profile >= 1"""
        a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
        self._raise(self._lib.srk_ba_joint_pose_prior_pass_ms(C.c_void_p(self._h), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def schur_fallback_landmarks(self):
        """landmarks of the uploaded scene that take the per-landmark Schur kernel (srk_ba_schur_fallback_landmarks)"""
        fn = self._lib.srk_ba_schur_fallback_landmarks
        fn.restype = C.c_int64
        n = int(fn(C.c_void_p(self._h)))
        self._raise(n)
        return n

    def set_schur_precision(self, fp32=False):
        """Opt-in mixed precision: fp32 run sums in the grouped Schur kernel (everything else stays fp64)."""
        self._raise(self._lib.srk_ba_set_schur_precision(C.c_void_p(self._h), C.c_int(int(bool(fp32)))))

    def set_profile(self, level=2):
        """0 = no device events (default of the library), 1 = per-phase events, 2 / True = + MFMA update events."""
        if level is True:
            level = 2
        self._raise(self._lib.srk_ba_set_profile(C.c_void_p(self._h), C.c_int(int(level))))

    def set_covisibility(self, min_cv):
        """Global covisibility for sharded runs (see covisibility()); None = dense."""
        if min_cv is None:
            self._raise(self._lib.srk_ba_set_covisibility(C.c_void_p(self._h), None))
        else:
            a = np.ascontiguousarray(min_cv, dtype=np.int32)
            self._raise(self._lib.srk_ba_set_covisibility(C.c_void_p(self._h), _p(a)))

    def set_rcs_mode(self, mode=2):
        """0 / False = dense, 1 = skyline as one chain, 2 / True = skyline cut into chunks (default)."""
        if mode is True:
            mode = 2
        self._raise(self._lib.srk_ba_set_rcs_mode(C.c_void_p(self._h), C.c_int(int(mode))))

    def rcs_chunks(self):
        return int(self._lib.srk_ba_rcs_chunks(C.c_void_p(self._h)))

    def solve_mfma_flops(self):
        return float(self._lib.srk_ba_solve_mfma_flops(C.c_void_p(self._h)))

    def rcs_fill(self):
        return float(self._lib.srk_ba_rcs_fill(C.c_void_p(self._h)))

    def set_stream(self, hip_stream_handle):
        self._raise(self._lib.srk_ba_set_stream(C.c_void_p(self._h), C.c_void_p(hip_stream_handle)))

    def set_allreduce(self, hook, rank, world):
        """hook: an ALLREDUCE_FN instance (see surikatoko_amd/dist.py); kept alive by this object."""
        self._hook = hook
        self._raise(self._lib.srk_ba_set_allreduce(C.c_void_p(self._h), hook, None, int(rank), int(world)))

    # native RCCL exchange (include/srk_ba.h): no Python in the data path
    def rccl_unique_id(self):
        """128 bytes of a fresh ncclUniqueId (rank 0 calls this and hands the bytes to the other ranks)."""
        buf = (C.c_ubyte * 128)()
        self._raise(self._lib.srk_ba_rccl_get_unique_id(buf))
        return bytes(buf)

    def rccl_init(self, unique_id, rank, world):
        """Collective: every rank creates the communicator on its handle's device; replaces an all-reduce callback."""
        assert len(unique_id) == 128
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        self._raise(self._lib.srk_ba_rccl_init(C.c_void_p(self._h), buf, C.c_int(int(rank)), C.c_int(int(world))))
        self._hook = None

    def rccl_init_second(self, unique_id):
        """Collective, after rccl_init: the second attempt slot's own communicator (keeps the attempt pairs with several ranks)."""
        assert len(unique_id) == 128
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        self._raise(self._lib.srk_ba_rccl_init_second(C.c_void_p(self._h), buf))

    def phase_error(self):
        e, seen = C.c_double(0), C.c_int64(0)
        self._raise(self._lib.srk_ba_phase_error(C.c_void_p(self._h), C.byref(e), C.byref(seen)))
        return e.value, seen.value

    def phase_derivatives(self):
        self._raise(self._lib.srk_ba_phase_derivatives(C.c_void_p(self._h)))

    def phase_schur(self, hessian_factor):
        self._raise(self._lib.srk_ba_phase_schur(C.c_void_p(self._h), C.c_double(hessian_factor)))

    def phase_solve(self):
        rc = self._lib.srk_ba_phase_solve(C.c_void_p(self._h))
        self._raise(rc)
        return rc == 0

    def phase_backsub(self, hessian_factor):
        self._raise(self._lib.srk_ba_phase_backsub(C.c_void_p(self._h), C.c_double(hessian_factor)))

    def phase_accept(self):
        self._raise(self._lib.srk_ba_phase_accept(C.c_void_p(self._h)))

    # ---- marginal covariances
    def _cov_selection(self, frames, points):
        M, N = self._scene.M, self._scene.N
        fr = np.arange(M, dtype=np.int32) if frames is None else np.ascontiguousarray(np.asarray(frames).reshape(-1), dtype=np.int32)
        pt = np.arange(N, dtype=np.int64) if points is None else np.ascontiguousarray(np.asarray(points).reshape(-1), dtype=np.int64)
        fv = self.frame_vars()
        return fr, pt, np.zeros((len(fr), fv, fv)), np.zeros((len(pt), 3, 3))

    def set_covariance_batch(self, max_columns=0):
        """cap a batch of right-hand-side columns of the covariance calls (harness knob; 0 = as many as fit 256 MB)"""
        self._raise(self._lib.srk_ba_set_covariance_batch(C.c_void_p(self._h), C.c_int64(int(max_columns))))

    def phase_covariance(self, frames=None, points=None):
        """(frame_blocks [n][FV][FV], point_blocks [n][3][3]): the diagonal blocks of the inverse of the system phase_schur(c) left
        in slot 0, in the resident (normalised) scene's variables; None = every frame / every landmark, an empty list = none.
        Consumes the system.  Raises numpy.linalg.LinAlgError when it is not positive definite."""
        fr, pt, fb, pb = self._cov_selection(frames, points)
        rc = self._lib.srk_ba_phase_covariance(C.c_void_p(self._h), C.c_int32(len(fr)), _p(fr) if len(fr) else None,
                                               _p(fb) if len(fr) else None, C.c_int64(len(pt)), _p(pt) if len(pt) else None,
                                               _p(pb) if len(pt) else None)
        self._raise(rc)
        if rc != 0:
            raise np.linalg.LinAlgError("srk_ba_phase_covariance: the system is not positive definite")
        return fb, pb

    def covariances(self, frames=None, points=None, sigma_pixels=1.0, caller_coordinates=True):
        """(frame_cov [n][FV][FV], point_cov [n][3][3]): marginal covariances of the resident scene's current state for pixel
        noise sigma_pixels, 2 (sigma_pixels / f0)^2 H^-1; in the coordinates of the uploaded arrays unless caller_coordinates is
        False.  None = every frame / every landmark, an empty list = none.  Raises numpy.linalg.LinAlgError when the undamped
        system is not positive definite (ten frame variables on a planar scene: use set_fixed_intrinsics)."""
        fr, pt, fb, pb = self._cov_selection(frames, points)
        rc = self._lib.srk_ba_covariances(C.c_void_p(self._h), C.c_double(float(sigma_pixels)), C.c_int32(len(fr)),
                                          _p(fr) if len(fr) else None, _p(fb) if len(fr) else None, C.c_int64(len(pt)),
                                          _p(pt) if len(pt) else None, _p(pb) if len(pt) else None, C.c_int(int(bool(caller_coordinates))))
        self._raise(rc)
        if rc != 0:
            raise np.linalg.LinAlgError("srk_ba_covariances: the system is not positive definite")
        return fb, pb

    # ---- cross-covariances between blocks and relative-pose covariances
    def _cross_args(self, frame_pairs, point_frame_pairs, point_pairs):
        """the nine pair arguments of the C calls, and the three output arrays"""
        fv = self.frame_vars()
        ff = np.asarray([] if frame_pairs is None else frame_pairs, dtype=np.int32).reshape(-1, 2)
        pf = np.asarray([] if point_frame_pairs is None else point_frame_pairs, dtype=np.int64).reshape(-1, 2)
        pp = np.asarray([] if point_pairs is None else point_pairs, dtype=np.int64).reshape(-1, 2)
        if pf.size and (pf[:, 1].min() < -2 ** 31 or pf[:, 1].max() >= 2 ** 31):
            raise ValueError("cross-covariances: a frame index is out of range")
        cols = [np.ascontiguousarray(ff[:, 0]), np.ascontiguousarray(ff[:, 1]), np.ascontiguousarray(pf[:, 0]),
                np.ascontiguousarray(pf[:, 1], dtype=np.int32), np.ascontiguousarray(pp[:, 0]), np.ascontiguousarray(pp[:, 1])]
        out = [np.zeros((len(ff), fv, fv)), np.zeros((len(pf), 3, fv)), np.zeros((len(pp), 3, 3))]
        args = []
        for k, o in enumerate(out):
            n = len(o)
            args += [C.c_int64(n), _p(cols[2 * k]) if n else None, _p(cols[2 * k + 1]) if n else None, _p(o) if n else None]
        return args, out, cols

    def phase_cross_covariance(self, frame_pairs=None, point_frame_pairs=None, point_pairs=None):
        """(frame x frame [n][FV][FV], landmark x frame [n][3][FV], landmark x landmark [n][3][3]): the requested blocks of the
        inverse of the system phase_schur(c) left in slot 0, in the resident (normalised) scene's variables.  frame_pairs
        [n][2] = (a, b): rows a, columns b; point_frame_pairs [n][2] = (landmark, frame); point_pairs [n][2]; caller's
        numbering, any order, repeats and a == b allowed.  Consumes the system.  Raises numpy.linalg.LinAlgError when it is
        not positive definite."""
        args, out, _keep = self._cross_args(frame_pairs, point_frame_pairs, point_pairs)
        rc = self._lib.srk_ba_phase_cross_covariance(C.c_void_p(self._h), *args)
        self._raise(rc)
        if rc != 0:
            raise np.linalg.LinAlgError("srk_ba_phase_cross_covariance: the system is not positive definite")
        return tuple(out)

    def cross_covariances(self, frame_pairs=None, point_frame_pairs=None, point_pairs=None, sigma_pixels=1.0, caller_coordinates=True):
        """the blocks of phase_cross_covariance for the resident scene's current state and pixel noise sigma_pixels,
        2 (sigma_pixels / f0)^2 H^-1; in the coordinates of the uploaded arrays unless caller_coordinates is False"""
        args, out, _keep = self._cross_args(frame_pairs, point_frame_pairs, point_pairs)
        rc = self._lib.srk_ba_cross_covariances(C.c_void_p(self._h), C.c_double(float(sigma_pixels)), *args,
                                                C.c_int(int(bool(caller_coordinates))))
        self._raise(rc)
        if rc != 0:
            raise np.linalg.LinAlgError("srk_ba_cross_covariances: the system is not positive definite")
        return tuple(out)

    def relative_pose_covariances(self, pairs, sigma_pixels=1.0):
        """[n][6][6]: the covariance, order [t; r], of the relative pose z = R_a (C_b - C_a), Z = R_a R_b^T of every pair
        (a, b), a != b, of the resident scene's current state, in the caller's world units and radians, cross term included"""
        pr = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        fa, fb = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        out = np.zeros((len(pr), 6, 6))
        rc = self._lib.srk_ba_relative_pose_covariances(C.c_void_p(self._h), C.c_double(float(sigma_pixels)), C.c_int32(len(pr)),
                                                        _p(fa) if len(pr) else None, _p(fb) if len(pr) else None,
                                                        _p(out) if len(pr) else None)
        self._raise(rc)
        if rc != 0:
            raise np.linalg.LinAlgError("srk_ba_relative_pose_covariances: the system is not positive definite")
        return out

    def joint_covariance(self, frames, points, sigma_pixels=1.0, caller_coordinates=True):
        """the dense symmetric covariance over [frames..., points...] (FV variables a frame, 3 a landmark), from one
        cross_covariances call with all pairs of the selection; meant for windows of tens of blocks"""
        fr = np.asarray(frames, dtype=np.int32).reshape(-1)
        pt = np.asarray(points, dtype=np.int64).reshape(-1)
        fv, nf, npt = self.frame_vars(), len(fr), len(pt)
        fi, fj = np.triu_indices(nf)
        pi, pj = np.triu_indices(npt)
        gi, gj = np.meshgrid(np.arange(npt), np.arange(nf), indexing="ij")
        ff, pf, pp = self.cross_covariances(np.stack([fr[fi], fr[fj]], axis=1), np.stack([pt[gi.ravel()], fr[gj.ravel()]], axis=1),
                                            np.stack([pt[pi], pt[pj]], axis=1), sigma_pixels, caller_coordinates)
        n = fv * nf + 3 * npt
        J = np.zeros((n, n))
        for k, (a, b) in enumerate(zip(fi, fj)):
            J[fv * a:fv * a + fv, fv * b:fv * b + fv] = ff[k]
            J[fv * b:fv * b + fv, fv * a:fv * a + fv] = ff[k].T
        for k, (i, j) in enumerate(zip(gi.ravel(), gj.ravel())):
            J[fv * nf + 3 * i:fv * nf + 3 * i + 3, fv * j:fv * j + fv] = pf[k]
            J[fv * j:fv * j + fv, fv * nf + 3 * i:fv * nf + 3 * i + 3] = pf[k].T
        for k, (a, b) in enumerate(zip(pi, pj)):
            J[fv * nf + 3 * a:fv * nf + 3 * a + 3, fv * nf + 3 * b:fv * nf + 3 * b + 3] = pp[k]
            J[fv * nf + 3 * b:fv * nf + 3 * b + 3, fv * nf + 3 * a:fv * nf + 3 * a + 3] = pp[k].T
        return J

    # ---- marginalisation priors in information form
    def _marg_args(self, frames, points):
        fr = np.ascontiguousarray(np.asarray([] if frames is None else frames).reshape(-1), dtype=np.int32)
        pt = np.ascontiguousarray(np.asarray([] if points is None else points).reshape(-1), dtype=np.int64)
        return fr, pt, [C.c_void_p(self._h), C.c_int32(len(fr)), _p(fr) if len(fr) else None, C.c_int64(len(pt)), _p(pt) if len(pt) else None]

    def marginalization_plan(self, frames, points):
        """the plan of marginalising the frames and landmarks given (caller's numbering, strictly ascending) on the resident
        scene, no kernel launched: (kept frames, counts dict).  Every refusal of the operation is a ValueError here."""
        fr, pt, args = self._marg_args(frames, points)
        cnt = MargCounts()
        kept = np.zeros(max(self._scene.M, 1), np.int32)
        self._raise(self._lib.srk_ba_marginalization_plan(*args, C.c_int32(kept.size), _p(kept), C.byref(cnt)))
        return kept[:cnt.n_kept].copy(), cnt.as_dict()

    def phase_marginalization(self, frames, points):
        """the staged form in the resident (normalised) scene's variables, dropped slots first, then the kept frames: a dict with
        kept, A0 / b0 (what the kernels give: observations and landmark priors, the landmarks eliminated), A1 / b1 (plus the
        host's factor terms) and report"""
        fr, pt, args = self._marg_args(frames, points)
        kept, _ = self.marginalization_plan(fr, pt)
        n = 6 * (len(fr) + len(kept))
        A0, b0, A1, b1 = np.zeros((n, n)), np.zeros(n), np.zeros((n, n)), np.zeros(n)
        nk, rep = C.c_int32(0), MargReport()
        kb = np.zeros(max(len(kept), 1), np.int32)
        self._raise(self._lib.srk_ba_phase_marginalization(*args, C.c_int32(len(kept)), _p(kb), C.byref(nk), _p(A0), _p(b0), _p(A1), _p(b1),
                                                           C.byref(rep)))
        return dict(kept=kb[:nk.value].copy(), A0=A0, b0=b0, A1=A1, b1=b1, report=rep.as_dict())

    def marginalization_prior(self, frames, points=None, sigma_pixels=None):
        """The Gaussian the factors touching the dropped frames and the marginalised landmarks leave on the frames that stay, in
        information form at the current poses (srk_ba_marginalization_prior).  points None: every landmark with a weighted
        observation in a dropped frame.  Returns a dict that set_joint_pose_priors accepts as a set (frames, R, C, info, mean; the
        frames in THIS scene's numbering -- renumber them for the reduced scene) plus eta and report; with sigma_pixels also
        information_metric = info / (sigma_pixels / f0)^2, the inverse covariance in world units.  Raises
        numpy.linalg.LinAlgError when the block of the dropped frames is not positive definite."""
        if points is None:
            points, _ = marginalization_landmarks(self._scene, frames, max_kept=self._scene.M, q=self.observation_information())
        fr, pt, args = self._marg_args(frames, points)
        kept, _ = self.marginalization_plan(fr, pt)
        k = len(kept)
        R, Cc, L, eta, m = np.zeros((k, 3, 3)), np.zeros((k, 3)), np.zeros((6 * k, 6 * k)), np.zeros(6 * k), np.zeros(6 * k)
        nk, rep = C.c_int32(0), MargReport()
        kb = np.zeros(max(k, 1), np.int32)
        rc = self._lib.srk_ba_marginalization_prior(*args, C.c_int32(k), _p(kb), C.byref(nk), _p(R), _p(Cc), _p(L), _p(eta), _p(m), C.byref(rep))
        self._raise(rc)
        if rc != 0:
            raise np.linalg.LinAlgError("srk_ba_marginalization_prior: " + self.last_error())
        out = dict(frames=kb[:nk.value].copy(), R=R, C=Cc, info=L, mean=m, eta=eta, report=rep.as_dict())
        if sigma_pixels is not None:
            out["information_metric"] = L / (float(sigma_pixels) / float(self._f0)) ** 2
        return out

    def triangulate(self, row_ptr, frame, uv, q=None, refine_attempts=0, refine_rel_change=1e-9, min_parallax_deg=0.0,
                    revert_normalization=True):
        """New landmarks from tracks over the resident scene's CURRENT poses and intrinsics, on the device (srk_ba_triangulate;
        after optimize(): the refined ones).  frame in the numbering of the uploaded scene.  Returns X [n][3] (in the uploaded
        arrays' coordinates with revert_normalization), quality [n][4] and status [n]: see triangulate.triangulate_tracks.  The
        resident scene is not modified."""
        from .triangulate import tri_options, tri_track_args
        n, rp, fr, m, w = tri_track_args(row_ptr, frame, uv, q)
        X, quality, status = np.zeros((n, 3)), np.zeros((n, 4)), np.zeros(n, np.uint32)
        opts = tri_options(refine_attempts, refine_rel_change, min_parallax_deg)
        self._raise(self._lib.srk_ba_triangulate(C.c_void_p(self._h), C.c_int64(n), _p(rp), _p(fr), _p(m), None if w is None else _p(w),
                                                 None if opts is None else C.byref(opts), C.c_int(int(bool(revert_normalization))), _p(X),
                                                 _p(quality), _p(status)))
        return X, quality, status

    def resect(self, row_ptr, point, uv, K, R0, T0, q=None, attempts=10, rel_change=1e-9, loss=None, delta=None, want_weights=False,
               revert_normalization=True):
        """The poses of new frames from their observations of the resident scene's CURRENT landmarks, on the device
        (srk_ba_resect; after optimize(): the refined ones).  point in the landmark numbering of the uploaded scene; K, R0, T0
        the new frames' intrinsics and predicted inverse poses in the uploaded arrays' coordinates.  Returns R, T, quality, info,
        status (and the robust weights with want_weights): see resect.resect_frames.  The resident scene is not modified."""
        from .resect import _outputs, _result, resect_frame_args, resect_options
        n, rp, pt, m, w, Kc, shared_k, R, T = resect_frame_args(row_ptr, point, uv, q, K, R0, T0)
        opts = resect_options(attempts, rel_change, loss, delta)
        out = _outputs(n, max(int(rp.max()), 0), want_weights)
        self._raise(self._lib.srk_ba_resect(C.c_void_p(self._h), C.c_int32(n), _p(rp), _p(pt), _p(m), None if w is None else _p(w), _p(Kc),
                                            C.c_int(int(shared_k)), _p(R), _p(T), C.byref(opts), C.c_int(int(bool(revert_normalization))),
                                            *[None if a is None else _p(a) for a in out]))
        return _result(out, want_weights)

    def locate(self, row_ptr, point, uv, K, q=None, hypotheses=256, inlier_pixels=4.0, seed=1, refine=None, want_inliers=False,
               want_weights=False, revert_normalization=True):
        """The poses of new frames from their observations of the resident scene's CURRENT landmarks alone, without a predicted
        pose, on the device (srk_ba_locate): P3P hypotheses scored on every observation, the best one optionally refined.  point
        in the landmark numbering of the uploaded scene; K the new frames' intrinsics.  Returns a locate.LocateResult: see
        locate.locate_frames.  The resident scene is not modified."""
        from .locate import LocateResult, _prepare
        frames, hyp, out, _keep = _prepare(row_ptr, point, uv, K, q, hypotheses, inlier_pixels, seed, refine, want_inliers, want_weights)
        self._raise(self._lib.srk_ba_locate(C.c_void_p(self._h), *frames, *hyp, C.c_int(int(bool(revert_normalization))),
                                            *[None if a is None else _p(a) for a in out]))
        return LocateResult(*out)

    def align(self, point, target, row_ptr=None, q=None, hypotheses=256, inlier_distance=None, seed=1, with_scale=True, refine_rounds=2,
              want_inliers=False, revert_normalization=True):
        """The similarity target ~ s R X + t between the resident scene's CURRENT landmarks `point` (the landmark numbering of the
        uploaded scene) and their targets [O][3] in another map, wrong correspondences among them, on the device (srk_ba_align;
        after optimize(): the refined landmarks).  row_ptr None: one set.  With revert_normalization the similarity maps the
        uploaded arrays' coordinates to the targets'.  Returns an align.AlignResult: see align.align_points.  The resident scene
        is not modified."""
        from .align import AlignResult, _options, _outputs
        pt = np.ascontiguousarray(point, dtype=np.int32).reshape(-1)
        b = np.ascontiguousarray(target, dtype=np.float64).reshape(-1, 3)
        w = None if q is None else np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
        rp = np.ascontiguousarray([0, pt.size] if row_ptr is None else row_ptr, dtype=np.int64).reshape(-1)
        n_obs = max(int(rp.max()), 0) if rp.size else 0
        if rp.size < 1 or pt.size < n_obs or b.shape[0] < n_obs or (w is not None and w.size < n_obs):
            raise ValueError("align: the correspondence arrays are shorter than row_ptr says")
        opts = _options(hypotheses, inlier_distance, seed, with_scale, refine_rounds)
        out = _outputs(rp.size - 1, n_obs, want_inliers)
        self._raise(self._lib.srk_ba_align(C.c_void_p(self._h), C.c_int32(rp.size - 1), _p(rp), _p(pt), _p(b), None if w is None else _p(w),
                                           C.byref(opts), C.c_int(int(bool(revert_normalization))), *[None if a is None else _p(a) for a in out]))
        return AlignResult(*out)

    def buffer(self, which):
        """flat download of a staged buffer; its layout follows frame_vars() (include/srk_ba.h SRK_BUF_*)"""
        n = self._lib.srk_ba_buffer_size(C.c_void_p(self._h), int(which))
        if n < 0:
            self._raise(int(n))
        out = np.zeros(max(n, 0))
        self._raise(self._lib.srk_ba_download(C.c_void_p(self._h), int(which), _p(out), C.c_int64(n)))
        return out

    def rcs_rows(self, rows):
        """rows of the padded reduced camera system (full frame-variable indexing, columns <= row filled); frame_vars() * M wide"""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        out = np.zeros((len(rows), self.frame_vars() * self._scene.M + 4 * self.intrinsic_groups()))
        self._raise(self._lib.srk_ba_download_rcs_rows(C.c_void_p(self._h), rows.ctypes.data_as(C.c_void_p),
                                                       C.c_int64(len(rows)), _p(out)))
        return out

    def dense_spd_solve(self, A, b):
        A = np.ascontiguousarray(A, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        n = A.shape[0]
        x = np.zeros(n)
        ms = C.c_double(0)
        rc = self._lib.srk_ba_dense_spd_solve(C.c_void_p(self._h), C.c_int64(n), _p(A), _p(b), _p(x), C.byref(ms))
        self._raise(rc)
        return rc == 0, x, ms.value

    # ---- helpers
    def last_error(self):
        return self._lib.srk_ba_last_error(C.c_void_p(self._h)).decode()

    def _criteria(self, term_crit):
        a = m = None
        self._keep = []
        if term_crit is not None:
            if term_crit.AllowedReprojErrRelativeChange() is not None:
                v = C.c_double(term_crit.AllowedReprojErrRelativeChange())
                self._keep.append(v)
                a = C.byref(v)
            if term_crit.MaxHessianFactor() is not None:
                v = C.c_double(term_crit.MaxHessianFactor())
                self._keep.append(v)
                m = C.byref(v)
        return a, m

    def _raise(self, rc):
        if rc >= 0:
            return
        msg = self.last_error()
        if rc == -1:
            raise ValueError("srk_ba: bad argument: " + msg)
        if rc == -3:
            raise RuntimeError("srk_ba: not possible in this state (no scene uploaded?): " + msg)
        if rc == -4:
            raise MemoryError("srk_ba: out of device memory: " + msg)
        raise RuntimeError("srk_ba: device error: " + msg)
