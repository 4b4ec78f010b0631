"""Cases of the marginalisation tests (tests/test_marginal_cpu.py, tests/test_gpu_marginal.py): scenes normalised on the host, the
frames D to drop, the landmarks P to marginalise and the settings beside them.  Strip widths: 6 n_slots + 1 columns padded to 16,
so n_slots in {1, 2, 3, 6, 17, 24, 40} gives partial and full tiles from one tile to the full sixteen; |P| in {0, 1, 5, 67, ~200,
1500} gives a partial K step, several of them and several workgroups' partial sums (512 rows = 128 landmarks a chunk).
"""
import numpy as np

import surikatoko_amd as sa
import constant_ref as kref
import covariance_cases as vc
import jointprior_ref as jr
import marginal_ref as mr
import prior_ref as pref
import relpose_ref as rr
import robust_ref as rob
import so3_ref as so3
import weighted_ref as wr

_cache = {}


def _norm(key, make):
    if key not in _cache:
        sc = make()
        ok, _ = sa.normalize_scene_inplace(sc)
        assert ok
        _cache[key] = sc
    return _cache[key].copy()


S8 = sa.SceneSpec(n_frames=8, grid_nx=10, grid_ny=8, vis_window=4, noise_uv_pix=0.3)
S12 = sa.SceneSpec(n_frames=12, grid_nx=10, grid_ny=8, vis_window=6, noise_uv_pix=0.3)
S40 = sa.SceneSpec(n_frames=40, grid_nx=50, grid_ny=30, vis_window=8, noise_uv_pix=0.3)


def s8():
    return _norm("s8", lambda: sa.generate_scene(S8)), S8.f0


def s12():
    return _norm("s12", lambda: sa.generate_scene(S12)), S12.f0


def s40():
    return _norm("s40", lambda: sa.generate_scene(S40)), S40.f0


def w8():
    return _norm("w8", lambda: sa.generate_scene(vc.W8_M70)), vc.W8_M70.f0


def w8_ragged():
    return _norm("w8r", lambda: sa.drop_observations(sa.generate_scene(vc.W8_M70), 0.2, seed=3)), vc.W8_M70.f0


def sub_scene(sc, keep):
    """the landmarks flagged in keep, all frames"""
    idx = np.flatnonzero(keep)
    rp = np.asarray(sc.row_ptr)
    obs = np.concatenate([np.arange(rp[i], rp[i + 1]) for i in idx])
    row_ptr = np.concatenate([[0], np.cumsum(rp[idx + 1] - rp[idx])]).astype(rp.dtype)
    return sa.Scene(sc.points[idx].copy(), sc.cam_R.copy(), sc.cam_T.copy(), sc.K, sc.shared_k, row_ptr,
                    np.ascontiguousarray(np.asarray(sc.obs_frame)[obs]), np.ascontiguousarray(np.asarray(sc.obs_uv)[obs]))


def tracks(sc):
    rp, fr = np.asarray(sc.row_ptr), np.asarray(sc.obs_frame)
    return [fr[rp[i]:rp[i + 1]] for i in range(sc.N)]


def seen_from(sc, frames):
    """landmarks with an observation in one of the frames, ascending"""
    return np.asarray([i for i, f in enumerate(tracks(sc)) if np.isin(f, frames).any()], dtype=np.int64)


def inside(sc, lo, hi):
    """landmarks whose tracks lie in the frames [lo, hi), ascending"""
    return np.asarray([i for i, f in enumerate(tracks(sc)) if f.min() >= lo and f.max() < hi], dtype=np.int64)


def _q_keep(sc, landmarks, n_keep):
    """information 1 everywhere, 0 on the observations behind the first n_keep of the landmarks given"""
    rp = np.asarray(sc.row_ptr)
    q = np.ones(int(rp[-1]))
    for i in landmarks:
        q[rp[i] + n_keep:rp[i + 1]] = 0.0
    return q


KERNEL_CASES = ["one_slot_centre_prior", "one_landmark_two_slots", "five_landmarks_three_slots", "w12_drop0", "w12_drop0_relpose_factor", "only_from_d",
                "ragged_huber_information_17_slots", "w8_24_slots_67", "w8_40_slots", "s40_1500_landmarks"]
EQUIVALENCE_CASES = ["w12_drop0", "w8_drop_two"]


def case(name):
    c = dict(name=name, fv=6, kind=rob.NONE, delta=None)
    if name == "one_slot_centre_prior":
        sc, f0 = s8()
        q = np.ones(sc.O)
        q[np.asarray(sc.obs_frame) == 3] = 0.0
        Cn = pref.centres(sc)
        pri = pref.Priors(fidx=[3, 5], fpos=Cn[[3, 5]] + [[0.01, -0.02, 0.005], [0.0, 0.01, 0.0]],
                          finfo=[np.diag([4.0, 2.0, 1.0]) + 0.5, np.eye(3)])
        c.update(scene=sc, f0=f0, D=[3], P=[], q=q, pri=pri, slots=1, used=0)
    elif name == "one_landmark_two_slots":
        sc, f0 = s8()
        c.update(scene=sc, f0=f0, D=[], P=[11], q=_q_keep(sc, [11], 2), slots=2, used=1)
    elif name == "five_landmarks_three_slots":
        sc, f0 = s8()
        five = [i for i, f in enumerate(tracks(sc)) if f[0] == 2][:5]
        once = [i for i, f in enumerate(tracks(sc)) if f[0] == 2][5]
        # (information may not leave a landmark with one weighted observation: a landmark seen once is one with a single observation)
        rp = np.asarray(sc.row_ptr)
        drop = np.zeros(sc.O, dtype=bool)
        drop[rp[once] + 1:rp[once + 1]] = True
        sc = wr.remove_observations(sc, drop)
        q = _q_keep(sc, five, 3)
        pri = pref.Priors(pidx=[five[1]], ppos=sc.points[[five[1]]] + 0.01, pinfo=[np.diag([3.0, 1.0, 2.0]) + 0.25])
        c.update(scene=sc, f0=f0, D=[], P=sorted(five + [once]), q=q, pri=pri, slots=3, used=5, skipped=1)
    elif name == "w12_drop0":
        sc, f0 = s12()
        c.update(scene=sc, f0=f0, D=[0], P=seen_from(sc, [0]), slots=6, used=len(seen_from(sc, [0])))
    elif name == "w12_drop0_relpose_factor":
        # a relative-pose factor (0, 2) is absorbed with the dropped frame 0; the factor (3, 7) is none of the call's business
        sc, f0 = s12()
        Z, z = zip(*[rr.relative_pose(sc, a, b) for a, b in ((0, 2), (3, 7))])
        Z = [Z[0] @ so3.exp(np.array([0.01, -0.02, 0.015])), Z[1]]
        z = [z[0] + [0.004, -0.002, 0.003], z[1]]
        fac = rr.Factors([0, 3], [2, 7], Z, z, [np.diag([40.0, 50.0, 60.0, 20.0, 25.0, 30.0]) + 2.0, np.eye(6)])
        c.update(scene=sc, f0=f0, D=[0], P=seen_from(sc, [0]), fac=fac, slots=6, used=len(seen_from(sc, [0])))
    elif name == "only_from_d":
        sc, f0 = s12()
        P = seen_from(sc, [0, 1])
        only = [i for i in P if tracks(sc)[i][0] == 0][:2]  # their weighted observations are those of frames 0 and 1 alone
        c.update(scene=sc, f0=f0, D=[0, 1], P=P, q=_q_keep(sc, only, 2), slots=7, used=len(P))
    elif name == "ragged_huber_information_17_slots":
        sc, f0 = w8_ragged()
        P = inside(sc, 30, 47)
        c.update(scene=sc, f0=f0, fv=10, D=[], P=P, q=wr.make_information(sc, 5), kind=rob.HUBER, delta=0.35, slots=17, used=len(P))
    elif name == "w8_24_slots_67":
        sc, f0 = w8()
        c.update(scene=sc, f0=f0, fv=10, D=[], P=inside(sc, 10, 34)[:67], slots=24, used=67)
    elif name == "w8_40_slots":
        sc, f0 = w8()
        P = inside(sc, 13, 53)
        c.update(scene=sc, f0=f0, D=list(range(20, 28)), P=P, slots=40, used=len(P), frame_order=np.random.RandomState(7).permutation(sc.M))
    elif name == "s40_1500_landmarks":
        sc, f0 = s40()
        c.update(scene=sc, f0=f0, D=list(range(8)), P=np.arange(sc.N), slots=40, used=sc.N)
    elif name == "w8_drop_two":
        sc, f0 = w8()
        c.update(scene=sc, f0=f0, D=[0, 1], P=seen_from(sc, [0, 1]))
    elif name == "lone_kept_frame":
        sc, f0 = s8()
        P = seen_from(sc, [0])
        c.update(scene=sc, f0=f0, D=[0], P=P, q=_q_keep(sc, P, 2))
    elif name == "chain":
        sc, f0 = s12()
        P0 = seen_from(sc, [0])
        P1 = np.setdiff1d(seen_from(sc, [1]), P0)
        c.update(scene=sc, f0=f0, P0=P0, P1=P1, **chain_reference(f0, sc, P0, P1))
    else:
        raise KeyError(name)
    return c


def set_on(h, c):
    """the case's settings on a surikatoko_amd.BundleAdjustmentKanatani, before the upload"""
    if c.get("q") is not None:
        h.set_observation_information(c["q"])
    if c.get("kind", rob.NONE) != rob.NONE:
        h.set_robust_loss({rob.HUBER: "huber", rob.CAUCHY: "cauchy"}[c["kind"]], c["delta"])
    if c.get("pri") is not None:
        c["pri"].set_on(h, True)
    if c.get("fac") is not None:
        c["fac"].set_on(h)
    if c.get("frame_order") is not None:
        h.set_frame_order(c["frame_order"])


def full_schur_complement(f0, sc, D):
    """the full scene's pose x pose system at c = 0 (factor-2 convention) with the frames D eliminated: (S, rhs) over the other
    frames' pose variables in their order, and the scaled condition number of the eliminated block"""
    g, V, U, W, _ = rob.derivatives(f0, sc)
    S, rhs, _ = kref.schur(sc, g, V, U, W, 0.0)
    D = np.asarray(D, dtype=np.int64)
    rest = np.setdiff1d(np.arange(sc.M), D)
    pose = lambda fr: (10 * fr[:, None] + 4 + np.arange(6)[None, :]).reshape(-1)  # noqa: E731
    d, r = pose(D), pose(rest)
    X = np.linalg.solve(S[np.ix_(d, d)], np.concatenate([S[np.ix_(d, r)], rhs[d, None]], axis=1))
    Sk = S[np.ix_(r, r)] - S[np.ix_(r, d)] @ X[:, :-1]
    return 0.5 * (Sk + Sk.T), rhs[r] - S[np.ix_(r, d)] @ X[:, -1], mr.scaled_cond(S[np.ix_(d, d)])


def chain_reference(f0, sc, P0, P1):
    """the chain identity on the yardstick alone: marginalise frame 0 with P0, absorb the result as a set while marginalising
    frame 1 with P1, against {0, 1} with P0 and P1 at once.  d_ref: the scaled distance of the two results, cond: the scaled
    condition number of the block of {0, 1}."""
    both = mr.system(f0, sc, [0, 1], np.union1d(P0, P1))
    Lb, eb = mr.eliminate(both["A1"], both["b1"], 2)
    one = mr.system(f0, sc, [0], P0)
    L1, e1 = mr.eliminate(one["A1"], one["b1"], 1)
    m1 = np.linalg.lstsq(L1, -e1, rcond=1e-13)[0]
    K1 = one["K"]
    R, Cn = sc.cam_R.reshape(-1, 3, 3), pref.centres(sc)
    sets = jr.Sets([dict(frames=K1, R=R[K1], C=Cn[K1], mean=m1, info=L1)])
    rp = np.asarray(sc.row_ptr)
    q = np.ones(int(rp[-1]))
    for i in P0:
        q[rp[i]:rp[i + 1]] = 0.0
    two = mr.system(f0, sc, [1], P1, q=q, sets=sets)
    L2, e2 = mr.eliminate(two["A1"], two["b1"], 1)
    assert list(two["K"]) == list(both["K"]) and two["sets"] == [0]
    dk = np.sqrt(np.abs(np.diag(Lb)))
    d_L = float((np.abs(L2 - Lb) / (dk[:, None] * dk[None, :])).max())
    d_e = float((np.abs(e2 - eb) / dk).max() / np.sqrt(rob.energy(f0, sc)))
    return dict(d_ref=max(d_L, d_e), cond=mr.scaled_cond(both["A1"][:12, :12]))
