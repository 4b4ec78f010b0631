"""Marginalisation priors without a GPU: the host half (surikatoko_amd/csrc/srk_marg.cpp) and the host
terms of a factor and a set (srk_factors.cpp) through a stand-alone program (tests/cpp/test_marg_plan.cpp), the dense elimination
and the revert map through the library's host-only entry points, all against numpy; and the conditions the GPU cases must meet."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import ba as B
import jointprior_ref as jr
import marginal_cases as mc
import marginal_ref as mr
import relpose_ref as rr
import so3_ref as so3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surikatoko_amd", "csrc")
EPS = np.finfo(np.float64).eps


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


def _build(cxx, out, extra=()):
    return subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "test_marg_plan.cpp"),
                           os.path.join(CSRC, "srk_marg.cpp"), os.path.join(CSRC, "srk_factors.cpp"), os.path.join(CSRC, "srk_plan.cpp"),
                           "-pthread", "-o", str(out)], capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("marg_bin") / "test_marg_plan"
    r = _build(_cxx(), exe)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _ints(v):
    v = np.asarray(v).reshape(-1)
    return f"{v.size} " + " ".join(str(int(x)) for x in v)


def _dbl(v):
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    return f"{v.size} " + " ".join(float(x).hex() for x in v)


def _plan_file(path, sc, D, P, q=None, frame_int=None, pt_prior=(), fr_prior=(), rp=((), ()), sets=(), flags=(0, 0, 0)):
    """the scene as the plan reads it; the internal landmark order is the caller's, the frames go through frame_int"""
    fi = np.arange(sc.M) if frame_int is None else np.asarray(frame_int)
    rp_ptr = np.asarray(sc.row_ptr)
    fr = fi[np.asarray(sc.obs_frame)]
    ptr, frames = [0], []
    for s in sets:
        frames += [int(fi[j]) for j in s]
        ptr.append(len(frames))
    lines = [str(sc.N), str(sc.M), _ints(rp_ptr), _ints(fr), _dbl([] if q is None else q), _ints(np.arange(sc.N)),
             _ints([] if frame_int is None else fi), _ints(pt_prior), _ints(sorted(int(fi[j]) for j in fr_prior)),
             _ints([fi[a] for a in rp[0]]), _ints([fi[b] for b in rp[1]]), _ints(ptr if sets else []), _ints(frames),
             *[str(int(f)) for f in flags], _ints(D), _ints(P)]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def _run_plan(program, path):
    r = subprocess.run([program, "plan", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    if lines[0].startswith("refused"):
        return lines[0][8:]
    head = [int(x) for x in lines[0].split()[1:]]
    out = dict(zip(("d", "k", "ldz", "n_rows", "n_stage", "n_single"), head))
    for line in lines[1:]:
        w = line.split()
        out[w[0]] = np.asarray([int(x) for x in w[1:]], dtype=np.int64)
    return out


# ------------------------------------------------------------------ the cases

def test_cases_are_well_conditioned_and_cover_the_strip_widths():
    """scaled condition numbers of A_DD and of every V_l below 1e10; the slot counts and landmark counts the kernels' paths need"""
    slots, used = set(), set()
    for name in mc.KERNEL_CASES + mc.EQUIVALENCE_CASES:
        c = mc.case(name)
        r = mr.system(c["f0"], c["scene"], c["D"], c["P"], c.get("q"), c["kind"], c["delta"], c.get("pri"), c.get("fac"))
        assert r["cond_V"] < 1e10
        nd = 6 * len(c["D"])
        if nd and r["used"].any():
            cond = mr.scaled_cond(r["A1"][:nd, :nd])
            print(f"{name}: cond(A_DD) {cond:.3e}, largest cond(V_l) {r['cond_V']:.3e}")
            assert cond < 1e10
        slots.add(len(r["slots"]))
        used.add(int(r["used"].sum()))
        if "slots" in c:
            assert len(r["slots"]) == c["slots"] and int(r["used"].sum()) == c["used"] and r["skipped"] == c.get("skipped", 0)
    assert {1, 2, 3, 17, 24, 40} <= slots and {1, 5, 67, 1500} <= used


def test_chain_identity_on_the_yardstick_alone():
    c = mc.case("chain")
    bound = 64 * EPS * c["cond"]
    print(f"chain identity, yardstick alone: d_ref {c['d_ref']:.3e}, cond(A_DD) {c['cond']:.3e}, bound {bound:.3e}")
    assert c["d_ref"] < 0.1 * bound


# ------------------------------------------------------------------ the plan

@pytest.mark.parametrize("name", ["five_landmarks_three_slots", "only_from_d", "w8_40_slots", "ragged_huber_information_17_slots"])
def test_plan_tables_against_the_numpy_selection(program, tmp_path, name):
    c = mc.case(name)
    sc, D, P, q = c["scene"], c["D"], c["P"], c.get("q")
    fi = c.get("frame_order")
    path = str(tmp_path / "plan")
    _plan_file(path, sc, D, P, q, fi)
    p = _run_plan(program, path)
    sel, single, K, _, _ = mr.select(sc, D, P, q)
    assert list(p["kept"]) == list(K) and (p["d"], p["k"]) == (len(D), len(K)) and p["n_single"] == single
    assert list(p["lm"]) == list(np.flatnonzero(sel)) and p["ldz"] == -(-(6 * (len(D) + len(K)) + 1) // 16) * 16
    fint = np.arange(sc.M) if fi is None else np.asarray(fi)
    assert list(p["slot_frame"]) == [int(fint[j]) for j in list(D) + list(K)]
    assert all(p["frame_slot"][p["slot_frame"][s]] == s for s in range(p["d"] + p["k"])) and (p["frame_slot"] >= 0).sum() == p["d"] + p["k"]
    rp = np.asarray(sc.row_ptr)
    cnt = rp[p["lm"] + 1] - rp[p["lm"]]
    assert list(p["lm_row"]) == list(4 * np.arange(len(p["lm"]))) and p["n_rows"] == 4 * len(p["lm"])
    assert list(p["lm_stage"]) == list(np.concatenate([[0], np.cumsum(cnt)[:-1]])) and p["n_stage"] == cnt.sum()
    # per slot: the staging rows of the weighted observations of its frame, landmarks ascending
    qq = np.ones(sc.O) if q is None else q
    want = [[] for _ in range(p["d"] + p["k"])]
    for l, i in enumerate(p["lm"]):
        for o in range(rp[i], rp[i + 1]):
            if qq[o] > 0:
                want[p["frame_slot"][fint[sc.obs_frame[o]]]].append(p["lm_stage"][l] + o - rp[i])
    assert list(p["slot_ptr"]) == list(np.concatenate([[0], np.cumsum([len(w) for w in want])]))
    assert list(p["slot_ent"]) == [e for w in want for e in w]


def test_plan_selects_priors_factors_and_whole_sets(program, tmp_path):
    sc, _ = mc.s12()
    P = mc.seen_from(sc, [0, 1])
    path = str(tmp_path / "plan")
    stays = int(np.setdiff1d(np.arange(sc.N), P)[0])  # a prior on a landmark that stays is none of the call's business
    pri = sorted([int(P[2]), stays])
    _plan_file(path, sc, [0, 1], P, pt_prior=pri, fr_prior=[1, 7], rp=([0, 3, 1], [2, 4, 9]), sets=[[1, 5, 11], [2, 6], [0, 3]])
    p = _run_plan(program, path)
    assert list(p["factors"]) == [0, 2] and list(p["sets"]) == [0, 2] and list(p["fr_priors"]) == [0]
    assert list(p["kept"]) == [2, 3, 4, 5, 6, 9, 11]
    assert list(p["lm_prior"]) == [pri.index(int(P[2])) if i == P[2] else -1 for i in p["lm"]]


def test_every_refusal(program, tmp_path):
    sc, _ = mc.w8()
    path = str(tmp_path / "plan")
    big = np.arange(sc.N)
    for D, P, flags, text in (([], [], (0, 0, 0), "both lists are empty"), ([3, 2], [], (0, 0, 0), "strictly ascending"),
                              ([2, 2], [], (0, 0, 0), "strictly ascending"), ([], [5, 4], (0, 0, 0), "strictly ascending"),
                              ([sc.M], [], (0, 0, 0), "beyond the scene"), ([-1], [], (0, 0, 0), "beyond the scene"),
                              ([], [sc.N], (0, 0, 0), "beyond the scene"), (list(range(9)), [], (0, 0, 0), "at most 8 frames"),
                              ([0], [], (0, 0, 0), "is observed from the dropped frame 0"), ([], big, (0, 0, 0), "70 kept frames, at most 32"),
                              ([], [1], (1, 0, 0), "constant blocks"), ([], [1], (0, 1, 0), "intrinsic groups"), ([], [1], (0, 0, 1), "more than one rank")):
        _plan_file(path, sc, D, P, flags=flags)
        why = _run_plan(program, path)
        assert isinstance(why, str) and text in why, (D, why)
    # switching the dropped frame's observations of the staying landmarks off lifts the observation refusal
    P, q = sa.marginalization_landmarks(sc, [0], max_kept=7)  # (tracks of 8 frames: 7 others)
    _plan_file(path, sc, [0], P, q)
    p = _run_plan(program, path)
    assert isinstance(p, dict) and p["k"] <= 7 and len(P) > 0


# ------------------------------------------------------------------ the host terms of a factor and a set

def _rot(axis, ang):
    return so3.exp(np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis) * ang) if ang else np.eye(3)


class _Poses:
    def __init__(self, R, T):
        self.cam_R, self.cam_T = np.asarray(R).reshape(-1, 9), np.asarray(T).reshape(-1, 3)


ANGLES = [0.0, 1e-9, 0.05, 1.0]


def _parse_terms(text, n):
    lines = text.splitlines()
    H = [np.array([float.fromhex(v) for v in lines[2 * i].split()[1:]]) for i in range(n)]
    g = [np.array([float.fromhex(v) for v in lines[2 * i + 1].split()[1:]]) for i in range(n)]
    return H, g


def test_relative_pose_terms_against_the_yardstick(program, tmp_path):
    rng = np.random.RandomState(3)
    path, rows, want = str(tmp_path / "rp"), [], []
    for ang in ANGLES:
        Ra, Rb = _rot([1, 2, 3], 0.4), _rot([-1, 0.5, 2], 0.9)
        Ta, Tb = rng.randn(3), rng.randn(3)
        so = _Poses([Ra, Rb], [Ta, Tb])
        Z0, z0 = rr.relative_pose(so, 0, 1)
        Z = Z0 @ _rot([0.3, -1, 0.2], ang).T  # the residual rotation Log(Z^T R_a R_b^T) has the angle asked for
        z = z0 + 0.01 * rng.randn(3)
        G = rng.randn(6, 6)
        L = G @ G.T
        fac = rr.Factors([0], [1], [Z], [z], [L])
        e, Ja, Jb = rr.jacobians(fac, so)
        assert abs(np.linalg.norm(e[0, 3:]) - ang) < 1e-12
        J = np.concatenate([Ja[0], Jb[0]], axis=1)
        want.append((J.T @ L @ J, J.T @ L @ e[0]))
        rows.append(" ".join(_dbl(v) for v in (Ra, Ta, Rb, Tb, Z, z, L)))
    with open(path, "w") as f:
        f.write(f"{len(rows)}\n" + "\n".join(rows) + "\n")
    r = subprocess.run([program, "relpose", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    H, g = _parse_terms(r.stdout, len(rows))
    for (Hw, gw), Hg, gg, ang in zip(want, H, g, ANGLES):
        eh, eg = np.abs(Hg.reshape(12, 12) - Hw).max() / np.abs(Hw).max(), np.abs(gg - gw).max() / max(np.abs(gw).max(), 1e-300)
        print(f"relative-pose terms at {ang} rad: H {eh:.2e}, g {eg:.2e}")
        assert eh < 1e-12 and eg < 1e-12


def test_joint_set_terms_against_the_yardstick(program, tmp_path):
    rng = np.random.RandomState(4)
    path, rows, want = str(tmp_path / "jp"), [], []
    for ang in ANGLES:
        k = 3
        R = np.stack([_rot(rng.randn(3), 0.3 + 0.2 * i) for i in range(k)])
        T = rng.randn(k, 3)
        so = _Poses(R, T)
        _, Cn = rr.poses(so)
        Rbar = np.stack([R[i] @ _rot(rng.randn(3), ang) for i in range(k)])  # Log(R^T Rbar) has the angle asked for
        Cbar = Cn + 0.01 * rng.randn(k, 3)
        G = rng.randn(6 * k, 6 * k)
        L = G @ G.T
        m = 0.01 * rng.randn(6 * k)
        s = dict(frames=np.arange(k, dtype=np.int32), R=Rbar, C=Cbar, mean=m, info=L)
        e, J = jr.jacobian(s, so)
        assert abs(np.linalg.norm((e + m)[3:6]) - ang) < 1e-12
        want.append((J.T @ L @ J, J.T @ L @ e))
        lin = np.concatenate([Rbar.reshape(k, 9), Cbar], axis=1)
        rows.append(f"{k} " + " ".join(_dbl(v) for v in (R, T, lin, m, L)))
    with open(path, "w") as f:
        f.write(f"{len(rows)}\n" + "\n".join(rows) + "\n")
    r = subprocess.run([program, "jprior", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    H, g = _parse_terms(r.stdout, len(rows))
    for (Hw, gw), Hg, gg, ang in zip(want, H, g, ANGLES):
        eh, eg = np.abs(Hg.reshape(Hw.shape) - Hw).max() / np.abs(Hw).max(), np.abs(gg - gw).max() / np.abs(gw).max()
        print(f"joint-set terms at {ang} rad: H {eh:.2e}, g {eg:.2e}")
        assert eh < 1e-12 and eg < 1e-12


# ------------------------------------------------------------------ the dense elimination

def _spd(rng, n, cond=1e3):
    Q, _ = np.linalg.qr(rng.randn(n, n))
    return (Q * np.logspace(0, np.log10(cond), n)) @ Q.T


@pytest.mark.parametrize("d,k", [(0, 2), (1, 1), (2, 5), (8, 32)])
def test_dense_elimination_against_numpy(d, k):
    rng = np.random.RandomState(10 * d + k)
    n = 6 * (d + k)
    A = _spd(rng, n)
    A = 0.5 * (A + A.T)
    b = rng.randn(n)
    L, eta, m, defect = sa.marginalize_dense(A, b, d, k)
    Lr, er = mr.eliminate(A, b, d)
    scale = np.sqrt(np.diag(Lr))
    bound = 64 * EPS * (mr.scaled_cond(A[:6 * d, :6 * d]) if d else 1.0) * n
    assert np.array_equal(L, L.T)
    assert (np.abs(L - Lr) / (scale[:, None] * scale[None, :])).max() < bound
    assert (np.abs(eta - er) / scale).max() < bound * np.abs(er / scale).max() * n
    mr_ = np.linalg.solve(Lr, -er)
    assert np.abs(m - mr_).max() < 64 * EPS * np.linalg.cond(Lr) * np.abs(mr_).max()
    assert defect < 64 * EPS * np.linalg.cond(Lr)


def test_dense_elimination_of_a_gauge_free_system():
    """the information of a real selection is singular along the seven gauge directions: Lam keeps them as null directions, m is
    a basic solution with zero components at the null pivots, and the defect stays below 64 eps cond (cond over the range)"""
    c = mc.case("w12_drop0")
    r = mr.system(c["f0"], c["scene"], c["D"], c["P"])
    d, k = 1, len(r["K"])
    L, eta, m, defect = sa.marginalize_dense(r["A1"], r["b1"], d, k)
    Lr, er = mr.eliminate(r["A1"], r["b1"], d)
    dk = np.sqrt(np.diag(Lr))
    assert (np.abs(L - Lr) / (dk[:, None] * dk[None, :])).max() < 64 * EPS * mr.scaled_cond(r["A1"][:6, :6])
    w = np.linalg.eigvalsh(Lr / dk[:, None] / dk[None, :])
    # the translations and the scale of the world are null to rounding; at this noisy (not optimised) scene the three rotations
    # of the world are only nearly so (scaled eigenvalues of 1e-8 .. 1e-6)
    n0 = int((w < 1e-12 * w.max()).sum())
    assert n0 == 4 and (w[4:7] < 1e-5 * w.max()).all()
    cond = w.max() / w[n0]
    print(f"gauge-free Lam: scaled eigenvalues {w[:8]}, cond over the range {cond:.3e}, defect {defect:.3e}, zero components {int((m == 0).sum())}")
    assert defect < 64 * EPS * cond and (m == 0).sum() == n0
    # the energy of the basic solution is the minimum: Lam m = -eta up to the defect
    assert np.abs(Lr @ m + er).max() <= 64 * EPS * cond * np.abs(er).max()


def test_dense_elimination_refuses_a_block_that_is_not_positive_definite():
    rng = np.random.RandomState(2)
    A = _spd(rng, 18)
    A[:6, :6] -= 2.0 * np.linalg.eigvalsh(A[:6, :6]).min() * np.eye(6)
    with pytest.raises(np.linalg.LinAlgError):
        sa.marginalize_dense(A, rng.randn(18), 1, 2)
    c = mc.case("lone_kept_frame")
    r = mr.system(c["f0"], c["scene"], c["D"], c["P"], c["q"])
    with pytest.raises(np.linalg.LinAlgError):  # one kept frame: the scale of the dropped frame's pose is free
        sa.marginalize_dense(r["A1"], r["b1"], 1, len(r["K"]))
    with pytest.raises(ValueError):
        sa.marginalize_dense(np.full((12, 12), np.nan), np.zeros(12), 1, 1)


# ------------------------------------------------------------------ the revert map

def test_revert_after_normalize_is_the_identity_and_keeps_the_energy():
    rng = np.random.RandomState(5)
    sc = sa.generate_scene(mc.S12)
    scn = sc.copy()
    ok, nrm = sa.normalize_scene_inplace(scn)
    assert ok
    k = 5
    fr = np.array([1, 2, 4, 7, 9], dtype=np.int32)
    R, Cn = rr.poses(sc)
    G = rng.randn(6 * k, 6 * k)
    L = G @ G.T
    m = 0.1 * rng.randn(6 * k)
    eta = -L @ m
    st = dict(frames=fr, R=R[fr], C=Cn[fr], mean=m, info=L)
    sn = B.normalize_joint_pose_priors(nrm, [st])[0]
    D = np.zeros((6 * k, 6 * k))
    R0 = np.array(list(nrm.R0)).reshape(3, 3)
    for i in range(k):
        D[6 * i:6 * i + 3, 6 * i:6 * i + 3] = nrm.world_scale * R0
        D[6 * i + 3:6 * i + 6, 6 * i + 3:6 * i + 6] = R0
    eta_n = np.linalg.solve(D.T, eta)
    Rb, Cb, Lb, eb, mb = sa.revert_marginalization_prior(nrm, sn["R"], sn["C"], sn["info"], eta_n, sn["mean"])
    for got, want in ((Rb, st["R"]), (Cb, st["C"]), (Lb, L), (eb, eta), (mb, m)):
        assert np.abs(got - want).max() < 1e-12 * max(np.abs(want).max(), 1.0)
    x = rng.randn(6 * k)
    e_w, e_n = mr.energy(L, eta, x), mr.energy(sn["info"], eta_n, D @ x)
    assert abs(e_w - e_n) < 1e-12 * abs(e_w)
    # the poses of the normalised scene map back onto the scene's
    Rn, Cnn = rr.poses(scn)
    Rb, Cb = sa.revert_marginalization_prior(nrm, Rn[fr], Cnn[fr])[:2]
    assert np.abs(Rb - R[fr]).max() < 1e-12 and np.abs(Cb - Cn[fr]).max() < 1e-12 * np.abs(Cn).max()


def test_marginalization_landmarks_bounds_the_kept_frames():
    sc, _ = mc.w8()
    for max_kept in (6, 10, 16):
        P, q = sa.marginalization_landmarks(sc, [10, 11], max_kept=max_kept)
        sel, single, K, _, _ = mr.select(sc, [10, 11], P, q)
        assert len(K) <= max_kept and single == 0 and sel.sum() == len(P) > 0


# ------------------------------------------------------------------ sanitizers

def test_unit_runs_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan over a plan with every family, a refusal and the host terms"""
    exe = tmp_path / "test_marg_plan_san"
    r = _build(_cxx(), exe, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    sc, _ = mc.s12()
    P = mc.seen_from(sc, [0, 1])
    path = str(tmp_path / "plan")
    _plan_file(path, sc, [0, 1], P, pt_prior=[int(P[2])], fr_prior=[1], rp=([0], [2]), sets=[[1, 5, 11]], frame_int=np.random.RandomState(1).permutation(sc.M))
    assert isinstance(_run_plan(str(exe), path), dict)
    _plan_file(path, sc, [0], [])
    assert isinstance(_run_plan(str(exe), path), str)
    w8, _ = mc.w8()
    _plan_file(path, w8, [], np.arange(w8.N))
    assert "kept frames" in _run_plan(str(exe), path)
    rp_file = str(tmp_path / "rp")
    eye, z3 = np.eye(3), np.zeros(3)
    with open(rp_file, "w") as f:
        f.write("1\n" + " ".join(_dbl(v) for v in (eye, z3, _rot([0, 0, 1], 0.3), np.ones(3), eye, np.ones(3), np.eye(6))) + "\n")
    r = subprocess.run([str(exe), "relpose", rp_file], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    jp_file = str(tmp_path / "jp")
    with open(jp_file, "w") as f:
        f.write("1\n2 " + " ".join(_dbl(v) for v in (np.stack([eye, eye]), np.zeros((2, 3)), np.concatenate([np.tile(eye.reshape(1, 9), (2, 1)), np.ones((2, 3))], axis=1),
                                                      np.zeros(12), np.eye(12))) + "\n")
    r = subprocess.run([str(exe), "jprior", jp_file], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
