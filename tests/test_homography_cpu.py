"""The two-view homography without a GPU: the yardstick (tests/homography_ref.py), the guards that keep the
compared decisions away from rounding, and the host half (surikatoko_amd/csrc/srk_homog.cpp): the argument checks, a walk of every
pair on the host in the kernels' own order of operations (srk_homography_host_pair), the decomposition on its own, and through a
stand-alone program (tests/cpp/test_homog_host.cpp) the sampler and the unit checks of the math header, the latter also under the
sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import homography as HG
import homography_cases as hc
import homography_ref as ref

from homography_cases import FIGURES, bounds, committed_figures, outlier_conditions


def cxx():
    return shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def build_host_program(out, extra=()):
    return subprocess.run([cxx(), "-std=c++17", "-O1", "-Wall", *extra, os.path.join(hc.ROOT, "tests", "cpp", "test_homog_host.cpp"),
                           os.path.join(hc.CSRC, "srk_homog.cpp"), "-o", str(out)], capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if cxx() is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("homog_bin") / "test_homog_host"
    r = build_host_program(exe)
    assert r.returncode == 0, r.stderr
    return str(exe)


# ------------------------------------------------------------------ the sampler
@pytest.mark.parametrize("n", [4, 5, 64, 1000])
def test_sampler_against_the_yardstick(program, tmp_path, n):
    out = str(tmp_path / "ranks.bin")
    for seed in (1, 0xFFFFFFFFFFFFFFFF):
        r = subprocess.run([program, "sampler", out, str(seed), str(n), "1024"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = np.fromfile(out, np.int64).reshape(1024, 4)
        want = np.array([ref.sample(seed, h, n) for h in range(1024)], dtype=np.int64)
        assert np.array_equal(got, want)
        assert got.min() >= 0 and got.max() < n
        assert all(len(set(row)) == 4 for row in got.tolist())
    if n > 5:
        assert len({tuple(row) for row in got.tolist()}) > 100          # and the draws differ from one another


# ------------------------------------------------------------------ the stand-alone program
def test_unit_checks_of_the_host_half(program):
    """the checks, the Jacobians against central differences, the Cholesky step, H = R + (T/d) N^T, proper rotations, three walks"""
    r = subprocess.run([program, "unit"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0 failure(s)", r.stdout + r.stderr


def test_unit_runs_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan"""
    if cxx() is None:
        pytest.skip("no host C++ compiler")
    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")             # whether the sanitizers' runtimes are there at all, asked of a trivial program
    r = subprocess.run([cxx(), *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("this compiler has no sanitizer runtime")
    exe = tmp_path / "test_homog_host_san"
    r = build_host_program(exe, flags)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), "unit"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0 failure(s)", r.stdout + r.stderr


def test_adjugate_basis_model_against_the_dlt(program, tmp_path):
    """noise-free samples of four matches (planes and rotations): the closed form through the projective basis against the SVD null
    space of the DLT matrix, as transfer distances at the corners of a 640 x 480 frame"""
    rng = np.random.default_rng(2710)
    ps = [hc.hpair(4, rng, "planar" if k % 2 else "rotation") for k in range(200)]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        np.array([len(ps)], np.int64).tofile(f)
        np.array([hc.F0]).tofile(f)
        np.array([p.uv_a for p in ps]).tofile(f)
        np.array([p.uv_b for p in ps]).tofile(f)
    r = subprocess.run([program, "model", src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(dst, np.uint8)
    G, ok = raw[:72 * len(ps)].view(np.float64).reshape(-1, 3, 3), raw[72 * len(ps):].view(np.int32)
    worst, compared = 0.0, 0
    for p, g, o in zip(ps, G, ok):
        want, margin = ref.dlt_model(p.uv_a, p.uv_b, hc.F0)
        assert (want is not None) == bool(o)
        if want is not None and margin > 1e-3:          # a sample's conditioning is 1 / margin: the well-spread ones carry the bound
            worst = max(worst, ref.corner_distance(g, want, hc.F0))
            compared += 1
            assert abs(np.linalg.norm(g) - 1.0) <= 1e-14 and (ref.homog(p.uv_a, hc.F0) @ g[2] > 0).all()
    print(f"adjugate basis against the DLT: largest corner distance {worst:.3e} px over {compared} samples")
    assert compared > 100 and worst <= 1e-9


def test_jacobi_eigenvalues_against_numpy(program, tmp_path):
    rng = np.random.default_rng(2711)
    A = rng.normal(size=(300, 3, 3))
    A = np.einsum("nij,nkj->nik", A, A)
    A[0], A[1], A[2] = np.eye(3), np.diag([3.0, 1.0, 1.0]), np.zeros((3, 3))
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        np.array([len(A)], np.int64).tofile(f)
        A.tofile(f)
    r = subprocess.run([program, "eig", src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got, want = np.fromfile(dst).reshape(-1, 3), np.linalg.eigvalsh(A)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


# ------------------------------------------------------------------ the guards
def _ragged_cases():
    for holes in (False, True):
        for H in hc.HYPOTHESES:
            for rounds in hc.ROUNDS:
                yield holes, H, rounds


def test_cases_have_a_clear_winner_and_no_pair_at_a_threshold():
    """On every committed pair the yardstick walks: for at least eight matches no other hypothesis within 1e-6 relative of the
    winner; no sample's triple within 10x of the collinearity bound, no q s within 1e-6 relative of tau^2 at a model whose inliers
    are taken, no gap within 10x of 1e-10, and no round between a tie to rounding and a clear decision.  No pair is skipped."""
    walked = 0
    for holes, H, rounds in _ragged_cases():
        scored = hc._scored(hc._ragged_t if holes else hc._ragged_f, H, hc.SAMPLER_SEED[(holes, H)], hc.TAU)
        for i, (A, y) in enumerate(zip(scored, hc.ragged_yardstick(holes, H, rounds))):
            assert y["status"] == 0, (holes, H, i)
            assert hc.at_a_threshold(A, y) is None, (holes, H, rounds, i, hc.at_a_threshold(A, y))
            assert y["homog"][1] < 8 or hc.winner_is_clear(y), (holes, H, i)
            walked += 1
    assert walked == 2 * len(hc.HYPOTHESES) * len(hc.ROUNDS) * len(hc.LENGTHS)


# ------------------------------------------------------------------ the host walk
def test_host_walk_against_the_yardstick_on_the_ragged_cases():
    """the kernels' order of operations on the host against the DLT / lstsq / SVD route: the same status, n, winner, inlier flags
    and counts; the score and G within the bounds the GPU tests use, which are ten times the largest distance measured here and
    written to profiles/homography/test_figures.json (never looser than 1e-6 relative / 1e-6 px)"""
    figures = []
    for holes, H, rounds in _ragged_cases():
        b = hc.ragged(holes)
        got = hc.host_walk(b, H, hc.SAMPLER_SEED[(holes, H)], rounds=rounds)
        hc.agree(b, hc.ragged_yardstick(holes, H, rounds), got, 1e-6, 1e-6, figures)
    score, pixels = max(f[0] for f in figures), max(f[1] for f in figures)
    print(f"host walk against the yardstick over {len(figures)} pairs: score {score:.3e} relative, corners {pixels:.3e} px")
    hc.write_figures("host_walk_against_yardstick", dict(score_relative=score, corner_pixels=pixels, pairs=len(figures)))
    fig = committed_figures()["host_walk_against_yardstick"]
    # the committed figures are this measurement: a run may differ from them by the libraries' rounding, not by a factor
    assert score <= 3.0 * fig["score_relative"] and pixels <= 3.0 * fig["corner_pixels"], (score, pixels, fig)
    assert 10.0 * fig["score_relative"] <= 1e-6 and 10.0 * fig["corner_pixels"] <= 1e-6


def test_host_walk_noise_free_planes():
    """40 matches on the plane, K_a != K_b: two poses, exactly one of them the truth (R, T / d with d the plane's distance from
    camera a, N) to 1e-9, the other not"""
    b, ps = hc.planar_pairs()
    got = hc.host_walk(b, 64, 1, tau=hc.OUTLIER_TAU)
    for i, p in enumerate(ps):
        assert got.status[i] == 0 and got.n_poses[i] == 2 and got.homog[i, 2] == 40 and got.inliers[40 * i:40 * i + 40].all()
        hc.check_poses(got, i)
        d = [max(np.abs(got.R[i, k] - p.R).max(), np.abs(got.T[i, k] - p.T / hc.PLANE_D).max(), np.abs(got.N[i, k] - hc.PLANE_N).max()) for k in range(2)]
        print(f"plane {i}: the candidates' distances from the truth {d[0]:.3e}, {d[1]:.3e}; gap {got.homog[i, 6]:.3e}")
        assert min(d) <= 1e-9 and max(d) > 1e-3
        assert got.front[i, 0] == 40
        assert ref.corner_distance(got.G[i], hc.true_homography(p), hc.F0) <= 1e-9


def test_host_walk_noise_free_rotations():
    """general points under a pure rotation: one pose, the rotation to 1e-9, T = N = 0, the gap at rounding, every match an inlier"""
    b, ps = hc.rotation_pairs()
    got = hc.host_walk(b, 64, 1, tau=hc.OUTLIER_TAU)
    for i, p in enumerate(ps):
        assert got.status[i] == 0 and got.n_poses[i] == 1 and got.homog[i, 6] <= 1e-10
        assert np.abs(got.R[i, 0] - p.R).max() <= 1e-9 and not got.T[i].any() and not got.N[i].any() and not got.R[i, 1].any()
        assert got.homog[i, 2] == 40 and got.inliers[40 * i:40 * i + 40].all()
        hc.check_poses(got, i)


@pytest.mark.parametrize("share", [0.3, 0.5])
def test_outliers_on_the_yardstick_then_on_the_host_walk(share):
    b, ps = hc.outliers(share)
    H = hc.outlier_hypotheses(share)
    assert H == {0.3: 26, 0.5: 108}[share] == sa.ransac_hypotheses(share, 0.999, 4)
    ys = hc.outlier_yardstick(share)
    want = outlier_conditions(b, ps, dict(inliers=[y["inliers"] for y in ys], G=[y["G"] for y in ys]))
    got = hc.host_walk(b, H, 1, tau=hc.OUTLIER_TAU, rounds=hc.OUTLIER_ROUNDS)
    have = outlier_conditions(b, ps, dict(inliers=[got.inliers[:200], got.inliers[200:]], G=got.G))
    print(f"share {share}: yardstick {want}, host walk {have}, rounds {got.homog[:, 5]}")
    hc.agree(b, ys, got, *bounds())


def test_host_walk_q_zero_is_the_pair_without_the_match():
    b = hc.rows(hc.ragged(True), range(len(hc.LENGTHS)))
    short, keep = hc.without_holes(b)
    x, y = hc.host_walk(b, 65, 7), hc.host_walk(short, 65, 7)
    for name in ("G", "H", "n_poses", "R", "T", "N", "front", "homog", "status"):
        assert np.array_equal(getattr(x, name).view(np.uint8), getattr(y, name).view(np.uint8)), name
    assert np.array_equal(x.inliers[keep], y.inliers) and not x.inliers[~keep].any()
    one = hc.SimpleNamespace(**{**vars(short), "q": np.ones_like(short.q)})
    none = hc.SimpleNamespace(**{**vars(short), "q": None})
    x, y = hc.host_walk(one, 65, 7), hc.host_walk(none, 65, 7)
    for name in ("G", "H", "R", "T", "N", "homog", "inliers"):
        assert np.array_equal(getattr(x, name).view(np.uint8), getattr(y, name).view(np.uint8)), name


def test_rounds_never_raise_the_score_and_none_returns_the_winner():
    b = hc.ragged(False)
    base = hc.host_walk(b, 64, 3, rounds=0)
    assert not base.homog[:, 5].any()
    for i in range(b.n):                        # the winning hypothesis unchanged: the model of its sample's four matches alone
        ua, ub, _ = hc.pair_obs(b, i)
        r = ref.sample(3, int(base.homog[i, 3]), len(ua))
        alone = HG.host_pair(b.f0, ua[r], ub[r], b.Ka[i], b.Kb[i], hypotheses=64, inlier_pixels=hc.TAU, seed=3, refine_rounds=0)
        assert ref.corner_distance(alone.G[0], base.G[i], b.f0) <= 1e-6
    last = base.homog[:, 0]
    for rounds in (1, 2, 4, 16):
        got = hc.host_walk(b, 64, 3, rounds=rounds)
        assert np.array_equal(got.homog[:, 3], base.homog[:, 3]) and (got.homog[:, 5] <= rounds).all()
        assert (got.homog[:, 0] <= last).all()
        last = got.homog[:, 0]
    assert (last < base.homog[:, 0]).any()


def test_decompose_homography_and_apply():
    b, ps = hc.planar_pairs()
    p = ps[0]
    H = p.R + np.outer(p.T, hc.PLANE_N) / hc.PLANE_D
    xa = ref.homog(p.uv_a, hc.F0) @ np.linalg.inv(p.Ka).T
    xb = ref.homog(p.uv_b, hc.F0) @ np.linalg.inv(p.Kb).T
    d = HG.decompose_homography(-3.0 * H, xa, xb)
    Hy, gap, poses = ref.decompose(-3.0 * H, xa, xb)
    assert d.n_poses == 2 and abs(d.gap - gap) <= 1e-12 and np.abs(d.H - Hy).max() <= 1e-13
    for k in range(2):
        assert min(max(np.abs(d.R[k] - R).max(), np.abs(d.T[k] - T).max(), np.abs(d.N[k] - N).max()) for R, T, N, _ in poses) <= 1e-12
        assert np.abs(d.H - (d.R[k] + np.outer(d.T[k], d.N[k]))).max() <= 1e-13
        assert np.abs(d.R[k] @ d.R[k].T - np.eye(3)).max() <= 1e-13 and abs(np.linalg.det(d.R[k]) - 1.0) <= 1e-13
    G = hc.true_homography(p)
    assert np.abs(HG.apply_homography(G, p.uv_a, hc.F0) - p.uv_b).max() <= 1e-9
    with pytest.raises(ValueError):
        HG.decompose_homography(H, xa, xb[:5])
    with pytest.raises(ValueError):
        HG.decompose_homography(H * np.nan, xa, xb)


# ------------------------------------------------------------------ the Python checks
def test_python_check_pairs_and_names():
    b = hc.ragged(True)
    args = (b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb)
    assert HG.check_pairs(*args, q=b.q) is None

    def bad(i, f, **kw):
        x = [np.array(v, copy=True) for v in args]
        f(x[i])
        return HG.check_pairs(*x, **{"q": b.q, **kw})
    assert "row_ptr[0]" in bad(0, lambda v: v.__setitem__(0, 1))
    assert "decreases at pair 3" in bad(0, lambda v: v.__setitem__(4, v[3] - 1))
    assert "decreases at pair 0" in bad(0, lambda v: v.__setitem__(1, -1))
    assert "uv_a of match 7 is not finite" in bad(1, lambda v: v.__setitem__((7, 1), np.nan))
    assert "uv_b of match 9 is not finite" in bad(2, lambda v: v.__setitem__((9, 0), np.inf))
    assert "K_a of pair 2 is not finite" in bad(3, lambda v: v.__setitem__((2, 1, 1), np.nan))
    assert "K_b of pair 1 is singular" in bad(4, lambda v: v.__setitem__((1, 2, 2), 0.0))
    q = b.q.copy()
    q[9] = -1.0
    assert "q of match 9" in HG.check_pairs(*args, q=q)
    q[9] = np.nan
    assert "q of match 9" in HG.check_pairs(*args, q=q)
    assert "hypotheses outside 1..4096" in HG.check_pairs(*args, hypotheses=0) and "hypotheses" in HG.check_pairs(*args, hypotheses=4097)
    for tau in (0.0, -1.0, np.nan, np.inf):
        assert "inlier_pixels" in HG.check_pairs(*args, inlier_pixels=tau)
    assert "refine_rounds outside 0..16" in HG.check_pairs(*args, refine_rounds=17) and "refine_rounds" in HG.check_pairs(*args, refine_rounds=-1)
    assert "split the batch" in HG.check_pairs(np.zeros((1 << 16) + 2, np.int64), np.zeros((0, 2)), np.zeros((0, 2)), hc.K0, hc.K1, hypotheses=4096)
    assert HG.default_homography_options() == dict(hypotheses=256, inlier_pixels=6.0, seed=1, refine_rounds=4)
    assert HG.homography_status_names(HG.HOMOGRAPHY_FEW_POINTS | HG.HOMOGRAPHY_NO_MODEL) == ["FEW_POINTS", "NO_MODEL"]
    assert sa.relate_homography is HG.relate_homography and sa.HOMOGRAPHY_NO_MODEL == 2
    assert sa.ransac_hypotheses(0.3, 0.999, 4) == 26 and sa.ransac_hypotheses(0.5, 0.999, 4) == 108
    with pytest.raises(ValueError):
        HG.check_pairs(b.row_ptr, b.uv_a[:5], b.uv_b, b.Ka, b.Kb)
    with pytest.raises(ValueError):
        HG.host_pair(hc.F0, b.uv_a[:5], b.uv_b[:4], hc.K0, hc.K1)
    with pytest.raises(ValueError):
        HG.host_pair(hc.F0, b.uv_a[:5], b.uv_b[:5], hc.K0, hc.K1, inlier_pixels=0.0)
