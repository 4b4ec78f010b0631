"""The two-view fundamental matrix without a GPU: the yardstick (tests/fundamental_ref.py) and the host half
(surikatoko_amd/csrc/srk_fund.cpp): the argument checks, a walk of every pair on the host in the kernels' own order of operations
(srk_fundamental_host_pair), the Python helpers, and through a stand-alone program (tests/cpp/test_fund_host.cpp) the sampler, the
seven-point model and the unit checks of the math header, the latter also under the sanitizers."""
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import fundamental as FD
from surikatoko_amd import homography as HG
import fundamental_cases as fc
import fundamental_ref as ref

from fundamental_cases import bounds, committed_figures


def cxx():
    return shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def build_host_program(out, extra=()):
    return subprocess.run([cxx(), "-std=c++17", "-O1", "-Wall", *extra, os.path.join(fc.ROOT, "tests", "cpp", "test_fund_host.cpp"),
                           os.path.join(fc.CSRC, "srk_fund.cpp"), "-o", str(out)], capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if cxx() is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("fund_bin") / "test_fund_host"
    r = build_host_program(exe)
    assert r.returncode == 0, r.stderr
    return str(exe)


# ------------------------------------------------------------------ the sampler
@pytest.mark.parametrize("n", [8, 9, 64, 1000])
def test_sampler_against_the_yardstick(program, tmp_path, n):
    out = str(tmp_path / "ranks.bin")
    for seed in (1, 0xFFFFFFFFFFFFFFFF):
        r = subprocess.run([program, "sampler", out, str(seed), str(n), "1024"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = np.fromfile(out, np.int64).reshape(1024, 8)
        want = np.array([ref.sample(seed, h, n) for h in range(1024)], dtype=np.int64)
        assert np.array_equal(got, want)
        assert got.min() >= 0 and got.max() < n
        assert all(len(set(row)) == 8 for row in got.tolist())
    if n > 9:
        assert len({tuple(row) for row in got.tolist()}) > 1000          # and the draws differ from one another


def test_sampler_has_a_stream_of_its_own():
    """the odd constant is none of locate's, relate's, align's and the homography's"""
    import align_ref
    import homography_ref
    import locate_ref
    import relate_ref
    mine = ref.mix(1, 0, 0)
    assert all(mine != m.mix(1, 0, 0) for m in (align_ref, homography_ref, locate_ref, relate_ref))


# ------------------------------------------------------------------ the stand-alone program
def test_unit_checks_of_the_host_half(program):
    """every text of the argument checks, the Jacobian against central differences, the 7 x 7 Cholesky step, F = U diag(1, sigma, 0)
    V^T with proper U, V (sigma = 1 and sigma near 0 included), the cubic with a vanishing leading coefficient, three walks"""
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
    exe = tmp_path / "test_fund_host_san"
    r = build_host_program(exe, flags)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), "unit"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0 failure(s)", r.stdout + r.stderr


def test_seven_point_model_against_the_truth_and_the_yardstick(program, tmp_path):
    """400 noise-free samples of seven matches (and the eighth that chooses) from general scenes: the best root against the true
    K_b^-T [T]x R K_a^-1 within 1e-9 entry by entry after norm and sign, on every sample whose seventh singular value exceeds 1e-4 of
    the first; the numbers of samples with one and with three real roots are the yardstick's, and both occur"""
    ps = fc.samples()
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        np.array([len(ps)], np.int64).tofile(f)
        np.array([fc.F0]).tofile(f)
        np.array([p.uv_a for p in ps]).tofile(f)
        np.array([p.uv_b for p in ps]).tofile(f)
    r = subprocess.run([program, "model", src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(dst, np.uint8)
    n = len(ps)
    F = raw[:72 * n].view(np.float64).reshape(-1, 3, 3)
    roots, ok = raw[72 * n:76 * n].view(np.int32), raw[76 * n:].view(np.int32)
    worst, worst_ref, compared, want_roots = 0.0, 0.0, 0, []
    for p, g, k, o in zip(ps, F, roots, ok):
        Fs, ratio = ref.seven_point(p.uv_a[:7], p.uv_b[:7], fc.F0)
        want_roots.append(len(Fs))
        assert o == 1 and k == len(Fs), (k, len(Fs), ratio)
        if ratio > 1e-4:
            truth = fc.true_fundamental(p)
            worst = max(worst, np.abs(ref.canonical(g) - truth).max())
            worst_ref = max(worst_ref, min(np.abs(ref.canonical(y) - truth).max() for y in Fs))
            compared += 1
            assert abs(np.linalg.norm(g) - 1.0) <= 1e-14
    ones, threes = int((roots == 1).sum()), int((roots == 3).sum())
    print(f"seven-point model against the truth: {worst:.3e} (the SVD route {worst_ref:.3e}) over {compared} of {n} samples; "
          f"{ones} with one real root, {threes} with three")
    assert ones == want_roots.count(1) and threes == want_roots.count(3) and ones > 0 and threes > 0 and ones + threes == n
    assert compared >= 390 and worst <= 1e-9
    fc.write_figures("seven_point_against_truth", dict(library=worst, svd_route=worst_ref, compared=compared, one_root=ones, three_roots=threes))


# ------------------------------------------------------------------ the host walk
def _ragged_cases():
    for holes in (False, True):
        for H in fc.HYPOTHESES:
            for rounds in fc.ROUNDS:
                yield holes, H, rounds


def test_host_walk_against_the_yardstick_on_the_ragged_cases():
    """the kernels' order of operations on the host against the SVD / polyfit / central-difference route: the same status, n, models,
    winner, inlier flags and counts; the score and F within the bounds the GPU tests use, which are ten times the largest distance
    measured here and written to profiles/fundamental/test_figures.json (never looser than 1e-6 relative / 1e-6 an entry).  The two
    routes differ in the Jacobian (exact against central differences with a step of 1e-6: 1e-10 relative) and so in every step;
    both stop by the same 1e-9 rule, after which the remaining step is of order 1e-8."""
    figures = []
    for holes, H, rounds in _ragged_cases():
        b = fc.ragged(holes)
        got = fc.host_walk(b, H, fc.SAMPLER_SEED, rounds=rounds)
        fc.agree(b, fc.ragged_yardstick(holes, H, rounds), got, 1e-6, 1e-6, figures)
    score, entry = max(f[0] for f in figures), max(f[1] for f in figures)
    print(f"host walk against the yardstick over {len(figures)} pairs: score {score:.3e} relative, F {entry:.3e} an entry")
    fc.write_figures("host_walk_against_yardstick", dict(score_relative=score, f_entry=entry, pairs=len(figures)))
    fig = committed_figures()["host_walk_against_yardstick"]
    # the committed figures are this measurement: a run may differ from them by the libraries' rounding, not by a factor
    assert score <= 3.0 * fig["score_relative"] and entry <= 3.0 * fig["f_entry"], (score, entry, fig)
    assert 10.0 * fig["score_relative"] <= 1e-6 and 10.0 * fig["f_entry"] <= 1e-6


def test_host_walk_noise_free_general_pairs():
    """every match an inlier, F the truth to 1e-9, the epipoles the projections of the other camera's centre to 1e-9"""
    b, ps = fc.general_pairs()
    got = fc.host_walk(b, 64, 1)
    for i, p in enumerate(ps):
        assert got.status[i] == 0 and got.fund[i, 2] == 40 and got.inliers[40 * i:40 * i + 40].all()
        fc.check_model(got, i)
        assert np.abs(got.F[i] - fc.true_fundamental(p)).max() <= 1e-9
        # camera b's centre -R^T T seen in a, camera a's centre (the origin) seen in b: homogeneous in (u, v, f0)
        ea, eb = p.Ka @ (-p.R.T @ p.T), p.Kb @ p.T
        for e, col in ((ea, got.V[i][:, 2]), (eb, got.U[i][:, 2])):
            e = e / np.linalg.norm(e)
            assert min(np.abs(col - e).max(), np.abs(col + e).max()) <= 1e-9


def test_noise_free_planes_and_rotations_have_no_model_and_the_homography_has():
    b, ps = fc.degenerate_pairs()
    got = fc.host_walk(b, 64, 1)
    assert (got.status == FD.FUNDAMENTAL_NO_MODEL).all() and not got.fund[:, 4].any() and not got.F.any()
    for i, p in enumerate(ps):
        ua, ub, _ = fc.pair_obs(b, i)
        for h in range(64):                      # every sample is without a model on the yardstick too
            r = ref.sample(1, h, 40)
            assert ref.seven_point(ua[r[:7]], ub[r[:7]], b.f0)[1] <= 1e-12
        hg = HG.host_pair(b.f0, ua, ub, p.Ka, p.Kb, hypotheses=64, seed=1)
        assert hg.status[0] == 0 and hg.homog[0, 2] == 40


def test_an_essential_matrix_has_sigma_one_and_the_rounds_never_raise_the_score():
    """K the identity in f0 units: F is an essential matrix, sigma = 1, the rotations of U and V about their third axes are one
    direction; the damped step is still defined, cond_1 reports it, the status stays 0"""
    b, p = fc.essential_pair()
    last = None
    for rounds in (0, 1, 2, 4, 8, 16):
        got = fc.host_walk(b, 64, 1, rounds=rounds)
        assert got.status[0] == 0
        fc.check_model(got, 0)
        assert last is None or got.fund[0, 0] <= last
        last = got.fund[0, 0]
        print(f"essential pair, {rounds} rounds: rms {got.fund[0, 0]:.6f}, sigma {got.sigma[0]:.6f}, cond_1 {got.fund[0, 10]:.3e}")
        assert got.sigma[0] >= 0.99
        assert np.isnan(got.fund[0, 10]) or got.fund[0, 10] >= 1e4
    assert np.abs(got.F[0] - fc.true_fundamental(p)).max() <= 1e-2


@pytest.mark.parametrize("share", [0.3, 0.5])
def test_outliers_on_the_yardstick_then_on_the_host_walk(share):
    b, ps = fc.outliers(share)
    H = fc.OUTLIER_HYPOTHESES[share]
    assert H >= sa.ransac_hypotheses(share, 0.999, 7) == ref.ransac_hypotheses(share, 0.999, 7)
    ys = fc.outlier_yardstick(share)
    got = fc.host_walk(b, H, 1, rounds=fc.OUTLIER_ROUNDS)
    for i, (p, y) in enumerate(zip(ps, ys)):
        moved = np.zeros(200, bool)
        moved[p.moved] = True
        flags = got.inliers[200 * i:200 * i + 200].astype(bool)
        ua, ub, _ = fc.pair_obs(b, i)
        in_band = int((np.abs(ref.sampson(y["F"], ua, ub, b.f0) - fc.TAU ** 2) <= fc.BAND).sum())
        print(f"share {share} pair {i}: {flags[~moved].mean():.3f} of the unmoved and {flags[moved].mean():.3f} of the moved flagged, "
              f"score {y['start']:.1f} -> {y['fund'][0] ** 2 * 200:.1f} px^2 in {int(y['fund'][7])} attempts, {in_band} matches in the band")
        assert in_band == 0
        assert flags[~moved].mean() >= 0.9 and flags[moved].mean() <= 0.05
    fc.agree(b, ys, got, *bounds())


def test_host_walk_q_zero_is_the_pair_without_the_match():
    b = fc.ragged(True)
    short, keep = fc.without_holes(b)
    x, y = fc.host_walk(b, 65, 7), fc.host_walk(short, 65, 7)
    for name in ("F", "U", "V", "sigma", "fund", "info", "status"):
        assert np.array_equal(getattr(x, name).view(np.uint8), getattr(y, name).view(np.uint8)), name
    assert np.array_equal(x.inliers[keep], y.inliers) and not x.inliers[~keep].any()
    one = SimpleNamespace(**{**vars(short), "q": np.ones_like(short.q)})
    none = SimpleNamespace(**{**vars(short), "q": None})
    x, y = fc.host_walk(one, 65, 7), fc.host_walk(none, 65, 7)
    for name in ("F", "U", "V", "sigma", "fund", "info", "inliers"):
        assert np.array_equal(getattr(x, name).view(np.uint8), getattr(y, name).view(np.uint8)), name


def test_rounds_never_raise_the_score_and_none_returns_the_winner():
    b = fc.ragged(False)
    base = fc.host_walk(b, 64, 3, rounds=0)
    assert not base.fund[:, 6].any() and not base.fund[:, 7].any()
    for i in range(1, b.n):                     # the winning hypothesis unchanged: the model of its sample's eight matches alone
        ua, ub, _ = fc.pair_obs(b, i)
        r = ref.sample(3, int(base.fund[i, 3]), len(ua))
        F, _, _ = ref.hypothesis(ua[r], ub[r], b.f0)
        U, V, sg = ref.represent(F)
        assert np.abs(ref.canonical(ref.build(U, V, sg)) - base.F[i]).max() <= 1e-9
    last = base.fund[1:, 0]
    for rounds in (1, 2, 8, 16):
        got = fc.host_walk(b, 64, 3, rounds=rounds)
        assert np.array_equal(got.fund[1:, 3], base.fund[1:, 3]) and (got.fund[1:, 7] <= rounds).all()
        assert (got.fund[1:, 0] <= last).all()
        last = got.fund[1:, 0]
    assert (last < base.fund[1:, 0]).any()


# ------------------------------------------------------------------ the Python helpers
def test_epipolar_lines_pass_through_the_matches():
    b, ps = fc.general_pairs()
    p = ps[0]
    F = fc.true_fundamental(p)
    l = FD.epipolar_lines(F, p.uv_a, fc.F0)
    assert np.abs(np.linalg.norm(l[:, :2], axis=1) - 1.0).max() <= 1e-14
    assert np.abs(np.sum(ref.homog(p.uv_b, fc.F0) * l, axis=1)).max() <= 1e-9
    l = FD.epipolar_lines(F.T, p.uv_b, fc.F0)
    assert np.abs(np.sum(ref.homog(p.uv_a, fc.F0) * l, axis=1)).max() <= 1e-9


def test_pose_from_fundamental_on_a_noise_free_pair():
    b, ps = fc.general_pairs()
    got = fc.host_walk(b, 64, 1)
    for i, p in enumerate(ps):
        R, T = FD.pose_from_fundamental(got.F[i], p.Ka, p.Kb, p.uv_a, p.uv_b, fc.F0, inliers=got.inliers[40 * i:40 * i + 40])
        assert np.abs(R - p.R).max() <= 1e-8 and np.abs(T - p.T).max() <= 1e-8, (i, np.abs(R - p.R).max(), np.abs(T - p.T).max())


def test_bootstrap_from_the_fundamental_matrix_next_to_relate():
    """relate's noisy bootstrap case (150 landmarks, 0.5 px of noise, 20 % wrong matches) on the host walks: the pose from
    pose_from_fundamental and relate's own, each refined by the pair refinement's host walk over its model's inliers.  Both RMS
    figures go to test_figures.json; nothing is asserted between them."""
    from surikatoko_amd import pair as PR
    from surikatoko_amd import relate as RL
    from test_gpu_relate import _bootstrap_case
    c = _bootstrap_case()
    fd = FD.host_pair(fc.F0, c.uv_a, c.uv_b, hypotheses=256, seed=1)
    R0, T0 = FD.pose_from_fundamental(fd.F[0], fc.K0, fc.K0, c.uv_a, c.uv_b, fc.F0, inliers=fd.inliers)
    rl = RL.host_pair(fc.F0, c.uv_a, c.uv_b, fc.K0, fc.K0, hypotheses=256, inlier_pixels=fc.TAU, seed=1)
    a = PR.host_pair(fc.F0, c.uv_a, c.uv_b, fc.K0, fc.K0, R0, T0, q=fd.inliers.astype(np.float64))[0]
    b = PR.host_pair(fc.F0, c.uv_a, c.uv_b, fc.K0, fc.K0, rl.R[0], rl.T[0], q=np.asarray(rl.inliers).astype(np.float64))[0]
    angle = lambda R: float(np.degrees(np.arccos(np.clip((np.trace(R @ c.R.T) - 1.0) / 2.0, -1.0, 1.0))))  # noqa: E731
    print(f"bootstrap: from F {int(fd.inliers.sum())} inliers, refined RMS {a.quality[0, 0]:.4f} px, rotation {angle(a.R[0]):.3f} deg; "
          f"from relate {int(np.asarray(rl.inliers).sum())} inliers, refined RMS {b.quality[0, 0]:.4f} px, rotation {angle(b.R[0]):.3f} deg")
    assert a.status[0] == 0 and np.isfinite(a.quality[0, 0])
    fc.write_figures("bootstrap_refined_rms_pixels", dict(from_fundamental=float(a.quality[0, 0]), from_relate=float(b.quality[0, 0]),
                                                        fundamental_inliers=int(fd.inliers.sum()), relate_inliers=int(np.asarray(rl.inliers).sum())))


def test_wrong_intrinsics_cost_relate_true_matches_on_the_host_walks():
    """both focal lengths off by 20 %: relate's host walk flags fewer of the unmoved matches than the fundamental matrix's, which
    never saw K (the seed of the GPU test, checked here first)"""
    from surikatoko_amd import relate as RL
    b, p, Ka, Kb = fc.wrong_k()
    unmoved = np.ones(200, bool)
    unmoved[p.moved] = False
    fd = fc.host_walk(b, 256, 1)
    rl = RL.host_pair(b.f0, b.uv_a, b.uv_b, Ka, Kb, hypotheses=256, inlier_pixels=fc.TAU, seed=1)
    n_fd, n_rl = int(fd.inliers[unmoved].sum()), int(np.asarray(rl.inliers)[unmoved].sum())
    print(f"wrong K: relate flags {n_rl} of {int(unmoved.sum())} unmoved matches, relate_uncalibrated {n_fd}")
    fc.write_figures("wrong_k_true_matches_flagged", dict(relate=n_rl, relate_uncalibrated=n_fd, unmoved=int(unmoved.sum())))
    assert n_fd > n_rl


def test_cpp_adapter_compiles_and_links(tmp_path):
    """RelateUncalibrated of the C++ adapter: tests/cpp/test_fund_adapter.cpp builds against the header and the library here; it
    runs where there is a device (tests/test_gpu_fundamental.py)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "-O1", "-std=c++17", "-I", os.path.join(fc.ROOT, "include"), "-I", os.path.join(fc.ROOT, "demos"),
                        os.path.join(fc.ROOT, "tests", "cpp", "test_fund_adapter.cpp"), "-o", str(tmp_path / "fund_adapter"),
                        "-L", os.path.join(fc.ROOT, "surikatoko_amd"), "-lsrk_ba",
                        "-Wl,-rpath," + os.path.join(fc.ROOT, "surikatoko_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_argument_checks_through_python():
    b = fc.ragged(False)
    ok = dict(row_ptr=b.row_ptr, uv_a=b.uv_a, uv_b=b.uv_b)
    assert FD.check_pairs(**ok) is None
    assert FD.default_fundamental_options() == dict(hypotheses=256, inlier_pixels=2.0, seed=1, refine_rounds=8)
    assert "hypotheses outside 1..4096" in FD.check_pairs(**ok, hypotheses=0)
    assert "hypotheses outside 1..4096" in FD.check_pairs(**ok, hypotheses=4097)
    assert "inlier_pixels" in FD.check_pairs(**ok, inlier_pixels=0.0)
    assert "inlier_pixels" in FD.check_pairs(**ok, inlier_pixels=np.inf)
    assert "refine_rounds outside 0..16" in FD.check_pairs(**ok, refine_rounds=17)
    assert "refine_rounds outside 0..16" in FD.check_pairs(**ok, refine_rounds=-1)
    bad = b.row_ptr.copy()
    bad[3] = bad[2] - 1
    assert "row_ptr decreases at pair 2" in FD.check_pairs(bad, b.uv_a, b.uv_b)
    bad = b.row_ptr.copy()
    bad[0] = 1
    assert "row_ptr[0] != 0" in FD.check_pairs(bad, b.uv_a, b.uv_b)
    ua = b.uv_a.copy()
    ua[5, 1] = np.nan
    assert "uv_a of match 5 is not finite" in FD.check_pairs(b.row_ptr, ua, b.uv_b)
    ub = b.uv_b.copy()
    ub[6, 0] = np.inf
    assert "uv_b of match 6 is not finite" in FD.check_pairs(b.row_ptr, b.uv_a, ub)
    q = np.ones(len(b.uv_a))
    q[2] = -0.5
    assert "q of match 2" in FD.check_pairs(b.row_ptr, b.uv_a, b.uv_b, q=q)
    with pytest.raises(ValueError):
        FD.check_pairs(b.row_ptr, b.uv_a[:10], b.uv_b)
    with pytest.raises(ValueError):
        FD.host_pair(0.0, b.uv_a[:9], b.uv_b[:9])
    assert FD.fundamental_status_names(3) == ["FEW_POINTS", "NO_MODEL"] and sa.FUNDAMENTAL_NO_MODEL == 2
