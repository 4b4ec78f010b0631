"""Batched triangulation without a GPU: the yardstick (tests/triangulate_ref.py) tied to the stored prototype
result and to the host function, the bound of the conditioning cases shown to be one the reference chain meets, and the host half
(surikatoko_amd/csrc/srk_tri.cpp) through a stand-alone program (tests/cpp/test_tri_host.cpp): the argument checks, the option
defaults, the coordinate map, and a walk of every track on the host in the kernel's own order of operations."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import load_golden
from surikatoko_amd import io as sio
from surikatoko_amd import triangulate as T
import triangulate_cases as tc
import triangulate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surikatoko_amd", "csrc")


# ------------------------------------------------------------------ the yardstick and the reference chain
def test_yardstick_linear_solve_agrees_with_the_prototype():
    g = load_golden("pyproto_dino_prep")
    f0 = float(g["f0"])
    for n, uv, P, X in zip(g["tri_n"], g["tri_uv"], g["tri_P"], g["tri_X"]):
        A, b = ref.system_from_P(f0, uv[:n], P[:n])
        Xy, _ = ref.solve_linear(A, b)
        assert np.abs(Xy - X).max() < 1e-9 * max(1.0, np.abs(X).max())   # the tolerance of tests/test_io_callers.py


def test_system_from_KRT_equals_system_from_P():
    rng = np.random.default_rng(0)
    R, Tr = tc.rig(6, 2.0, rng, wobble=0.3)
    K = np.broadcast_to(tc.K0, (6, 3, 3)).copy()
    K[:, 0, 1] = rng.normal(size=6) * 1e-3   # a skew, so that every entry of K takes part
    uv = rng.uniform(0, 800, (6, 2))
    q = rng.uniform(0.5, 2, 6)
    for w in (None, q):
        A1, b1 = ref.system_from_KRT(tc.F0, uv, R, Tr, K, w)
        A2, b2 = ref.system_from_P(tc.F0, uv, ref.proj_mats(R, Tr, K), w)
        scale = np.abs(A2).max()
        assert np.abs(A1 - A2).max() <= 16 * ref.EPS * scale and np.abs(b1 - b2).max() <= 16 * ref.EPS * np.abs(b2).max()


@pytest.mark.parametrize("ratio", tc.RATIOS)
@pytest.mark.parametrize("n_views", tc.VIEWS)
def test_host_function_meets_the_conditioning_bound(n_views, ratio):
    """srk_triangulate_least_squares (Householder QR, the reference's algorithm) within 8 eps cond_2(A) |X| of the truth: the bound
    the device is held to is one the reference chain meets (it measured <= 0.61 of eps cond |X| here, as did the yardstick)"""
    b = tc.conditioning(n_views, ratio)
    worst = 0.0
    for i in range(b.n):
        Xh = sio.triangulate_least_squares(tc.track(b, i)[1], tc.host_P(b, i), b.f0)
        worst = max(worst, np.linalg.norm(Xh - b.X_true[i]) / tc.cond_bound(b, i, b.X_true[i]))
    assert worst <= 1.0


def test_normal_equations_miss_the_bound_at_low_parallax():
    """what the GPU test rejects: A^T A x = A^T b delivers eps cond^2; at cond 2e3 and 2e5 it misses 8 eps cond |X|"""
    for ratio in tc.RATIOS[1:]:
        b = tc.conditioning(8, ratio)
        miss = 0
        for i in range(b.n):
            A, rhs = tc.system(b, i)
            Xn = np.linalg.solve(A.T @ A, A.T @ rhs)
            miss += np.linalg.norm(Xn - b.X_true[i]) > tc.cond_bound(b, i, b.X_true[i])
        assert miss > b.n // 2


def test_threshold_cases_have_no_track_at_the_threshold():
    """the (attempts, rel_change) pairs of the GPU test that split the tracks: the yardstick's relative decrease of E stays 1e-3
    (relative) away from the threshold on every track, so a difference in the last bits of E cannot flip a status"""
    b = tc.noisy()
    for attempts, rel in ((1, 2e-4), (2, 3e-11)):
        hit = 0
        for i in range(b.n):
            fr, uv = tc.track(b, i)
            P, q = ref.proj_mats(b.R[fr], b.T[fr], b.K[fr]), np.ones(len(fr))
            X, _ = ref.solve_linear(*ref.system_from_P(b.f0, uv, P, q))
            E = ref.energy_terms(b.f0, uv, P, q, X)[0]
            _, _, capped, log = ref.refine(b.f0, uv, P, q, X, attempts, rel)
            hit += capped
            for accepted, Xn in log:
                assert accepted
                En = ref.energy_terms(b.f0, uv, P, q, Xn)[0]
                assert abs((E - En) / E - rel) > 1e-3 * rel, i
                E = En
        assert 0 < hit < b.n


# ------------------------------------------------------------------ the host half
def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


def _build(cxx, out, extra=()):
    return subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "test_tri_host.cpp"),
                           os.path.join(CSRC, "srk_tri.cpp"), "-o", str(out)], capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tri_bin") / "test_tri_host"
    r = _build(_cxx(), exe)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _walk(program, tmp_path, b, **kw):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    tc.write_host_input(src, b, **kw)
    r = subprocess.run([program, "tracks", src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return tc.read_host_output(dst, b.n)


def test_checks_defaults_and_coordinate_map(program):
    r = subprocess.run([program, "unit"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_unit_runs_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan: the unit checks and a ragged batch with weights and refinement"""
    exe = tmp_path / "test_tri_host_san"
    r = _build(_cxx(), exe, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), "unit"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    b = tc.ragged(257)
    q = np.random.default_rng(1).choice([0.0, 0.5, 1.0, 2.0], len(b.frame))
    X, quality, status = _walk(str(exe), tmp_path, b, q=q, refine_attempts=3, refine_rel_change=1e-9, min_parallax_deg=1.0)
    assert len(status) == b.n


def test_python_check_and_revert():
    assert T.check_tracks([0, 2], [0, 1], np.zeros((2, 2)), 2) is None
    assert "out of range" in T.check_tracks([0, 2], [0, 2], np.zeros((2, 2)), 2)
    assert "decreases" in T.check_tracks([0, 2, 1], [0, 1], np.zeros((2, 2)), 2)
    assert "not finite" in T.check_tracks([0, 2], [0, 1], [[0, np.nan], [0, 0]], 2)
    assert "refine_attempts" in T.check_tracks([0, 2], [0, 1], np.zeros((2, 2)), 2, refine_attempts=65)
    assert T.default_tri_options() == dict(refine_attempts=10, refine_rel_change=1e-9, min_parallax_deg=0.0)
    assert T.tri_status_names(T.TRI_FEW_VIEWS | T.TRI_LOW_PARALLAX) == ["FEW_VIEWS", "LOW_PARALLAX"]


@pytest.mark.parametrize("ratio", tc.RATIOS)
def test_host_walk_meets_the_conditioning_bound(program, tmp_path, ratio):
    """the kernel's order of operations (Givens rotations per lane, the merge tree of eight lanes) on the host"""
    for n_views in tc.VIEWS:
        b = tc.conditioning(n_views, ratio)
        X, quality, status = _walk(program, tmp_path, b)
        assert not np.any(status)
        assert max(np.linalg.norm(X[i] - b.X_true[i]) / tc.cond_bound(b, i, b.X_true[i]) for i in range(b.n)) <= 1.0
        assert np.all(quality[:, 3] == n_views)


def test_host_walk_ragged_weights_and_refinement_against_the_yardstick(program, tmp_path):
    b = tc.ragged(257)
    X, quality, status = _walk(program, tmp_path, b)
    lengths = np.diff(b.row_ptr)
    assert np.all(status[lengths < 2] == ref.FEW_VIEWS) and np.all(np.isnan(X[lengths < 2])) and np.all(status[lengths >= 2] == 0)
    assert np.array_equal(quality[:, 3], lengths.astype(np.float64))
    for i in np.flatnonzero(lengths >= 2):
        Xy, qy, _, _ = ref.triangulate_track(b.f0, *tc.track(b, i), b.R, b.T, b.K)
        assert np.linalg.norm(X[i] - Xy) <= tc.cond_bound(b, i, Xy)
        assert abs(quality[i, 1] - qy[1]) <= np.degrees(100 * ref.EPS)
    # q = 0 is the track without the observation, bit for bit
    n = tc.noisy()
    q = np.random.default_rng(5).uniform(0.5, 2.0, len(n.frame))
    off = n.row_ptr[:-1] + np.arange(n.n) % 3
    q[off] = 0.0
    keep = q > 0
    short = tc.batch([(n.frame[n.row_ptr[i]:n.row_ptr[i + 1]][keep[n.row_ptr[i]:n.row_ptr[i + 1]]],
                       n.uv[n.row_ptr[i]:n.row_ptr[i + 1]][keep[n.row_ptr[i]:n.row_ptr[i + 1]]]) for i in range(n.n)], n.R, n.T, n.K)
    a = _walk(program, tmp_path, n, q=q, refine_attempts=5, refine_rel_change=1e-9)
    c = _walk(program, tmp_path, short, q=q[keep], refine_attempts=5, refine_rel_change=1e-9)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, c))
    # the refinement's statuses are the yardstick's
    for attempts, rel in ((1, 2e-4), (2, 3e-11), (6, 1e-6), (20, 0.0)):
        X, quality, status = _walk(program, tmp_path, n, refine_attempts=attempts, refine_rel_change=rel)
        want = [ref.triangulate_track(n.f0, *tc.track(n, i), n.R, n.T, n.K, refine_attempts=attempts, refine_rel_change=rel) for i in range(n.n)]
        assert np.array_equal(status, np.array([w[2] for w in want], np.uint32))
        assert np.allclose(quality[:, 0], [w[1][0] for w in want], rtol=1e-9)
