"""Batched camera resection without a GPU: the yardstick (tests/resect_ref.py) checked against finite
differences, the guard that keeps the compared decisions away from rounding, and the host half (surikatoko_amd/csrc/srk_resect.cpp)
through a stand-alone program (tests/cpp/test_resect_host.cpp): the argument checks, the option defaults, the coordinate maps, and a
walk of every frame on the host in the kernel's own order of operations."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from surikatoko_amd import resect as RS
import resect_cases as rc
import resect_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surikatoko_amd", "csrc")
LOSSES = ((ref.NONE, None), (ref.HUBER, 2.0), (ref.CAUCHY, 2.0))


# ------------------------------------------------------------------ the yardstick's derivatives
def _fd_case(angle, sigma, offset):
    """40 points seen from a pose whose rotation has the given angle; the pose handed out is `offset` away from the true one"""
    rng = np.random.default_rng(7)
    axis = rng.normal(size=3)
    R, T = ref.so3_exp(axis / np.linalg.norm(axis) * angle), np.array([0.1, -0.2, 0.3])
    X = (rc.landmarks(40, rng) - T) @ R                          # the points in front of the camera whatever its rotation
    uv = rc.project(rc.K0, R, T, X) + sigma * rng.normal(size=(40, 2))
    q = rng.uniform(0.5, 2.0, 40)
    q[::9] = 0.0
    return X, uv, q, ref.move(R, T, offset)


@pytest.mark.parametrize("kind,delta", LOSSES)
@pytest.mark.parametrize("angle", [0.0, 1e-9, 0.05, 1.0])
def test_gradient_against_finite_differences(angle, kind, delta):
    """2 g is the gradient of E through the pose update, at a pose 2 px off on noisy data (Huber at 2 px is then in both
    of its regimes).  Central differences at h = 1e-6: truncation ~ h^2, rounding ~ eps E / h, both below 1e-6 of |2 g|."""
    X, uv, q, (R, T) = _fd_case(angle, 1.0, np.array([2e-3, -1e-3, 3e-3, 1e-3, 2e-3, -1e-3]))
    E, H, g, w, _ = ref.terms(rc.F0, uv, X, q, rc.K0, R, T, kind, delta)
    assert np.all(w[q == 0] == 0) and (kind != ref.HUBER or 0 < np.count_nonzero(w[q > 0] < 1) < np.count_nonzero(q > 0))
    h, fd = 1e-6, np.zeros(6)
    for i in range(6):
        d = np.zeros(6)
        d[i] = h
        fd[i] = (ref.terms(rc.F0, uv, X, q, rc.K0, *ref.move(R, T, d), kind, delta)[0]
                 - ref.terms(rc.F0, uv, X, q, rc.K0, *ref.move(R, T, -d), kind, delta)[0]) / (2 * h)
    assert np.abs(fd - 2 * g).max() <= 1e-6 * np.abs(2 * g).max()


@pytest.mark.parametrize("kind,delta", LOSSES)
@pytest.mark.parametrize("angle", [0.0, 1e-9, 0.05, 1.0])
def test_hessian_against_finite_differences(angle, kind, delta):
    """2 H is the Hessian of E where the residuals vanish (noise-free data at the true pose: the Gauss-Newton matrix drops exactly
    the terms that carry a residual, and every loss is s + O(s^2) there).  Second central differences at h = 1e-5 move the
    projections by ~1e-2 px: s / delta^2 ~ 1e-5, truncation ~ h^2; the bound is 1e-3 of the largest entry."""
    X, uv, q, (R, T) = _fd_case(angle, 0.0, np.zeros(6))
    E, H, g, _, _ = ref.terms(rc.F0, uv, X, q, rc.K0, R, T, kind, delta)
    assert E < 1e-18 and np.abs(g).max() < 1e-6

    def energy(d):
        return ref.terms(rc.F0, uv, X, q, rc.K0, *ref.move(R, T, d), kind, delta)[0]
    h, fd, eye = 1e-5, np.zeros((6, 6)), np.eye(6)
    for i in range(6):
        for j in range(i, 6):
            fd[i, j] = fd[j, i] = (energy(h * (eye[i] + eye[j])) - energy(h * (eye[i] - eye[j])) - energy(h * (eye[j] - eye[i]))
                                   + energy(-h * (eye[i] + eye[j]))) / (4 * h * h)
    assert np.abs(fd - 2 * H).max() <= 1e-3 * np.abs(2 * H).max()


def test_pose_update_is_the_documented_perturbation():
    R, T = rc.true_pose(np.random.default_rng(1))
    d = np.array([0.1, -0.2, 0.3, 0.02, -0.01, 0.03])
    Rn, Tn = ref.move(R, T, d)
    assert np.allclose(ref.centre(Rn, Tn), ref.centre(R, T) + d[:3], atol=1e-15)
    assert np.allclose(Rn.T, ref.so3_exp(d[3:]) @ R.T, atol=1e-15) and abs(np.linalg.det(Rn) - 1) < 1e-14


# ------------------------------------------------------------------ the threshold guard
def _guarded(b, attempts, rel_change, **kw):
    ys = [rc.yardstick(b, i, attempts=attempts, rel_change=rel_change, **kw) for i in range(b.n)]
    for i, y in enumerate(ys):
        assert rc.margins_ok(y["log"], rel_change), (i, attempts, rel_change)
    return ys


@pytest.mark.parametrize("attempts,rel_change", rc.DECISION_PAIRS)
def test_decision_cases_have_no_frame_at_a_threshold(attempts, rel_change):
    """every accept margin |E_cand - E_cur| of the yardstick above 1e-9 E and every stop test a factor 2 away from rel_change E, on
    every frame: a difference in the last bits of E cannot flip a decision, so device and yardstick must agree on all of them"""
    b = rc.decisions()
    ys = _guarded(b, attempts, rel_change)
    capped = sum(bool(y["status"] & ref.NOT_CONVERGED) for y in ys)
    if attempts > 1:
        assert 0 < capped < b.n      # the pair splits the frames
    else:
        assert capped == b.n


def test_ragged_and_loss_cases_have_no_frame_at_a_threshold():
    for holes in (False, True):
        ys = rc.ragged_yardstick(holes)
        for i, y in enumerate(ys):
            assert rc.margins_ok(y["log"], rc.RAGGED_OPTIONS[holes][1]), (holes, i)
        capped = sum(bool(y["status"] & ref.NOT_CONVERGED) for y in ys)
        assert 0 < capped < sum(y["status"] != ref.FEW_POINTS for y in ys)
    for loss, (attempts, rel_change) in rc.LOSS_OPTIONS.items():
        _guarded(rc.outliers(), attempts, rel_change, kind=RS.LOSS_KINDS[loss], delta=rc.LOSS_DELTA)


def test_accuracy_yardstick_is_at_rounding_level():
    """the noise-free cases of the GPU test: the yardstick itself ends within 1 eps sqrt(cond_2(H_s)) of the truth (measured 0.12;
    rotation <= 3e-15 rad, centre / depth <= 3e-15, E <= 2e-24 px^2, cond_2(H_s) 1e2 .. 1e5), the unit the device's bound is 10 x of"""
    ys, worst = rc.accuracy_yardstick()
    b = rc.accuracy()
    print(f"yardstick: worst error {worst:.3f} eps sqrt(cond_2(H_s))")
    assert worst <= 1.0
    assert all(y["E"] <= 1e-22 for y in ys) and all(max(rc.pose_error(y["R"], y["T"], b.frames[i])) < 1e-13 for i, y in enumerate(ys))


# ------------------------------------------------------------------ the host half
def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


def _build(cxx, out, extra=()):
    return subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "test_resect_host.cpp"),
                           os.path.join(CSRC, "srk_resect.cpp"), "-o", str(out)], capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("resect_bin") / "test_resect_host"
    r = _build(_cxx(), exe)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _walk(program, tmp_path, b, want_weights=False, **kw):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    rc.write_host_input(src, b, want_weights=want_weights, **kw)
    r = subprocess.run([program, "frames", src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return rc.read_host_output(dst, b, want_weights)


def test_checks_defaults_and_coordinate_maps(program):
    r = subprocess.run([program, "unit"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_unit_runs_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan: the unit checks and a ragged batch with q = 0 in between"""
    exe = tmp_path / "test_resect_host_san"
    r = _build(_cxx(), exe, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), "unit"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    b = rc.rows(rc.ragged(True), range(40))
    out = _walk(str(exe), tmp_path, b, want_weights=True, attempts=3, rel_change=1e-9, kind=ref.CAUCHY, delta=2.0)
    assert len(out[4]) == b.n


def _agree(got, ys, b, kind=ref.NONE, delta=None):
    """The walk's outputs against the yardstick's, frame by frame; returns the largest pose distance in Newton-step units.  E to
    1e-12: against the yardstick's E at the walk's own pose on every frame, and against the yardstick's own result where its run
    ended by the stop test.  (Where a run ends at its cap the gradient is not small, and two poses a rounding apart -- 1e-15 --
    differ in E by 2 g d ~ 1e-8 E: that is the pose's distance, bounded below in its own unit, not an error of E.)"""
    R, T, quality, info, status, logs, w = got
    worst = 0.0
    for i, y in enumerate(ys):
        assert status[i] == y["status"], i
        assert list(logs[i]) == [int(a) for a, _, _ in y["log"]], i                 # the accept / reject sequence
        assert quality[i, 5] == y["quality"][5] and quality[i, 1] == y["quality"][1], i
        if y["status"] & ref.FEW_POINTS:
            assert np.array_equal(R[i], b.R0[i]) and np.array_equal(T[i], b.T0[i]) and np.isnan(quality[i, 3])
            continue
        E = quality[i, 0] ** 2 * quality[i, 1]
        tol = rc.energy_tolerance(b, i, E, quality[i, 1])
        assert abs(E - rc.energy_at(b, i, R[i], T[i], kind, delta)) <= tol, i
        if not y["status"] & ref.NOT_CONVERGED:
            assert abs(E - y["E"]) <= tol, i
        worst = max(worst, rc.pose_units(R[i], T[i], y))
    return worst


def test_host_walk_against_the_yardstick_on_the_ragged_cases(program, tmp_path):
    """the kernel's order of operations (the deal to 64 lanes by rank, the tree down by 32 .. 1, the written-out 6 x 6 solve) on the
    host: the same decisions on every frame, E to 1e-12, the pose within the bound the device is held to"""
    worst = 0.0
    for holes in (False, True):
        b = rc.ragged(holes)
        attempts, rel_change = rc.RAGGED_OPTIONS[holes]
        worst = max(worst, _agree(_walk(program, tmp_path, b, attempts=attempts, rel_change=rel_change), rc.ragged_yardstick(holes), b))
    print(f"host walk against the yardstick: {worst:.3e} Newton steps")
    assert worst <= 1.0    # measured 0.1: a rounding-level difference is a small part of the step that remains; the device gets 10 x this


@pytest.mark.parametrize("attempts,rel_change", rc.DECISION_PAIRS)
def test_host_walk_decisions(program, tmp_path, attempts, rel_change):
    b = rc.decisions()
    ys = [rc.yardstick(b, i, attempts=attempts, rel_change=rel_change) for i in range(b.n)]
    _agree(_walk(program, tmp_path, b, attempts=attempts, rel_change=rel_change), ys, b)


@pytest.mark.parametrize("loss", ["huber", "cauchy"])
def test_host_walk_losses(program, tmp_path, loss):
    b = rc.outliers()
    attempts, rel_change = rc.LOSS_OPTIONS[loss]
    kind = RS.LOSS_KINDS[loss]
    ys = [rc.yardstick(b, i, attempts=attempts, rel_change=rel_change, kind=kind, delta=rc.LOSS_DELTA) for i in range(b.n)]
    got = _walk(program, tmp_path, b, want_weights=True, attempts=attempts, rel_change=rel_change, kind=kind, delta=rc.LOSS_DELTA)
    _agree(got, ys, b, kind, rc.LOSS_DELTA)
    assert np.abs(got[6] - np.concatenate([y["w"] for y in ys])).max() <= 1e-10


def test_host_walk_q_zero_is_the_frame_without_the_observation(program, tmp_path):
    b = rc.rows(rc.ragged(True), range(60))
    keep = b.q > 0
    rp = np.concatenate([[0], np.cumsum([np.count_nonzero(keep[b.row_ptr[i]:b.row_ptr[i + 1]]) for i in range(b.n)])]).astype(np.int64)
    short = rc.SimpleNamespace(f0=b.f0, n=b.n, row_ptr=rp, point=b.point[keep], uv=b.uv[keep], q=b.q[keep], X=b.X, K=b.K, R0=b.R0, T0=b.T0)
    a = _walk(program, tmp_path, b, attempts=5, rel_change=1e-9)
    c = _walk(program, tmp_path, short, attempts=5, rel_change=1e-9)
    assert all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a[:5], c[:5]))


# ------------------------------------------------------------------ the Python checks
def test_python_check_frames_and_names():
    b = rc.rows(rc.ragged(True), range(12))
    args = (b.row_ptr, b.point, b.uv, b.X, b.K, b.R0, b.T0)
    assert RS.check_frames(*args, q=b.q) is None

    def bad(i, f, **kw):
        a = [np.array(x, copy=True) for x in args]
        f(a[i])
        return RS.check_frames(*a, **kw)
    assert "row_ptr[0]" in bad(0, lambda a: a.__setitem__(0, 1))
    assert "decreases at frame 3" in bad(0, lambda a: a.__setitem__(4, a[3] - 1))
    assert "out of range" in bad(1, lambda a: a.__setitem__(5, len(b.X)))
    assert "out of range" in bad(1, lambda a: a.__setitem__(5, -1))
    assert "uv of observation 7" in bad(2, lambda a: a.__setitem__((7, 1), np.nan))
    assert "landmark 3 is not finite" in bad(3, lambda a: a.__setitem__((3, 0), np.inf))
    assert "K of frame 2" in bad(4, lambda a: a.__setitem__((2, 1, 1), np.nan))
    assert "R0 of frame 1 is not finite" in bad(5, lambda a: a.__setitem__((1, 0, 0), np.nan))
    assert "not orthogonal to 1e-9" in bad(5, lambda a: a.__setitem__((1, 0, 0), a[1, 0, 0] + 1e-6))
    assert "T0 of frame 4" in bad(6, lambda a: a.__setitem__((4, 2), np.inf))
    q = b.q.copy()
    q[9] = -1.0
    assert "q of observation 9" in RS.check_frames(*args, q=q)
    assert "attempts" in RS.check_frames(*args, attempts=65) and "attempts" in RS.check_frames(*args, attempts=-1)
    assert "rel_change" in RS.check_frames(*args, rel_change=-1e-3) and "rel_change" in RS.check_frames(*args, rel_change=np.nan)
    assert "loss_kind" in RS.check_frames(*args, loss=3)
    assert "loss_delta_pixels" in RS.check_frames(*args, loss="huber") and "loss_delta_pixels" in RS.check_frames(*args, loss="cauchy", delta=0.0)
    assert RS.check_frames(*args, loss="cauchy", delta=2.0, attempts=64, rel_change=0.0) is None
    assert RS.default_resect_options() == dict(attempts=10, rel_change=1e-9, loss_kind=0, loss_delta_pixels=0.0)
    assert RS.resect_status_names(RS.RESECT_FEW_POINTS | RS.RESECT_NOT_CONVERGED) == ["FEW_POINTS", "NOT_CONVERGED"]
    with pytest.raises(ValueError):
        RS.check_frames(b.row_ptr, b.point[:5], b.uv, b.X, b.K, b.R0, b.T0)


def test_python_revert_inverts_the_normalisation():
    import surikatoko_amd as sa
    sc = sa.generate_scene(sa.SceneSpec(n_frames=4, grid_nx=4, grid_ny=3, vis_window=4))
    R0, T0 = sc.cam_R.reshape(-1, 3, 3).copy(), sc.cam_T.reshape(-1, 3).copy()
    n = sc.copy()
    ok, nrm = sa.normalize_scene_inplace(n)
    assert ok
    A = np.random.default_rng(3).normal(size=(4, 6, 6))
    info_n = A @ A.transpose(0, 2, 1) + 6 * np.eye(6)
    R, T, info = RS.revert(nrm, n.cam_R.reshape(-1, 3, 3), n.cam_T.reshape(-1, 3), info_n)
    assert np.abs(R - R0).max() < 1e-14 and np.abs(T - T0).max() < 1e-13
    # info goes by the inverse of what revert_covariances does to a pose covariance: the two stay inverses of each other
    cov, _ = sa.revert_covariances(nrm, frame_cov=np.linalg.inv(info_n))
    assert np.abs(cov @ info - np.eye(6)).max() < 1e-12
