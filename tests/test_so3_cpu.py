"""The three SO(3) formulas of the factor kernels (rp_log, rp_jrinv, jp_jlinv in surikatoko_amd/csrc/srk_ba_kernels.hip, and
so3_log in srk_factors.cpp) against the independent reference of tests/so3_ref.py, over the whole range of residual angles,
without a device: the numpy restatement of the kernels' formulas (so3_ref.kernel_*), and the host residual functions through
the stand-alone program tests/cpp/test_factor_tables.cpp.

Bounds.  eps = 2^-52.  Log: 16 eps absolute (3.6e-15 rad); the Jacobians: 16 eps per entry.  The formulas measure at most
4.5e-16 and 4.2e-16 over the sweep (the tests print the maxima), so the bounds leave a factor of eight; the formulas before
the path near pi and the half-angle form exceed them from pi - 1e-3 on, which test_formulas_before_the_repair_miss_the_bounds
holds on to.  The host functions' rotation rows: 1e-13 absolute -- two 3 x 3 products of entries <= 1 leave about 6 sqrt(3) eps
in the antisymmetric part, which angle / sin(angle) <= 6.2 multiplies up to the switch at cos = -0.9 (1.5e-14), less beyond
it; the bound is twice the 4.8e-14 that a switch as late as 3 rad would give."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import surikatoko_amd as sa
import factor_table_cases as ftc
import jointprior_ref as jr
import relpose_ref as rr
import so3_ref as so3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surikatoko_amd", "csrc")
EPS = float(np.finfo(np.float64).eps)
BOUND = 16 * EPS
AXES = so3.axes(8)
SWEEP = so3.SWEEP


def test_the_sweep_has_an_angle_on_either_side_of_every_switch():
    sn = np.sin(SWEEP)
    assert 0.0 in SWEEP and max(SWEEP) == np.pi - 1e-9
    assert any(0 < s < 1e-4 and s > 0.9e-4 for s in sn) and any(1e-4 < s < 1.1e-4 for s in sn)          # the series of Log
    assert any(0.9e-6 < a * a < 1e-6 for a in SWEEP) and any(1e-6 < a * a < 1.1e-6 for a in SWEEP)       # the series of k
    assert any(2.2 < a * a < so3.K_HALF_T2 for a in SWEEP) and any(so3.K_HALF_T2 <= a * a < 2.3 for a in SWEEP)
    cs = np.cos(SWEEP)
    assert any(so3.LOG_PI_COS < c < -0.89 for c in cs) and any(-0.91 < c < so3.LOG_PI_COS for c in cs)   # the axis near pi
    assert all(a in SWEEP for a in so3.AT_SWITCHES)
    assert np.count_nonzero(AXES[0]) == 1 and np.allclose(np.linalg.norm(AXES, axis=1), 1.0, atol=1e-15)


def test_reference_is_exact_where_the_zero_residual_tests_need_it():
    """Exp(0) = I and Log of a symmetric matrix next to I = 0, exactly; Log(Exp(phi)) = phi and the differences reproduce the
    closed forms of the Jacobians' first two terms at a moderate angle (a check of the reference's conventions: Jr^-1 has
    +[phi]x / 2, Jl^-1 has -[phi]x / 2, and Jl^-1 = Jr^-1^T)"""
    assert np.array_equal(so3.exp(np.zeros(3)), np.eye(3))
    assert np.array_equal(so3.log(np.eye(3)), np.zeros(3))
    Z = so3.exp(0.3 * AXES[2])
    S = Z.T @ Z
    assert np.array_equal(S, S.T) and np.array_equal(so3.log(S), np.zeros(3))
    assert np.array_equal(so3.jr_inv(np.zeros(3)), np.eye(3)) and np.array_equal(so3.jl_inv(np.zeros(3)), np.eye(3))
    phi = 0.7 * AXES[3]
    assert np.abs(so3.log(so3.exp(phi)) - phi).max() < 4 * EPS
    Jr, Jl = so3.jr_inv(phi), so3.jl_inv(phi)
    assert np.array_equal(Jl, Jr.T)
    assert np.abs(0.5 * (Jr - Jr.T) - 0.5 * rr.skew(phi)).max() < 4 * EPS
    # Jr^-1(phi) phi = phi: the rotation about its own axis
    assert np.abs(Jr @ phi - phi).max() < 4 * EPS
    # and against a double-precision difference of the composition itself
    h = 1e-6
    for c in range(3):
        d = np.zeros(3)
        d[c] = h
        fd = (so3.log(so3.exp(phi) @ so3.exp(d)) - so3.log(so3.exp(phi) @ so3.exp(-d))) / (2 * h)
        assert np.abs(fd - Jr[:, c]).max() < 1e-9


@pytest.mark.parametrize("angle", SWEEP)
def test_kernel_formulas_against_the_reference(angle):
    """kernel_log on the rotation matrix rounded to double, kernel_jr_inv and kernel_jl_inv on the rotation vector, eight axes"""
    d_log = d_jr = d_jl = 0.0
    for ax in AXES:
        phi = angle * ax
        M = so3.exp(phi)
        want = so3.log(M)
        assert np.abs(want - phi).max() <= max(4 * EPS, 4.0 * EPS / max(np.pi - angle, 1e-6))  # the reference inverts its own Exp
        d_log = max(d_log, float(np.abs(so3.kernel_log(M) - want).max()))
        d_jr = max(d_jr, float(np.abs(so3.kernel_jr_inv(phi) - so3.jr_inv(phi)).max()))
        d_jl = max(d_jl, float(np.abs(so3.kernel_jl_inv(phi) - so3.jl_inv(phi)).max()))
    print(f"angle {angle:.12g}: Log off by {d_log:.2e}, Jr^-1 by {d_jr:.2e}, Jl^-1 by {d_jl:.2e} (bound {BOUND:.2e})")
    assert d_log <= BOUND and d_jr <= BOUND and d_jl <= BOUND


def _half_turns():
    seeded = so3.exp(np.pi * AXES[3])
    return [("x", np.diag([1.0, -1.0, -1.0]), np.array([1.0, 0, 0])), ("y", np.diag([-1.0, 1.0, -1.0]), np.array([0, 1.0, 0])),
            ("z", np.diag([-1.0, -1.0, 1.0]), np.array([0, 0, 1.0])), ("seeded", seeded, so3.log(seeded) / np.pi)]


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_kernel_log_at_exactly_pi(which):
    name, M, axis = _half_turns()[which]
    got = so3.kernel_log(M)
    print(f"half a turn about {name}: {got}, norm - pi = {np.linalg.norm(got) - np.pi:.2e}")
    assert np.all(np.isfinite(got))
    assert abs(np.linalg.norm(got) - np.pi) <= BOUND
    assert min(np.abs(got - np.pi * axis).max(), np.abs(got + np.pi * axis).max()) < 1e-12
    J = so3.kernel_jr_inv(got)
    assert np.all(np.isfinite(J)) and np.all(np.isfinite(so3.kernel_jl_inv(got)))


def test_formulas_before_the_repair_miss_the_bounds():
    """what the sweep is for: the antisymmetric-part Log and the (1 + cos) / sin form of k stay inside the bounds up to 3 rad,
    exceed them at pi - 1e-3, pi - 1e-6 and pi - 1e-9, and the old Log gives NaN at diag(1, -1, -1)"""
    for angle in SWEEP:
        d_log = d_j = 0.0
        for ax in AXES:
            phi = angle * ax
            M = so3.exp(phi)
            d_log = max(d_log, float(np.abs(so3.kernel_log_old(M) - so3.log(M)).max()))
            d_j = max(d_j, float(np.abs(so3.kernel_jr_inv(phi, so3.kernel_k_old) - so3.jr_inv(phi)).max()))
        print(f"angle {angle:.12g}: old Log off by {d_log:.2e}, old Jr^-1 by {d_j:.2e}")
        if angle <= 3.0:
            assert d_log <= BOUND and d_j <= BOUND
        else:
            assert d_log > BOUND and d_j > BOUND
    for name, M, axis in _half_turns()[:3]:
        assert np.all(np.isnan(so3.kernel_log_old(M)))


def test_a_wrong_series_coefficient_or_a_flipped_sign_fails_the_sweep():
    """the sweep is sharp enough to see the mistakes it is there for: 1 / 6 -> 1 / 5 in the series of Log moves the result by
    sin^2 / 30 of the angle, 3.3e-14 rad at 0.99e-4 rad, the last angle that takes the series, nine times the bound; 1 / 12 ->
    1 / 6 in the series of k moves Jr^-1 by t^2 / 12 = 8e-8 at 0.99e-3 rad; and -[phi]x / 2 for +[phi]x / 2 moves it by the
    angle itself, above the bound at every angle of the sweep from 1e-8 on.  (The t^4 coefficient 3 / 40 of Log is below
    the rounding of a double wherever the series is taken: no test can see it, and it does no harm.)"""
    phi = 0.99e-4 * AXES[3]
    M = so3.exp(phi)
    v = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    s2 = float(v @ v)
    assert np.array_equal(v * (1.0 + s2 / 6.0 + 3.0 * s2 * s2 / 40.0), so3.kernel_log(M))  # the series is what runs there
    assert np.abs(v * (1.0 + s2 / 5.0 + 3.0 * s2 * s2 / 40.0) - so3.log(M)).max() > BOUND
    phi = 0.99e-3 * AXES[3]
    wrong_k = lambda t2: (1.0 / 6.0 + t2 / 720.0) if t2 < 1e-6 else so3.kernel_k(t2)  # noqa: E731
    assert np.abs(so3.kernel_jr_inv(phi, wrong_k) - so3.jr_inv(phi)).max() > BOUND
    for angle in SWEEP[2:]:
        phi = angle * AXES[3]
        assert np.abs(so3.kernel_jl_inv(phi) - so3.jr_inv(phi)).max() > BOUND


# ------------------------------------------------------------------ the host residual functions (srk_factors.cpp)

@pytest.fixture(scope="module")
def host_residuals(tmp_path_factory):
    """the 'r' lines of tests/cpp/test_factor_tables.cpp for the cases factor_table_cases.SO3_NAMES, built and run as
    tests/test_factor_tables_cpu.py builds and runs it"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("so3_cases")
    exe = d / "test_factor_tables"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_factor_tables.cpp"),
                        os.path.join(CSRC, "srk_factors.cpp"), os.path.join(CSRC, "srk_plan.cpp"), "-pthread", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    files = []
    for name in ftc.SO3_NAMES:
        sc = ftc.case(name)["scene"].copy()
        ok, nrm = sa.normalize_scene_inplace(sc)
        assert ok
        files.append(str(d / name))
        ftc.write_case(files[-1], name, nrm)
    r = subprocess.run([str(exe), *files], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out, cur = {}, None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "case":
            cur = out.setdefault(w[1], {})
        elif w[0] == "r":
            cur[w[1]] = np.array([float.fromhex(v) for v in w[2:]])
    return out


def test_host_residual_functions_over_the_sweep(host_residuals):
    """srk_relpose_residuals and srk_jprior_residuals at every (angle, axis) of the sweep: rotation rows within 1e-13 of the
    reference, translation rows within 1e-10 of the extent (tests/test_factor_tables_cpu.py)"""
    combos = ftc.so3_combinations()
    worst = {}
    seen = 0
    for part, name in enumerate(ftc.SO3_NAMES):
        c = ftc.case(name)
        sc, r = c["scene"], host_residuals[name]
        ext = float(np.abs(sc.points - sc.points.mean(axis=0)).max())
        mine = combos[ftc.SO3_PER_CASE * part:ftc.SO3_PER_CASE * (part + 1)]
        want_f, got_f = rr.residuals(c["fac"], sc), r["relpose"].reshape(-1, 6)
        sets = c["sets"][0]
        want_j, got_j = np.concatenate(jr.residuals(sets, sc)).reshape(-1, 6), r["jprior"].reshape(-1, 6)
        mean = np.concatenate([s["mean"] for s in sets.sets]).reshape(-1, 6)
        assert got_f.shape == want_f.shape == got_j.shape == want_j.shape == (len(mine), 6)
        assert np.abs(got_f[:, :3] - want_f[:, :3]).max() < 1e-10 * ext and np.abs(got_j[:, :3] - want_j[:, :3]).max() < 1e-10 * ext
        for k, (angle, ax) in enumerate(mine):
            # the case is what it says: the residual rotation of factor and slot k has the angle of the combination
            assert abs(np.linalg.norm(want_f[k, 3:]) - angle) < 1e-14 and abs(np.linalg.norm(want_j[k, 3:] + mean[k, 3:]) - angle) < 1e-14
            d = max(float(np.abs(got_f[k, 3:] - want_f[k, 3:]).max()), float(np.abs(got_j[k, 3:] - want_j[k, 3:]).max()))
            worst[angle] = max(worst.get(angle, 0.0), d)
            seen += 1
    assert seen == len(SWEEP) * ftc.SO3_AXES and sorted(worst) == sorted(SWEEP)
    for angle in SWEEP:
        print(f"angle {angle:.12g}: host rotation rows off by {worst[angle]:.2e}")
    assert max(worst.values()) < 1e-13
