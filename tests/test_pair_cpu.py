"""Two-view pose refinement without a GPU: the yardstick (tests/pair_ref.py) against difference quotients of
its own residual, the guard that keeps the compared decisions away from rounding, and the host half
(surikatoko_amd/csrc/srk_pair.cpp): the walk of every pair in the kernel's own order of operations through the library, the checks,
the factor helper, and the stand-alone program (tests/cpp/test_pair_host.cpp), also under the sanitizers."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import pair as PR
import pair_cases as pc
import pair_ref as ref
import relate_cases as rc
import relpose_ref
import resect_cases


@pytest.fixture(scope="module")
def program():
    if rc.cxx() is None:
        pytest.skip("no host C++ compiler")
    return pc.host_program()


# ------------------------------------------------------------------ the yardstick's Jacobian
def test_yardstick_jacobian_against_difference_quotients():
    """The analytic J against central differences of the yardstick's own r at step h = 1e-6, on the pair of 200 matches at its off
    start.  The bound is the difference quotient's own error, per entry: the truncation h^2 |r'''| / 6, with r''' taken from a
    five-point quotient at step 1e-3, and the rounding 2 (c eps A) / (2 h): r is a quotient whose numerator p_b . F p_a is a sum
    of nine products that cancel, so one value of r carries about c eps A with A = sum |F_ij p_b,i p_a,j| / sqrt(den) and c = 8
    for the products, the sums, and F itself (an inverse and two products of 3 x 3 matrices).  Measured: the largest difference is
    9e-8 px / rad at |J| up to 590, a fifth of the bound."""
    b = pc.ragged(False)
    i = len(pc.LENGTHS) - 1
    uva, uvb, _ = pc.pair_obs(b, i)
    R, T, Ka, Kb, f0 = b.R0[i], b.T0[i], b.Ka[i], b.Kb[i], b.f0
    J = ref.jacobian(f0, uva, uvb, Ka, Kb, R, T)

    def r_at(k, step):
        d = np.zeros(5)
        d[k] = step
        return ref.signed_residuals(f0, uva, uvb, Ka, Kb, *ref.move(R, T, d))
    F = rc.ref.fundamental(ref.skew(T) @ R, Ka, Kb)
    pa, pb = np.column_stack([uva, np.full(len(uva), f0)]), np.column_stack([uvb, np.full(len(uvb), f0)])
    la, lb = pa @ F.T, pb @ F
    A = np.einsum("oi,ij,oj->o", np.abs(pb), np.abs(F), np.abs(pa)) / np.sqrt(la[:, 0] ** 2 + la[:, 1] ** 2 + lb[:, 0] ** 2 + lb[:, 1] ** 2)
    h, h3 = 1e-6, 1e-3
    worst = 0.0
    for k in range(5):
        quotient = (r_at(k, h) - r_at(k, -h)) / (2 * h)
        third = (r_at(k, 2 * h3) - 2 * r_at(k, h3) + 2 * r_at(k, -h3) - r_at(k, -2 * h3)) / (2 * h3 ** 3)
        bound = h * h * np.abs(third) / 6 + 8 * ref.EPS * A / h
        ratio = np.abs(J[:, k] - quotient) / bound
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio <= 1.0), (k, int(np.argmax(ratio)), float(ratio.max()))
    print(f"analytic J against central differences: largest |J| {np.abs(J).max():.3e}, largest difference / bound {worst:.3f}")


# ------------------------------------------------------------------ the guard
def test_cases_have_no_pair_at_a_threshold():
    """on every named ragged case, both hole variants, the yardstick's own log stays away from every threshold: none of them is
    excused by the filter of pc.agree.  Some pairs stop by the test, some at the cap."""
    for holes in (False, True):
        rel_change = pc.RAGGED_OPTIONS[holes][1]
        ys = pc.ragged_yardstick(holes)
        assert len(ys) == len(pc.LENGTHS) and [int(y["quality"][1]) for y in ys] == list(pc.LENGTHS)
        for i, y in enumerate(ys):
            assert resect_cases.margins_ok(y["log"], rel_change), (holes, i, y["log"])
        live = [y for y in ys if not y["status"] & ref.FEW_POINTS]
        capped = sum(bool(y["status"] & ref.NOT_CONVERGED) for y in live)
        assert len(live) == 8 and 0 < capped < len(live)


# ------------------------------------------------------------------ the host walk
@pytest.mark.parametrize("holes", [False, True])
def test_host_terms_against_the_yardstick(holes):
    """H and g of the host walk at the start pose against the yardstick's at the same pose, to 1e-12 of the largest entry (a sum of
    n <= 200 products), and sum q s against the sum relate's score gives with an infinite tau"""
    b = pc.ragged(holes)
    got, grads, _ = pc.host_walk(b, attempts=0)
    for i in range(b.n):
        uva, uvb, q = pc.pair_obs(b, i)
        n = got.quality[i, 1]
        if n < 5:
            continue
        E, H, g, _ = ref.terms(b.f0, uva, uvb, q, b.Ka[i], b.Kb[i], b.R0[i], b.T0[i])
        assert np.abs(got.info[i] * b.f0 ** 2 - H).max() <= 1e-12 * np.abs(H).max(), i
        assert np.abs(grads[i] - g).max() <= 1e-12 * np.abs(g).max(), i
        s = rc.ref.sampson(rc.ref.fundamental(ref.skew(b.T0[i]) @ b.R0[i], b.Ka[i], b.Kb[i]), uva, uvb, b.f0)
        score = float(np.sum((np.ones(len(s)) if q is None else q) * s))
        assert abs(got.quality[i, 0] ** 2 * n - score) <= pc.energy_tolerance(b, i, score, n), i
        assert np.array_equal(got.R[i], b.R0[i]) and np.array_equal(got.T[i], b.T0[i]), i          # attempts = 0: bit for bit


def test_host_walk_against_the_yardstick_on_the_ragged_cases():
    """the kernel's order of operations (the deal to 64 lanes by rank, the tree down by 32 .. 1, the written-out 5 x 5 solve) on the
    host: the same decisions on every pair, E_pair within the bound, the pose within the bound the device is held to"""
    worst = pc.host_walk_floor()
    print(f"host walk against the yardstick: {worst:.3e} Newton steps")
    assert worst <= 1.0    # a rounding-level difference is a small part of the step that remains; the device gets 10 x the measured value


@pytest.mark.parametrize("loss", ["huber", "cauchy"])
def test_host_walk_with_a_loss(loss):
    b = pc.ragged(True)
    kind = {"huber": ref.HUBER, "cauchy": ref.CAUCHY}[loss]
    ys = pc.tagged([pc.yardstick(b, i, attempts=3, rel_change=0.0, kind=kind, delta=1.0) for i in range(b.n)], 0.0)
    got, _, logs = pc.host_walk(b, 3, 0.0, loss=loss, delta=1.0, want_weights=True)
    pc.agree(got, ys, b, kind, 1.0, logs=logs, bound=1.0)
    assert np.abs(got.weights - np.concatenate([y["w"] for y in ys])).max() <= 1e-10
    assert not got.weights[b.q == 0].any()


def test_host_walk_bits_and_ordering():
    """q = 0 gives the bits of the pair without the match, q all 1 those of q NULL, and E_out <= E_start on every case"""
    b = pc.ragged(True)
    short, keep = pc.without_holes(b)
    short.R0, short.T0 = b.R0, b.T0
    a, ga, _ = pc.host_walk(b, 4, 1e-6, loss="cauchy", delta=1.0, want_weights=True)
    c, gc, _ = pc.host_walk(short, 4, 1e-6, loss="cauchy", delta=1.0, want_weights=True)
    for x, y in zip(a[:7] + (ga, a.weights[keep]), c[:7] + (gc, c.weights)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    one = rc.SimpleNamespace(**{**vars(short), "q": np.ones_like(short.q)})
    none = rc.SimpleNamespace(**{**vars(short), "q": None})
    for x, y in zip(pc.host_walk(one, 4, 1e-6)[0][:7], pc.host_walk(none, 4, 1e-6)[0][:7]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    for holes in (False, True):
        bb = pc.ragged(holes)
        start, end = pc.host_walk(bb, 0)[0], pc.host_walk(bb, 10, 1e-9)[0]
        live = start.quality[:, 1] >= 5
        assert np.all(end.quality[live, 0] <= start.quality[live, 0])


def test_status_words():
    b = pc.ragged(False)
    few = pc.host_walk(pc.rows(b, [1]))[0]
    assert few.status[0] == PR.PAIR_FEW_POINTS and np.isnan(few.quality[0, 3]) and np.array_equal(few.R[0], b.R0[1])
    one = pc.host_walk(pc.rows(b, [9]), attempts=1)[0]
    assert one.status[0] == PR.PAIR_NOT_CONVERGED and one.quality[0, 5] == 1
    flat = pc.host_walk(pc.copies(), attempts=2)[0]
    assert (flat.status[0] & PR.PAIR_DEGENERATE) or flat.quality[0, 3] >= 1e12, (flat.status, flat.quality)
    assert PR.pair_status_names(PR.PAIR_FEW_POINTS | PR.PAIR_DEGENERATE | PR.PAIR_NOT_CONVERGED) == ["FEW_POINTS", "DEGENERATE", "NOT_CONVERGED"]
    assert sa.default_pair_options() == dict(attempts=10, rel_change=1e-9, loss_kind=0, loss_delta_pixels=0.0, inliers_only=0)


# ------------------------------------------------------------------ the factor helper
@pytest.mark.parametrize("baseline", [0.5, 4.0])
def test_factor_helper(baseline):
    """For 20 random d = [w; beta] of length 1e-4: the pose moved by d, the factor's residual [e_t; e_r] between frame a = (I, 0) and
    the moved frame b at the baseline (tests/relpose_ref.py), and e^T L e = d^T info d to the second order; L [z; 0] = 0; and the
    setter's check accepts the factor."""
    b = pc.ragged(False)
    i = len(pc.LENGTHS) - 1
    uva, uvb, _ = pc.pair_obs(b, i)
    res = PR.host_pair(b.f0, uva, uvb, b.Ka[i], b.Kb[i], b.R0[i], b.T0[i])[0]
    R, T, info, basis = res.R[0], res.T[0], res.info[0], res.basis[0]
    Z, z, L21 = sa.relative_pose_factor(R, T, info, basis, baseline)
    L = relpose_ref.full(L21)[0]
    assert np.array_equal(Z, R.T) and np.abs(z + baseline * R.T @ T).max() <= 4 * ref.EPS * baseline
    assert np.abs(L @ np.concatenate([z, np.zeros(3)])).max() <= 1e-12 * np.abs(L).max() * baseline
    w = np.linalg.eigvalsh(L)
    assert w[0] >= -1e-12 * w[-1] and w[1] > 1e-9 * w[-1]                       # positive semi-definite, of rank 5
    fac = relpose_ref.Factors([0], [1], Z, z, L)
    rng = np.random.default_rng(2680)
    for _ in range(20):
        d = rng.normal(size=5)
        d *= 1e-4 / np.linalg.norm(d)
        Rm, Tm = ref.move(R, T, d)
        so = rc.SimpleNamespace(cam_R=np.stack([np.eye(3), Rm]), cam_T=np.stack([np.zeros(3), baseline * Tm]))
        e = relpose_ref.residuals(fac, so)[0]
        want, got = d @ info @ d, e @ L @ e
        assert abs(got - want) <= 10 * 1e-4 * want, (got, want)
    why = C.c_char_p()
    fa, fb = np.array([0], np.int32), np.array([1], np.int32)
    code = sa.lib().srk_ba_check_relative_pose_factors(C.c_int32(1), *[x.ctypes.data_as(C.c_void_p) for x in (fa, fb, Z, z, L21)], C.byref(why))
    assert code == 0, why.value
    with pytest.raises(ValueError):
        sa.relative_pose_factor(R, T, info, basis, 0.0)


# ------------------------------------------------------------------ the checks
def test_python_check_pairs():
    """one refusal per rule, with its text"""
    b = pc.ragged(True)
    args = (b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb, b.R0, b.T0)
    assert PR.check_pairs(*args, q=b.q) is None

    def bad(i, f, **kw):
        a = [np.array(x, copy=True) for x in args]
        f(a[i])
        return PR.check_pairs(*a, **kw)
    assert "row_ptr[0]" in bad(0, lambda a: a.__setitem__(0, 1))
    assert "decreases at pair 3" in bad(0, lambda a: a.__setitem__(4, a[3] - 1))
    assert "uv_a of match 7" in bad(1, lambda a: a.__setitem__((7, 1), np.nan))
    assert "uv_b of match 9" in bad(2, lambda a: a.__setitem__((9, 0), np.inf))
    assert "K_a of pair 2 is not finite" in bad(3, lambda a: a.__setitem__((2, 1, 1), np.nan))
    assert "K_b of pair 2 is singular" in bad(4, lambda a: a.__setitem__((2, 2), np.zeros(3)))
    assert "R0 of pair 5 is not finite" in bad(5, lambda a: a.__setitem__((5, 1, 1), np.nan))
    assert "R0 of pair 5 is not orthogonal" in bad(5, lambda a: a.__setitem__((5, 1, 1), a[5, 1, 1] + 1e-6))
    assert "R0 of pair 5 has determinant" in bad(5, lambda a: a.__setitem__(5, -a[5]))
    assert "T0 of pair 6 is not finite" in bad(6, lambda a: a.__setitem__((6, 0), np.inf))
    assert "T0 of pair 6 is not a unit vector" in bad(6, lambda a: a.__setitem__(6, a[6] * (1 + 1e-8)))
    q = b.q.copy()
    q[9] = -1.0
    assert "q of match 9" in PR.check_pairs(*args, q=q)
    q[9] = np.inf
    assert "q of match 9" in PR.check_pairs(*args, q=q)
    assert "attempts outside 0..64" in PR.check_pairs(*args, attempts=-1) and "attempts outside 0..64" in PR.check_pairs(*args, attempts=65)
    assert PR.check_pairs(*args, attempts=0) is None and PR.check_pairs(*args, attempts=64) is None
    assert "rel_change" in PR.check_pairs(*args, rel_change=-1.0) and "rel_change" in PR.check_pairs(*args, rel_change=np.nan)
    assert "loss_kind outside 0..2" in PR.check_pairs(*args, loss=3, delta=1.0)
    assert "loss_delta_pixels" in PR.check_pairs(*args, loss="huber", delta=0.0) and "loss_delta_pixels" in PR.check_pairs(*args, loss="cauchy")
    assert "inliers_only must be 0 or 1" in PR.check_pairs(*args, inliers_only=2)
    assert "inliers_only has no meaning" in PR.check_pairs(*args, inliers_only=1)
    with pytest.raises(ValueError):
        PR.check_pairs(b.row_ptr, b.uv_a[:5], b.uv_b, b.Ka, b.Kb, b.R0, b.T0)
    with pytest.raises(ValueError):
        PR.check_pairs(b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb, b.R0[:3], b.T0)
    with pytest.raises(ValueError):
        PR.pair_options(loss="tukey")


def test_checks_and_defaults(program):
    r = subprocess.run([program, "unit"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0 failure(s)", r.stdout + r.stderr


def test_unit_runs_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan: the checks, walks with q = 0 in between and every loss, the
    factor helper"""
    if rc.cxx() is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "test_pair_host_san"
    r = pc.build_host_program(exe, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), "unit"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0 failure(s)", r.stdout + r.stderr
