"""The two-view fundamental matrix on the device: the kernels of srk_fund.hip against the numpy yardstick
(tests/fundamental_ref.py: SVD, polyfit, central differences) on the cases of tests/fundamental_cases.py, the bits, the status words,
the outliers, the noise-free pairs, a wrong K next to relate_frames, the argument checks and the C++ adapter."""
import ctypes as C
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import _lib
from surikatoko_amd import ba as B
from surikatoko_amd import fundamental as FD
import fundamental_cases as fc
import fundamental_ref as ref
from fundamental_cases import bounds

pytestmark = pytest.mark.gpu
ROOT = fc.ROOT


@pytest.fixture(scope="module")
def h():
    ba = sa.BundleAdjustmentKanatani(0)
    yield ba
    ba.close()


def _run(h, b, q="own", **kw):
    kw.setdefault("inlier_pixels", fc.TAU)
    kw.setdefault("want_inliers", True)
    return sa.relate_uncalibrated(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, q=b.q if isinstance(q, str) else q, **kw)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1)


def _same_bits(a, b, fields=("F", "U", "V", "sigma", "fund", "info", "status")):
    return all(np.array_equal(_bits(getattr(a, f)), _bits(getattr(b, f))) for f in fields)


def _pair(res, i):
    """pair i of a result as a result of one pair, without the inlier flags"""
    return FD.FundamentalResult(*[res[k][i:i + 1] for k in range(7)], None)


# ------------------------------------------------------------------ against the yardstick
@pytest.mark.parametrize("rounds", fc.ROUNDS)
@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("hypotheses", fc.HYPOTHESES)
def test_every_length_against_the_yardstick(h, hypotheses, holes, rounds):
    """the device is held to ten times the host walk's recorded distance from the yardstick (profiles/fundamental/test_figures.json)"""
    b = fc.ragged(holes)
    got = _run(h, b, hypotheses=hypotheses, seed=fc.SAMPLER_SEED, refine_rounds=rounds)
    worst = fc.agree(b, fc.ragged_yardstick(holes, hypotheses, rounds), got, *bounds())
    print(f"H {hypotheses} holes {holes} rounds {rounds}: score {worst[0]:.3e} relative, F {worst[1]:.3e} an entry; bounds {bounds()}")
    assert got.status[0] == FD.FUNDAMENTAL_FEW_POINTS and not got.status[1:].any()


@pytest.mark.parametrize("n_pairs", fc.BATCH_SIZES)
def test_batches_of_unequal_pairs(h, n_pairs):
    b = fc.many(n_pairs)
    got = _run(h, b, hypotheses=64)
    fc.agree(b, fc.many_yardstick(n_pairs), got, *bounds())
    if n_pairs > 1:
        assert got.status[1] == FD.FUNDAMENTAL_FEW_POINTS and got.fund[1, 1] == 7
    if n_pairs > 4:
        assert got.status[2] == FD.FUNDAMENTAL_FEW_POINTS and got.fund[2, 1] == 0


def test_a_pairs_bits_do_not_depend_on_the_batch_and_two_runs_agree(h):
    b = fc.many(17)
    whole = _run(h, b, hypotheses=65, seed=5)
    again = _run(h, b, hypotheses=65, seed=5)
    assert _same_bits(whole, again) and np.array_equal(whole.inliers, again.inliers)
    for i in range(b.n):
        alone = _run(h, fc.rows(b, [i]), hypotheses=65, seed=5)
        s = slice(int(b.row_ptr[i]), int(b.row_ptr[i + 1]))
        assert _same_bits(alone, _pair(whole, i)), i
        assert np.array_equal(alone.inliers, whole.inliers[s]), i


def test_unit_information_is_no_information_and_zero_is_absence(h):
    b = fc.ragged(True)
    short, keep = fc.without_holes(b)
    x, y = _run(h, b, hypotheses=65, seed=7), _run(h, short, hypotheses=65, seed=7)
    assert _same_bits(x, y)
    assert np.array_equal(x.inliers[keep], y.inliers) and not x.inliers[~keep].any()
    one, none = _run(h, short, q=np.ones_like(short.q), hypotheses=65, seed=7), _run(h, short, q=None, hypotheses=65, seed=7)
    assert _same_bits(one, none) and np.array_equal(one.inliers, none.inliers)


def test_no_rounds_return_the_winning_hypothesis_and_rounds_never_raise_the_score(h):
    b = fc.ragged(False)
    base = _run(h, b, hypotheses=64, seed=3, refine_rounds=0)
    host = fc.host_walk(b, 64, 3, rounds=0)
    assert not base.fund[:, 6].any() and not base.fund[:, 7].any()
    assert np.array_equal(base.fund[:, [1, 2, 4, 6, 7, 11]], host.fund[:, [1, 2, 4, 6, 7, 11]]) and np.array_equal(base.inliers, host.inliers)
    big = base.fund[:, 1] > 9                    # eight or nine matches draw orderings of the same samples: the winner is one of a tie
    assert np.array_equal(base.fund[big, 3], host.fund[big, 3])
    last = base.fund[1:, 0]
    for rounds in (1, 8, 16):
        got = _run(h, b, hypotheses=64, seed=3, refine_rounds=rounds)
        assert np.array_equal(got.fund[1:, 3], base.fund[1:, 3]) and (got.fund[1:, 7] <= rounds).all() and (got.fund[1:, 0] <= last).all()
        last = got.fund[1:, 0]
    assert (last < base.fund[1:, 0]).any()


# ------------------------------------------------------------------ outliers
@pytest.mark.parametrize("share", [0.3, 0.5])
def test_outliers(h, share):
    """200 matches with a share of the targets replaced: the inlier flags are the yardstick's outside a band of 1e-9 px^2 around
    tau^2 (the committed seeds keep the yardstick's own count of matches inside that band at zero)"""
    b, ps = fc.outliers(share)
    got = _run(h, b, hypotheses=fc.OUTLIER_HYPOTHESES[share], refine_rounds=fc.OUTLIER_ROUNDS)
    ys = fc.outlier_yardstick(share)
    for i, (p, y) in enumerate(zip(ps, ys)):
        ua, ub, _ = fc.pair_obs(b, i)
        assert int((np.abs(ref.sampson(y["F"], ua, ub, b.f0) - fc.TAU ** 2) <= fc.BAND).sum()) == 0
        assert np.array_equal(got.inliers[200 * i:200 * i + 200], y["inliers"]), i
        moved = np.zeros(200, bool)
        moved[p.moved] = True
        flags = got.inliers[200 * i:200 * i + 200].astype(bool)
        print(f"share {share} pair {i}: {flags[~moved].mean():.3f} of the unmoved and {flags[moved].mean():.3f} of the moved flagged, "
              f"{int(got.fund[i, 6])} of {int(got.fund[i, 7])} attempts accepted")
    fc.agree(b, ys, got, *bounds())


# ------------------------------------------------------------------ noise-free pairs
def test_noise_free_general_pairs(h):
    b, ps = fc.general_pairs()
    got = _run(h, b, hypotheses=64)
    for i, p in enumerate(ps):
        assert got.status[i] == 0 and got.fund[i, 2] == 40 and got.inliers[40 * i:40 * i + 40].all()
        fc.check_model(got, i)
        assert np.abs(got.F[i] - fc.true_fundamental(p)).max() <= 1e-9
        ea, eb = p.Ka @ (-p.R.T @ p.T), p.Kb @ p.T
        for e, col in ((ea, got.V[i][:, 2]), (eb, got.U[i][:, 2])):
            e = e / np.linalg.norm(e)
            assert min(np.abs(col - e).max(), np.abs(col + e).max()) <= 1e-9


def test_noise_free_planes_and_rotations_have_no_model(h):
    b, _ = fc.degenerate_pairs()
    got = _run(h, b, hypotheses=64)
    assert (got.status == FD.FUNDAMENTAL_NO_MODEL).all() and not got.fund[:, 4].any() and (got.fund[:, 1] == 40).all()
    assert not got.F.any() and not got.info.any() and not got.sigma.any() and not got.inliers.any()
    assert all(np.array_equal(got.U[i], np.eye(3)) and np.array_equal(got.V[i], np.eye(3)) for i in range(b.n))
    assert np.isnan(got.fund[:, [0, 3, 5, 8, 10]]).all() and not got.fund[:, [2, 6, 7, 9, 11]].any()
    host = fc.host_walk(b, 64, 1)
    assert np.array_equal(host.status, got.status) and np.array_equal(host.fund, got.fund, equal_nan=True)
    hg = sa.relate_homography(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb, hypotheses=64)
    assert not hg.status.any() and (hg.homog[:, 2] == 40).all()


# ------------------------------------------------------------------ a wrong K
def test_a_wrong_k_costs_relate_true_matches(h):
    """both focal lengths off by 20 %: relate_frames flags fewer of the unmoved matches than relate_uncalibrated on the same matches"""
    b, p, Ka, Kb = fc.wrong_k()
    unmoved = np.ones(200, bool)
    unmoved[p.moved] = False
    fd = _run(h, b, hypotheses=256)
    rl = sa.relate_frames(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, Ka, Kb, hypotheses=256, inlier_pixels=fc.TAU, seed=1, want_inliers=True)
    n_fd, n_rl = int(fd.inliers[unmoved].sum()), int(np.asarray(rl.inliers)[unmoved].sum())
    print(f"wrong K: relate flags {n_rl} of {int(unmoved.sum())} unmoved matches, relate_uncalibrated {n_fd}")
    fc.write_figures("wrong_k_true_matches_flagged_on_the_device", dict(relate=n_rl, relate_uncalibrated=n_fd, unmoved=int(unmoved.sum())))
    assert n_fd > n_rl


# ------------------------------------------------------------------ bad arguments
def test_bad_arguments_launch_nothing(h):
    """one case per check through the handle: the text is set, the outputs and the kernel time of the last good call stay what they were"""
    b = fc.ragged(True)
    _run(h, b, hypotheses=64)
    ms = FD.last_kernel_ms(h)
    assert ms[0] > 0 and 0 < ms[1] <= ms[0]
    O, n = int(b.row_ptr[-1]), b.n
    out = [np.full((n, 9), 7.0), np.full((n, 9), 7.0), np.full((n, 9), 7.0), np.full(n, 7.0), np.full((n, 12), 7.0), np.full((n, 49), 7.0),
           np.full(n, 7, np.uint32), np.full(O, 7, np.uint8)]
    good = dict(rp=b.row_ptr, a=b.uv_a, b=b.uv_b, q=b.q, f0=b.f0, lo=(64, fc.TAU, 1, 8), outs=tuple(range(8)))

    def call(**kw):
        a = dict(good, **kw)
        arr = {k: None if a[k] is None else np.ascontiguousarray(a[k], np.int64 if k == "rp" else np.float64) for k in ("rp", "a", "b", "q")}
        lo = _lib.FundamentalOptions(*a["lo"])
        p = {k: None if v is None else B._p(v) for k, v in arr.items()}
        code = sa.lib().srk_relate_uncalibrated(C.c_void_p(h._h), C.c_double(a["f0"]), C.c_int32(n), p["rp"], p["a"], p["b"], p["q"], C.byref(lo),
                                                *[B._p(o) if k in a["outs"] else None for k, o in enumerate(out)])
        return code, h.last_error()

    def changed(name, index, value):
        a = np.array(good[name], copy=True)
        a[index] = value
        return {name: a}
    cases = [
        (changed("rp", 0, 1), "row_ptr[0]"), (changed("rp", 4, b.row_ptr[3] - 1), "decreases"), (changed("rp", 1, -1), "decreases at pair 0"),
        (changed("q", 3, -1.0), "q of match 3"), (changed("q", 3, np.nan), "q of match 3"),
        (changed("a", (40, 1), np.nan), "uv_a of match 40"), (changed("b", (2, 0), np.inf), "uv_b of match 2"),
        (dict(lo=(0, fc.TAU, 1, 8)), "hypotheses"), (dict(lo=(4097, fc.TAU, 1, 8)), "hypotheses"), (dict(lo=(64, 0.0, 1, 8)), "inlier_pixels"),
        (dict(lo=(64, np.inf, 1, 8)), "inlier_pixels"), (dict(lo=(64, fc.TAU, 1, 17)), "refine_rounds"), (dict(lo=(64, fc.TAU, 1, -1)), "refine_rounds"),
        (dict(f0=0.0), "f0"), (dict(f0=np.nan), "f0"), (dict(a=None), "NULL match array"), (dict(b=None), "NULL match array"),
    ] + [(dict(outs=tuple(k for k in range(8) if k != miss)), "NULL output array") for miss in range(7)]
    for kw, text in cases:
        code, why = call(**kw)
        assert code == -1 and text in why, (text, code, why)
        assert FD.last_kernel_ms(h) == ms
    assert all(np.all(a == 7) for a in out)                    # nothing written
    code, _ = call(outs=tuple(range(7)))                       # inlier_out may be NULL
    assert code == 0 and not np.any(out[0] == 7) and np.all(out[7] == 7)
    code, _ = call()                                           # and the same call with good arguments runs
    assert code == 0 and not np.any(out[7] == 7) and FD.last_kernel_ms(h)[0] > 0


# ------------------------------------------------------------------ the C++ adapter
def test_cpp_adapter_fundamental(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "fund_adapter"
    r = subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "demos"),
                        os.path.join(ROOT, "tests", "cpp", "test_fund_adapter.cpp"), "-o", str(exe),
                        "-L", os.path.join(ROOT, "surikatoko_amd"), "-lsrk_ba",
                        "-Wl,-rpath," + os.path.join(ROOT, "surikatoko_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fundamental adapter ok" in r.stdout
