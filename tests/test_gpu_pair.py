"""Two-view pose refinement on the device: srk_refine_pairs and srk_relate_frames_refined against the numpy
yardstick (tests/pair_ref.py) and the host walk of a pair, the bits of a pair in and out of a batch, the chained call against its
two halves, the status words, the refusals, the bootstrap and the C++ adapter."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import _lib
from surikatoko_amd import pair as PR
from surikatoko_amd import relate as RL
import pair_cases as pc
import pair_ref as ref
import relate_cases as rc
import resect_cases

pytestmark = pytest.mark.gpu
FIGURES = os.path.join(pc.ROOT, "profiles", "pair", "test_figures.json")


@pytest.fixture(scope="module")
def h():
    ba = sa.BundleAdjustmentKanatani(0)
    yield ba
    ba.close()


@pytest.fixture(scope="module")
def floor():
    """the largest distance, in Newton-step units, between the yardstick and the host walk over the two ragged batches: computed
    on the CPU (tests/test_pair_cpu.py holds it below 1), the device is held to ten times this"""
    return pc.host_walk_floor()


def _run(h, b, q="own", **kw):
    kw.setdefault("want_weights", True)
    return sa.refine_pairs(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb, b.R0, b.T0, q=b.q if isinstance(q, str) else q, **kw)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1)


def _pair_bits(res, b, i):
    s = slice(int(b.row_ptr[i]), int(b.row_ptr[i + 1]))
    return np.concatenate([_bits(res.R[i]), _bits(res.T[i]), _bits(res.E[i]), _bits(res.quality[i]), _bits(res.info[i]), _bits(res.basis[i]),
                           _bits(res.status[i:i + 1]), _bits(res.weights[s])])


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ------------------------------------------------------------------ against the host walk and the yardstick
@pytest.mark.parametrize("holes", [False, True])
def test_every_length_against_the_yardstick(h, floor, holes):
    """weighted lengths 0, 4, 5, 6, 63, 64, 65, 128, 129, 200 with half a pixel of noise; with holes, q = 0 entries in between"""
    b = pc.ragged(holes)
    attempts, rel_change = pc.RAGGED_OPTIONS[holes]
    ys = pc.tagged(pc.ragged_yardstick(holes), rel_change)
    assert all(resect_cases.margins_ok(y["log"], rel_change) for y in ys)          # no named case is excused
    got = _run(h, b, attempts=attempts, rel_change=rel_change)
    worst = pc.agree(got, ys, b, bound=10 * floor)
    walk = pc.host_walk(b, attempts, rel_change, want_weights=True)[0]
    for i, y in enumerate(ys):
        assert got.status[i] == walk.status[i] and np.array_equal(got.quality[i, [1, 4, 5]], walk.quality[i, [1, 4, 5]], equal_nan=True), i
        assert np.abs(got.info[i] - y["info"]).max() <= 1e-9 * max(np.abs(y["info"]).max(), 1e-300) * max(1.0, 10 * floor), i
    assert np.abs(got.weights - np.concatenate([y["w"] for y in ys])).max() <= 1e-10
    print(f"pose distance in Newton steps: host walk {floor:.3e}, device {worst:.3e}, bound {10 * floor:.3e}")


# ------------------------------------------------------------------ bits
def test_a_pairs_bits_do_not_depend_on_the_batch(h):
    """pair i alone, in a batch of 3 and in the batch of 130 unequal pairs (33 workgroups of four waves)"""
    whole = pc.many()
    assert whole.n == pc.BATCH_SIZES[-1]
    big = _run(h, whole, attempts=6, rel_change=1e-4)
    for idx in ([0, 1, 3], [127, 128, 129], [64, 2, 5]):
        small = pc.rows(whole, idx)
        three = _run(h, small, attempts=6, rel_change=1e-4)
        for k, i in enumerate(idx):
            one = _run(h, pc.rows(whole, [i]), attempts=6, rel_change=1e-4)
            assert np.array_equal(_pair_bits(one, pc.rows(whole, [i]), 0), _pair_bits(big, whole, i)), i
            assert np.array_equal(_pair_bits(three, small, k), _pair_bits(big, whole, i)), i
    assert big.status[2] == PR.PAIR_FEW_POINTS and np.count_nonzero(big.status == 0) > whole.n // 2


def test_q_zero_is_the_pair_without_the_match(h):
    b = pc.ragged(True)
    short, keep = pc.without_holes(b)
    short.R0, short.T0 = b.R0, b.T0
    a, c = _run(h, b, attempts=3, loss="cauchy", delta=1.0), _run(h, short, attempts=3, loss="cauchy", delta=1.0)
    assert _same(a[:7], c[:7]) and np.array_equal(_bits(a.weights[keep]), _bits(c.weights)) and not a.weights[~keep].any()
    one = _run(h, short, q=np.ones_like(short.q), attempts=3)
    none = _run(h, short, q=None, attempts=3)
    assert _same(one, none)


def test_shared_k_gives_the_bits_of_per_pair_arrays(h):
    b = pc.rows(pc.many(), range(9))
    Ka, Kb = np.repeat(rc.K0[None], b.n, axis=0), np.repeat(rc.K1[None], b.n, axis=0)
    per = sa.refine_pairs(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, Ka, Kb, b.R0, b.T0, attempts=3, want_weights=True)
    shared = sa.refine_pairs(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, rc.K0, rc.K1, b.R0, b.T0, attempts=3, want_weights=True)
    assert _same(per, shared)


def test_evaluate_only_returns_the_start(h):
    b = pc.ragged(True)
    got = _run(h, b, attempts=0)
    assert np.array_equal(_bits(got.R), _bits(b.R0)) and np.array_equal(_bits(got.T), _bits(b.T0)) and not got.quality[:, 5].any()
    assert not np.any(got.status & PR.PAIR_NOT_CONVERGED)
    full = _run(h, b, attempts=10)
    live = got.quality[:, 1] >= 5
    assert np.all(full.quality[live, 0] <= got.quality[live, 0])               # E_out <= E_start


# ------------------------------------------------------------------ the chained call
def _start_of(rel):
    """the start poses the chained call refines from: relate's, and (I, (1, 0, 0)) for a pair that was not related"""
    R0, T0 = rel.R.copy(), rel.T.copy()
    R0[rel.status != 0], T0[rel.status != 0] = np.eye(3), np.array([1.0, 0.0, 0.0])
    return R0, T0


@pytest.mark.parametrize("inliers_only", [False, True])
def test_chained_call_is_its_two_halves(h, inliers_only):
    """related, related_status and the inlier flags are those of srk_relate_frames; R, T, E, quality, info, basis, status and the
    weights those of srk_refine_pairs from the related poses -- with inliers_only, called with q * inliers.  The ragged batch holds
    pairs of 0, 4 and 5 matches, which relate does not relate: they are refined from (I, (1, 0, 0))."""
    b = pc.ragged(True)
    kw = dict(hypotheses=64, inlier_pixels=rc.TAU, seed=3)
    rel = sa.relate_frames(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb, q=b.q, want_inliers=True, **kw)
    opts = dict(attempts=4, rel_change=1e-6, loss="huber", delta=1.5)
    both, res = sa.relate_frames(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb, q=b.q, want_inliers=True,
                                 refine=dict(opts, inliers_only=inliers_only, want_weights=True), **kw)
    assert np.count_nonzero(rel.status) == 3 and np.count_nonzero(rel.status == 0) == 7
    assert _same((both.related, both.status, both.inliers), (rel.related, rel.status, rel.inliers))
    R0, T0 = _start_of(rel)
    q = b.q * rel.inliers if inliers_only else b.q
    alone = sa.refine_pairs(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb, R0, T0, q=q, want_weights=True, **opts)
    assert _same(res, alone) and _same((both.R, both.T, both.E), (alone.R, alone.T, alone.E))
    # without inlier_out and without the weights the same bits come back
    _, lean = sa.relate_frames(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb, q=b.q, refine=dict(opts, inliers_only=inliers_only), **kw)
    assert _same(lean[:7], alone[:7]) and lean.weights is None


def test_outliers(h, floor):
    """16 pairs of 200 matches, 0.5 px of noise, 30 % of the matches replaced, 256 hypotheses; refined on the winner's inliers with
    a Cauchy loss at the inlier threshold.  The device agrees with the yardstick refined from the same start, and the median
    rotation and direction errors to the truth after the refinement do not exceed those before (a numpy run of the yardstick from
    the host walk of relate, before committing the seed: see profiles/pair/test_figures.json)."""
    b = pc.outliers()
    attempts, rel_change = pc.OUTLIER_OPTIONS
    kw = dict(hypotheses=pc.OUTLIER_HYPOTHESES, inlier_pixels=pc.OUTLIER_TAU, seed=1)
    rel = sa.relate_frames(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb, want_inliers=True, **kw)
    both, res = sa.relate_frames(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb, want_inliers=True,
                                 refine=dict(attempts=attempts, rel_change=rel_change, loss="cauchy", delta=pc.OUTLIER_TAU, inliers_only=True,
                                             want_weights=True), **kw)
    assert not rel.status.any() and np.array_equal(rel.inliers, both.inliers)
    q = rel.inliers.astype(np.float64)
    ys = []
    for i in range(b.n):
        uva, uvb, _ = pc.pair_obs(b, i)
        s = slice(int(b.row_ptr[i]), int(b.row_ptr[i + 1]))
        ys.append(ref.refine_pair(b.f0, uva, uvb, q[s], b.Ka[i], b.Kb[i], rel.R[i], rel.T[i], attempts=attempts, rel_change=rel_change, kind=ref.CAUCHY,
                                  delta=pc.OUTLIER_TAU))
    view = rc.SimpleNamespace(**{**vars(b), "q": q, "R0": rel.R, "T0": rel.T})
    worst = pc.agree(res, pc.tagged(ys, rel_change), view, ref.CAUCHY, pc.OUTLIER_TAU, bound=10 * floor)
    before = np.array([pc.pose_error(rel.R[i], rel.T[i], b.R[i], b.T[i]) for i in range(b.n)])
    after = np.array([pc.pose_error(res.R[i], res.T[i], b.R[i], b.T[i]) for i in range(b.n)])
    figures = dict(pairs=b.n, rotation_before=float(np.median(before[:, 0])), rotation_after=float(np.median(after[:, 0])),
                   direction_before=float(np.median(before[:, 1])), direction_after=float(np.median(after[:, 1])), newton_units=worst)
    print("outliers:", json.dumps(figures))
    assert figures["rotation_after"] <= figures["rotation_before"] and figures["direction_after"] <= figures["direction_before"]
    saved = json.load(open(FIGURES)) if os.path.exists(FIGURES) else {}
    # the figures are written where none are recorded yet; recorded ones are left alone (the inequality above is the check)
    if "outliers_gpu" not in saved and os.path.isdir(os.path.dirname(FIGURES)) and os.access(os.path.dirname(FIGURES), os.W_OK):
        saved["outliers_gpu"] = figures
        with open(FIGURES, "w") as f:
            json.dump(saved, f, indent=1, sort_keys=True)
            f.write("\n")


# ------------------------------------------------------------------ status words
def test_status_words(h):
    b = pc.ragged(False)
    few = _run(h, pc.rows(b, [1]), attempts=5)                                    # four matches
    assert few.status[0] == PR.PAIR_FEW_POINTS and np.isnan(few.quality[0, 3]) and np.array_equal(few.R[0], b.R0[1]) and np.array_equal(few.T[0], b.T0[1])
    one = _run(h, pc.rows(b, [9]), attempts=1, rel_change=1e-9)                   # one attempt from the off start
    assert one.status[0] == PR.PAIR_NOT_CONVERGED and one.quality[0, 5] == 1
    c = pc.copies()
    flat = _run(h, c, attempts=2)
    assert (flat.status[0] & PR.PAIR_DEGENERATE) or flat.quality[0, 3] >= 1e12, (flat.status, flat.quality)
    assert PR.pair_status_names(PR.PAIR_FEW_POINTS | PR.PAIR_NOT_CONVERGED) == ["FEW_POINTS", "NOT_CONVERGED"]


# ------------------------------------------------------------------ bad arguments
def test_bad_arguments_launch_nothing(h):
    """one case per check: SRK_E_ARGS, the text is set, the outputs and the kernel time of the last good call stay what they were"""
    b = pc.ragged(True)
    _run(h, b, attempts=2)
    ms = PR.last_kernel_ms(h)
    assert ms > 0
    n, O = b.n, int(b.row_ptr[-1])
    L = _lib.lib()
    out = [np.full((n, 9), -7.5), np.full((n, 3), -7.5), np.full((n, 9), -7.5), np.full((n, 6), -7.5), np.full((n, 25), -7.5), np.full((n, 6), -7.5),
           np.full(n, 7, np.uint32), np.full(O, -7.5)]
    base = dict(f0=b.f0, row_ptr=b.row_ptr.copy(), uv_a=b.uv_a.copy(), uv_b=b.uv_b.copy(), q=b.q.copy(), Ka=b.Ka.copy(), Kb=b.Kb.copy(),
                R0=b.R0.copy(), T0=b.T0.copy(), opts=(3, 1e-9, 0, 0.0, 0), null=())

    def call(**kw):
        a = {**base, **kw}
        po = _lib.PairOptions(*a["opts"])
        ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
        outs = [None if k in a["null"] else ptr(o) for k, o in enumerate(out)]
        code = L.srk_refine_pairs(C.c_void_p(h._h), C.c_double(a["f0"]), C.c_int32(n), ptr(a["row_ptr"]), ptr(a["uv_a"]), ptr(a["uv_b"]), ptr(a["q"]),
                                  ptr(a["Ka"]), ptr(a["Kb"]), C.c_int(0), ptr(a["R0"]), ptr(a["T0"]), C.byref(po), *outs)
        return code, h.last_error()

    def changed(key, where, value):
        x = base[key].copy()
        x[where] = value
        return {key: x}
    cases = [(changed("row_ptr", 3, b.row_ptr[2] - 1), "decreases at pair 2"), (changed("row_ptr", 0, -1), "row_ptr[0]"),
             (changed("uv_a", (4, 0), np.nan), "uv_a of match 4"), (changed("uv_b", (5, 1), np.inf), "uv_b of match 5"),
             (changed("Ka", (1, 0, 0), np.nan), "K_a of pair 1 is not finite"), (changed("Kb", (2, 2), 0.0), "K_b of pair 2 is singular"),
             (changed("q", 3, -0.5), "q of match 3"), (changed("q", 3, np.inf), "q of match 3"),
             (changed("R0", (2, 0, 0), np.nan), "R0 of pair 2 is not finite"), (changed("R0", (2, 0, 0), 0.9), "R0 of pair 2 is not orthogonal"),
             (changed("T0", (4, 1), np.inf), "T0 of pair 4 is not finite"), (changed("T0", 4, 1.001 * b.T0[4]), "T0 of pair 4 is not a unit vector"),
             (dict(opts=(-1, 1e-9, 0, 0.0, 0)), "attempts outside 0..64"), (dict(opts=(65, 1e-9, 0, 0.0, 0)), "attempts outside 0..64"),
             (dict(opts=(3, -1.0, 0, 0.0, 0)), "rel_change"), (dict(opts=(3, np.nan, 0, 0.0, 0)), "rel_change"),
             (dict(opts=(3, 1e-9, 3, 1.0, 0)), "loss_kind outside 0..2"), (dict(opts=(3, 1e-9, 1, 0.0, 0)), "loss_delta_pixels"),
             (dict(opts=(3, 1e-9, 0, 0.0, 2)), "inliers_only must be 0 or 1"), (dict(opts=(3, 1e-9, 0, 0.0, 1)), "inliers_only has no meaning"),
             (dict(f0=0.0), "f0"), (dict(uv_b=None), "NULL match array"), (dict(Ka=None), "intrinsics array is NULL"), (dict(R0=None), "NULL start pose")]
    cases += [(dict(null=(k,)), "NULL output") for k in range(7)]
    for kw, text in cases:
        code, why = call(**kw)
        assert code == -1, (text, code)                      # SRK_E_ARGS
        assert text in why, (text, why)
        assert PR.last_kernel_ms(h) == ms
    assert all(np.all((a == 7) | (a == -7.5)) for a in out)    # nothing written
    code, _ = call(null=(7,))                                  # w_out may be NULL
    assert code == 0 and not np.any(out[3] == -7.5) and not np.any(out[6] == 7) and np.all(out[7] == -7.5) and PR.last_kernel_ms(h) > 0
    # the chained call: its own refusals
    with pytest.raises(Exception, match="inliers_only must be 0 or 1"):
        sa.relate_frames(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb, q=b.q, hypotheses=8, refine=dict(inliers_only=2))
    with pytest.raises(Exception, match="hypotheses outside"):
        sa.relate_frames(h, b.f0, b.row_ptr, b.uv_a, b.uv_b, b.Ka, b.Kb, q=b.q, hypotheses=0, refine=dict(attempts=2))


# ------------------------------------------------------------------ the bootstrap
def test_bootstrap_with_refinement(h):
    """relate's bootstrap case (150 landmarks, 0.5 px of noise, 20 % wrong matches): the scene triangulated from the refined pose has
    an RMS reprojection error not above that of the scene triangulated from the five-point winner"""
    rng = np.random.default_rng(2490)
    R = rc.rotation(np.array([0.05, -0.12, 0.04]))
    T = np.array([0.55, 0.75, 0.36])
    T /= np.linalg.norm(T)
    X = rc.points(150, rng)
    X[:, 2] *= 0.6
    ua, ub = rc.pixels(rc.K0, X) + 0.5 * rng.normal(size=(150, 2)), rc.pixels(rc.K0, X @ R.T + T) + 0.5 * rng.normal(size=(150, 2))
    moved = rng.choice(150, 30, replace=False)
    ub[moved] = np.column_stack([rng.uniform(-100.0, 700.0, 30), rng.uniform(-150.0, 600.0, 30)])
    H = RL.ransac_hypotheses(0.2, 0.999, 5)

    def rms(tv):
        err = [rc.pixels(rc.K0, tv.points @ tv.cam_R[f].T + tv.cam_T[f]) - tv.obs_uv.reshape(-1, 2, 2)[:, f] for f in range(2)]
        return float(np.sqrt(np.mean(np.sum(np.concatenate(err) ** 2, axis=1)) / 2.0))
    plain = sa.two_view_scene(h, rc.F0, ua, ub, rc.K0, rc.K0, hypotheses=H, inlier_pixels=rc.TAU)
    fine = sa.two_view_scene(h, rc.F0, ua, ub, rc.K0, rc.K0, hypotheses=H, inlier_pixels=rc.TAU,
                             refine=dict(attempts=10, loss="cauchy", delta=rc.TAU, inliers_only=True))
    assert len(fine.points) >= 100 and not np.isin(fine.match, moved).any()
    a, c = rms(plain), rms(fine)
    ea, ec = pc.pose_error(plain.cam_R[1], plain.cam_T[1], R, T), pc.pose_error(fine.cam_R[1], fine.cam_T[1], R, T)
    print(f"bootstrap: RMS {a:.4f} -> {c:.4f} px per coordinate, rotation {ea[0]:.3e} -> {ec[0]:.3e} rad, direction {ea[1]:.3e} -> {ec[1]:.3e} rad")
    assert c <= a and fine.relate.status[0] == 0


# ------------------------------------------------------------------ the C++ adapter
def test_cpp_adapter_pair(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "pair_adapter"
    r = subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(pc.ROOT, "include"), "-I", os.path.join(pc.ROOT, "demos"),
                        os.path.join(pc.ROOT, "tests", "cpp", "test_pair_adapter.cpp"), "-o", str(exe),
                        "-L", os.path.join(pc.ROOT, "surikatoko_amd"), "-lsrk_ba",
                        "-Wl,-rpath," + os.path.join(pc.ROOT, "surikatoko_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "pair adapter ok" in r.stdout
