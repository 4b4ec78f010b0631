"""The factor settings (surikatoko_amd/csrc/srk_factors.cpp) without a GPU: a stand-alone program (tests/cpp/test_factor_tables.cpp,
that unit and the scene planner alone) selects and builds every family's tables for the cases of tests/factor_table_cases.py;
every count and every table's size and digest must be those the commit before the unit existed computed inside its upload
(tests/golden/factor_tables_parent.json).  The golden was dumped from that commit on an MI355X: a temporary patch of its
srk_ba_host.hip (not committed) wrote the digests at the host-to-device copies of its five apply_* functions and of the pairs
it handed the planner as rel_a / rel_b, while every case was uploaded once.  Its psd verdicts are those of that commit's
relpose_info_psd, read through srk_ba_check_relative_pose_factors.  The residual functions are compared with the yardsticks."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import surikatoko_amd as sa
import factor_table_cases as ftc
import jointprior_ref as jr
import prior_ref as pref
import relpose_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surikatoko_amd", "csrc")
with open(os.path.join(ROOT, "tests", "golden", "factor_tables_parent.json")) as _f:
    GOLDEN = json.load(_f)


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


def _build(cxx, out, extra=()):
    return subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "test_factor_tables.cpp"),
                           os.path.join(CSRC, "srk_factors.cpp"), os.path.join(CSRC, "srk_plan.cpp"), "-pthread", "-o", str(out)],
                          capture_output=True, text=True)


@pytest.fixture(scope="module")
def case_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("factor_cases")
    files = []
    for name in ftc.NAMES:
        sc = ftc.case(name)["scene"].copy()
        ok, nrm = sa.normalize_scene_inplace(sc)  # the library's srk_ba_normalize_scene, as the upload calls it
        assert ok
        files.append(str(d / name))
        ftc.write_case(files[-1], name, nrm)
    psd = str(d / "psd_matrices")
    with open(psd, "wb") as f:
        f.write(np.ascontiguousarray(ftc.psd_matrices()).tobytes())
    return files, psd


def _parse(text):
    out, cur = {}, None
    for line in text.splitlines():
        w = line.split()
        if w[0] == "case":
            cur = out.setdefault(w[1], {"s": {}, "t": {}, "x": {}, "r": {}})
        elif w[0] == "t":
            cur["t"][w[1]] = [int(w[2]), w[3]]
        elif w[0] == "r":
            cur["r"][w[1]] = np.array([float.fromhex(v) for v in w[2:]])
        else:
            cur[w[0]][w[1]] = int(w[2])
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("factor_bin") / "test_factor_tables"
    r = _build(_cxx(), exe)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    return str(exe)


@pytest.fixture(scope="module")
def tables(program, case_files):
    r = subprocess.run([program, *case_files[0]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return _parse(r.stdout)


def test_unit_includes_no_hip_header():
    for name in ("srk_factors.cpp", "srk_factors.hpp"):
        with open(os.path.join(CSRC, name)) as f:
            assert not [line for line in f if line.lstrip().startswith("#include") and "hip" in line]


@pytest.mark.parametrize("name", ftc.NAMES)
def test_tables_are_the_parent_commits(tables, name):
    got, want = tables[name], GOLDEN["cases"][name]
    assert got["s"] == want["s"]
    assert sorted(got["t"]) == sorted(want["t"])
    wrong = {k: (got["t"][k], want["t"][k]) for k in want["t"] if got["t"][k] != want["t"][k]}
    assert not wrong, wrong
    assert got["x"]["snapshot_ignores_information"] == 1


def test_every_case_takes_its_branch(tables):
    s = {k: v["s"] for k, v in tables.items()}
    n = {k: {a: b[0] for a, b in v["t"].items()} for k, v in tables.items()}
    assert s["c_nf16_reordered"]["n_cst_frames"] == 4 and s["c_nf16_frames_and_landmarks_fixed_k"]["n_cst_pts"] > 0
    assert s["p_nf16_zero_prior_among_live"]["n_pri_frames"] == 1 and s["p_nf16_reordered"]["n_pri_frames"] == 4
    assert s["r_nf16_zero_factor_among_live"]["n_rp"] == 3 and n["r_nf16_zero_factor_among_live"]["rel_a"] == 3
    assert s["j_sixteen_frames_the_limit"]["n_jp_pairs"] == 120 and n["j_sixteen_frames_the_limit"]["jp_info"] == 96 * 96
    assert s["j_three_frames_one_zero_block"]["n_jp_pairs"] == 2
    assert s["j_two_sets_sharing_frame_5"]["n_jp_frames"] == 5 and n["j_two_sets_sharing_frame_5"]["jp_fr_ent"] == 6
    assert n["j_pair_with_relative_pose_factor"]["rel_a"] == 2  # the set's pair is the factor's: once in the planner's list
    assert s["j_mode_one_all_zero_set"]["n_jp"] == 2
    assert n["i_ragged_20"]["info_qf"] == 0 and n["i_two_kernel_60"]["info_qf"] == n["i_two_kernel_60"]["info_q"] > 0
    a = s["all_five_nf16_10_tiles"]
    assert a["info_on"] == 1 and min(a["n_cst_pts"], a["n_cst_frames"], a["n_pri_pts"], a["n_pri_frames"], a["n_rp"], a["n_jp"], a["n_jp_pairs"]) > 0
    for k in ("off_constant", "off_priors", "off_relpose", "off_jprior", "nothing_set"):
        assert not any(s[k].values()) and not any(v for key, v in n[k].items() if key != "cst_frame_int")
    assert n["off_constant"]["cst_frame_int"] == 24 and n["nothing_set"]["cst_frame_int"] == 0


def test_info_psd_gives_the_parent_commits_verdicts(program, case_files):
    r = subprocess.run([program, "psd", case_files[1]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(line.split()[3]) for line in r.stdout.splitlines()]
    assert got == GOLDEN["psd"] == [1, 1, 1, 0, 1]


RESIDUAL_CASES = ["residual_angles", "all_five_nf16_10_tiles", "r_ragged_pairs_given_backwards", "j_two_sets_sharing_frame_5", "p_nf2_full_information_rotated_world"]


@pytest.mark.parametrize("name", RESIDUAL_CASES)
def test_residuals_are_the_yardsticks(tables, name):
    """tolerances of the GPU residual tests: 1e-10 of the scene extent for translations, 1e-10 for rotations"""
    c = ftc.case(name)
    sc, r = c["scene"], tables[name]["r"]
    ext = float(np.abs(sc.points - sc.points.mean(axis=0)).max())
    if c["pri"] is not None:
        dp, df = pref.offsets(c["pri"][0], sc)
        assert np.abs(r["prior_points"].reshape(-1, 3) - dp).max(initial=0) < 1e-10 * ext
        assert np.abs(r["prior_frames"].reshape(-1, 3) - df).max(initial=0) < 1e-10 * ext
    if c["fac"] is not None:
        want, got = rr.residuals(c["fac"], sc), r["relpose"].reshape(-1, 6)
        assert np.abs(got[:, :3] - want[:, :3]).max() < 1e-10 * ext and np.abs(got[:, 3:] - want[:, 3:]).max() < 1e-10
    if c["sets"] is not None:
        want, got = np.concatenate(jr.residuals(c["sets"][0], sc)).reshape(-1, 6), r["jprior"].reshape(-1, 6)
        assert np.abs(got[:, :3] - want[:, :3]).max() < 1e-10 * ext and np.abs(got[:, 3:] - want[:, 3:]).max() < 1e-10
    if name == "residual_angles":  # both branches of the logarithm are taken, at the angles the case asks for
        ang = np.linalg.norm(r["relpose"].reshape(-1, 6)[:, 3:], axis=1)
        assert abs(ang[0] - 1e-5) < 1e-12 and abs(ang[1] - (np.pi / 2 - 1e-3)) < 1e-9 and ang[3] < 1e-12
        ang = np.linalg.norm((r["jprior"] + c["sets"][0].sets[0]["mean"]).reshape(-1, 6)[:, 3:], axis=1)
        assert abs(ang[0] - 1e-5) < 1e-12 and abs(ang[1] - (np.pi / 2 + 1e-3)) < 1e-9


def test_unit_runs_clean_under_the_sanitizers(tmp_path, case_files):
    """the same stand-alone program with AddressSanitizer and UBSan, over every case"""
    exe = tmp_path / "test_factor_tables_san"
    r = _build(_cxx(), exe, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    for args in (case_files[0], ["psd", case_files[1]]):
        r = subprocess.run([str(exe), *args], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
