"""The scene planner (surikatoko_amd/csrc/srk_plan.cpp) without a GPU: a stand-alone program (tests/cpp/test_scene_plan.cpp,
the planner unit alone) plans the cases of tests/scene_plan_cases.py; every scalar decision and every table's size and digest
must be those the commit before the planner existed computed inside its upload (tests/golden/scene_plan_parent.json, dumped
from that commit at its host-to-device copies, 256 compute units).  Each case is there for a branch; the scalars say it is taken."""
import json
import os
import shutil
import subprocess

import pytest

import scene_plan_cases as spc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surikatoko_amd", "csrc")
with open(os.path.join(ROOT, "tests", "golden", "scene_plan_parent.json")) as _f:
    GOLDEN = json.load(_f)


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


def _build(cxx, out, extra=()):
    return subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "test_scene_plan.cpp"),
                           os.path.join(CSRC, "srk_plan.cpp"), "-pthread", "-o", str(out)], capture_output=True, text=True)


@pytest.fixture(scope="module")
def case_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan_cases")
    files = []
    for name in spc.NAMES:
        files.append(str(d / name))
        spc.write_case(files[-1], name)
    return files


def _parse(text):
    out, cur = {}, None
    for line in text.splitlines():
        w = line.split()
        if w[0] == "case":
            cur = out.setdefault(w[1], {"s": {}, "t": {}, "x": {}})
        elif w[0] == "t":
            cur["t"][w[1]] = [int(w[2]), w[3]]
        else:
            cur[w[0]][w[1]] = int(w[2])
    return out


@pytest.fixture(scope="module")
def plans(tmp_path_factory, case_files):
    exe = tmp_path_factory.mktemp("plan_bin") / "test_scene_plan"
    r = _build(_cxx(), exe)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    r = subprocess.run([str(exe), *case_files], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return _parse(r.stdout)


def test_planner_includes_no_hip_header():
    for name in ("srk_plan.cpp", "srk_plan.hpp", "srk_limits.hpp"):
        with open(os.path.join(CSRC, name)) as f:
            assert not [line for line in f if line.lstrip().startswith("#include") and "hip" in line]


@pytest.mark.parametrize("name", spc.NAMES)
def test_tables_are_the_parent_commits(plans, name):
    got, want = plans[name], GOLDEN[name]
    assert got["s"] == want["s"]
    assert sorted(got["t"]) == sorted(want["t"])
    wrong = {k: (got["t"][k], want["t"][k]) for k in want["t"] if got["t"][k] != want["t"][k]}
    assert not wrong, wrong


def test_every_case_takes_its_branch(plans):
    s = {k: v["s"] for k, v in plans.items()}
    n = {k: {a: b[0] for a, b in v["t"].items()} for k, v in plans.items()}
    a = s["a_uniform"]  # two frame lists = two uniform runs before the cut
    assert a["n_groups"] > 2 and a["n_mm_uniform"] == a["n_groups"] and a["n_mm_ragged"] == 0
    assert a["jac_runs"] == 1 and a["jac_runs_masked"] == 0 and a["jr_tasks"] > 0
    b = s["b_ragged"]
    assert b["n_mm_ragged"] > 0 and b["jac_runs"] == 1 and b["jac_runs_masked"] == 1 and n["b_ragged"]["jr_group"] == b["jr_tasks"] > 0
    c = s["c_mid_wide"]
    assert c["n_groups_mid"] > 0 and c["n_groups_wide"] > 0 and c["n_cal_list"] > 0 and n["c_mid_wide"]["cal_list"] == c["n_cal_list"]
    d = s["d_all_visible_30"]
    assert d["n_long_runs"] > 0 and d["n_long_items"] > 0 and d["long_fb"] == 8 and d["jr_own_runs"] == 1 and n["d_all_visible_30"]["jd_mask"] == 100
    e = s["e_all_visible_40"]
    assert e["n_long_runs"] > 0 and e["long_fb"] == 8 and e["jr_own_runs"] == 0
    e = s["e_all_visible_60"]
    assert e["n_long_runs"] > 0 and e["jr_own_runs"] == 0 and e["jac_runs"] == 0 and e["jac_fused"] == 0
    assert n["e_all_visible_60"]["fobs_pt"] == n["e_all_visible_60"]["fobs_of"] == 60 * 40
    assert s["f_over_4096"]["n_generic"] == 1 and n["f_over_4096"]["gen_list"] == 1
    assert s["g_long_fb16"]["long_fb"] == 16 and s["g_long_fb16"]["n_long_runs"] >= 103
    for k in ("h_shuffled_auto", "h_shuffled_given"):
        assert n[k]["frame_int"] == n[k]["frame_user"] == 12 and n[k]["obs_rank"] == n[k]["obs_frame"] > 0
        assert s[k]["frame_order_supplied"] == (1 if k == "h_shuffled_given" else 0)
        # the shuffle undone: from there on the plan is (b)'s
        assert plans[k]["t"]["grp_frames"] == plans["b_ragged"]["t"]["grp_frames"] and plans[k]["t"]["obs_frame"] == plans["b_ragged"]["t"]["obs_frame"]
    assert n["i_threaded_sort"]["perm"] == 40000 and plans["i_threaded_sort"]["x"]["perm_is_stable_sort"] == 1
    for k in ("j_uniform_det", "j_ragged_det"):
        assert s[k]["det_active"] == 1 and s[k]["ds_n_pairs"] == n[k]["ds_pair_fa"] > 0 and n[k]["dj_ptr"] > 0 and n[k]["ds_f_ent"] > 0
    k = "k_empty_multi_rank"
    assert n[k]["frame_int"] == 0 and n[k]["min_cv"] == 12 and plans[k]["x"]["min_cv_max"] == 0
    assert plans["b_ragged"]["x"]["min_cv_max"] > 0


def test_planner_runs_clean_under_the_sanitizers(tmp_path, case_files):
    """the same stand-alone program with AddressSanitizer and UBSan, over every case"""
    exe = tmp_path / "test_scene_plan_san"
    r = _build(_cxx(), exe, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), *case_files], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
