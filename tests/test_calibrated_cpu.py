"""Calibrated bundle adjustment (srk_ba_set_fixed_intrinsics) without a GPU: the C ABI entry points exist, the yardstick
of tests/calibrated_ref.py is the 6-variable Gauss-Newton step, and the C++ adapter's extension compiles."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import surikatoko_amd as sa
from surikatoko_amd import _lib
import calibrated_ref as cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_exports_fixed_intrinsics_entry_points_and_refuses_null():
    L = _lib.lib()
    for name in ("srk_ba_set_fixed_intrinsics", "srk_ba_frame_vars"):
        assert hasattr(L, name)
    L.srk_ba_set_fixed_intrinsics.argtypes = [C.c_void_p, C.c_int]
    L.srk_ba_frame_vars.argtypes = [C.c_void_p]
    assert L.srk_ba_set_fixed_intrinsics(None, 1) == -1  # SRK_E_ARGS
    assert L.srk_ba_set_fixed_intrinsics(None, 0) == -1
    assert L.srk_ba_frame_vars(None) == -1


def _dense_calibrated_step(gradE, V, U, W, row_ptr, obs_frame, N, M, c, comp=1):
    """the damped 6-variable normal equations assembled densely from the oracle's blocks, gauge variables removed:
    (H + c diag(H)) delta = -grad  (bundle-adj-kanatani.cpp:1819,1831)"""
    n = 3 * N + 6 * M
    H = np.zeros((n, n))
    for i in range(N):
        H[3 * i:3 * i + 3, 3 * i:3 * i + 3] = V[i]
    for j in range(M):
        a = 3 * N + 6 * j
        H[a:a + 6, a:a + 6] = U[j][4:, 4:]
    for i in range(N):
        for o in range(row_ptr[i], row_ptr[i + 1]):
            a = 3 * N + 6 * obs_frame[o]
            H[3 * i:3 * i + 3, a:a + 6] = W[o][:, 4:]
            H[a:a + 6, 3 * i:3 * i + 3] = W[o][:, 4:].T
    g = np.concatenate([gradE[:3 * N], gradE[3 * N:].reshape(M, 10)[:, 4:].reshape(-1)])
    H[np.diag_indices(n)] *= 1 + c
    fixed = set(range(3 * N, 3 * N + 6)) | {3 * N + 6 + comp}
    keep = np.array([k not in fixed for k in range(n)])
    x = np.zeros(n)
    x[keep] = np.linalg.solve(H[np.ix_(keep, keep)], -g[keep])
    return x


@pytest.mark.parametrize("c", [1e-4, 1e-1])
def test_yardstick_is_the_six_variable_gauss_newton_step(orc, c):
    spec = sa.SceneSpec(n_frames=5, grid_nx=4, grid_ny=3, vis_window=3)
    sc = sa.generate_scene(spec)
    so = orc.Scene(sc.points, sc.cam_R, sc.cam_T, sc.K, sc.shared_k, sc.row_ptr, sc.obs_frame, sc.obs_uv)
    assert orc.normalize(so)[0]
    N, M = so.N, so.M
    out = cref.step(orc, spec.f0, so, c, want_system=True)
    assert out["ok"]
    fr = out["corr10"][3 * N:].reshape(M, 10)
    assert np.all(fr[:, :4] == 0)  # the intrinsic corrections are exactly 0
    x = _dense_calibrated_step(out["gradE10"], out["V"], out["U10"], out["W10"], so.row_ptr, so.obs_frame, N, M, c)
    den = np.abs(x).max()
    assert np.abs(out["corr"] - x).max() / den < 1e-10
    # the compact system: gauge rows and columns empty, the rest symmetric
    S = out["S"]
    fixed = np.where(cref.compact_to_reduced(M) < 0)[0]
    assert len(fixed) == 7 and np.all(S[fixed] == 0) and np.all(S[:, fixed] == 0)
    assert np.abs(S - S.T).max() <= 1e-12 * np.abs(S).max()


def test_adapter_header_with_set_fixed_intrinsics_compiles(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "t.cpp"
    src.write_text('#include "suriko_amd/bundle-adj-kanatani.hpp"\n'
                   "void f(suriko_amd::BundleAdjustmentKanatani& ba) { ba.SetFixedIntrinsics(true); (void)ba.VarsCount(); }\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
