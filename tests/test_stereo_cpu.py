"""Stereo calibration, the parts that need no GPU: the yardstick's own Jacobian against finite differences of its own
residual, the host route of rigCovariance against the dense inverse, the start-point arithmetic, the exported symbols
and the argument checks that come before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest

import stereo_yardstick as sy
from camera_calibration_amd import _native as nat
from camera_calibration_amd import stereo
from conftest import ROOT

NEW_SYMBOLS = ("calib_stereo_normal_eq", "calib_stereo_step_delta", "calib_refine_stereo")


def _stencil(f, x, j, h):
    """fourth-order central difference of f along coordinate j"""
    def at(s):
        y = x.copy()
        y[j] += s * h
        return f(y)
    return (-at(2) + 8 * at(1) - 8 * at(-1) + at(-2)) / (12 * h)


def test_yardstick_jacobian_against_fourth_order_differences_of_its_own_residual():
    """M = 3, mixed models, ragged counts, rig and pose angles away from 0 and one pose angle EXACTLY 0 (the identity
    quirk). Per column: the stencil at steps h and 2 h differ by the stencil's own error; the bar is ten times that."""
    prob, Ps = sy.makeStereo(3, "radtan", "fisheye", countsA=(20, 0, 11), countsB=(9, 14, 17))
    Ps = Ps.copy()
    Ps[6 + 6 * 1 + 2] = 0.0                              # rho_z of view 1
    assert np.all(np.abs(Ps[:3]) > 1.0)
    J = sy.jacobianDense(prob, Ps)

    def f(p):
        return -sy.residualVector(prob, p)               # the projection, up to the constant sensor points
    worstRatio = 0.0
    for j in range(Ps.shape[0]):
        h = 2e-2 if (j % 6) < 3 else 1e-3                # degrees | metres
        d1, d2 = _stencil(f, Ps, j, h), _stencil(f, Ps, j, 2 * h)
        own = np.abs(d1 - d2).max()
        got = np.abs(J[:, j] - d1).max()
        print(f"column {j:2d}: |J| max {np.abs(J[:, j]).max():.3e}  stencil's own error {own:.3e}  bar {10 * own:.3e}  "
              f"analytic - stencil {got:.3e}")
        assert np.abs(J[:, j]).max() > 0
        assert got <= 10 * own, (j, got, own)
        worstRatio = max(worstRatio, got / own)
    print(f"worst (analytic - stencil) / (stencil's own error): {worstRatio:.3f}")
    # the rig columns of camera a's rows are exactly zero
    assert not J[:2 * prob["xyz_a"].shape[0], :6].any()


def test_rig_covariance_from_blocks_equals_the_dense_inverse():
    prob, PsTrue = sy.makeStereo(4, "fisheye", "radtan", noiseSigma=0.3, countsA=(30, 54, 0, 12), countsB=(54, 0, 25, 40))
    Ps = sy.perturbed(PsTrue, 0.05, 0.01, 0.02, 0.001)
    nb = sy.normalBlocks(prob, Ps)
    n = prob["xyz_a"].shape[0] + prob["xyz_b"].shape[0]
    C = stereo.rigCovarianceFromBlocks(nb["B"], nb["E"], nb["V"], nb["sseA"] + nb["sseB"], n)
    Cd = sy.covarianceDense(prob, Ps)
    scale = np.sqrt(np.outer(np.diagonal(Cd), np.diagonal(Cd)))
    rel = np.abs(C - Cd) / scale
    print(f"rig covariance, blocks vs dense: max |dC_ij| / sqrt(C_ii C_jj) = {rel.max():.3e}; std {np.sqrt(np.diagonal(C))}")
    assert rel.max() <= 1e-9
    assert np.allclose(C, C.T, rtol=0, atol=1e-12 * scale.max())


def test_rig_covariance_needs_degrees_of_freedom():
    with pytest.raises(ValueError, match="degrees of freedom"):
        stereo.rigCovarianceFromBlocks(np.eye(6), np.zeros((1, 6, 6)), np.eye(6)[None], 1.0, 6)      # 12 equations, 12 unknowns
    stereo.rigCovarianceFromBlocks(np.eye(6), np.zeros((1, 6, 6)), np.eye(6)[None], 1.0, 7)


def _exactPoses(M=7):
    _, Ps = sy.makeStereo(M)
    T = sy.parametersToPoses(Ps[:6])[0]
    Wa = sy.parametersToPoses(Ps[6:])
    return T, Wa, T @ Wa


def test_start_point_recovers_the_rig_from_exact_poses():
    T, Wa, Wb = _exactPoses()
    okA = np.array([1, 1, 0, 1, 0, 1, 1], dtype=bool)
    okB = np.array([1, 0, 1, 1, 1, 1, 0], dtype=bool)
    junk = np.tile(np.diag([1.0, -1.0, -1.0, 1.0]), (7, 1, 1))                 # what an unsolved view holds must not matter
    T0, W0 = stereo.rigStartPoint(np.where(okA[:, None, None], Wa, junk), np.where(okB[:, None, None], Wb, junk), okA, okB)
    print(f"start point: |T0 - T| {np.abs(T0 - T).max():.3e}  |W0 - Wa| {np.abs(W0 - Wa).max():.3e}")
    assert np.abs(T0 - T).max() <= 1e-9
    assert np.abs(W0 - Wa).max() <= 1e-9
    assert abs(np.linalg.det(T0[:3, :3]) - 1.0) <= 1e-12
    e = stereo.posesToParameters(W0)
    assert np.abs(stereo.parametersToPoses(e) - W0).max() <= 1e-12


def test_start_point_raises_for_a_view_nobody_solved_and_without_a_common_view():
    _, Wa, Wb = _exactPoses(3)
    with pytest.raises(ValueError, match="view 1"):
        stereo.rigStartPoint(Wa, Wb, [True, False, True], [True, False, True])
    with pytest.raises(ValueError, match="both cameras"):
        stereo.rigStartPoint(Wa, Wb, [True, False, True], [False, True, False])


def test_header_declares_and_library_exports_the_stereo_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "calib_lm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(calib_[a-z0-9_]+)\s*\(", text))
    lib = nat.loadLibrary()
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in include/calib_lm.h"
        assert n in nat.SIGNATURES, f"{n} has no ctypes signature"
        assert hasattr(lib, n), f"{n} is not exported by the library"
    import camera_calibration_amd as cca
    for n in ("stereoCalibrate", "calibrateStereo", "StereoCalibration"):
        assert hasattr(cca, n) and hasattr(cca.stereo, n)
    for n in ("stereoNormalEquations", "stereoStepDelta", "refineStereo"):
        assert hasattr(cca.engine, n)


def _cProblem(prob, **over):
    keep = {k: np.ascontiguousarray(v) for k, v in prob.items() if isinstance(v, np.ndarray)}
    for k, v in over.items():
        if isinstance(v, np.ndarray):
            keep[k] = v
    f = dict(model_a=prob["model_a"], model_b=prob["model_b"], num_views=sy.numViews(prob))
    f.update({k: v for k, v in over.items() if not isinstance(v, np.ndarray)})
    for c in ("a", "b"):
        f["offs_" + c] = nat.i64ptr(keep["offs_" + c])
        for k in ("uv_", "xyz_", "shared_"):
            f[k + c] = nat.dptr(keep[k + c])
    return nat.StereoProblem(**f), keep


def test_argument_checks_return_invalid_before_any_device_call():
    """On a machine without a GPU a device call would give CALIB_E_HIP: CALIB_E_INVALID shows the check came first."""
    lib = nat.loadLibrary()
    prob, Ps = sy.makeStereo(3, countsA=(5, 6, 7), countsB=(7, 6, 5))
    Ps = np.ascontiguousarray(Ps)
    K = Ps.shape[0]

    def calls(p, iters=5):
        out = np.empty(K)
        sse, it = ctypes.c_double(), ctypes.c_int()
        return (lib.calib_stereo_normal_eq(ctypes.byref(p), nat.dptr(Ps), None, None, None, nat.dptr(out), None, 0),
                lib.calib_stereo_step_delta(ctypes.byref(p), nat.dptr(Ps), 1e-3, nat.dptr(out), 0),
                lib.calib_refine_stereo(ctypes.byref(p), nat.dptr(out), iters, 1e-3, 1e-10, 1e10, 1e-12, ctypes.byref(sse),
                                        None, ctypes.byref(it), None, 0))
    good, keep = _cProblem(prob)
    assert lib.calib_refine_stereo(ctypes.byref(good), nat.dptr(Ps.copy()), 0, 1e-3, 1e-10, 1e10, 1e-12, None, None, None,
                                   None, 0) == nat.E_INVALID                       # max_iters <= 0
    assert lib.calib_refine_stereo(ctypes.byref(good), nat.dptr(Ps.copy()), -3, 1e-3, 1e-10, 1e10, 1e-12, None, None, None,
                                   None, 0) == nat.E_INVALID
    bad = [
        _cProblem(prob, model_a=2), _cProblem(prob, model_b=-1),                   # bad model id
        _cProblem(prob, offs_a=np.array([0, 5, 4, 18], dtype=np.int64)),           # non-monotone
        _cProblem(prob, offs_b=np.array([0, 7, 13, 12], dtype=np.int64)),
        _cProblem(prob, offs_b=np.array([-2, 7, 13, 18], dtype=np.int64)),         # negative
        _cProblem(prob, offs_a=np.array([0, -1, 11, 18], dtype=np.int64)),
        _cProblem(prob, num_views=0),
    ]
    for p, k in bad:
        assert calls(p) == (nat.E_INVALID,) * 3
    assert lib.calib_stereo_step_delta(ctypes.byref(good), None, 1e-3, None, 0) == nat.E_INVALID      # NULL Ps
    with pytest.raises(ValueError):
        from camera_calibration_amd import engine
        engine.refineStereo(*sy.engineCameras(prob), Ps, 0)
