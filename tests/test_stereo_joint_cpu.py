"""Joint stereo calibration, the parts that need no GPU: the yardstick's joint Jacobian against finite differences of its
own residual, its block route against its dense route on every case the GPU tests use, the host route of the joint
covariance against the dense inverse, the exported symbols and the Python surface, the argument checks that come before
any device call, and the resolution of fixed names into the joint mask."""
import ctypes
import os
import re

import numpy as np
import pytest

import stereo_joint_yardstick as jy
import stereo_yardstick as sy
from camera_calibration_amd import _native as nat
from camera_calibration_amd import engine, stereo
from conftest import ROOT

NEW_SYMBOLS = ("calib_stereo_joint_normal_eq", "calib_stereo_joint_step_delta", "calib_refine_stereo_joint")
PAIRS = [("radtan", "radtan"), ("radtan", "fisheye"), ("fisheye", "radtan"), ("fisheye", "fisheye")]
# the ragged case of tests/test_gpu_stereo_joint.py
NA, NB = (7, 0, 16, 3, 33, 70, 54, 40), (5, 9, 0, 17, 64, 70, 0, 60)


def raggedCase(pair):
    prob, PsTrue = sy.makeStereo(8, pair[0], pair[1], board=(10, 7, 0.05), noiseSigma=0.3, countsA=NA, countsB=NB)
    return prob, PsTrue, jy.perturbedJoint(prob, PsTrue, 1.0, 0.03, 1.0, 0.01)


def _stencil(f, x, j, h):
    """fourth-order central difference of f along coordinate j"""
    def at(s):
        y = x.copy()
        y[j] += s * h
        return f(y)
    return (-at(2) + 8 * at(1) - 8 * at(-1) + at(-2)) / (12 * h)


@pytest.mark.parametrize("pair", [("radtan", "fisheye"), ("fisheye", "radtan")], ids=lambda p: f"{p[0]}-{p[1]}")
def test_yardstick_joint_jacobian_against_fourth_order_differences_of_its_own_residual(pair):
    """M = 3, mixed models, ragged counts. Per column: the stencil at steps h and 2 h differ by the stencil's truncation
    error, and its four evaluations, each rounded to eps |f|, weigh 18 / (12 h) in all: its own error is the sum of the
    two (the projection is exactly linear in uc and vc: there the truncation term is 0 and only the rounding is left);
    the bar is ten times that. Steps: 1e-3 relative for the focal lengths and the principal point, 1e-3 absolute for the
    skew and the distortion coefficients, 2e-2 degrees, 1e-3 metres."""
    prob, Ps = sy.makeStereo(3, pair[0], pair[1], countsA=(20, 0, 11), countsB=(9, 14, 17))
    La, Lb, S = jy.sizes(prob)
    Pj = jy.join(prob, Ps)
    J = jy.jacobianDense(prob, Pj)
    assert J.shape == (2 * (31 + 40), S + 18)

    def f(p):
        return -jy.residualVector(prob, p)               # the projection, up to the constant sensor points

    def step(j):
        if j < La + Lb:
            c = j if j < La else j - La
            return 1e-3 * abs(Pj[j]) if c in (0, 1, 3, 4) else 1e-3
        return 2e-2 if ((j - La - Lb) % 6) < 3 else 1e-3
    # |f| of the rounding term: the projections themselves (the residual subtracts the sensor points, here equal to them)
    worstRatio, fmax = 0.0, max(np.abs(prob["uv_a"]).max(), np.abs(prob["uv_b"]).max())
    for j in range(Pj.shape[0]):
        h = step(j)
        d1, d2 = _stencil(f, Pj, j, h), _stencil(f, Pj, j, 2 * h)
        own = np.abs(d1 - d2).max() + 1.5 * np.finfo(float).eps * fmax / h
        got = np.abs(J[:, j] - d1).max()
        print(f"column {j:2d}: |J| max {np.abs(J[:, j]).max():.3e}  stencil's own error {own:.3e}  bar {10 * own:.3e}  "
              f"analytic - stencil {got:.3e}")
        assert np.abs(J[:, j]).max() > 0
        assert got <= 10 * own, (j, got, own)
        worstRatio = max(worstRatio, got / own)
    print(f"worst (analytic - stencil) / (stencil's own error): {worstRatio:.3f}")
    na2 = 2 * prob["xyz_a"].shape[0]
    assert not J[:na2, La:S].any()                       # camera a's rows: no shared_b, no rig
    assert not J[na2:, :La].any()                        # camera b's rows: no shared_a


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_block_route_and_dense_route_of_the_yardstick_agree(pair):
    """on the ragged case of the GPU tests, with and without a mask: the bars of the GPU step test (1e-9) stand on a
    yardstick whose two routes agree to 1e-11"""
    prob, _, Pj = raggedCase(pair)
    La, Lb, S = jy.sizes(prob)
    J = jy.jacobianDense(prob, Pj)
    nb = jy.normalBlocks(prob, Pj)
    JTJ = J.T @ J
    assert np.abs(nb["B"] - JTJ[:S, :S]).max() <= 1e-12 * np.abs(JTJ[:S, :S]).max()
    assert np.abs(nb["g"] - J.T @ jy.residualVector(prob, Pj)).max() <= 1e-12 * np.abs(nb["g"]).max()
    assert not nb["B"][:La, La:].any()
    # masks: none, both cameras, the last distortion coefficient of each camera (both skews fixed put the
    # fisheye-fisheye pair's two routes 2.3e-11 apart at lambda 1e-3: that case was replaced, not the bar)
    for mask in (0, (1 << La + Lb) - 1, 1 << La - 1 | 1 << La + Lb - 1):
        for lam in (1e-3, 10.0):
            d, b = jy.stepDense(prob, Pj, lam, mask), jy.stepFromBlocks(nb, lam, mask)
            rel = np.linalg.norm(d - b) / np.linalg.norm(d)
            print(f"{pair} mask {mask:#x} lambda {lam}: |blocks - dense| / |dense| = {rel:.3e}")
            assert rel <= 1e-11
            assert not d[:S][[s for s in range(S) if mask >> s & 1]].any()


def test_all_camera_bits_fixed_is_the_rig_only_problem():
    prob, PsTrue, Pj = raggedCase(("radtan", "fisheye"))
    La, Lb, S = jy.sizes(prob)
    p, Ps = jy.split(prob, Pj)
    d = jy.stepDense(prob, Pj, 1e-3, (1 << La + Lb) - 1)
    ref = sy.stepDense(p, Ps, 1e-3)
    rel = np.linalg.norm(d[La + Lb:] - ref) / np.linalg.norm(ref)
    print(f"joint step with both cameras fixed vs the rig-only dense step: {rel:.3e}")
    assert rel <= 1e-11


def test_joint_covariance_from_blocks_equals_the_dense_inverse():
    prob, PsTrue = sy.makeStereo(6, "fisheye", "radtan", noiseSigma=0.3, countsA=(30, 54, 0, 12, 54, 54),
                                 countsB=(54, 0, 25, 40, 54, 54))
    Pj = jy.join(prob, sy.perturbed(PsTrue, 0.05, 0.01, 0.02, 0.001))
    La, Lb, S = jy.sizes(prob)
    nb = jy.normalBlocks(prob, Pj)
    n = prob["xyz_a"].shape[0] + prob["xyz_b"].shape[0]
    for mask in (0, 0b100 | 1 << La + 2 | 1 << S - 1):
        C = stereo.jointCovarianceFromBlocks(nb["B"], nb["E"], nb["V"], nb["sseA"] + nb["sseB"], n, mask)
        Cd = jy.covarianceDense(prob, Pj, mask)
        rel = np.abs(C - Cd).max() / np.abs(Cd).max()
        print(f"joint covariance mask {mask:#x}, blocks vs dense: {rel:.3e} of the largest entry")
        assert rel <= 1e-9
        fixedIdx = [s for s in range(S) if mask >> s & 1]
        assert not C[fixedIdx].any() and not C[:, fixedIdx].any()
    with pytest.raises(ValueError, match="degrees of freedom"):
        stereo.jointCovarianceFromBlocks(nb["B"], nb["E"], nb["V"], 1.0, (S + 36) // 2)


def test_header_declares_and_library_exports_the_joint_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "calib_lm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(calib_[a-z0-9_]+)\s*\(", text))
    lib = nat.loadLibrary()
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in include/calib_lm.h"
        assert n in nat.SIGNATURES, f"{n} has no ctypes signature"
        assert hasattr(lib, n), f"{n} is not exported by the library"
    assert lib.calib_version() >= 460
    for n in ("stereoJointNormalEquations", "stereoJointStepDelta", "refineStereoJoint"):
        assert hasattr(engine, n)
    import inspect
    import camera_calibration_amd as cca
    sig = inspect.signature(cca.stereoCalibrate).parameters
    assert sig["refineCameras"].default is False and sig["fixedA"].default is None and sig["fixedB"].default is None
    assert inspect.signature(cca.calibrateStereo).parameters["joint"].default is False
    for n in ("covariance", "rigCovariance", "jointParameterNames", "cameras", "rectify", "triangulate"):
        assert hasattr(cca.StereoCalibration, n)


def _cProblem(prob, **over):
    """the C struct with shared_a / shared_b NULL: the joint calls do not read them"""
    keep = {k: np.ascontiguousarray(v) for k, v in prob.items() if isinstance(v, np.ndarray)}
    for k, v in over.items():
        if isinstance(v, np.ndarray):
            keep[k] = v
    f = dict(model_a=prob["model_a"], model_b=prob["model_b"], num_views=sy.numViews(prob))
    f.update({k: v for k, v in over.items() if not isinstance(v, np.ndarray)})
    for c in ("a", "b"):
        f["offs_" + c] = nat.i64ptr(keep["offs_" + c])
        for k in ("uv_", "xyz_"):
            f[k + c] = nat.dptr(keep[k + c])
    return nat.StereoProblem(**f), keep


def test_argument_checks_return_invalid_before_any_device_call():
    """On a machine without a GPU a device call would give CALIB_E_HIP: CALIB_E_INVALID shows the check came first."""
    lib = nat.loadLibrary()
    prob, Ps = sy.makeStereo(3, countsA=(5, 6, 7), countsB=(7, 6, 5))       # radtan / fisheye: S = 25
    Pj = np.ascontiguousarray(jy.join(prob, Ps))
    K = Pj.shape[0]
    assert jy.sizes(prob)[2] == 25

    def calls(p, mask=0, iters=5, P=Pj):
        out = np.empty(K)
        sse, it = ctypes.c_double(), ctypes.c_int()
        inout = None if P is None else nat.dptr(P.copy())
        return (lib.calib_stereo_joint_normal_eq(ctypes.byref(p), None if P is None else nat.dptr(P), None, None, None,
                                                 nat.dptr(out), None, 0),
                lib.calib_stereo_joint_step_delta(ctypes.byref(p), None if P is None else nat.dptr(P), mask, 1e-3,
                                                  nat.dptr(out), 0),
                lib.calib_refine_stereo_joint(ctypes.byref(p), inout, mask, iters, 1e-3, 1e-10, 1e10, 1e-12, ctypes.byref(sse),
                                              None, ctypes.byref(it), None, 0))
    good, keep = _cProblem(prob)
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
    assert calls(good, P=None) == (nat.E_INVALID,) * 3                             # NULL Pj
    assert calls(good, iters=0)[2] == nat.E_INVALID and calls(good, iters=-3)[2] == nat.E_INVALID
    for mask in (1 << 25, 1 << 63, (1 << 64) - 1):                                 # a bit at or above S
        assert calls(good, mask=mask)[1:] == (nat.E_INVALID,) * 2
    # a good call gets past the checks: without a device it is CALIB_E_HIP, with one it succeeds
    assert calls(good, mask=1 << 24)[1] in (0, nat.E_HIP)
    with pytest.raises(ValueError):
        engine.refineStereoJoint(*sy.engineCameras(prob), Pj, 0)
    with pytest.raises(ValueError, match="shape"):
        engine.stereoJointStepDelta(*sy.engineCameras(prob), Pj[:-1], 1e-3)
    with pytest.raises(ValueError, match="mask"):
        engine.stereoJointStepDelta(*sy.engineCameras(prob), Pj, 1e-3, fixedMask=1 << 25)


def test_fixed_names_resolve_into_the_joint_mask_and_names():
    R, F = nat.MODEL_RADTAN, nat.MODEL_FISHEYE
    names = stereo.jointParameterNames(R, F)
    assert len(names) == 25 and names[0] == "a.alpha" and names[9] == "a.k3" and names[10] == "b.alpha"
    assert names[18] == "b.k4" and names[19:] == ("rig.rx", "rig.ry", "rig.rz", "rig.tx", "rig.ty", "rig.tz")
    assert stereo.jointFixed(R, F, None, None) == (0, {})
    mask, values = stereo.jointFixed(R, F, "skew", {"k4": 0.0, "focal": None})
    assert mask == 0b100 | (0b11 | 1 << 8) << 10 and values == {10 + 8: 0.0}
    mask, values = stereo.jointFixed(F, R, "all", ["tangential"])
    assert mask == (1 << 9) - 1 | (0b11 << 7) << 9 and values == {}
    mask, values = stereo.jointFixed(R, R, 0b1, {"uc": 320.0})
    assert mask == 0b1 | 0b1000 << 10 and values == {13: 320.0}
    with pytest.raises(ValueError, match="p1"):
        stereo.jointFixed(R, F, None, "p1")                                        # the fisheye model has no p1
    with pytest.raises(ValueError, match="refineCameras"):
        stereo.stereoCalibrate([None], [None], ("radtan", np.eye(3), np.zeros(5)), ("radtan", np.eye(3), np.zeros(5)),
                               fixedA="skew")
