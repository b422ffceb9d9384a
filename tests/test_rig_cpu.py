"""The multi-camera rig without a GPU: the yardstick (tests/rig_yardstick.py) against the stereo yardstick at N = 2, the
start point from per-camera poses (rig.rigStartPoints), the result's arithmetic, the argument checks of the C ABI (which
return before any device call) and the guard of the GPU noisy-loop comparison."""
import ctypes
import os
import re

import numpy as np
import pytest

import camera_calibration_amd as cca
import rig_yardstick as ry
import stereo_yardstick as sy
from camera_calibration_amd import _native as nat
from camera_calibration_amd import engine, rig, stereo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("calib_rig_normal_eq", "calib_rig_step_delta", "calib_refine_rig")


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()


def test_two_cameras_are_the_stereo_yardstick():
    counts = [(7, 0, 16, 3, 33), (5, 9, 0, 17, 54)]
    prob, PrTrue = ry.makeRig(2, 5, ["radtan", "fisheye"], counts, noiseSigma=0.3)
    ps = ry.asStereo(prob)
    Pr = ry.perturbed(prob, PrTrue, 0.3, 0.02, 0.2, 0.004)
    a, b = ry.normalBlocks(prob, Pr), sy.normalBlocks(ps, Pr)
    worst = {k: rel(a[k], b[k]) for k in ("B", "E", "V", "g")}
    worst["sse"] = max(abs(a["sseCam"][0] / b["sseA"] - 1), abs(a["sseCam"][1] / b["sseB"] - 1))
    worst["jacobian"] = rel(ry.jacobianDense(prob, Pr), sy.jacobianDense(ps, Pr))
    for lam in (1e-3, 10.0):
        worst[f"step {lam}"] = rel(ry.stepDense(prob, Pr, lam), sy.stepDense(ps, Pr, lam))
    sseR, PrR, traceR = ry.refineDense(prob, Pr, 12)
    sseS, PsS, traceS = sy.refineDense(ps, Pr, 12)
    assert traceR.shape == traceS.shape
    worst["trace"] = rel(traceR, traceS)
    worst["refined"] = rel(PrR, PsS)
    worst["covariance"] = rel(ry.covarianceDense(prob, PrR), sy.covarianceDense(ps, PsS))
    print(f"N = 2, rig yardstick vs stereo yardstick: {worst}")
    assert max(worst.values()) <= 1e-13


def test_yardstick_blocks_and_dense_jacobian_agree_for_eight_cameras():
    rng = np.random.default_rng(5)
    counts = rng.choice([0, 1, 5, 16], size=(8, 3)).tolist()
    counts[0] = [0, 5, 16]
    for c in range(1, 8):
        counts[c][c % 3] = 5
    prob, PrTrue = ry.makeRig(8, 3, None, counts, noiseSigma=0.3)
    Pr = ry.perturbed(prob, PrTrue, 0.3, 0.02, 0.2, 0.004)
    J = ry.jacobianDense(prob, Pr)
    nb = ry.normalBlocks(prob, Pr)
    S = 42
    JTJ = J.T @ J
    assert rel(nb["B"], JTJ[:S, :S]) <= 1e-13
    for i in range(3):
        assert rel(nb["V"][i], JTJ[S + 6 * i:S + 6 * i + 6, S + 6 * i:S + 6 * i + 6]) <= 1e-13
        assert np.abs(nb["E"][i] - JTJ[:S, S + 6 * i:S + 6 * i + 6]).max() <= 1e-13 * np.abs(JTJ).max()
    assert rel(nb["g"], J.T @ ry.residualVector(prob, Pr)) <= 1e-13
    assert rel(ry.stepBlocks(prob, Pr, 1e-3), ry.stepDense(prob, Pr, 1e-3)) <= 1e-9
    # the analytic Jacobian against central differences of the projection
    h, k = 1e-6, [0, 7, 41, 42, 47, 59]
    for j in k:
        d = np.zeros_like(Pr)
        d[j] = h
        num = (np.concatenate([y.ravel() for y in ry.project(prob, Pr + d)]) -
               np.concatenate([y.ravel() for y in ry.project(prob, Pr - d)])) / (2 * h)
        assert np.abs(num - J[:, j]).max() <= 1e-6 * max(1.0, np.abs(J[:, j]).max())


def _poses(prob, PrTrue):
    """board in camera c for every camera and view, from the truth"""
    T = ry.rigTransforms(prob, PrTrue)
    W0 = ry.parametersToPoses(PrTrue[ry.numRig(prob):])
    return T, W0, np.einsum("cij,mjk->cmik", T, W0)


def test_start_points_follow_a_chain_of_shared_views():
    prob, PrTrue = ry.makeRig(3, 5)
    T, W0, W = _poses(prob, PrTrue)
    # camera 2 shares views with camera 1 only (3, 4); view 4 is seen by camera 2 alone
    ok = np.array([[1, 1, 1, 0, 0], [0, 1, 1, 1, 0], [0, 0, 0, 1, 1]], dtype=bool)
    W = np.where(ok[:, :, None, None], W, np.nan)                  # an unsolved pose is never read
    Ts, Ws = rig.rigStartPoints(W, ok)
    print(f"chain: |T - truth| {np.abs(Ts - T).max():.3e}, |W0 - truth| {np.abs(Ws - W0).max():.3e}")
    assert np.array_equal(Ts[0], np.eye(4))
    assert np.abs(Ts - T).max() <= 1e-12 and np.abs(Ws - W0).max() <= 1e-12
    # the edge is an average over the shared views: off by +d in one and -d in the other gives the truth's translation
    Wn = np.where(ok[:, :, None, None], np.einsum("cij,mjk->cmik", T, W0), 0.0)
    Wn[1, 1, :3, 3] += 0.01
    Wn[1, 2, :3, 3] -= 0.01
    Ts, _ = rig.rigStartPoints(Wn, ok)
    assert np.abs(Ts[1] - T[1]).max() <= 1e-12
    # breadth first, neighbours in index order: with every pair sharing a view, every camera hangs off camera 0
    full = np.ones((3, 5), dtype=bool)
    Wf = np.einsum("cij,mjk->cmik", T, W0)
    Wf[1, :, :3, 3] += 0.02                                        # camera 1's poses are off: through it camera 2 would be too
    Ts, Ws = rig.rigStartPoints(Wf, full)
    assert np.abs(Ts[2] - T[2]).max() <= 1e-12 and np.abs(Ts[1] - T[1]).max() > 1e-3
    assert np.abs(Ws - W0).max() <= 1e-12                          # poses from the lowest-indexed camera: camera 0


def test_start_points_name_what_is_missing():
    prob, PrTrue = ry.makeRig(4, 4)
    T, W0, W = _poses(prob, PrTrue)
    ok = np.array([[1, 1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 1], [0, 0, 0, 1]], dtype=bool)
    with pytest.raises(ValueError, match="camera 2"):
        rig.rigStartPoints(W, ok)
    ok = np.array([[1, 1, 0, 0], [1, 0, 0, 1], [0, 1, 0, 1], [0, 0, 0, 1]], dtype=bool)
    with pytest.raises(ValueError, match="view 2"):
        rig.rigStartPoints(W, ok)
    with pytest.raises(ValueError, match="N,M,4,4"):
        rig.rigStartPoints(W[0], ok)


def test_result_composes_transforms_and_names_its_parameters():
    prob, PrTrue = ry.makeRig(4, 3, counts=[(6, 0, 6), (6, 6, 0), (0, 6, 6), (0, 0, 0)])
    res = rig.RigCalibration(1.5, PrTrue, 3, np.zeros((3, 5 + 18)), [1.0, 0.5, 0.25, 0.0], ry.engineCameras(prob), 0)
    T = ry.rigTransforms(prob, PrTrue)
    assert res.T.shape == (4, 4, 4) and np.array_equal(res.T[0], np.eye(4)) and np.abs(res.T - T).max() <= 1e-15
    assert len(res.W) == 3 and res.sse == 1.75 and res.sseBeforeLastUpdate == 1.5 and res.iters == 3
    assert list(res.numPoints) == [12, 12, 12, 0]
    assert np.allclose(res.rms[:3], np.sqrt(np.array([1.0, 0.5, 0.25]) / 12), rtol=1e-15) and np.isnan(res.rms[3])
    X = np.array([0.3, -0.2, 1.1, 1.0])
    for a in range(4):
        for b in range(4):
            Tab = res.transform(a, b)
            assert np.abs(Tab @ (T[a] @ X) - T[b] @ X).max() <= 1e-14
            assert np.abs(Tab @ res.transform(b, a) - np.eye(4)).max() <= 1e-14
    assert np.abs(res.transform(0, 2) - T[2]).max() <= 1e-15
    names = res.parameterNames()
    assert len(names) == 18 and names[0] == "rig1.rx" and names[5] == "rig1.tz" and names[-1] == "rig3.tz"
    cams = res.cameras()
    assert [c[0] for c in cams] == ["radtan", "fisheye", "radtan", "fisheye"]
    assert np.array_equal(cams[1][1], ry.cameraOf(1, "fisheye")[0])
    with pytest.raises(ValueError, match="camera 0"):
        res.rigCovariance(0)


def test_header_declares_and_library_exports_the_rig_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "calib_lm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(calib_[a-z0-9_]+)\s*\(", text))
    lib = nat.loadLibrary()
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in include/calib_lm.h"
        assert n in nat.SIGNATURES, f"{n} has no ctypes signature"
        assert hasattr(lib, n), f"{n} is not exported by the library"
    assert "CALIB_RIG_MAX_CAMERAS 8" in text and nat.RIG_MAX_CAMERAS == 8
    assert lib.calib_version() >= 470
    for n in ("rigNormalEquations", "rigStepDelta", "refineRig"):
        assert hasattr(engine, n)
    for n in ("rigCalibrate", "calibrateRig", "RigCalibration", "rigStartPoints"):
        assert hasattr(cca, n)
    for n in ("transform", "covariance", "rigCovariance", "parameterNames", "rectify", "triangulate"):
        assert hasattr(cca.RigCalibration, n)
    assert stereo.rigStartPoint is cca.stereo.rigStartPoint        # the two-camera start point stays what it was


def _cProblem(prob, cameras=None, **over):
    """the C struct of a yardstick problem; cameras: {index: {field: value}} replaces fields of single cameras (a numpy
    array is passed as its pointer, None as NULL), over replaces fields of the problem"""
    N = ry.numCameras(prob)
    arr = (nat.RigCamera * N)()
    keep = [arr]
    for c in range(N):
        f = {"model": prob["models"][c], "offs": prob["offs"][c], "uv": prob["uv"][c], "xyz": prob["xyz"][c],
             "shared": prob["shared"][c]}
        f.update((cameras or {}).get(c, {}))
        keep.append(f)
        arr[c] = nat.RigCamera(f["model"], None if f["offs"] is None else nat.i64ptr(f["offs"]),
                               *(None if f[k] is None else nat.dptr(np.ascontiguousarray(f[k])) for k in ("uv", "xyz", "shared")))
    f = dict(num_cameras=N, num_views=ry.numViews(prob), cameras=arr)
    f.update(over)
    return nat.RigProblem(**f), keep


def test_argument_checks_return_invalid_before_any_device_call():
    """On a machine without a GPU a device call would give CALIB_E_HIP: CALIB_E_INVALID shows the check came first."""
    lib = nat.loadLibrary()
    prob, PrTrue = ry.makeRig(3, 3, counts=[(5, 6, 7), (7, 6, 5), (4, 0, 9)])
    Pr = np.ascontiguousarray(PrTrue)
    K = Pr.shape[0]

    def calls(p, iters=5, P=Pr):
        out = np.empty(K)
        sse, it = ctypes.c_double(), ctypes.c_int()
        ptr = None if p is None else ctypes.byref(p)
        inout = None if P is None else nat.dptr(P.copy())
        return (lib.calib_rig_normal_eq(ptr, None if P is None else nat.dptr(P), None, None, None, nat.dptr(out), None, 0),
                lib.calib_rig_step_delta(ptr, None if P is None else nat.dptr(P), 1e-3, nat.dptr(out), 0),
                lib.calib_refine_rig(ptr, inout, iters, 1e-3, 1e-10, 1e10, 1e-12, ctypes.byref(sse), None, ctypes.byref(it),
                                     None, 0))
    i64 = lambda *v: np.array(v, dtype=np.int64)                                   # noqa: E731
    good, keepGood = _cProblem(prob)
    bad = [
        _cProblem(prob, num_cameras=1), _cProblem(prob, num_cameras=0), _cProblem(prob, num_cameras=9),   # N outside [2, 8]
        _cProblem(prob, num_cameras=-3),
        _cProblem(prob, {0: {"model": 2}}), _cProblem(prob, {2: {"model": -1}}),     # bad model id
        _cProblem(prob, num_views=0), _cProblem(prob, num_views=-1),
        _cProblem(prob, {1: {"offs": i64(0, 7, 6, 18)}}),                            # decreases
        _cProblem(prob, {2: {"offs": i64(0, 4, 4, 3)}}),
        _cProblem(prob, {0: {"offs": i64(1, 5, 11, 18)}}),                           # does not start at 0
        _cProblem(prob, {2: {"offs": i64(-2, 4, 4, 13)}}),
        _cProblem(prob, {1: {"offs": None}}), _cProblem(prob, {0: {"uv": None}}),    # NULL inputs
        _cProblem(prob, {2: {"xyz": None}}), _cProblem(prob, {1: {"shared": None}}),
        _cProblem(prob, cameras=None),
    ]
    bad[-1][0].cameras = ctypes.POINTER(nat.RigCamera)()                            # NULL camera array
    for n, (p, k) in enumerate(bad):
        assert calls(p) == (nat.E_INVALID,) * 3, f"bad problem {n}"
    assert calls(good, P=None) == (nat.E_INVALID,) * 3                              # NULL Pr
    assert calls(None) == (nat.E_INVALID,) * 3                                      # NULL problem
    assert calls(good, iters=0)[2] == nat.E_INVALID and calls(good, iters=-3)[2] == nat.E_INVALID
    # a good call gets past the checks: without a device it is CALIB_E_HIP, with one it succeeds
    assert calls(good)[1] in (0, nat.E_HIP)
    cams = ry.engineCameras(prob)
    with pytest.raises(ValueError, match="2 to 8"):
        engine.rigStepDelta(cams[:1], Pr[12:], 1e-3)
    with pytest.raises(ValueError, match="shape"):
        engine.rigStepDelta(cams, Pr[:-1], 1e-3)
    with pytest.raises(ValueError, match="views"):
        engine.rigNormalEquations(cams[:2] + ((cams[2][0], cams[2][1], cams[2][2][:-1], cams[2][3][:4], cams[2][4][:4]),), Pr)
    with pytest.raises(ValueError):
        engine.refineRig(cams, Pr, 0)


def test_noisy_problem_leaves_eight_decided_iterations_on_the_yardstick():
    """The GPU noisy-loop test compares the trace up to the first iteration whose accept margin is below 1e-12 err on the
    yardstick (ry.decidedRows). That the chosen problem leaves at least 8 such rows is a property of the yardstick
    alone, asserted here so that the GPU test cannot pass by comparing nothing."""
    prob, PrTrue, Pr0, (sseY, PrY, traceY) = ry.noisyCase()
    n = ry.decidedRows(traceY)
    margin = np.abs(traceY[:, 2] - traceY[:, 1]) / traceY[:, 1]
    print(f"noisy case: {len(traceY)} yardstick iterations, {n} with decided lambda; margins {margin[:n]}")
    assert n >= 8
    assert (margin[:n - 1] > 1e-12).all()
    assert traceY.shape[1] == 5 + 12 and traceY[0, 3] == ry.NOISY_LAMBDA
    assert np.abs(PrY[:12] - PrTrue[:12]).max() < 0.5                # it converges to the truth's neighbourhood
