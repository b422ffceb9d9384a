"""Joint rig calibration, the parts that need no GPU: the yardstick's joint Jacobian against finite differences of its own
residual, N = 2 against the joint stereo yardstick, all camera bits fixed against the rig-only yardstick, its block route
against its dense route on the cases the GPU tests use, its two loops, the exported symbols and the Python surface, the
argument checks that come before any device call, and the resolution of names, masks and fixedRigs."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import rig_joint_yardstick as qy
import rig_yardstick as ry
import stereo_joint_yardstick as jy
from camera_calibration_amd import _native as nat
from camera_calibration_amd import engine, rig
from conftest import ROOT

NEW_SYMBOLS = ("calib_rig_joint_normal_eq", "calib_rig_joint_step_delta", "calib_refine_rig_joint")


def _stencil(f, x, j, h):
    """fourth-order central difference of f along coordinate j"""
    def at(s):
        y = x.copy()
        y[j] += s * h
        return f(y)
    return (-at(2) + 8 * at(1) - 8 * at(-1) + at(-2)) / (12 * h)


def test_yardstick_joint_jacobian_against_fourth_order_differences_of_its_own_residual():
    """N = 3 (radtan, fisheye, radtan), M = 3, ragged counts, by test_stereo_joint_cpu.py's rule. Per column: the stencil
    at steps h and 2 h differ by the stencil's truncation error, and its four evaluations, each rounded to eps |f|, weigh
    18 / (12 h) in all: its own error is the sum of the two; the bar is ten times that. Steps: 1e-3 relative for the
    focal lengths and the principal point, 1e-3 absolute for the skew and the distortion coefficients, 2e-2 degrees,
    1e-3 metres."""
    prob, Pr = ry.makeRig(3, 3, ["radtan", "fisheye", "radtan"], [(20, 0, 11), (9, 14, 17), (12, 8, 0)])
    S, off, L = qy.layout(prob)
    Pq = qy.join(prob, Pr)
    J = qy.jacobianDense(prob, Pq)
    assert S == 10 + 15 + 16 and J.shape == (2 * (31 + 40 + 20), S + 18)
    names = rig.jointParameterNames(prob["models"])

    def f(p):
        return -qy.residualVector(prob, p)               # the projection, up to the constant sensor points

    def step(j):
        if j < S:
            n = names[j].split(".")[1]
            if n in ("alpha", "beta", "uc", "vc"):
                return 1e-3 * abs(Pq[j])
            return 2e-2 if n in ("rx", "ry", "rz") else 1e-3
        return 2e-2 if ((j - S) % 6) < 3 else 1e-3
    worstRatio, fmax = 0.0, max(np.abs(uv).max() for uv in prob["uv"])
    for j in range(Pq.shape[0]):
        h = step(j)
        d1, d2 = _stencil(f, Pq, j, h), _stencil(f, Pq, j, 2 * h)
        own = np.abs(d1 - d2).max() + 1.5 * np.finfo(float).eps * fmax / h
        got = np.abs(J[:, j] - d1).max()
        print(f"column {j:2d} {names[j] if j < S else 'pose':>10s}: |J| max {np.abs(J[:, j]).max():.3e}  stencil's own error "
              f"{own:.3e}  bar {10 * own:.3e}  analytic - stencil {got:.3e}")
        assert np.abs(J[:, j]).max() > 0
        assert got <= 10 * own, (j, got, own)
        worstRatio = max(worstRatio, got / own)
    print(f"worst (analytic - stencil) / (stencil's own error): {worstRatio:.3f}")
    # no row touches two cameras
    r = 0
    for c in range(3):
        n2 = 2 * prob["xyz"][c].shape[0]
        w = L[c] + (6 if c else 0)
        other = np.ones(S, dtype=bool)
        other[off[c]:off[c] + w] = False
        assert not J[r:r + n2, :S][:, other].any()
        r += n2


def test_two_cameras_equal_the_joint_stereo_yardstick():
    """N = 2: Pq is Pj. Blocks, step (with and without a mask) and the trace of the dense loop within 1e-13."""
    prob, PrTrue = ry.makeRig(2, 6, ["radtan", "fisheye"], [(54, 30, 0, 54, 17, 54), (54, 54, 40, 0, 54, 9)], noiseSigma=0.3)
    Pq = qy.perturbedJoint(prob, PrTrue, 1.0, 0.03, 1.0, 0.01)
    sp = ry.asStereo(prob)
    a, b = qy.normalBlocks(prob, Pq), jy.normalBlocks(sp, Pq)
    worst = 0.0
    for k in ("B", "E", "V", "g"):
        worst = max(worst, np.abs(a[k] - b[k]).max() / np.abs(b[k]).max())
    worst = max(worst, abs(a["sseCam"][0] - b["sseA"]) / b["sseA"], abs(a["sseCam"][1] - b["sseB"]) / b["sseB"])
    print(f"N = 2 blocks vs the joint stereo yardstick: {worst:.3e}")
    assert worst <= 1e-13
    for mask in (0, 0b100 | 1 << 12 | 0x3f << 19):
        d, ref = qy.stepDense(prob, Pq, 1e-3, mask), jy.stepDense(sp, Pq, 1e-3, mask)
        rel = np.linalg.norm(d - ref) / np.linalg.norm(ref)
        print(f"N = 2 step, mask {mask:#x}: {rel:.3e}")
        assert rel <= 1e-13
    tq, tj = qy.refineDense(prob, Pq, 6)[2], jy.refineDense(sp, Pq, 6)[2]
    assert tq.shape == tj.shape and np.array_equal(tq[:, [0, 3, 4]], tj[:, [0, 3, 4]])
    rel = np.abs(tq - tj).max() / np.abs(tj).max()
    print(f"N = 2 trace of six iterations: {rel:.3e}")
    assert rel <= 1e-13


def test_all_camera_bits_fixed_is_the_rig_only_problem():
    prob, _, Pq, _ = qy.blocksCase(3)
    S = qy.layout(prob)[0]
    p, Pr = qy.split(prob, Pq)
    d = qy.stepDense(prob, Pq, 1e-3, qy.cameraMask(prob))
    ref = ry.stepDense(p, Pr, 1e-3)
    got = np.concatenate((d[qy.columnsOfPr(prob)], d[S:]))
    rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print(f"joint step with every camera fixed vs the rig-only dense step: {rel:.3e}")
    assert rel <= 1e-11
    assert not d[:S][[s for s in range(S) if qy.cameraMask(prob) >> s & 1]].any()


@pytest.mark.parametrize("key", [2, 3, 4, 8, "8r"])
def test_block_route_and_dense_route_of_the_yardstick_agree_on_the_blocks_cases(key):
    """M = 17, ragged counts, S up to 122: the bars of the GPU step tests (1e-9) stand on a yardstick whose two routes
    agree to 1e-11 at lambda = 1e-3 and 10"""
    prob, _, Pq, nb = qy.blocksCase(key)
    S, off, L = qy.layout(prob)
    J = qy.jacobianDense(prob, Pq)
    JTJ = J.T @ J
    assert np.abs(nb["B"] - JTJ[:S, :S]).max() <= 1e-12 * np.abs(JTJ[:S, :S]).max()
    assert np.abs(nb["g"] - J.T @ qy.residualVector(prob, Pq)).max() <= 1e-12 * np.abs(nb["g"]).max()
    for c in range(len(L)):
        w = L[c] + (6 if c else 0)
        assert not nb["B"][off[c]:off[c] + w, off[c] + w:].any()
    for lam in (1e-3, 10.0):
        d, b = qy.stepDense(prob, Pq, lam), qy.stepFromBlocks(nb, lam)
        rel = np.linalg.norm(d - b) / np.linalg.norm(d)
        print(f"{key}: S = {S}, cond {np.linalg.cond(JTJ):.2e}, lambda {lam}: |blocks - dense| / |dense| = {rel:.3e}")
        assert rel <= 1e-11


def test_block_route_and_dense_route_agree_on_the_size_and_mask_cases():
    """the other cases on which a GPU test compares a step: the M = 17 size case (the larger ones have no dense route)
    and the masks of the GPU mask tests on the N = 3 blocks case. (The loop tests compare no step: iterations, decisions
    and end points.)"""
    cases = [("sizes 17",) + qy.sizesCase(17) + (0,)]
    prob, _, Pq, _ = qy.blocksCase(3)
    cases += [("camera bits", prob, Pq, qy.cameraMask(prob)), ("rig 2", prob, Pq, qy.rigMask(prob, 2)),
              ("mixed", prob, Pq, MIXED_MASK(prob))]
    for name, prob, Pq, mask in cases:
        for lam in (1e-3, 10.0):
            d, b = qy.stepDense(prob, Pq, lam, mask), qy.stepBlocks(prob, Pq, lam, mask)
            rel = np.linalg.norm(d - b) / np.linalg.norm(d)
            print(f"{name}, mask {mask:#x}, lambda {lam}: |blocks - dense| / |dense| = {rel:.3e}")
            assert rel <= 1e-11


def MIXED_MASK(prob):
    """the mask of the GPU bit test: camera 0's skew, camera 1's last coefficient, camera 2's principal point, rig 1's tz"""
    _, off, L = qy.layout(prob)
    return 1 << 2 | 1 << (off[1] + L[1] - 1) | 0b11 << (off[2] + 3) | 1 << (off[1] + L[1] + 5)


def test_noise_free_loop_ends_by_the_stop_rule():
    prob, PqTrue, Pq0, (err, Pq, trace) = qy.noiseFreeCase()
    print(f"noise-free, N = 4, M = 20: {len(trace)} iterations, accepted {trace[:, 4]}, err {err:.3e}, "
          f"|Pq - truth| max {np.abs(Pq - PqTrue).max():.3e}")
    assert len(trace) < 50 and err < 1e-12 and trace[:, 4].all()
    assert np.abs(Pq - PqTrue).max() <= 1e-9


def test_noisy_loop_leaves_decided_rows():
    prob, _, Pq0, (err, Pq, trace) = qy.noisyCase()
    n = ry.decidedRows(trace)
    print(f"noisy, N = 3, M = 8: {len(trace)} iterations, lambda {trace[:, 3]}, accepted {trace[:, 4]}, decided rows {n}")
    assert n >= 6


def test_header_declares_and_library_exports_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "calib_lm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(calib_[a-z0-9_]+)\s*\(", text))
    lib = nat.loadLibrary()
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in include/calib_lm.h"
        assert n in nat.SIGNATURES, f"{n} has no ctypes signature"
        assert hasattr(lib, n), f"{n} is not exported by the library"
    assert lib.calib_version() >= 490
    for n in ("rigJointNormalEquations", "rigJointStepDelta", "refineRigJoint"):
        assert hasattr(engine, n)
    import camera_calibration_amd as cca
    sig = inspect.signature(cca.rigCalibrate).parameters
    assert sig["refineCameras"].default is False and sig["fixed"].default is None and sig["fixedRigs"].default == ()
    assert inspect.signature(cca.calibrateRig).parameters["joint"].default is False
    for n in ("covariance", "rigCovariance", "jointParameterNames", "cameras", "rectify", "triangulate", "triangulateAll"):
        assert hasattr(cca.RigCalibration, n)


def _cProblem(prob, numCameras=None, numViews=None, models=None, offs=None, nullCameras=False):
    """the C struct with every shared pointer NULL: the joint calls do not read them"""
    N = ry.numCameras(prob)
    arr = (nat.RigCamera * N)()
    keep = [arr]
    for c in range(N):
        o = np.ascontiguousarray((offs or {}).get(c, prob["offs"][c]), dtype=np.int64)
        uv, xyz = np.ascontiguousarray(prob["uv"][c]), np.ascontiguousarray(prob["xyz"][c])
        keep += [o, uv, xyz]
        arr[c] = nat.RigCamera((models or {}).get(c, prob["models"][c]), nat.i64ptr(o), nat.dptr(uv), nat.dptr(xyz), None)
    p = nat.RigProblem(N if numCameras is None else numCameras, ry.numViews(prob) if numViews is None else numViews,
                       None if nullCameras else arr)
    return p, keep


def test_argument_checks_return_invalid_before_any_device_call():
    """On a machine without a GPU a device call would give CALIB_E_HIP: CALIB_E_INVALID shows the check came first."""
    lib = nat.loadLibrary()
    prob, Pr = ry.makeRig(3, 3, ["radtan", "fisheye", "radtan"], [(5, 6, 7), (7, 6, 5), (6, 6, 6)])
    Pq = np.ascontiguousarray(qy.join(prob, Pr))
    K, S = Pq.shape[0], qy.layout(prob)[0]
    assert S == 41

    def words(mask):
        return (ctypes.c_uint64 * 2)(mask & (2 ** 64 - 1), mask >> 64)

    def calls(p, mask=0, iters=5, P=Pq):
        out = np.empty(K)
        sse, it = ctypes.c_double(), ctypes.c_int()
        inout = None if P is None else nat.dptr(P.copy())
        return (lib.calib_rig_joint_normal_eq(ctypes.byref(p), None if P is None else nat.dptr(P), None, None, None,
                                              nat.dptr(out), None, 0),
                lib.calib_rig_joint_step_delta(ctypes.byref(p), None if P is None else nat.dptr(P), words(mask), 1e-3,
                                               nat.dptr(out), 0),
                lib.calib_refine_rig_joint(ctypes.byref(p), inout, words(mask), iters, 1e-3, 1e-10, 1e10, 1e-12,
                                           ctypes.byref(sse), None, ctypes.byref(it), None, 0))
    good, keep = _cProblem(prob)
    bad = [
        _cProblem(prob, models={0: 2}), _cProblem(prob, models={2: -1}),                   # bad model id
        _cProblem(prob, offs={0: [0, 5, 4, 18]}), _cProblem(prob, offs={2: [0, 7, 13, 12]}),   # non-monotone
        _cProblem(prob, offs={1: [-2, 7, 13, 18]}),                                        # does not start at 0
        _cProblem(prob, numViews=0), _cProblem(prob, numCameras=1), _cProblem(prob, numCameras=9),
        _cProblem(prob, nullCameras=True),
    ]
    for p, k in bad:
        assert calls(p) == (nat.E_INVALID,) * 3
    assert calls(good, P=None) == (nat.E_INVALID,) * 3                                     # NULL Pq
    assert calls(good, iters=0)[2] == nat.E_INVALID and calls(good, iters=-3)[2] == nat.E_INVALID
    for mask in (1 << 41, 1 << 63, 1 << 64, 1 << 127, (1 << 128) - 1):                     # a bit at or above S
        assert calls(good, mask=mask)[1:] == (nat.E_INVALID,) * 2
    # a good call gets past the checks: without a device it is CALIB_E_HIP, with one it succeeds
    assert calls(good, mask=1 << 40)[1] in (0, nat.E_HIP)
    assert lib.calib_rig_joint_step_delta(ctypes.byref(good), nat.dptr(Pq), None, 1e-3, None, 0) in (0, nat.E_HIP)
    cams = qy.engineCameras(prob)
    with pytest.raises(ValueError):
        engine.refineRigJoint(cams, Pq, 0)
    with pytest.raises(ValueError, match="shape"):
        engine.rigJointStepDelta(cams, Pq[:-1], 1e-3)
    with pytest.raises(ValueError, match="mask"):
        engine.rigJointStepDelta(cams, Pq, 1e-3, fixedMask=1 << 41)
    with pytest.raises(ValueError, match="2 to 8"):
        engine.rigJointStepDelta(cams[:1], Pq, 1e-3)


def test_names_masks_and_fixed_rigs_resolve():
    R, F = nat.MODEL_RADTAN, nat.MODEL_FISHEYE
    names = rig.jointParameterNames([R, F, R])
    assert len(names) == 41 and names[0] == "cam0.alpha" and names[9] == "cam0.k3" and names[10] == "cam1.alpha"
    assert names[18] == "cam1.k4" and names[19:25] == ("rig1.rx", "rig1.ry", "rig1.rz", "rig1.tx", "rig1.ty", "rig1.tz")
    assert names[25] == "cam2.alpha" and names[34] == "cam2.k3" and names[35] == "rig2.rx" and names[40] == "rig2.tz"
    assert engine.rigJointLayout([R, F, R]) == (41, (0, 10, 25), (10, 9, 10))
    assert engine.rigJointLayout([R] * 8)[0] == 122
    assert rig.jointFixed([R, F, R]) == (0, {})
    mask, values = rig.jointFixed([R, F, R], ["skew", {"k4": 0.0, "focal": None}, None], (2,))
    assert mask == 0b100 | (0b11 | 1 << 8) << 10 | 0x3f << 35 and values == {10 + 8: 0.0}
    mask, values = rig.jointFixed([F, R], ["all", ["tangential"]], [1])
    assert mask == (1 << 9) - 1 | (0b11 << 7) << 9 | 0x3f << 19 and values == {}
    mask, values = rig.jointFixed([R] * 8, [None] * 7 + [{"uc": 320.0}], (7,))
    assert mask == 0b1000 << 106 | 0x3f << 116 and values == {109: 320.0} and mask >> 122 == 0
    with pytest.raises(ValueError, match="p1"):
        rig.jointFixed([R, F], [None, "p1"])                                               # the fisheye model has no p1
    with pytest.raises(ValueError, match="per camera"):
        rig.jointFixed([R, F], ["skew"])
    for badRig in (0, 2, -1, "1"):
        with pytest.raises(ValueError, match="no rig"):
            rig.jointFixed([R, F], None, (badRig,))
    cams = [("radtan", np.eye(3), np.zeros(5))] * 2
    with pytest.raises(ValueError, match="refineCameras"):
        rig.rigCalibrate([[None], [None]], cams, fixed=["skew", None])
    with pytest.raises(ValueError, match="refineCameras"):
        rig.rigCalibrate([[None], [None]], cams, fixedRigs=(1,))
    # Pq packs and unpacks camera-major
    shared = [np.arange(10.0), 100 + np.arange(9.0), 200 + np.arange(10.0)]
    Pr = 1000 + np.arange(12.0 + 18)
    Pq = rig.packJoint(shared, Pr)
    assert np.array_equal(Pq[:10], shared[0]) and np.array_equal(Pq[19:25], Pr[:6]) and np.array_equal(Pq[35:41], Pr[6:12])
    back, PrBack = rig.unpackJoint([R, F, R], Pq)
    assert all(np.array_equal(a, b) for a, b in zip(back, shared)) and np.array_equal(PrBack, Pr)
