"""Robust losses on the rig solvers, the parts that need no GPU: the yardstick's dense and block routes against each
other on the cases the GPU tests use, rho' against differences of rho, Huber's continuity, the loss-spec parser, the
argument checks that come before any device call, the Python surface, and -- on the yardstick alone -- the condition that
makes the GPU loop test mean something: on the outlier case a robust loop ends near the fit of the clean data while the
plain loop does not."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import rig_joint_yardstick as qy
import rig_robust_yardstick as rb
import rig_yardstick as ry
from camera_calibration_amd import _native as nat
from camera_calibration_amd import engine, rig
from conftest import ROOT

NEW_SYMBOLS = ("calib_rig_robust_normal_eq", "calib_rig_robust_step_delta", "calib_refine_rig_robust", "calib_rig_residuals")
BLOCK_LOSSES = (("huber", 9.0), ("cauchy", 9.0))


def relMax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("loss", BLOCK_LOSSES, ids=lambda l: l[0])
@pytest.mark.parametrize("key", [2, 3, "8r"])
def test_yardstick_block_route_against_its_dense_route(key, loss):
    """B, E, V, g of the weighted blocks against J_w^T J_w and J_w^T r_w of the weighted dense problem, and the step
    through the Schur complement against the dense solve, masked and not: 1e-11. At delta = 9 px between a quarter and
    three quarters of the points lie above delta, so both branches of a loss weigh in."""
    prob, counts, Pq, _ = qy.blocksCase(key)
    S = qy.layout(prob)[0]
    above = np.concatenate(rb.squares(prob, Pq)) > loss[1] ** 2
    nb = rb.normalBlocks(prob, Pq, loss)
    sw = rb.rowWeights(prob, Pq, loss)
    J = qy.jacobianDense(prob, Pq) * sw[:, None]
    r = qy.residualVector(prob, Pq) * sw
    JTJ, g = J.T @ J, J.T @ r
    M = qy.M_BLOCKS
    worst = {"B": relMax(nb["B"], JTJ[:S, :S]), "g": relMax(nb["g"], g),
             "E": max(relMax(nb["E"][i], JTJ[:S, S + 6 * i:S + 6 * i + 6]) for i in range(M)),
             "V": max(relMax(nb["V"][i], JTJ[S + 6 * i:S + 6 * i + 6, S + 6 * i:S + 6 * i + 6]) for i in range(M))}
    mask = qy.rigMask(prob, 1) | qy.cameraMask(prob, [0])
    steps = {}
    for m in (0, mask):
        d, ref = rb.stepBlocks(prob, Pq, 1e-3, loss, m), rb.stepDense(prob, Pq, 1e-3, loss, m)
        steps[m] = np.linalg.norm(d - ref) / np.linalg.norm(ref)
    costs = np.abs(nb["costCam"] - rb.costCam(prob, Pq, loss)).max()
    print(f"{key} {loss}: {above.mean():.3f} of the points above delta (median |r| {np.sqrt(np.median(np.concatenate(rb.squares(prob, Pq)))):.2f} px); "
          f"blocks vs dense {worst}; steps {steps}")
    assert 0.25 <= above.mean() <= 0.75
    assert max(worst.values()) <= 1e-11 and max(steps.values()) <= 1e-11 and costs == 0.0
    assert np.isclose(rb.cost(prob, Pq, loss), nb["costCam"].sum(), rtol=1e-14)


def test_no_loss_is_the_plain_yardstick():
    prob, counts, Pq, ref = qy.blocksCase(3)
    nb = rb.normalBlocks(prob, Pq, None)
    for k in ("B", "E", "V", "g"):
        assert np.array_equal(nb[k], ref[k])
    assert np.allclose(nb["costCam"], ref["sseCam"], rtol=1e-14, atol=0)      # per point first, then the points: another order
    assert np.array_equal(rb.stepDense(prob, Pq, 1e-3, None), qy.stepDense(prob, Pq, 1e-3))
    huge = rb.normalBlocks(prob, Pq, ("huber", 1e150))             # a weight of exactly 1
    assert all(np.array_equal(huge[k], ref[k]) for k in ("B", "E", "V", "g"))


@pytest.mark.parametrize("loss", [("huber", 1.0), ("huber", 9.0), ("cauchy", 1.0), ("cauchy", 9.0)])
def test_weight_is_the_derivative_of_rho(loss):
    """central difference of rho at step h = 1e-5 s: truncation h^2 |rho'''| / 6 <= 1e-10 relative (|rho'''| s^2 <= a few
    rho' for both losses), rounding eps rho / h ~ 1e-11 relative. Bar 1e-8 relative; no s within h of Huber's kink."""
    d2 = loss[1] ** 2
    s = np.concatenate((np.geomspace(1e-4, 0.98, 40), np.geomspace(1.02, 1e5, 60))) * d2
    h = 1e-5 * s
    fd = (rb.rho(loss, s + h) - rb.rho(loss, s - h)) / (2 * h)
    w = rb.weight(loss, s)
    rel = np.abs(fd / w - 1).max()
    print(f"{loss}: rho' vs central difference, relative {rel:.3e}")
    assert rel <= 1e-8
    assert np.array_equal(engine.lossWeight(loss, s), w) and np.array_equal(engine.lossRho(loss, s), rb.rho(loss, s))
    assert (w > 0).all() and (w <= 1).all() and (np.diff(w) <= 0).all()      # a loss never weighs up, never more with distance


def test_huber_is_continuous_at_the_threshold_and_both_are_plain_near_zero():
    for d in (0.5, 1.0, 9.0):
        loss, s0 = ("huber", d), d * d
        below, above = np.nextafter(s0, 0.0), np.nextafter(s0, np.inf)
        for f in (rb.rho, rb.weight):
            at, lo, hi = float(f(loss, s0)), float(f(loss, below)), float(f(loss, above))
            assert abs(lo - at) <= 4 * np.finfo(float).eps * abs(at) and abs(hi - at) <= 4 * np.finfo(float).eps * abs(at)
        assert float(rb.rho(loss, s0)) == s0 and float(rb.weight(loss, s0)) == 1.0
        assert float(rb.rho(loss, 0.0)) == 0.0 and float(rb.weight(loss, 0.0)) == 1.0
        c = ("cauchy", d)
        assert float(rb.rho(c, 0.0)) == 0.0 and float(rb.weight(c, 0.0)) == 1.0
        tiny = 1e-12 * s0
        assert abs(float(rb.rho(c, tiny)) / tiny - 1) <= 1e-11


def test_loss_spec_parser():
    assert engine.parseLoss(None) is None
    assert engine.parseLoss("huber") == ("huber", 1.0) and engine.parseLoss("cauchy") == ("cauchy", 1.0)
    assert engine.parseLoss(("cauchy", 2)) == ("cauchy", 2.0) and engine.parseLoss(["huber", np.float64(0.5)]) == ("huber", 0.5)
    assert engine.parseLoss(engine.parseLoss(("huber", 3.0))) == ("huber", 3.0)
    for bad in ("tukey", "", "Huber", 1.0, ("huber",), ("huber", 1.0, 2.0), ("huber", 0.0), ("huber", -1.0),
                ("cauchy", float("nan")), ("cauchy", float("inf")), ("huber", "1"), ("huber", None), ("huber", True),
                (1, 1.0), {"huber": 1.0}):
        with pytest.raises(ValueError, match="loss"):
            engine.parseLoss(bad)
    cams = [("radtan", np.eye(3), np.zeros(5))] * 2
    with pytest.raises(ValueError, match="loss"):
        rig.rigCalibrate([[None], [None]], cams, loss="tukey")
    with pytest.raises(ValueError, match="loss"):
        rig.rigCalibrate([[None], [None]], cams, loss=("huber", 0.0))
    with pytest.raises(ValueError, match="refineCameras"):         # a loss alone does not free the cameras
        rig.rigCalibrate([[None], [None]], cams, loss="huber", fixedRigs=(1,))


def test_header_declares_and_library_exports_the_entry_points():
    raw = open(os.path.join(ROOT, "include", "calib_lm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(calib_[a-z0-9_]+)\s*\(", text))
    lib = nat.loadLibrary()
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in include/calib_lm.h"
        assert n in nat.SIGNATURES, f"{n} has no ctypes signature"
        assert hasattr(lib, n), f"{n} is not exported by the library"
    assert lib.calib_version() >= 500
    for name, value in (("CALIB_LOSS_NONE", nat.LOSS_NONE), ("CALIB_LOSS_HUBER", nat.LOSS_HUBER), ("CALIB_LOSS_CAUCHY", nat.LOSS_CAUCHY)):
        assert re.search(rf"#define {name} {value}\b", text)
    assert "calib_loss_t" in text and ctypes.sizeof(nat.Loss) == 16 and nat.Loss.scale.offset == 8
    for n in ("rigRobustNormalEquations", "rigRobustStepDelta", "refineRigRobust", "rigResiduals", "parseLoss"):
        assert hasattr(engine, n)
    assert "rigRobust" in engine._SOLVERS
    import camera_calibration_amd as cca
    assert inspect.signature(cca.rigCalibrate).parameters["loss"].default is None
    assert inspect.signature(cca.calibrateRig).parameters["loss"].default is None
    assert "loss" not in inspect.signature(cca.stereoCalibrate).parameters      # two cameras go through rigCalibrate
    for n in ("residuals", "weights", "covariance"):
        assert hasattr(cca.RigCalibration, n)


def _cProblem(prob):
    N = ry.numCameras(prob)
    arr = (nat.RigCamera * N)()
    keep = [arr]
    for c in range(N):
        o, uv, xyz = (np.ascontiguousarray(prob[k][c]) for k in ("offs", "uv", "xyz"))
        keep += [o, uv, xyz]
        arr[c] = nat.RigCamera(prob["models"][c], nat.i64ptr(o), nat.dptr(uv), nat.dptr(xyz), None)
    return nat.RigProblem(N, ry.numViews(prob), arr), keep


def test_argument_checks_return_invalid_before_any_device_call():
    """On a machine without a GPU a device call would give CALIB_E_HIP: CALIB_E_INVALID shows the check came first."""
    lib = nat.loadLibrary()
    prob, Pr = ry.makeRig(3, 3, ["radtan", "fisheye", "radtan"], [(5, 6, 7), (7, 6, 5), (6, 6, 6)])
    Pq = np.ascontiguousarray(qy.join(prob, Pr))
    K = Pq.shape[0]
    p, keep = _cProblem(prob)

    def calls(loss, mask=None, iters=5, P=Pq, problem=p):
        out = np.empty(K)
        cost, it = ctypes.c_double(), ctypes.c_int()
        lp = None if loss is None else ctypes.byref(nat.Loss(*loss))
        Pp = None if P is None else nat.dptr(P)
        return (lib.calib_rig_robust_normal_eq(ctypes.byref(problem), Pp, lp, None, None, None, nat.dptr(out), None, 0),
                lib.calib_rig_robust_step_delta(ctypes.byref(problem), Pp, mask, lp, 1e-3, nat.dptr(out), 0),
                lib.calib_refine_rig_robust(ctypes.byref(problem), None if P is None else nat.dptr(P.copy()), mask, lp, iters,
                                            1e-3, 1e-10, 1e10, 1e-12, ctypes.byref(cost), None, ctypes.byref(it), None, 0))
    for bad in ((7, 1.0), (-1, 1.0), (3, 1.0), (nat.LOSS_HUBER, 0.0), (nat.LOSS_HUBER, -1.0), (nat.LOSS_CAUCHY, float("nan")),
                (nat.LOSS_CAUCHY, float("inf")), (nat.LOSS_HUBER, -float("inf"))):
        assert calls(bad) == (nat.E_INVALID,) * 3, bad
    for loss in ((nat.LOSS_HUBER, 1.0), (nat.LOSS_CAUCHY, 2.5), (nat.LOSS_NONE, 1.0), (nat.LOSS_NONE, float("nan")), None):
        # what the joint rig entry points reject, under a loss, under none and delegated
        assert calls(loss, P=None) == (nat.E_INVALID,) * 3
        assert calls(loss, iters=0)[2] == nat.E_INVALID
        assert calls(loss, mask=(ctypes.c_uint64 * 2)(0, 1 << 40))[1:] == (nat.E_INVALID,) * 2      # a bit at or above S = 41
        assert calls(loss, problem=nat.RigProblem(3, 0, p.cameras)) == (nat.E_INVALID,) * 3
        assert calls(loss)[1] in (0, nat.E_HIP)                    # a good call gets past the checks
    res = np.empty((sum(int(o[-1]) for o in prob["offs"]), 2))
    assert lib.calib_rig_residuals(ctypes.byref(p), None, nat.dptr(res), 0) == nat.E_INVALID
    assert lib.calib_rig_residuals(ctypes.byref(p), nat.dptr(Pq), None, 0) == nat.E_INVALID
    assert lib.calib_rig_residuals(ctypes.byref(nat.RigProblem(9, 3, p.cameras)), nat.dptr(Pq), nat.dptr(res), 0) == nat.E_INVALID
    assert lib.calib_rig_residuals(ctypes.byref(p), nat.dptr(Pq), nat.dptr(res), 0) in (0, nat.E_HIP)
    cams = qy.engineCameras(prob)
    with pytest.raises(ValueError, match="loss"):
        engine.refineRigRobust(cams, Pq, 5, "tukey")
    with pytest.raises(ValueError, match="loss"):
        engine.rigRobustStepDelta(cams, Pq, 1e-3, ("huber", -1.0))
    with pytest.raises(ValueError, match="loss"):
        engine.rigRobustNormalEquations(cams, Pq, ("cauchy", float("inf")))
    with pytest.raises(ValueError, match="shape"):
        engine.rigResiduals(cams, Pq[:-1])
    with pytest.raises(ValueError, match="mask"):
        engine.rigRobustStepDelta(cams, Pq, 1e-3, "huber", fixedMask=1 << 41)


def test_outlier_case_is_what_it_says():
    oc = rb.outlierCase()
    for c, (flag, u, u0) in enumerate(zip(oc["displaced"], oc["prob"]["uv"], oc["clean"]["uv"])):
        moved = np.linalg.norm(u - u0, axis=1)
        assert flag.sum() == max(1, round(0.05 * flag.size)) and (moved[~flag] == 0).all()
        assert (moved[flag] >= 15 - 1e-9).all() and (moved[flag] <= 40 + 1e-9).all()
    again = rb.outlierCase()
    assert again is oc


@pytest.mark.parametrize("joint", [False, True], ids=["rig-only", "joint"])
def test_robust_loop_ends_near_the_clean_fit_and_the_plain_one_does_not(joint):
    """The outlier case at delta = 1 px, one plain loop and one robust loop from its result, in the yardstick: the robust
    result's largest rig error is at most 3 x that of the plain fit of the problem WITHOUT outliers, the plain fit WITH
    them at least 10 x. Measured with OUTLIER_SEED = 23: rig-only 1.07 x (Huber), 0.79 x (Cauchy) and 21.6 x; joint
    1.11 x, 1.28 x and 54.2 x. The robust traces leave at least five decided rows for the GPU test to follow."""
    oc, run = rb.outlierCase(), rb.outlierLoops(joint)
    prob, PqTrue = oc["prob"], oc["PqTrue"]
    clean = rb.rigError(prob, run["clean"][1], PqTrue)
    plain = rb.rigError(prob, run["plain"][1], PqTrue)
    print(f"{'joint' if joint else 'rig-only'}: largest rig error, clean data {clean:.4f}, plain fit with outliers {plain:.4f} "
          f"({plain / clean:.1f} x)")
    assert plain >= 10 * clean
    for loss, (cost, Pq, trace) in run["robust"].items():
        err, n = rb.rigError(prob, Pq, PqTrue), ry.decidedRows(trace)
        print(f"  {loss}: {err:.4f} ({err / clean:.2f} x), {len(trace)} iterations, decided rows {n}, accepted {trace[:, 4]}")
        assert err <= 3 * clean
        assert n >= 5
        assert cost == trace[-1, 1] and (np.diff(trace[:, 1]) <= 0).all()     # sum rho never grows


def test_weights_single_out_the_displaced_corners():
    """What the public-surface GPU test asserts of weights(), on the yardstick alone: below 0.5 on at least 90 % of the
    displaced corners, above 0.5 on at least 90 % of the others, at the joint robust results."""
    oc, run = rb.outlierCase(), rb.outlierLoops(True)
    flag = np.concatenate(oc["displaced"])
    for loss, (_, Pq, _) in run["robust"].items():
        w = np.concatenate(rb.weights(oc["prob"], Pq, loss))
        low, high = (w[flag] < 0.5).mean(), (w[~flag] > 0.5).mean()
        print(f"{loss}: weight < 0.5 on {low:.3f} of the displaced corners, > 0.5 on {high:.3f} of the others")
        assert low >= 0.9 and high >= 0.9
