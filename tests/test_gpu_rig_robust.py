"""Robust losses on the rig solvers on the device against tests/rig_robust_yardstick.py (numpy fp64 on the oracle's camera
model): the weighted blocks, a weight of exactly 1, one step with and without a mask, the sizes of the two reductions,
the loop on the outlier case, fixed bits, the residual kernel, delegation and errors, the public surface. Bars are those
of tests/test_gpu_rig_joint.py (blocks 1e-11 of the block's largest entry, per-camera sums 1e-12 relative, a solved step
1e-9 in relative 2-norm); every test prints what it measured. tests/test_rig_robust_cpu.py holds the yardstick's side.

Shapes are test_gpu_rig_joint.py's: 17 ragged views with 0 / 1 / 5 / 16 / 17 / 33 / 54 / 64 / 70 points per camera and view
(batch edges of 32 and 64, zero bands of E), N = 2, 3 and 8 radtan cameras (S = 122). At delta = 9 px about half of the
points of those cases lie above delta (median |r| 8.8 to 9.1 px): both branches of a loss weigh in."""
import ctypes

import numpy as np
import pytest

import camera_calibration_amd as cca
import rig_joint_yardstick as qy
import rig_robust_yardstick as rb
import rig_yardstick as ry
from camera_calibration_amd import _native as nat
from camera_calibration_amd import engine

pytestmark = pytest.mark.gpu

M_BLOCKS = qy.M_BLOCKS
BLOCK_LOSSES = (("huber", 9.0), ("cauchy", 9.0))
_cache = {}


def relMax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def widths(prob):
    S, off, L = qy.layout(prob)
    return S, off, L, [L[c] + (6 if c else 0) for c in range(len(L))]


def yardstickBlocks(key, loss):
    if ("blocks", key, loss) not in _cache:
        prob, counts, Pq, _ = qy.blocksCase(key)
        _cache["blocks", key, loss] = rb.normalBlocks(prob, Pq, loss)
    return _cache["blocks", key, loss]


@pytest.mark.parametrize("loss", BLOCK_LOSSES, ids=lambda l: l[0])
@pytest.mark.parametrize("key", [2, 3, "8r"])
def test_blocks_against_the_yardstick(key, loss):
    prob, counts, Pq, _ = qy.blocksCase(key)
    ref = yardstickBlocks(key, loss)
    S, off, L, W = widths(prob)
    N, M = len(L), M_BLOCKS
    above = (np.concatenate(rb.squares(prob, Pq)) > loss[1] ** 2).mean()
    ne = engine.rigRobustNormalEquations(qy.engineCameras(prob), Pq, loss)
    assert ne["B"].shape == (S, S) and ne["E"].shape == (M, S, 6) and ne["V"].shape == (M, 6, 6)
    assert ne["g"].shape == (S + 6 * M,) and ne["costCam"].shape == (N,)
    worst = {"B": 0.0, "g_shared": 0.0, "E": 0.0}
    offDiagonal = ne["B"].copy()
    for c in range(N):
        sl = slice(off[c], off[c] + W[c])
        worst["B"] = max(worst["B"], relMax(ne["B"][sl, sl], ref["B"][sl, sl]))
        worst["g_shared"] = max(worst["g_shared"], relMax(ne["g"][sl], ref["g"][sl]))
        offDiagonal[sl, sl] = 0.0
        for i in range(M):
            if counts[c][i]:
                worst["E"] = max(worst["E"], relMax(ne["E"][i, sl], ref["E"][i, sl]))
            else:                                                  # the camera missed the view: its band is exactly zero
                assert not ne["E"][i, sl].any() and not ref["E"][i, sl].any()
    worst["V"] = max(relMax(ne["V"][i], ref["V"][i]) for i in range(M))
    worst["g_view"] = max(relMax(ne["g"][S + 6 * i:S + 6 * i + 6], ref["g"][S + 6 * i:S + 6 * i + 6]) for i in range(M))
    cost = np.abs(ne["costCam"] - ref["costCam"]) / ref["costCam"]
    print(f"{key} {loss}: S = {S}, {above:.3f} of the points above delta; blocks vs yardstick, relative to each block's "
          f"largest entry: {worst}; costCam relative {cost}")
    assert 0.25 <= above <= 0.75                                   # both branches are exercised
    assert not offDiagonal.any() and np.array_equal(ne["B"], ne["B"].T)
    assert max(worst.values()) <= 1e-11
    assert cost.max() <= 1e-12


@pytest.mark.parametrize("key", [3, "8r"])
def test_a_weight_of_one_is_exact(key):
    """Huber with delta = 1e150: s <= delta^2 everywhere, w = 1, sqrt(w) = 1, and a product with 1.0 is exact"""
    prob, counts, Pq, _ = qy.blocksCase(key)
    cams = qy.engineCameras(prob)
    plain = engine.rigJointNormalEquations(cams, Pq)
    ne = engine.rigRobustNormalEquations(cams, Pq, ("huber", 1e150))
    cost = np.abs(ne["costCam"] - plain["sseCam"]) / plain["sseCam"]
    print(f"{key}: Huber at 1e150 px vs calib_rig_joint_normal_eq: bitwise {[np.array_equal(ne[k], plain[k]) for k in 'BEVg']}, "
          f"costCam vs sseCam relative {cost}")
    for k in "BEVg":
        assert ne[k].tobytes() == plain[k].tobytes()
    assert cost.max() <= 1e-12


def stepMask(prob):
    """one camera and one rig fixed"""
    return qy.cameraMask(prob, [1]) | qy.rigMask(prob, 2 if ry.numCameras(prob) > 2 else 1)


@pytest.mark.parametrize("loss", BLOCK_LOSSES, ids=lambda l: l[0])
@pytest.mark.parametrize("lam", [1e-3, 10.0])
@pytest.mark.parametrize("key", [3, "8r"])
def test_step_against_the_weighted_dense_solve(key, lam, loss):
    prob, counts, Pq, _ = qy.blocksCase(key)
    S = qy.layout(prob)[0]
    cams = qy.engineCameras(prob)
    for mask in (0, stepMask(prob)):
        ref = rb.stepDense(prob, Pq, lam, loss, mask)
        d = engine.rigRobustStepDelta(cams, Pq, lam, loss, mask)
        rel = np.linalg.norm(d - ref) / np.linalg.norm(ref)
        relShared = np.linalg.norm(d[:S] - ref[:S]) / np.linalg.norm(ref[:S])
        print(f"{key} {loss}, lambda {lam}, mask {mask:#x}: |delta - dense| / |dense| = {rel:.3e} (shared part {relShared:.3e})")
        assert rel <= 1e-9 and relShared <= 1e-9
        fixedIdx = [s for s in range(S) if mask >> s & 1]
        assert not d[fixedIdx].any() and d[[s for s in range(S) if s not in fixedIdx]].all()


@pytest.mark.parametrize("M", [1, 2, 257, 4099])
def test_sizes_of_the_two_reductions(M):
    """test_gpu_rig_joint.py's sizes under a loss: M = 1 and 2 with every camera bit fixed; 257 fills 129 and 65 partial
    rows; 4099 makes the waves loop over views and fills every partial row. The median |r| of these cases is 8.6 to 10 px:
    at delta = 9 px points lie on both sides. One step against the block-wise weighted Schur step; two calls are bitwise
    equal."""
    prob, Pq = qy.sizesCase(M)
    S = qy.layout(prob)[0]
    mask = qy.cameraMask(prob) if M <= 2 else 0
    cams = qy.engineCameras(prob)
    for loss in BLOCK_LOSSES:
        above = (np.concatenate(rb.squares(prob, Pq)) > loss[1] ** 2).mean()
        d1 = engine.rigRobustStepDelta(cams, Pq, 1e-3, loss, mask)
        d2 = engine.rigRobustStepDelta(cams, Pq, 1e-3, loss, mask)
        ref = rb.stepBlocks(prob, Pq, 1e-3, loss, mask)
        rel = np.linalg.norm(d1 - ref) / np.linalg.norm(ref)
        relShared = np.linalg.norm(d1[:S] - ref[:S]) / np.linalg.norm(ref[:S])
        print(f"M = {M} {loss}: {above:.3f} above delta; |delta - blockwise| / |blockwise| = {rel:.3e} (shared part {relShared:.3e})")
        assert 0.0 < above < 1.0
        assert np.array_equal(d1, d2)
        assert rel <= 1e-9 and relShared <= 1e-9
    n1, n2 = (engine.rigRobustNormalEquations(cams, Pq, ("cauchy", 9.0)) for _ in range(2))
    assert all(np.array_equal(n1[k], n2[k]) for k in n1)
    ref = rb.costCam(prob, Pq, ("cauchy", 9.0))
    assert (np.abs(n1["costCam"] - ref) <= 1e-12 * ref).all()
    r1, r2 = (engine.refineRigRobust(cams, Pq, 3, ("huber", 9.0), mask) for _ in range(2))
    assert r1[0] == r2[0] and np.array_equal(r1[1], r2[1]) and np.array_equal(r1[3], r2[3]) and np.array_equal(r1[4], r2[4])


@pytest.mark.parametrize("loss", rb.LOOP_LOSSES, ids=lambda l: l[0])
@pytest.mark.parametrize("joint", [False, True], ids=["rig-only", "joint"])
def test_loop_follows_the_yardstick(joint, loss):
    """the outlier case: from the yardstick's plain result, the robust loop of the device beside the yardstick's"""
    oc, run = rb.outlierCase(), rb.outlierLoops(joint)
    prob, PqTrue, mask = oc["prob"], oc["PqTrue"], run["mask"]
    S = qy.layout(prob)[0]
    costY, PqY, traceY = run["robust"][loss]
    cost, Pq, iters, trace, costCam = engine.refineRigRobust(qy.engineCameras(prob), run["plain"][1], 50, loss, mask)
    n = min(ry.decidedRows(traceY), iters)
    clean = rb.rigError(prob, run["clean"][1], PqTrue)
    err = rb.rigError(prob, Pq, PqTrue)
    print(f"{'joint' if joint else 'rig-only'} {loss}: iters {iters} (yardstick {len(traceY)}), decided rows {n}; lambda "
          f"{trace[:n, 3]}; max rel d cost(P) {np.abs(trace[:n, 1] / traceY[:n, 1] - 1).max():.3e}; cost {cost:.12e} "
          f"(yardstick {costY:.12e}); largest rig error {err:.4f} = {err / clean:.2f} x the clean fit's")
    assert n >= 5                                                  # test_rig_robust_cpu asserts the yardstick's side of this
    assert trace.shape == (iters, 5 + S)
    assert np.array_equal(trace[:n, 3], traceY[:n, 3])
    assert np.array_equal(trace[:n - 1, 4], traceY[:n - 1, 4])
    assert cost == trace[-1, 1]
    cY = rb.costCam(prob, Pq, loss)                                # the yardstick's sums of rho at the returned point
    print(f"costCam {costCam} vs the yardstick's at the returned point: {np.abs(costCam - cY) / cY}")
    assert (np.abs(costCam - cY) <= 1e-12 * cY).all()
    assert err <= 3 * clean
    fixedIdx = [s for s in range(S) if mask >> s & 1]
    assert Pq[fixedIdx].tobytes() == run["plain"][1][fixedIdx].tobytes()


def test_fixed_parameters_keep_their_bits():
    """eight radtan cameras, S = 122: a fixed -0.0 in mask word 0 and one in mask word 1 through accepted robust steps"""
    prob, counts, Pq, _ = qy.blocksCase("8r")
    S, off, L, W = widths(prob)
    mask = 1 << 2 | 1 << (off[6] + 2) | qy.rigMask(prob, 7) | 0b11 << (off[1] + 3)
    assert off[6] + 2 >= 64
    Pq0 = Pq.copy()
    Pq0[2] = -0.0                                                  # camera 0's skew
    Pq0[off[6] + 2] = -0.0                                         # camera 6's: mask word 1
    cost, P, iters, trace, _ = engine.refineRigRobust(qy.engineCameras(prob), Pq0, 6, ("huber", 9.0), mask)
    accepted = int(trace[:, 4].sum())
    fixedIdx = [s for s in range(S) if mask >> s & 1]
    print(f"{iters} iterations, {accepted} accepted; fixed {fixedIdx}: {P[fixedIdx]}")
    assert accepted >= 3
    assert P[fixedIdx].tobytes() == Pq0[fixedIdx].tobytes() and np.signbit(P[2]) and np.signbit(P[off[6] + 2])
    free = [s for s in range(S) if s not in fixedIdx]
    assert (P[free] != Pq0[free]).all()
    for row in trace:
        assert row[5:][fixedIdx].tobytes() == Pq0[fixedIdx].tobytes()


def test_residuals_against_the_yardstick():
    prob, counts, Pq, _ = qy.blocksCase(3)
    cams = qy.engineCameras(prob)
    res = engine.rigResiduals(cams, Pq)
    ref = rb.residuals(prob, Pq)
    worst = max(np.abs(a - b).max() for a, b in zip(res, ref))
    sse = np.array([float(np.sum(r * r)) for r in res])
    plain = engine.rigJointNormalEquations(cams, Pq)["sseCam"]
    print(f"residuals vs the yardstick: {worst:.3e} px; per-camera sum of squares vs sseCam: {np.abs(sse - plain) / plain}")
    assert [r.shape for r in res] == [(int(o[-1]), 2) for o in prob["offs"]]
    assert worst <= 1e-9
    assert (np.abs(sse - plain) <= 1e-12 * plain).all()
    # a camera that missed a view contributes no rows: camera 1 has none of view 0, and its rows are those of the others
    assert counts[1][0] == 0 and res[1].shape[0] == sum(counts[1][1:])
    # the rows of the other views are untouched canaries: nothing is written past the (sum n_c, 2) doubles
    p, keep, M, S, P, _ = engine._rigJoint(cams, Pq)
    n = sum(r.shape[0] for r in res)
    buf = np.full((n + 8, 2), 7.25)
    assert nat.loadLibrary().calib_rig_residuals(ctypes.byref(p), nat.dptr(P), nat.dptr(buf), 0) == 0
    assert np.array_equal(buf[:n], np.concatenate(res)) and (buf[n:] == 7.25).all()


def rawRefine(prob, Pq, loss, mask=0, maxIters=10):
    p, keep, M, S, P, words = engine._rigJoint(qy.engineCameras(prob), Pq, mask)
    out = P.copy()
    lp = None if loss is None else ctypes.byref(nat.Loss(*loss))
    rc = nat.loadLibrary().calib_refine_rig_robust(ctypes.byref(p), nat.dptr(out), words, lp, maxIters, 1e-3, 1e-10, 1e10,
                                                   1e-12, None, None, None, None, 0)
    return rc, out


def test_delegation_and_errors():
    prob, _, Pq0, _ = qy.noisyCase()
    cams = qy.engineCameras(prob)
    plain = engine.refineRigJoint(cams, Pq0, 8)
    for loss in (None, (nat.LOSS_NONE, 0.0)):                       # NULL, and kind NONE whatever its scale
        p, keep, M, S, P, words = engine._rigJoint(cams, Pq0)
        out, cam, trace = P.copy(), np.empty(3), np.zeros((8, 5 + S))
        cost, it = ctypes.c_double(), ctypes.c_int()
        lp = None if loss is None else ctypes.byref(nat.Loss(*loss))
        rc = nat.loadLibrary().calib_refine_rig_robust(ctypes.byref(p), nat.dptr(out), None, lp, 8, engine.LAMBDA_INITIAL,
                                                       engine.LAMBDA_MIN, engine.LAMBDA_MAX, engine.PT_ERROR_MIN,
                                                       ctypes.byref(cost), nat.dptr(cam), ctypes.byref(it), nat.dptr(trace), 0)
        assert rc == 0 and it.value == plain[2] and cost.value == plain[0]
        assert out.tobytes() == plain[1].tobytes() and trace[:it.value].tobytes() == plain[3].tobytes()
        assert cam.tobytes() == plain[4].tobytes()
    a, b = engine.rigRobustNormalEquations(cams, Pq0, None), engine.rigJointNormalEquations(cams, Pq0)
    assert all(a[k].tobytes() == b[k].tobytes() for k in "BEVg") and a["costCam"].tobytes() == b["sseCam"].tobytes()
    assert engine.rigRobustStepDelta(cams, Pq0, 1e-3, None).tobytes() == engine.rigJointStepDelta(cams, Pq0, 1e-3).tobytes()
    for bad in ((7, 1.0), (nat.LOSS_HUBER, 0.0), (nat.LOSS_HUBER, -1.0), (nat.LOSS_CAUCHY, float("nan")),
                (nat.LOSS_CAUCHY, float("inf"))):
        rc, out = rawRefine(prob, Pq0, bad)
        assert rc == nat.E_INVALID and np.array_equal(out, Pq0), bad
    # the singular problems of the plain solver, under a loss: a free camera that sees nothing, a view with two points
    models, full = ["radtan", "fisheye", "radtan"], (54,) * 6
    for counts in ([full, (0,) * 6, full], [(54, 1, 54, 54, 54, 54), (54, 0, 54, 54, 54, 54), (54, 1, 54, 54, 54, 54)],
                   [(54, 54, 0, 54, 54, 54)] * 3):
        sp, PrTrue = ry.makeRig(3, 6, models, counts, noiseSigma=0.3)
        P0 = qy.perturbedJoint(sp, PrTrue, 0.2, 0.01, 0.1, 0.002, intrinsics=0.01)
        for loss in ((nat.LOSS_HUBER, 1.0), (nat.LOSS_CAUCHY, 1.0)):
            rc, out = rawRefine(sp, P0, loss)
            assert rc == nat.E_SINGULAR and np.array_equal(out, P0)
    with pytest.raises(np.linalg.LinAlgError):
        engine.rigRobustStepDelta(qy.engineCameras(sp), P0, 1e-3, "huber")


def startCameras(prob):
    """the outlier case's cameras as rigCalibrate takes them, each 1 % off in its intrinsics"""
    models = ["radtan", "fisheye", "radtan"]
    off1 = qy.perturbedShared(prob, intrinsics=0.01, distortion=0.0)
    return [(m, np.array([[s[0], s[2], s[3]], [0.0, s[1], s[4]], [0.0, 0.0, 1.0]]), s[5:]) for m, s in zip(models, off1)]


@pytest.mark.parametrize("loss", ["huber", ("cauchy", 1.0)], ids=["huber", "cauchy"])
def test_rig_calibrate_with_a_loss(loss):
    oc = rb.outlierCase()
    prob, PqTrue = oc["prob"], oc["PqTrue"]
    S = qy.layout(prob)[0]
    spec = engine.parseLoss(loss)
    res = cca.rigCalibrate(ry.detections(prob), startCameras(prob), refineCameras=True, loss=loss)
    clean = rb.rigError(prob, rb.outlierLoops(True)["clean"][1], PqTrue)
    cols = qy.columnsOfPr(prob)
    err = rb.rigError(prob, res.Pq, PqTrue)
    errOnly = float(np.abs(res.rigOnly.Pr[:12] - PqTrue[cols]).max())
    print(f"rigCalibrate(loss={loss!r}): rig-only (plain) largest rig error {errOnly:.4f}, robust joint {err:.4f} "
          f"({err / clean:.2f} x the clean fit's {clean:.4f}); cost {res.cost:.6e}, rms {res.rms}, rig-only rms {res.rigOnly.rms}")
    assert res.loss == spec and res.rigOnly.loss is None and res.rigOnly.Pq is None and res.fixedMask == 0
    assert res.Pq.shape == (S + 48,) and res.trace.shape == (res.iters, 5 + S)
    # the CPU test's conditions (3 x and 10 x the clean fit's error) put the two at least 10 / 3 apart; rigOnly here is the
    # plain fit with the cameras 1 % off held, not the plain joint fit, so it is measured against the robust result itself
    assert err <= 3 * clean and errOnly >= 10 / 3 * err
    # cost is the sum of rho, rms the plain one: both at the result, against the yardstick
    assert np.allclose(res.costCam, rb.costCam(prob, res.Pq, spec), rtol=1e-12, atol=0) and res.cost == float(res.costCam.sum())
    sse = np.array(qy.error(prob, res.Pq))
    assert np.allclose(res.sseCam, sse, rtol=1e-12, atol=0) and np.allclose(res.rms, np.sqrt(sse / res.numPoints), rtol=1e-12)
    assert res.cost < res.sse
    # residuals and weights
    r, w = res.residuals(), res.weights()
    assert [a.shape for a in r] == [(int(n), 2) for n in res.numPoints] and [a.shape for a in w] == [(int(n),) for n in res.numPoints]
    assert max(np.abs(a - b).max() for a, b in zip(r, rb.residuals(prob, res.Pq))) <= 1e-9
    flag, wAll = np.concatenate(oc["displaced"]), np.concatenate(w)
    low, high = (wAll[flag] < 0.5).mean(), (wAll[~flag] > 0.5).mean()
    print(f"weights: < 0.5 on {low:.3f} of the displaced corners, > 0.5 on {high:.3f} of the others")
    assert low >= 0.9 and high >= 0.9
    # covariance of the weighted blocks
    C, Cd = res.covariance(), rb.covarianceDense(prob, res.Pq, spec)
    rel = np.abs(C - Cd).max() / np.abs(Cd).max()
    print(f"covariance vs the weighted dense inverse: {rel:.3e} of its largest entry")
    assert C.shape == (S, S) and rel <= 1e-9
    assert np.array_equal(res.rigCovariance(2), C[35:41, 35:41])


def test_rig_calibrate_with_a_loss_and_the_cameras_held():
    """refineCameras=False: the robust loop holds every camera bit; covariance() is the rig block, as a rig-only result's"""
    oc = rb.outlierCase()
    prob, PqTrue = oc["prob"], oc["PqTrue"]
    cams = ry.cameraTuples(prob, ["radtan", "fisheye", "radtan"])  # the true cameras
    res = cca.rigCalibrate(ry.detections(prob), cams, loss="huber")
    plain = cca.rigCalibrate(ry.detections(prob), cams)
    clean = rb.rigError(prob, rb.outlierLoops(False)["clean"][1], PqTrue)
    err, errPlain = rb.rigError(prob, res.Pq, PqTrue), rb.rigError(prob, qy.join(oc["clean"], plain.Pr), PqTrue)
    print(f"cameras held: largest rig error plain {errPlain:.4f}, Huber {err:.4f} ({err / clean:.2f} x the clean fit's)")
    assert plain.loss is None and plain.Pq is None and np.array_equal(plain.Pr, res.rigOnly.Pr)     # no loss: nothing changed
    assert res.fixedMask == qy.cameraMask(prob) and err <= 3 * clean and errPlain >= 10 * clean
    for c, (t, A, k) in enumerate(res.cameras()):
        assert np.array_equal(A, cams[c][1]) and np.array_equal(k, np.asarray(cams[c][2], dtype=np.float64))
    C = res.covariance()
    cols = qy.columnsOfPr(prob)
    Cd = rb.covarianceDense(prob, res.Pq, ("huber", 1.0), res.fixedMask)[np.ix_(cols, cols)]
    rel = np.abs(C - Cd).max() / np.abs(Cd).max()
    print(f"rig covariance vs the weighted dense inverse: {rel:.3e}")
    assert C.shape == (12, 12) and rel <= 1e-9 and len(res.parameterNames()) == 12
    assert np.array_equal(res.rigCovariance(2), C[6:12, 6:12])
