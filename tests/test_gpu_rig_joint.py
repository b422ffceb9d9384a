"""Joint rig calibration on the device against tests/rig_joint_yardstick.py (numpy fp64 on the oracle's camera model): the
block-arrow normal equations, one LM step up to the largest factorisation, the sizes of the two reductions, the fixed
mask over cameras and rigs, N = 2 against the joint stereo solver, the whole loop noise-free and noisy, the singular
problems, and the public surface. Bars are those of tests/test_gpu_stereo_joint.py (blocks 1e-11 of the block's largest
entry, per-camera errors 1e-12 relative, a solved step 1e-9 in relative 2-norm, shared parameters 1e-7, rigs and poses
1e-9 from the truth); every test prints what it measured. tests/test_rig_joint_cpu.py holds the yardstick's side: its two
routes agree to 1e-11 on these cases.

Shapes: 17 views are one past eight two-view workgroups of the blocks kernel and one past four four-view passes of the
Schur kernel; per camera and view 0, 1, 5, 16, 17, 33, 54, 64 and 70 points of a 10 x 8 board are none, fewer than one
four-row MFMA group, a partial group, exactly and one more than half a 32-row pass, one more than a pass, and exactly and
more than a 64-point batch; N = 2, 3 and 8 are the smallest, the first with a zero block in B, and the largest (mixed:
S = 118; all radtan: S = 122, the largest Cholesky)."""
import ctypes

import numpy as np
import pytest

import camera_calibration_amd as cca
import rig_joint_yardstick as qy
import rig_yardstick as ry
from camera_calibration_amd import _native as nat
from camera_calibration_amd import engine
from oracle import calib_oracle as orc

pytestmark = pytest.mark.gpu

M_BLOCKS = qy.M_BLOCKS
_cache = {}


def relMax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def widths(prob):
    S, off, L = qy.layout(prob)
    return S, off, L, [L[c] + (6 if c else 0) for c in range(len(L))]


@pytest.mark.parametrize("key", [2, 3, 8])
def test_blocks_against_the_yardstick(key):
    prob, counts, Pq, ref = qy.blocksCase(key)
    S, off, L, W = widths(prob)
    N, M = len(L), M_BLOCKS
    ne = engine.rigJointNormalEquations(qy.engineCameras(prob), Pq)
    assert ne["B"].shape == (S, S) and ne["E"].shape == (M, S, 6) and ne["V"].shape == (M, 6, 6)
    assert ne["g"].shape == (S + 6 * M,) and ne["sseCam"].shape == (N,)
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
    worst["g_view"] = max(relMax(ne["g"][S + 6 * i:S + 6 + 6 * i], ref["g"][S + 6 * i:S + 6 + 6 * i]) for i in range(M))
    sse = np.abs(ne["sseCam"] - ref["sseCam"]) / ref["sseCam"]
    print(f"{key}: S = {S}; blocks vs yardstick, relative to each block's largest entry: {worst}; sse_cam relative {sse}")
    assert not offDiagonal.any()                                   # B outside its diagonal blocks: exactly zero
    assert np.array_equal(ne["B"], ne["B"].T)
    for i in range(M):
        assert np.array_equal(ne["V"][i], ne["V"][i].T)
    assert max(worst.values()) <= 1e-11
    assert sse.max() <= 1e-12


@pytest.mark.parametrize("lam", [1e-3, 10.0])
@pytest.mark.parametrize("key", [3, 8, "8r"])
def test_step_against_the_dense_solve(key, lam):
    """"8r": eight radtan cameras, S = 122, the largest factorisation"""
    prob, counts, Pq, _ = qy.blocksCase(key)
    S = qy.layout(prob)[0]
    ref = qy.stepDense(prob, Pq, lam)
    d = engine.rigJointStepDelta(qy.engineCameras(prob), Pq, lam)
    rel = np.linalg.norm(d - ref) / np.linalg.norm(ref)
    relShared = np.linalg.norm(d[:S] - ref[:S]) / np.linalg.norm(ref[:S])
    print(f"{key}: S = {S}, lambda {lam}: |delta - dense| / |dense| = {rel:.3e} (shared part {relShared:.3e})")
    assert rel <= 1e-9 and relShared <= 1e-9


@pytest.mark.parametrize("M", [1, 2, 17, 257, 4099])
def test_sizes_of_the_two_reductions(M):
    """N = 3, 6 to 12 points per camera and view; M = 1 and 2 with every camera bit fixed (so few views do not fix three
    cameras), the others free. The blocks kernel's grid is min(ceil(M / 2), 512) two-wave workgroups whose waves stride
    over the views, the Schur kernel's min(ceil(M / 4), 128) workgroups that stride over four-view passes; the
    one-workgroup sums read the rows eight at a time. M = 17: 9 workgroups, the last with one view (8 + 1 rows); 5
    passes, the last with one view. M = 257: 129 and 65 rows, no workgroup loops. M = 4099: both grids are full (512 and
    128 rows, whole groups of eight) and loop, the first three waves / the first workgroup one trip longer than the
    others, the last pass with three views. No further M is needed: every level has a full and a partial group. One step
    against the block-wise numpy Schur step (bar of the step test); every call is bitwise equal to its repeat."""
    prob, Pq = qy.sizesCase(M)
    S = qy.layout(prob)[0]
    mask = qy.cameraMask(prob) if M <= 2 else 0
    cams = qy.engineCameras(prob)
    d1 = engine.rigJointStepDelta(cams, Pq, 1e-3, mask)
    d2 = engine.rigJointStepDelta(cams, Pq, 1e-3, mask)
    ref = qy.stepBlocks(prob, Pq, 1e-3, mask)
    rel = np.linalg.norm(d1 - ref) / np.linalg.norm(ref)
    relShared = np.linalg.norm(d1[:S] - ref[:S]) / np.linalg.norm(ref[:S])
    print(f"M = {M}: |delta - blockwise| / |blockwise| = {rel:.3e} (shared part {relShared:.3e})")
    assert np.array_equal(d1, d2)
    assert rel <= 1e-9 and relShared <= 1e-9
    r1 = engine.refineRigJoint(cams, Pq, 3, mask)
    r2 = engine.refineRigJoint(cams, Pq, 3, mask)
    assert r1[0] == r2[0] and np.array_equal(r1[1], r2[1]) and np.array_equal(r1[3], r2[3]) and np.array_equal(r1[4], r2[4])
    n1, n2 = engine.rigJointNormalEquations(cams, Pq), engine.rigJointNormalEquations(cams, Pq)
    assert all(np.array_equal(n1[k], n2[k]) for k in n1)
    nb = qy.normalBlocks(prob, Pq)
    relB, relG = relMax(n1["B"], nb["B"]), relMax(n1["g"][:S], nb["g"][:S])
    print(f"M = {M}: B {relB:.3e}, g_shared {relG:.3e}")
    assert relB <= 1e-11 and relG <= 1e-11
    assert (np.abs(n1["sseCam"] - nb["sseCam"]) <= 1e-12 * nb["sseCam"]).all()


def mixedMask(prob):
    """camera 0's skew, camera 1's last coefficient, camera 2's principal point, rig 1's tz"""
    _, off, L = qy.layout(prob)
    return 1 << 2 | 1 << (off[1] + L[1] - 1) | 0b11 << (off[2] + 3) | 1 << (off[1] + L[1] + 5)


def test_mask_over_cameras_and_rigs():
    prob, counts, Pq, _ = qy.blocksCase(3)
    S, off, L, W = widths(prob)
    cams = qy.engineCameras(prob)
    # every camera bit set: the rig-only problem at Pq's cameras
    p, Pr = qy.split(prob, Pq)
    camMask = qy.cameraMask(prob)
    d = engine.rigJointStepDelta(cams, Pq, 1e-3, camMask)
    ref = engine.rigStepDelta(ry.engineCameras(p), Pr, 1e-3)
    got = np.concatenate((d[qy.columnsOfPr(prob)], d[S:]))
    rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print(f"every camera bit set vs calib_rig_step_delta: {rel:.3e}")
    assert rel <= 1e-9
    assert not d[:S][[s for s in range(S) if camMask >> s & 1]].any()
    # one whole rig fixed; a mask over cameras and a rig
    for name, mask in (("rig 2", qy.rigMask(prob, 2)), ("mixed", mixedMask(prob))):
        for lam in (1e-3, 10.0):
            d = engine.rigJointStepDelta(cams, Pq, lam, mask)
            ref = qy.stepDense(prob, Pq, lam, mask)
            rel = np.linalg.norm(d - ref) / np.linalg.norm(ref)
            print(f"mask {name} {mask:#x}, lambda {lam}: |delta - dense| / |dense| = {rel:.3e}")
            assert rel <= 1e-9
            fixedIdx = [s for s in range(S) if mask >> s & 1]
            assert not d[fixedIdx].any() and d[[s for s in range(S) if s not in fixedIdx]].all()


def test_fixed_parameters_keep_their_bits():
    """through several accepted iterations, -0.0 included: a fixed parameter is copied, not added to"""
    prob, counts, Pq, _ = qy.blocksCase(3)
    S, off, L, W = widths(prob)
    mask = mixedMask(prob)
    Pq0 = Pq.copy()
    Pq0[2] = -0.0                                                  # camera 0's skew
    sse, P, iters, trace, _ = engine.refineRigJoint(qy.engineCameras(prob), Pq0, 6, mask)
    accepted = int(trace[:, 4].sum())
    fixedIdx = [s for s in range(S) if mask >> s & 1]
    print(f"{iters} iterations, {accepted} accepted; fixed {fixedIdx}: {P[fixedIdx]}")
    assert accepted >= 3
    assert P[fixedIdx].tobytes() == Pq0[fixedIdx].tobytes() and np.signbit(P[2])
    free = [s for s in range(S) if s not in fixedIdx]
    assert (P[free] != Pq0[free]).all()
    for row in trace:
        assert row[5:][fixedIdx].tobytes() == Pq0[fixedIdx].tobytes()


def test_two_cameras_against_the_joint_stereo_solver():
    prob, counts, Pq, _ = qy.blocksCase(2)
    cams = qy.engineCameras(prob)
    S = qy.layout(prob)[0]
    a, b = engine.rigJointNormalEquations(cams, Pq), engine.stereoJointNormalEquations(*cams, Pq)
    worst = {k: relMax(a[k], b[k]) for k in ("B", "g")}
    worst["E"] = max(relMax(a["E"][i], b["E"][i]) for i in range(M_BLOCKS))
    worst["V"] = max(relMax(a["V"][i], b["V"][i]) for i in range(M_BLOCKS))
    sse = max(abs(a["sseCam"][0] / b["sseA"] - 1), abs(a["sseCam"][1] / b["sseB"] - 1))
    steps = {}
    for lam in (1e-3, 10.0):
        dq, dj = engine.rigJointStepDelta(cams, Pq, lam), engine.stereoJointStepDelta(*cams, Pq, lam)
        steps[lam] = np.linalg.norm(dq - dj) / np.linalg.norm(dj)
    sseQ, PQ, itQ, trQ, camQ = engine.refineRigJoint(cams, Pq, 4)
    sseJ, PJ, itJ, trJ, (eA, eB) = engine.refineStereoJoint(*cams, Pq, 4)
    print(f"N = 2 vs the joint stereo solver: blocks {worst}, sse {sse:.3e}, steps {steps}; after 4 iterations lambda "
          f"{trQ[:, 3]} / {trJ[:, 3]}, accepted {trQ[:, 4]} / {trJ[:, 4]}, sse {sseQ:.12e} / {sseJ:.12e}")
    assert max(worst.values()) <= 1e-11 and sse <= 1e-12
    assert max(steps.values()) <= 1e-9
    assert itQ == itJ == 4 and trQ.shape == trJ.shape == (4, 5 + S)
    assert np.array_equal(trQ[:, 3:5], trJ[:, 3:5])                # lambda and the decisions


def truthBars(prob, P, PTrue):
    """-> (shared parameters, rigs, pose matrices): largest absolute distance, as test_gpu_stereo_joint.py measures them"""
    S, off, L = qy.layout(prob)
    cols = qy.columnsOfPr(prob)
    shared = np.setdiff1d(np.arange(S), cols)
    dW = np.abs(ry.parametersToPoses(P[S:]) - ry.parametersToPoses(PTrue[S:])).max()
    return np.abs(P[shared] - PTrue[shared]).max(), np.abs(P[cols] - PTrue[cols]).max(), dW


def test_loop_noise_free_recovers_the_truth():
    prob, PqTrue, Pq0, (sseY, PqY, traceY) = qy.noiseFreeCase()
    S = qy.layout(prob)[0]
    sse, Pq, iters, trace, sseCam = engine.refineRigJoint(qy.engineCameras(prob), Pq0, 50)
    dS, dR, dP = truthBars(prob, Pq, PqTrue)
    print(f"noise-free N = 4, M = 20: iters {iters} (yardstick {len(traceY)}), sse {sse:.3e}, accepted {trace[:, 4]}; from "
          f"the truth: shared {dS:.3e}, rigs {dR:.3e}, poses {dP:.3e}; sse at the result {sseCam.sum():.3e}")
    assert iters == len(traceY) and trace.shape == (iters, 5 + S)
    assert sse < orc.PT_ERROR_MIN or not (orc.LAMBDA_MIN < trace[-1, 3] * (0.1 if trace[-1, 4] else 10) < orc.LAMBDA_MAX)
    assert dS <= 1e-7 and dR <= 1e-9 and dP <= 1e-9
    assert np.array_equal(trace[0, 5:], Pq0[:S])


def test_loop_noisy_follows_the_yardstick():
    prob, PqTrue, Pq0, (sseY, PqY, traceY) = qy.noisyCase()
    S = qy.layout(prob)[0]
    sse, Pq, iters, trace, sseCam = engine.refineRigJoint(qy.engineCameras(prob), Pq0, 50)
    n = min(ry.decidedRows(traceY), iters)
    print(f"noisy: iters {iters} (yardstick {len(traceY)}), rows with decided lambda {n}; lambda {trace[:n, 3]}; max rel d "
          f"err(P) {np.abs(trace[:n, 1] / traceY[:n, 1] - 1).max():.3e}, d err(P + delta) "
          f"{np.abs(trace[:n, 2] / traceY[:n, 2] - 1).max():.3e}; sse {sse:.12e} (yardstick {sseY:.12e})")
    assert n >= 6                                                  # test_rig_joint_cpu asserts the yardstick's side of this
    assert trace.shape == (iters, 5 + S)
    assert np.array_equal(trace[:n, 3], traceY[:n, 3])
    assert np.array_equal(trace[:n - 1, 4], traceY[:n - 1, 4])
    assert sse == trace[-1, 1]
    eY = np.array(qy.error(prob, Pq))                              # the yardstick's errors at the returned point
    print(f"sseCam {sseCam} vs the yardstick's at the returned point: {np.abs(sseCam - eY) / eY}")
    assert (np.abs(sseCam - eY) <= 1e-12 * eY).all()


def rawRefine(prob, Pq, mask=0, maxIters=10):
    """calib_refine_rig_joint's return code and Pq_inout as it leaves them"""
    p, keep, M, S, P, words = engine._rigJoint(qy.engineCameras(prob), Pq, mask)
    out = P.copy()
    rc = nat.loadLibrary().calib_refine_rig_joint(ctypes.byref(p), nat.dptr(out), words, maxIters, 1e-3, 1e-10, 1e10, 1e-12,
                                                  None, None, None, None, 0)
    return rc, out


def test_singular_problems_return_singular_and_leave_the_point():
    models = ["radtan", "fisheye", "radtan"]
    full = (54,) * 6
    # a free camera c >= 1 that sees nothing; fixed with its rig, the problem is solvable
    prob, PrTrue = ry.makeRig(3, 6, models, [full, (0,) * 6, full], noiseSigma=0.3)
    Pq0 = qy.perturbedJoint(prob, PrTrue, 0.2, 0.01, 0.1, 0.002, intrinsics=0.01)
    rc, out = rawRefine(prob, Pq0)
    assert rc == nat.E_SINGULAR and np.array_equal(out, Pq0)
    with pytest.raises(np.linalg.LinAlgError):
        engine.rigJointStepDelta(qy.engineCameras(prob), Pq0, 1e-3)
    rc, out = rawRefine(prob, Pq0, qy.cameraMask(prob, [1]))      # the camera alone is not enough: its rig is free
    assert rc == nat.E_SINGULAR and np.array_equal(out, Pq0)
    mask = qy.cameraMask(prob, [1]) | qy.rigMask(prob, 1)
    rc, out = rawRefine(prob, Pq0, mask)
    S = qy.layout(prob)[0]
    fixedIdx = [s for s in range(S) if mask >> s & 1]
    print(f"camera 1 without points, fixed with its rig: rc {rc}")
    assert rc == 0 and np.isfinite(out).all() and out[fixedIdx].tobytes() == Pq0[fixedIdx].tobytes()
    assert not np.array_equal(out, Pq0)
    # free camera 0 that sees nothing; fixed, the poses hang on cameras 1 and 2
    prob, PrTrue = ry.makeRig(3, 6, models, [(0,) * 6, full, full], noiseSigma=0.3)
    Pq0 = qy.perturbedJoint(prob, PrTrue, 0.2, 0.01, 0.1, 0.002, intrinsics=0.01)
    rc, out = rawRefine(prob, Pq0)
    assert rc == nat.E_SINGULAR and np.array_equal(out, Pq0)
    rc, out = rawRefine(prob, Pq0, qy.cameraMask(prob, [0]))
    print(f"camera 0 without points, fixed: rc {rc}")
    assert rc == 0 and np.isfinite(out).all() and np.array_equal(out[:10], Pq0[:10])
    # a view with two points in total
    prob, PrTrue = ry.makeRig(3, 6, models, [(54, 1, 54, 54, 54, 54), (54, 0, 54, 54, 54, 54), (54, 1, 54, 54, 54, 54)])
    Pq0 = qy.perturbedJoint(prob, PrTrue, 0.2, 0.01, 0.1, 0.002, intrinsics=0.01)
    rc, out = rawRefine(prob, Pq0)
    assert rc == nat.E_SINGULAR and np.array_equal(out, Pq0)
    # an empty view among good ones
    prob, PrTrue = ry.makeRig(3, 6, models, [(54, 54, 0, 54, 54, 54)] * 3)
    Pq0 = qy.perturbedJoint(prob, PrTrue, 0.2, 0.01, 0.1, 0.002, intrinsics=0.01)
    rc, out = rawRefine(prob, Pq0)
    assert rc == nat.E_SINGULAR and np.array_equal(out, Pq0)
    ne = engine.rigJointNormalEquations(qy.engineCameras(prob), Pq0)             # the blocks themselves are defined
    assert not ne["V"][2].any() and not ne["E"][2].any() and np.isfinite(ne["B"]).all()


def surfaceCase():
    """a noisy three-camera set (0.3 px), every camera 1 % off in its intrinsics: rig-only and joint results, once"""
    if "surface" not in _cache:
        models = ["radtan", "fisheye", "radtan"]
        counts = [(54, 54, 54, 0, 54, 54, 54, 54), (54, 54, 54, 54, 54, 0, 54, 54), (54, 0, 54, 54, 54, 54, 54, 40)]
        prob, PrTrue = ry.makeRig(3, 8, models, counts, noiseSigma=0.3)
        off1 = qy.perturbedShared(prob, intrinsics=0.01, distortion=0.0)
        cams = [(m, np.array([[s[0], s[2], s[3]], [0.0, s[1], s[4]], [0.0, 0.0, 1.0]]), s[5:]) for m, s in zip(models, off1)]
        res = cca.rigCalibrate(ry.detections(prob), cams, refineCameras=True)
        _cache["surface"] = (prob, PrTrue, models, cams, res)
    return _cache["surface"]


def test_rig_calibrate_with_the_cameras_refined():
    prob, PrTrue, models, cams, res = surfaceCase()
    S = 41
    print(f"rigCalibrate(refineCameras=True): rig-only sse {res.rigOnly.sse:.6e} in {res.rigOnly.iters} iterations, joint sse "
          f"{res.sse:.6e} in {res.iters}; rms {res.rms}")
    assert res.Pq.shape == (S + 48,) and res.fixedMask == 0 and res.rigOnly.Pq is None
    assert res.sse < res.rigOnly.sse
    assert res.trace.shape == (res.iters, 5 + S) and res.T.shape == (3, 4, 4) and len(res.W) == 8
    assert len(res.jointParameterNames()) == S and res.jointParameterNames()[19] == "rig1.rx"
    # the refined cameras are Pq's
    for c, (t, A, k) in enumerate(res.cameras()):
        o = (0, 10, 25)[c]
        assert t == models[c] and A[0, 0] == res.Pq[o] and A[1, 2] == res.Pq[o + 4] and np.array_equal(k, res.Pq[o + 5:o + 5 + len(k)])
    assert not np.array_equal(res.cameras()[0][1], res.rigOnly.cameras()[0][1])
    # covariance against the dense inverse at the result
    C, Cd = res.covariance(), qy.covarianceDense(prob, res.Pq)
    rel = np.abs(C - Cd).max() / np.abs(Cd).max()
    print(f"covariance vs the dense inverse: {rel:.3e} of its largest entry; rig 1 std {np.sqrt(np.diagonal(res.rigCovariance(1)))}")
    assert C.shape == (S, S) and rel <= 1e-9
    assert np.array_equal(res.rigCovariance(2), C[35:41, 35:41])
    # the refined cameras feed triangulateAll: the corners of view 2, which every camera saw in full
    full, _ = ry.makeRig(3, 8, models)
    o = full["offs"][0]
    p, Pr = qy.split(full, res.Pq)
    uv = ry.project(p, Pr)                                         # projected with the refined cameras, rigs and poses
    X = res.triangulateAll([u[o[2]:o[3]] for u in uv])
    W2 = res.W[2]
    want = full["xyz"][0][o[2]:o[3]] @ W2[:3, :3].T + W2[:3, 3]
    print(f"triangulateAll with the refined cameras: |X - board in camera 0| {np.abs(X - want).max():.3e}")
    assert X.shape == want.shape and np.abs(X - want).max() <= 1e-9
    # fixed and fixedRigs reach the solver: what they name keeps its bits
    res2 = cca.rigCalibrate(ry.detections(prob), cams, refineCameras=True, fixed=[None, {"k4": 0.0}, "focal"], fixedRigs=(2,))
    assert res2.fixedMask == 1 << 18 | 0b11 << 25 | 0x3f << 35 and res2.Pq[18] == 0.0
    start = cca.rig.packJoint([qy.perturbedShared(prob, 0.01, 0.0)[c] for c in range(3)], res2.rigOnly.Pr)
    assert res2.Pq[[25, 26]].tobytes() == start[[25, 26]].tobytes() and res2.Pq[35:41].tobytes() == start[35:41].tobytes()
    Cf = res2.covariance()
    fixedIdx = [s for s in range(S) if res2.fixedMask >> s & 1]
    assert not Cf[fixedIdx].any() and not Cf[:, fixedIdx].any() and np.diagonal(Cf)[[0, 19]].all()


def test_calibrate_rig_joint_ends_by_the_stop_rule():
    models = ["radtan", "radtan", "radtan"]
    counts = [(54, 54, 54, 0, 54, 54, 54, 54), (54, 54, 54, 54, 54, 0, 54, 54), (54, 0, 54, 54, 54, 54, 54, 40)]
    prob, PrTrue = ry.makeRig(3, 8, models, counts, noiseSigma=0.3)
    results, res = cca.calibrateRig(ry.detections(prob), models, 50, joint=True)
    print(f"calibrateRig(joint=True): iters {res.iters}, sse {res.sse:.6e} (rig-only {res.rigOnly.sse:.6e}), last lambda "
          f"{res.trace[-1, 3]:.1e}")
    assert len(results) == 3 and res.Pq is not None
    assert res.iters < 50 and res.trace.shape == (res.iters, 5 + 42)      # ended through the stop rule, not the cap
    assert not (orc.LAMBDA_MIN < res.trace[-1, 3] * (0.1 if res.trace[-1, 4] else 10) < orc.LAMBDA_MAX)
    assert res.sse <= res.rigOnly.sse
    for (_, A, _, k), (t, A1, k1) in zip(results, res.rigOnly.cameras()):        # the mono results stay as they were
        assert np.array_equal(A, A1) and np.array_equal(np.ravel(k), k1)
