"""Joint stereo calibration on the device against tests/stereo_joint_yardstick.py (numpy fp64 on the oracle's camera
model): the block-arrow normal equations, one LM step, the fixed mask, the whole loop noise-free and noisy, the sizes of
the view reduction, the singular problems, the covariance and the public surface. Bars are the project's own for the
analogous stereo tests (blocks 1e-11 of the block's largest entry, a solved step 1e-9 in relative 2-norm); every test
prints what it measured."""
import ctypes

import numpy as np
import pytest

import camera_calibration_amd as cca
import stereo_joint_yardstick as jy
import stereo_yardstick as sy
from camera_calibration_amd import _native as nat
from camera_calibration_amd import engine
from oracle import calib_oracle as orc

pytestmark = pytest.mark.gpu

PAIRS = [("radtan", "radtan"), ("radtan", "fisheye"), ("fisheye", "radtan"), ("fisheye", "fisheye")]
# per view: below a 4-point group, at and across a 16-lane group, a full 64-point batch, across one (70), empty sides, a
# 3-point view
NA, NB = (7, 0, 16, 3, 33, 70, 54, 40), (5, 9, 0, 17, 64, 70, 0, 60)
_cache = {}


def blocksCase(pair):
    """the M = 8 ragged problem of a model pair at a point away from the solution (rig and poses as sy.perturbed(PsTrue,
    1.0, 0.03, 1.0, 0.01), intrinsics off by 2 %, distortion by 10 %), with the yardstick's blocks (once)"""
    if pair not in _cache:
        prob, PsTrue = sy.makeStereo(8, pair[0], pair[1], board=(10, 7, 0.05), noiseSigma=0.3, countsA=NA, countsB=NB)
        Pj = jy.perturbedJoint(prob, PsTrue, 1.0, 0.03, 1.0, 0.01)
        _cache[pair] = (prob, Pj, jy.normalBlocks(prob, Pj))
    return _cache[pair]


def relMax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def cameraBits(prob):
    La, Lb, _ = jy.sizes(prob)
    return (1 << La + Lb) - 1


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_blocks_against_the_yardstick(pair):
    prob, Pj, ref = blocksCase(pair)
    La, Lb, S = jy.sizes(prob)
    ne = engine.stereoJointNormalEquations(*sy.engineCameras(prob), Pj)
    a, b, r = slice(0, La), slice(La, La + Lb), slice(La + Lb, S)
    br = slice(La, S)
    worst = {"B_aa": relMax(ne["B"][a, a], ref["B"][a, a]), "B_(b,rig)": relMax(ne["B"][br, br], ref["B"][br, br]),
             "g_a": relMax(ne["g"][a], ref["g"][a]), "g_b": relMax(ne["g"][b], ref["g"][b]),
             "g_rig": relMax(ne["g"][r], ref["g"][r])}
    worst["E_a"] = max(relMax(ne["E"][i][a], ref["E"][i][a]) for i in range(8) if NA[i])
    worst["E_b"] = max(relMax(ne["E"][i][b], ref["E"][i][b]) for i in range(8) if NB[i])
    worst["E_rig"] = max(relMax(ne["E"][i][r], ref["E"][i][r]) for i in range(8) if NB[i])
    worst["V"] = max(relMax(ne["V"][i], ref["V"][i]) for i in range(8))
    worst["g_view"] = max(relMax(ne["g"][S + 6 * i:S + 6 * i + 6], ref["g"][S + 6 * i:S + 6 * i + 6]) for i in range(8))
    sse = (abs(ne["sseA"] - ref["sseA"]) / ref["sseA"], abs(ne["sseB"] - ref["sseB"]) / ref["sseB"])
    print(f"{pair}: blocks vs yardstick, relative to each block's largest entry: {worst}; sse_ab relative {sse}")
    for i in range(8):
        if not NA[i]:
            assert not ne["E"][i][a].any() and not ref["E"][i][a].any()        # no camera-a rows: exactly zero
        if not NB[i]:
            assert not ne["E"][i][br].any() and not ref["E"][i][br].any()      # no camera-b rows: exactly zero
        assert np.array_equal(ne["V"][i], ne["V"][i].T)
    assert np.array_equal(ne["B"], ne["B"].T)
    assert not ne["B"][a, br].any() and not ne["B"][br, a].any()               # no row touches both: exactly zero
    assert max(worst.values()) <= 1e-11
    assert max(sse) <= 1e-12


@pytest.mark.parametrize("lam", [1e-3, 10.0])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_step_against_the_dense_solve(pair, lam):
    prob, Pj, nb = blocksCase(pair)
    d = engine.stereoJointStepDelta(*sy.engineCameras(prob), Pj, lam)
    ref = jy.stepDense(prob, Pj, lam)
    routes = np.linalg.norm(jy.stepFromBlocks(nb, lam) - ref) / np.linalg.norm(ref)
    rel = np.linalg.norm(d - ref) / np.linalg.norm(ref)
    S = jy.sizes(prob)[2]
    print(f"{pair} lambda {lam}: |delta - dense| / |dense| = {rel:.3e} (shared part "
          f"{np.linalg.norm(d[:S] - ref[:S]) / np.linalg.norm(ref[:S]):.3e}); the yardstick's two routes {routes:.3e}")
    assert routes <= 1e-11
    assert rel <= 1e-9


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_fixed_mask_all_camera_bits_is_the_rig_only_step_and_a_cleared_mask_leaves_no_trace(pair):
    prob, Pj, nb = blocksCase(pair)
    La, Lb, S = jy.sizes(prob)
    cams = sy.engineCameras(prob)
    free = engine.stereoJointStepDelta(*cams, Pj, 1e-3)
    for lam in (1e-3, 10.0):
        d = engine.stereoJointStepDelta(*cams, Pj, lam, fixedMask=cameraBits(prob))
        p, Ps = jy.split(prob, Pj)
        ref = engine.stereoStepDelta(*sy.engineCameras(p), Ps, lam)
        rel = np.linalg.norm(d[La + Lb:] - ref) / np.linalg.norm(ref)
        print(f"{pair} lambda {lam}: cameras fixed, |rig and poses - calib_stereo_step_delta| / | | = {rel:.3e}")
        assert not d[:La + Lb].any()
        assert rel <= 1e-9
    # some parameters fixed: against the yardstick with those columns removed
    mask = 1 << La - 1 | 1 << La + Lb - 1 | 1 << S - 1
    d = engine.stereoJointStepDelta(*cams, Pj, 1e-3, fixedMask=mask)
    ref = jy.stepDense(prob, Pj, 1e-3, mask)
    rel = np.linalg.norm(d - ref) / np.linalg.norm(ref)
    print(f"{pair}: mask {mask:#x}, |delta - dense| / |dense| = {rel:.3e}")
    assert rel <= 1e-9 and not d[[La - 1, La + Lb - 1, S - 1]].any()
    assert np.array_equal(engine.stereoJointStepDelta(*cams, Pj, 1e-3), free)          # set, then cleared


def test_a_fixed_parameter_keeps_its_bits_through_a_refinement():
    prob, Pj, _ = blocksCase(("radtan", "fisheye"))
    La, Lb, S = jy.sizes(prob)
    Pj = Pj.copy()
    Pj[2] = -0.0                                                                        # camera a's skew
    held = [2, La - 1, La + 3, S - 4]                                                   # a.gamma a.k3 b.uc rig.rz
    mask = sum(1 << s for s in held)
    sse, out, iters, trace, _ = engine.refineStereoJoint(*sy.engineCameras(prob), Pj, 12, fixedMask=mask)
    moved = np.flatnonzero(out[:S] != Pj[:S])
    print(f"fixed {held}: {iters} iterations, accepted {int(trace[:, 4].sum())}, sse {trace[0, 1]:.4e} -> {sse:.4e}; "
          f"shared unknowns that moved: {moved.tolist()}")
    assert trace[:, 4].sum() >= 3
    assert out[held].tobytes() == Pj[held].tobytes() and np.signbit(out[2])
    assert sorted(set(range(S)) - set(moved.tolist())) == held


def loopCase(pair):
    if ("loop", pair) not in _cache:
        prob, PsTrue = sy.makeStereo(6, pair[0], pair[1])
        Pj0 = jy.perturbedJoint(prob, PsTrue, 1.0, 0.03, 1.0, 0.01)
        _cache[("loop", pair)] = (prob, jy.join(prob, PsTrue), Pj0, jy.refineDense(prob, Pj0, 50))
    return _cache[("loop", pair)]


@pytest.mark.parametrize("pair", [("fisheye", "radtan"), ("radtan", "radtan")], ids=lambda p: f"{p[0]}-{p[1]}")
def test_loop_noise_free_recovers_the_truth(pair):
    """M = 6 views of a 9 x 6 board; start: rig and poses off by 1 degree and 3 % / 1 %, intrinsics by 2 %, distortion by
    10 %."""
    prob, PjTrue, Pj0, (sseY, PjY, traceY) = loopCase(pair)
    La, Lb, S = jy.sizes(prob)
    sse, Pj, iters, trace, (sseA, sseB) = engine.refineStereoJoint(*sy.engineCameras(prob), Pj0, 50)
    dShared = np.abs(Pj[:La + Lb] - PjTrue[:La + Lb]).max()
    dRig = np.abs(Pj[La + Lb:S] - PjTrue[La + Lb:S]).max()
    dW = np.abs(sy.parametersToPoses(Pj[S:]) - sy.parametersToPoses(PjTrue[S:])).max()
    print(f"{pair}: iters {iters} (yardstick {len(traceY)}), rejects {int((trace[:, 4] == 0).sum())}, sse {sse:.3e} "
          f"(yardstick {sseY:.3e}), last lambda {trace[-1, 3]:.1e}, |shared - truth| {dShared:.3e}, |rig - truth| "
          f"{dRig:.3e}, |W - truth| {dW:.3e}, sse at the result {sseA + sseB:.3e}")
    assert iters < 50 and trace.shape == (iters, 5 + S)          # ended through the stop rule, not the iteration cap
    assert sse < orc.PT_ERROR_MIN or not (orc.LAMBDA_MIN < trace[-1, 3] * (0.1 if trace[-1, 4] else 10) < orc.LAMBDA_MAX)
    assert abs(iters - len(traceY)) <= 2
    assert dShared <= 1e-7
    assert dRig <= 1e-9
    assert dW <= 1e-9
    assert np.array_equal(trace[0, 5:], Pj0[:S])


def decidedRows(traceY):
    """Leading rows of the yardstick's trace whose lambda is fixed by decisions with a margin: |err(P + delta) - err(P)|
    above 1e-12 err(P). Two fixed-order fp64 sums of ~1e3 terms agree to ~1e-13 relative, so a smaller margin is decided
    by the summation order and no two implementations need agree on it; every later lambda depends on that decision."""
    margin = np.abs(traceY[:, 2] - traceY[:, 1]) > 1e-12 * traceY[:, 1]
    firstOpen = int(np.argmin(margin)) if not margin.all() else len(traceY)
    return min(firstOpen + 1, len(traceY))


def noisyData():
    if "noisy" not in _cache:
        _cache["noisy"] = sy.makeStereo(6, "radtan", "fisheye", noiseSigma=0.3, countsA=(54, 30, 0, 54, 17, 54),
                                        countsB=(54, 54, 40, 0, 54, 9))
    return _cache["noisy"]


def test_loop_noisy_follows_the_yardstick():
    prob, PsTrue = noisyData()
    La, Lb, S = jy.sizes(prob)
    Pj0 = jy.perturbedJoint(prob, PsTrue, 1.0, 0.03, 1.0, 0.01)
    sseY, PjY, traceY = jy.refineDense(prob, Pj0, 50)
    sse, Pj, iters, trace, (sseA, sseB) = engine.refineStereoJoint(*sy.engineCameras(prob), Pj0, 50)
    n = min(decidedRows(traceY), iters)
    print(f"noisy: iters {iters} (yardstick {len(traceY)}), rows with decided lambda {n}; lambda {trace[:n, 3]}; "
          f"max rel d err(P) {np.abs(trace[:n, 1] / traceY[:n, 1] - 1).max():.3e}, d err(P + delta) "
          f"{np.abs(trace[:n, 2] / traceY[:n, 2] - 1).max():.3e}; sse {sse:.12e} (yardstick {sseY:.12e})")
    assert n >= 5
    assert np.array_equal(trace[:n, 3], traceY[:n, 3])
    assert np.array_equal(trace[:n - 1, 4], traceY[:n - 1, 4])
    assert np.allclose(trace[:n, 1:3], traceY[:n, 1:3], rtol=1e-9, atol=0)
    assert sse == trace[-1, 1]                                   # err(P) of the last iteration, before its update
    eA, eB = jy.error(prob, Pj)
    assert abs(sseA - eA) <= 1e-12 * eA and abs(sseB - eB) <= 1e-12 * eB


def test_stereo_calibrate_refines_the_cameras_and_its_covariance_counts_them():
    """the public surface on the noisy data: refineCameras continues from the rig-only result and cannot end above it;
    covariance() against the yardstick's dense inverse, fixed rows and columns exact zeros"""
    prob, PsTrue = noisyData()
    La, Lb, S = jy.sizes(prob)
    detA, detB = sy.detections(prob)
    camA = ("radtan", sy.A_A["radtan"] * np.array([[1.01, 1, 0.99], [1, 0.99, 1.01], [1, 1, 1]]), sy.K_A["radtan"])
    camB = ("fisheye", sy.A_B * np.array([[0.99, 1, 1.01], [1, 1.01, 0.99], [1, 1, 1]]), sy.K_B["fisheye"])
    rigOnly = cca.stereoCalibrate(detA, detB, camA, camB)
    res = cca.stereoCalibrate(detA, detB, camA, camB, refineCameras=True)
    held = cca.stereoCalibrate(detA, detB, camA, camB, refineCameras=True, fixedA="skew", fixedB={"k4": -0.0})
    print(f"stereoCalibrate: rig only sse {rigOnly.sse:.6e} ({rigOnly.iters} iterations), joint {res.sse:.6e} ({res.iters}), "
          f"joint with a.gamma, b.k4 fixed {held.sse:.6e} ({held.iters})")
    assert rigOnly.Pj is None and np.array_equal(res.rigOnly.Ps, rigOnly.Ps) and res.rigOnly.sse == rigOnly.sse
    assert res.sse <= rigOnly.sse and held.sse <= rigOnly.sse
    assert res.trace.shape == (res.iters, 5 + S) and res.Pj.shape == (S + 36,) and len(res.W) == 6
    assert res.jointParameterNames()[La + Lb - 1:La + Lb + 1] == ("b.k4", "rig.rx")
    (ta, Aa, ka), (tb, Ab, kb) = res.cameras()
    assert (ta, tb) == ("radtan", "fisheye")
    assert np.array_equal(sy.sharedOf(Aa, ka), res.Pj[:La]) and np.array_equal(sy.sharedOf(Ab, kb), res.Pj[La:La + Lb])
    assert not np.array_equal(Aa, camA[1])
    assert held.Pj[2] == camA[1][0, 1] and held.Pj[La + Lb - 1].tobytes() == np.float64(-0.0).tobytes()
    for r, mask in ((res, 0), (held, 1 << 2 | 1 << La + Lb - 1)):
        assert r.fixedMask == mask
        C = r.covariance()
        Cd = jy.covarianceDense(prob, r.Pj, mask)
        rel = np.abs(C - Cd).max() / np.abs(Cd).max()
        fixedIdx = [s for s in range(S) if mask >> s & 1]
        print(f"  mask {mask:#x}: covariance vs dense {rel:.3e} of its largest entry; rig std {np.sqrt(np.diagonal(C)[-6:])} "
              f"(rig only: {np.sqrt(np.diagonal(rigOnly.rigCovariance()))})")
        assert rel <= 1e-9
        assert not C[fixedIdx].any() and not C[:, fixedIdx].any()
        assert np.array_equal(r.rigCovariance(), C[-6:, -6:])
    with pytest.raises(ValueError, match="joint run"):
        rigOnly.covariance()


@pytest.mark.parametrize("M", [3, 17, 257, 4099])
def test_sizes_of_the_view_reduction(M):
    """4 + 4 points per view; 3 views leave a workgroup of the blocks kernel (4 views) part empty, 17 and 257 are one past a
    16-view workgroup of the Schur kernel and past 16 of them, 4099 is 1025 blocks partials: past a multiple of the 4 x 8
    rows the sum takes at once. One step against the block-wise numpy Schur step (bar of the step test); two identical
    calls are bitwise equal."""
    prob, PsTrue = sy.makeStereo(M, "radtan", "fisheye", noiseSigma=0.3, countsA=[4] * M, countsB=[4] * M)
    Pj = jy.perturbedJoint(prob, PsTrue, 0.2, 0.01, 0.1, 0.002, intrinsics=0.002, distortion=0.01)
    S = jy.sizes(prob)[2]
    cams = sy.engineCameras(prob)
    d1 = engine.stereoJointStepDelta(*cams, Pj, 1e-3)
    d2 = engine.stereoJointStepDelta(*cams, Pj, 1e-3)
    nb = jy.normalBlocks(prob, Pj)
    ref = jy.stepFromBlocks(nb, 1e-3)
    rel = np.linalg.norm(d1 - ref) / np.linalg.norm(ref)
    relS = np.linalg.norm(d1[:S] - ref[:S]) / np.linalg.norm(ref[:S])
    print(f"M = {M}: |delta - blockwise| / |blockwise| = {rel:.3e} (shared part {relS:.3e})")
    assert np.array_equal(d1, d2)
    assert rel <= 1e-9 and relS <= 1e-9
    r1 = engine.refineStereoJoint(*cams, Pj, 3)
    r2 = engine.refineStereoJoint(*cams, Pj, 3)
    assert r1[0] == r2[0] and np.array_equal(r1[1], r2[1]) and np.array_equal(r1[3], r2[3]) and r1[4] == r2[4]
    ne = engine.stereoJointNormalEquations(*cams, Pj)
    assert relMax(ne["B"], nb["B"]) <= 1e-11 and relMax(ne["g"][:S], nb["g"][:S]) <= 1e-11


@pytest.mark.parametrize("M", [1, 2])
def test_one_and_two_views_with_both_cameras_fixed(M):
    prob, PsTrue = sy.makeStereo(M, "radtan", "fisheye", noiseSigma=0.3, countsA=[4] * M, countsB=[4] * M)
    Pj = jy.perturbedJoint(prob, PsTrue, 0.2, 0.01, 0.1, 0.002, intrinsics=0.002, distortion=0.01)
    cams, mask = sy.engineCameras(prob), cameraBits(prob)
    d1 = engine.stereoJointStepDelta(*cams, Pj, 1e-3, fixedMask=mask)
    d2 = engine.stereoJointStepDelta(*cams, Pj, 1e-3, fixedMask=mask)
    ref = jy.stepBlocks(prob, Pj, 1e-3, mask)
    rel = np.linalg.norm(d1 - ref) / np.linalg.norm(ref)
    print(f"M = {M}, cameras fixed: |delta - blockwise| / |blockwise| = {rel:.3e}")
    assert np.array_equal(d1, d2)
    assert rel <= 1e-9
    r1 = engine.refineStereoJoint(*cams, Pj, 3, fixedMask=mask)
    r2 = engine.refineStereoJoint(*cams, Pj, 3, fixedMask=mask)
    assert r1[0] == r2[0] and np.array_equal(r1[1], r2[1]) and np.array_equal(r1[3], r2[3]) and r1[4] == r2[4]


def rawRefine(prob, Pj, mask=0, maxIters=10):
    """calib_refine_stereo_joint's return code and Pj_inout as it leaves them"""
    p, keep, M = engine._stereoProblem(*sy.engineCameras(prob))
    out = np.ascontiguousarray(Pj).copy()
    rc = nat.loadLibrary().calib_refine_stereo_joint(ctypes.byref(p), nat.dptr(out), mask, maxIters, 1e-3, 1e-10, 1e10, 1e-12,
                                                     None, None, None, None, 0)
    return rc, out


def test_singular_problems_return_singular_and_leave_the_point_alone():
    # a view with 2 points in total
    prob, PsTrue = sy.makeStereo(4, countsA=(20, 1, 20, 20), countsB=(20, 1, 20, 20))
    Pj0 = jy.join(prob, sy.perturbed(PsTrue, 0.2, 0.01, 0.1, 0.002))
    rc, out = rawRefine(prob, Pj0)
    assert rc == nat.E_SINGULAR and np.array_equal(out, Pj0)
    with pytest.raises(np.linalg.LinAlgError):
        engine.stereoJointStepDelta(*sy.engineCameras(prob), Pj0, 1e-3)
    # an empty view among good ones
    prob, PsTrue = sy.makeStereo(4, countsA=(20, 20, 0, 20), countsB=(20, 20, 0, 20))
    Pj0 = jy.join(prob, sy.perturbed(PsTrue, 0.2, 0.01, 0.1, 0.002))
    rc, out = rawRefine(prob, Pj0)
    assert rc == nat.E_SINGULAR and np.array_equal(out, Pj0)
    ne = engine.stereoJointNormalEquations(*sy.engineCameras(prob), Pj0)            # the blocks themselves are defined
    assert not ne["V"][2].any() and not ne["E"][2].any() and np.isfinite(ne["B"]).all()
    # camera a sees nothing: free, its block of the reduced system is zero; fixed, the problem is camera b's alone
    prob, PsTrue = sy.makeStereo(5, countsA=(0, 0, 0, 0, 0), countsB=(54, 54, 54, 54, 54))
    La, Lb, S = jy.sizes(prob)
    Pj0 = jy.join(prob, sy.perturbed(PsTrue, 0.2, 0.01, 0.1, 0.002))
    rc, out = rawRefine(prob, Pj0)
    assert rc == nat.E_SINGULAR and np.array_equal(out, Pj0)
    rc, out = rawRefine(prob, Pj0, mask=(1 << La) - 1, maxIters=50)
    e0, e1 = sum(jy.error(prob, Pj0)), sum(jy.error(prob, out))
    print(f"camera a sees nothing, fixed: rc {rc}, sse {e0:.3e} -> {e1:.3e}")
    assert rc == 0 and np.isfinite(out).all() and np.array_equal(out[:La], Pj0[:La])
    assert e1 < e0
