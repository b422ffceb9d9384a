"""Stereo calibration on the device against tests/stereo_yardstick.py (numpy fp64 on the oracle's camera model): the
block-arrow normal equations, one LM step, the whole loop noise-free and noisy, the sizes of the view reduction, the
singular and degenerate problems, and the public surface. Bars are the project's own for the analogous mono tests
(blocks 1e-11 of the block's largest entry, a solved step 1e-9 in relative 2-norm, parameters 1e-9 / poses 1e-7); every
test prints what it measured."""
import ctypes

import numpy as np
import pytest

import camera_calibration_amd as cca
import stereo_yardstick as sy
from camera_calibration_amd import _native as nat
from camera_calibration_amd import engine
from oracle import calib_oracle as orc

pytestmark = pytest.mark.gpu

PAIRS = [("radtan", "radtan"), ("radtan", "fisheye"), ("fisheye", "radtan"), ("fisheye", "fisheye")]
NA, NB = (7, 0, 16, 3, 33), (5, 9, 0, 17, 64)           # below, at and above a 16-lane group and a wave; empty sides
_cache = {}


def blocksCase(pair):
    """the M = 5 ragged problem of a model pair at a point away from the solution, with the yardstick's blocks (once)"""
    if pair not in _cache:
        prob, PsTrue = sy.makeStereo(5, pair[0], pair[1], board=(10, 7, 0.05), noiseSigma=0.3, countsA=NA, countsB=NB)
        Ps = sy.perturbed(PsTrue, 0.3, 0.02, 0.2, 0.004)
        _cache[pair] = (prob, Ps, sy.normalBlocks(prob, Ps))
    return _cache[pair]


def relMax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_blocks_against_the_yardstick(pair):
    prob, Ps, ref = blocksCase(pair)
    ne = engine.stereoNormalEquations(*sy.engineCameras(prob), Ps)
    worst = {"B": relMax(ne["B"], ref["B"]), "g_rig": relMax(ne["g"][:6], ref["g"][:6])}
    worst["E"] = max(relMax(ne["E"][i], ref["E"][i]) for i in range(5) if NB[i])
    worst["V"] = max(relMax(ne["V"][i], ref["V"][i]) for i in range(5))
    worst["g_view"] = max(relMax(ne["g"][6 + 6 * i:12 + 6 * i], ref["g"][6 + 6 * i:12 + 6 * i]) for i in range(5))
    sse = (abs(ne["sseA"] - ref["sseA"]) / ref["sseA"], abs(ne["sseB"] - ref["sseB"]) / ref["sseB"])
    print(f"{pair}: blocks vs yardstick, relative to each block's largest entry: {worst}; sse_ab relative {sse}")
    for i in range(5):
        if not NB[i]:
            assert not ne["E"][i].any() and not ref["E"][i].any()          # no camera-b rows: exactly zero
        assert np.array_equal(ne["V"][i], ne["V"][i].T)
    assert np.array_equal(ne["B"], ne["B"].T)
    assert max(worst.values()) <= 1e-11
    assert max(sse) <= 1e-12


@pytest.mark.parametrize("lam", [1e-3, 10.0])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_step_against_the_dense_solve(pair, lam):
    prob, Ps, _ = blocksCase(pair)
    d = engine.stereoStepDelta(*sy.engineCameras(prob), Ps, lam)
    ref = sy.stepDense(prob, Ps, lam)
    rel = np.linalg.norm(d - ref) / np.linalg.norm(ref)
    print(f"{pair} lambda {lam}: |delta - dense| / |dense| = {rel:.3e}")
    assert rel <= 1e-9


@pytest.mark.parametrize("pair", [("fisheye", "radtan"), ("radtan", "fisheye")], ids=lambda p: f"{p[0]}-{p[1]}")
def test_loop_noise_free_recovers_the_truth(pair):
    """M = 6 views of a 9 x 6 board; start: rig off by 2 degrees and 5 % of the baseline, poses by 1 degree and 1 %
    (the yardstick alone converges from there in 5 iterations)."""
    prob, PsTrue = sy.makeStereo(6, pair[0], pair[1])
    Ps0 = sy.perturbed(PsTrue, 2.0, 0.05, 1.0, 0.01)
    sse, Ps, iters, trace, (sseA, sseB) = engine.refineStereo(*sy.engineCameras(prob), Ps0, 50)
    sseY, PsY, traceY = sy.refineDense(prob, Ps0, 50)
    dW = np.abs(sy.parametersToPoses(Ps[6:]) - sy.parametersToPoses(PsTrue[6:])).max()
    print(f"{pair}: iters {iters} (yardstick {len(traceY)}), sse {sse:.3e} (yardstick {sseY:.3e}), last lambda "
          f"{trace[-1, 3]:.1e}, |rig - truth| {np.abs(Ps[:6] - PsTrue[:6]).max():.3e}, |W - truth| {dW:.3e}, "
          f"sse at the result {sseA + sseB:.3e}")
    assert iters < 50 and trace.shape == (iters, 11)             # ended through the stop rule, not the iteration cap
    assert sse < orc.PT_ERROR_MIN or not (orc.LAMBDA_MIN < trace[-1, 3] * (0.1 if trace[-1, 4] else 10) < orc.LAMBDA_MAX)
    assert np.abs(Ps[:6] - PsTrue[:6]).max() <= 1e-9
    assert dW <= 1e-9
    assert abs(iters - len(traceY)) <= 2
    assert np.array_equal(trace[0, 5:], Ps0[:6])


def decidedRows(traceY):
    """Leading rows of the yardstick's trace whose lambda is fixed by decisions with a margin: |err(P + delta) - err(P)|
    above 1e-12 err(P). Two fixed-order fp64 sums of ~1e3 terms agree to ~1e-13 relative, so a smaller margin is decided
    by the summation order and no two implementations need agree on it; every later lambda depends on that decision."""
    margin = np.abs(traceY[:, 2] - traceY[:, 1]) > 1e-12 * traceY[:, 1]
    firstOpen = int(np.argmin(margin)) if not margin.all() else len(traceY)
    return min(firstOpen + 1, len(traceY))


def noisyCase():
    if "noisy" not in _cache:
        prob, PsTrue = sy.makeStereo(6, "radtan", "fisheye", noiseSigma=0.3, countsA=(54, 30, 0, 54, 17, 54),
                                     countsB=(54, 54, 40, 0, 54, 9))
        Ps0 = sy.perturbed(PsTrue, 0.5, 0.02, 0.3, 0.005)
        _cache["noisy"] = (prob, PsTrue, Ps0, sy.refineDense(prob, Ps0, 50))
    return _cache["noisy"]


def test_loop_noisy_follows_the_yardstick():
    prob, PsTrue, Ps0, (sseY, PsY, traceY) = noisyCase()
    sse, Ps, iters, trace, (sseA, sseB) = engine.refineStereo(*sy.engineCameras(prob), Ps0, 50)
    n = min(decidedRows(traceY), iters)
    dRig = np.abs(Ps[:6] - PsY[:6]) / np.maximum(1.0, np.abs(PsY[:6]))
    dPose = np.abs(Ps[6:] - PsY[6:]).max()
    print(f"noisy: iters {iters} (yardstick {len(traceY)}), rows with decided lambda {n}; lambda {trace[:n, 3]}; "
          f"max rel d err(P) {np.abs(trace[:n, 1] / traceY[:n, 1] - 1).max():.3e}, d err(P + delta) "
          f"{np.abs(trace[:n, 2] / traceY[:n, 2] - 1).max():.3e}; rig diff {dRig.max():.3e}, pose diff {dPose:.3e}; "
          f"sse {sse:.12e} (yardstick {sseY:.12e})")
    assert n >= 5
    assert np.array_equal(trace[:n, 3], traceY[:n, 3])
    assert np.array_equal(trace[:n - 1, 4], traceY[:n - 1, 4])
    assert np.allclose(trace[:n, 1:3], traceY[:n, 1:3], rtol=1e-9, atol=0)
    assert np.allclose(trace[:n, 5:], traceY[:n, 5:], rtol=0, atol=1e-9)
    assert dRig.max() <= 1e-9
    assert dPose <= 1e-7
    # the reference's return convention: err(P) of the last iteration, before its update
    assert sse == trace[-1, 1]
    assert abs(sse - sseY) <= 1e-9 * sseY
    eA, eB = sy.error(prob, Ps)
    assert abs(sseA - eA) <= 1e-12 * eA and abs(sseB - eB) <= 1e-12 * eB


@pytest.mark.parametrize("M", [1, 2, 17, 257, 4099])
def test_sizes_of_the_view_reduction(M):
    """4 + 4 points per view; 17 and 257 views are one past a 16-view workgroup and past 16 of them, 4099 is more
    workgroup partials than one wave sums at once. One step against the block-wise numpy Schur step (bar of the step
    test); two identical calls are bitwise equal."""
    prob, PsTrue = sy.makeStereo(M, "radtan", "fisheye", noiseSigma=0.3, countsA=[4] * M, countsB=[4] * M)
    Ps = sy.perturbed(PsTrue, 0.2, 0.01, 0.1, 0.002)
    cams = sy.engineCameras(prob)
    d1 = engine.stereoStepDelta(*cams, Ps, 1e-3)
    d2 = engine.stereoStepDelta(*cams, Ps, 1e-3)
    ref = sy.stepBlocks(prob, Ps, 1e-3)
    rel = np.linalg.norm(d1 - ref) / np.linalg.norm(ref)
    relRig = np.linalg.norm(d1[:6] - ref[:6]) / np.linalg.norm(ref[:6])
    print(f"M = {M}: |delta - blockwise| / |blockwise| = {rel:.3e} (rig part {relRig:.3e})")
    assert np.array_equal(d1, d2)
    assert rel <= 1e-9 and relRig <= 1e-9
    r1 = engine.refineStereo(*cams, Ps, 3)
    r2 = engine.refineStereo(*cams, Ps, 3)
    assert r1[0] == r2[0] and np.array_equal(r1[1], r2[1]) and np.array_equal(r1[3], r2[3]) and r1[4] == r2[4]
    ne = engine.stereoNormalEquations(*cams, Ps)
    nb = sy.normalBlocks(prob, Ps)
    assert relMax(ne["B"], nb["B"]) <= 1e-11 and relMax(ne["g"][:6], nb["g"][:6]) <= 1e-11


def rawRefine(prob, Ps, maxIters=10):
    """calib_refine_stereo's return code and Ps_inout as it leaves them"""
    p, keep, M = engine._stereoProblem(*sy.engineCameras(prob))
    out = np.ascontiguousarray(Ps).copy()
    rc = nat.loadLibrary().calib_refine_stereo(ctypes.byref(p), nat.dptr(out), maxIters, 1e-3, 1e-10, 1e10, 1e-12, None,
                                               None, None, None, 0)
    return rc, out


def test_singular_and_degenerate_problems_do_not_fault():
    # a view with 2 points in total
    prob, PsTrue = sy.makeStereo(4, countsA=(20, 1, 20, 20), countsB=(20, 1, 20, 20))
    Ps0 = sy.perturbed(PsTrue, 0.2, 0.01, 0.1, 0.002)
    rc, out = rawRefine(prob, Ps0)
    assert rc == nat.E_SINGULAR and np.array_equal(out, Ps0)
    with pytest.raises(np.linalg.LinAlgError):
        engine.stereoStepDelta(*sy.engineCameras(prob), Ps0, 1e-3)
    # no view has points in camera b: nothing constrains the rig
    prob, PsTrue = sy.makeStereo(4, countsA=(20, 20, 20, 20), countsB=(0, 0, 0, 0))
    Ps0 = sy.perturbed(PsTrue, 0.2, 0.01, 0.1, 0.002)
    rc, out = rawRefine(prob, Ps0)
    assert rc == nat.E_SINGULAR and np.array_equal(out, Ps0)
    # an empty view among good ones
    prob, PsTrue = sy.makeStereo(4, countsA=(20, 20, 0, 20), countsB=(20, 20, 0, 20))
    Ps0 = sy.perturbed(PsTrue, 0.2, 0.01, 0.1, 0.002)
    rc, out = rawRefine(prob, Ps0)
    assert rc == nat.E_SINGULAR and np.array_equal(out, Ps0)
    ne = engine.stereoNormalEquations(*sy.engineCameras(prob), Ps0)             # the blocks themselves are defined
    assert not ne["V"][2].any() and not ne["E"][2].any() and np.isfinite(ne["B"]).all()
    # only ONE view has camera-b points (6 of them): enough for the rig
    prob, PsTrue = sy.makeStereo(4, countsA=(20, 20, 20, 20), countsB=(0, 6, 0, 0))
    Ps0 = sy.perturbed(PsTrue, 0.5, 0.02, 0.3, 0.005)
    rc, out = rawRefine(prob, Ps0, 50)
    print(f"one view with camera-b points: rc {rc}, |rig - truth| {np.abs(out[:6] - PsTrue[:6]).max():.3e}")
    assert rc == 0 and np.isfinite(out).all()
    assert np.abs(out[:6] - PsTrue[:6]).max() <= 1e-6


def test_stereo_calibrate_recovers_the_rig_with_views_missing_from_either_camera():
    prob, PsTrue = sy.makeStereo(7, "radtan", "fisheye", countsA=(54, 0, 54, 40, 54, 0, 54), countsB=(54, 54, 0, 54, 30, 54, 54))
    detA, detB = sy.detections(prob)
    camA = ("radtan", sy.A_A["radtan"], sy.K_A["radtan"])
    camB = ("fisheye", sy.A_B, sy.K_B["fisheye"])
    res = cca.stereoCalibrate(detA, detB, camA, camB)
    T = sy.parametersToPoses(PsTrue[:6])[0]
    dW = max(np.abs(w - wt).max() for w, wt in zip(res.W, sy.parametersToPoses(PsTrue[6:])))
    print(f"stereoCalibrate: iters {res.iters}, sse {res.sse:.3e}, |T - truth| {np.abs(res.T - T).max():.3e}, "
          f"|W - truth| {dW:.3e}, sseA {res.sseA:.3e} sseB {res.sseB:.3e} rms {res.rmsA:.3e} {res.rmsB:.3e}")
    assert np.abs(res.T - T).max() <= 1e-9
    assert np.array_equal(res.T[:3, :3], res.R) and np.array_equal(res.T[:3, 3], res.t)
    assert abs(res.sseA + res.sseB - res.sse) <= 1e-12 * res.sse
    assert res.sse < 1e-12 and res.sseBeforeLastUpdate < 1e-9
    assert res.trace.shape == (res.iters, 11) and len(res.W) == 7
    with pytest.raises(ValueError, match="view 1"):
        cca.stereoCalibrate([detA[0], None, detA[2]], [detB[0], None, detB[2]], camA, camB)
    with pytest.raises(ValueError, match="both cameras"):
        cca.stereoCalibrate([detA[0], None], [None, detB[1]], camA, camB)


def test_calibrate_stereo_and_rig_covariance_on_a_noisy_set():
    prob, PsTrue = sy.makeStereo(8, "radtan", "radtan", noiseSigma=0.3, countsA=(54, 54, 54, 0, 54, 54, 54, 54),
                                 countsB=(54, 54, 54, 54, 54, 0, 54, 54))
    detA, detB = sy.detections(prob)
    (sa, Aa, Wa, ka), (sb, Ab, Wb, kb), res = cca.calibrateStereo(detA, detB, "radtan", "radtan", 50)
    assert len(Wa) == 7 and len(Wb) == 7
    # the yardstick's LM on the same problem (the cameras calibrateStereo found) from the truth's neighbourhood
    probY = dict(prob, shared_a=sy.sharedOf(Aa, ka), shared_b=sy.sharedOf(Ab, kb))
    sseY, PsY, traceY = sy.refineDense(probY, sy.perturbed(PsTrue, 0.1, 0.01, 0.1, 0.002), 50)
    dRig = np.abs(res.Ps[:6] - PsY[:6]) / np.maximum(1.0, np.abs(PsY[:6]))
    dPose = np.abs(res.Ps[6:] - PsY[6:]).max()
    C = res.rigCovariance()
    Cd = sy.covarianceDense(probY, res.Ps)
    scale = np.sqrt(np.outer(np.diagonal(Cd), np.diagonal(Cd)))
    relC = (np.abs(C - Cd) / scale).max()
    print(f"calibrateStereo: iters {res.iters}, sse {res.sse:.6e} (yardstick {sseY:.6e}), rig diff {dRig.max():.3e}, pose "
          f"diff {dPose:.3e}; covariance vs dense {relC:.3e}\n  rig std  {np.sqrt(np.diagonal(C))}\n  rig error "
          f"{np.abs(res.Ps[:6] - PsTrue[:6])}")
    assert dRig.max() <= 1e-9
    assert dPose <= 1e-7
    assert abs(res.sse - sseY) <= 1e-9 * sseY and abs(res.sseA + res.sseB - res.sse) <= 1e-12 * res.sse
    assert relC <= 1e-8
