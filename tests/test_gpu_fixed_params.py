"""Fixed shared parameters in the LM loop and the per-view pose-only refinement, on the GPU.

The reference has no mask to run, so the yardstick for the mask is the reference ALGORITHM on the restricted
problem, written here from the oracle's public pieces: orc.jacobianDense with the fixed columns deleted, the dense
inv() step of src/calibrate.py:152, orc.reprojectionError and the lambda rule of :155-168 (maskedDenseRefine). The
yardstick for the pose kernel is the same loop per view on the six view columns of orc.jacobianCompact
(posesYardstick). Poses are compared as 4x4 transforms, never as Euler angles: on the radtan golden the yardstick and
Pfinal differ by 360 degrees in an angle while describing the same rotation.

Tolerances are the project's stated ones: a step against the dense inv() step 1e-8 relative norm;
converged shared parameters 1e-9 absolute on noise-free data; iteration counts within +-2 between device and oracles
with identical accept / reject decisions while they are well separated. "Well separated" here: the yardstick's
candidate and current errors differ by more than 1e-6 relative and the current error is above 1e-13 -- device and
oracle errors agree to 1e-9 relative above that floor, so a decision with a 1e-6 margin cannot flip."""
import functools
import os
import socket

import numpy as np
import pytest

import camera_calibration_amd as cca
from camera_calibration_amd import _native as nat
from camera_calibration_amd import engine, fixed, synthetic
from conftest import loadGolden
from oracle import calib_oracle as orc

pytestmark = pytest.mark.gpu

GOLDENS = {"radtan": ("g2_config1_radtan.npz", orc.RADTAN), "fisheye": ("g2_config1_fisheye.npz", orc.FISHEYE)}
MASK_KEYS = ("gamma", "gamma_lastk", "pp", "allk", "all")


def maskOf(key, name):
    names = fixed.sharedNames(engine.MODEL_IDS[name])
    sel = {"gamma": ("gamma",), "gamma_lastk": ("gamma", names[-1]), "pp": ("uc", "vc"), "allk": ("distortion",),
           "all": ("all",)}[key]
    return fixed.resolveFixed(names, sel)[0]


def bitsOf(mask):
    return [i for i in range(32) if mask >> i & 1]


# ---- the yardstick: the reference's dense loop on the problem without the fixed columns ------------------------
def maskedDenseStep(model, P, offs, s, m, lam, F):
    J = orc.jacobianDense(model, P, offs, m)
    free = np.setdiff1d(np.arange(J.shape[1]), F)
    Jf = J[:, free]
    r = (np.asarray(s) - orc.projectAllPoints(model, P, offs, m)).reshape(-1, 1)
    JTJ = Jf.T @ Jf
    delta = np.zeros(J.shape[1])
    delta[free] = (np.linalg.inv(JTJ + lam * np.diag(np.diagonal(JTJ))) @ Jf.T @ r).ravel()
    return delta


def maskedDenseRefine(model, P0, offs, s, m, maxIters, F):
    """orc.refineDense (src/calibrate.py:143-171) with the step of the column-deleted problem
    -> (error before the last update, P, trace rows (iter, err, err candidate, lambda, accepted))"""
    Pt = np.array(P0, dtype=np.float64).ravel()
    lam, trace, err = orc.LAMBDA_INITIAL, [], None
    for it in range(maxIters):
        delta = maskedDenseStep(model, Pt, offs, s, m, lam, F)
        err = orc.reprojectionError(model, Pt, offs, s, m)
        err1 = orc.reprojectionError(model, Pt + delta, offs, s, m)
        accepted = bool(err1 < err)
        trace.append((it, err, err1, lam, float(accepted)))
        if accepted:
            Pt = Pt + delta
            lam /= 10
        else:
            lam *= 10
        if not (orc.LAMBDA_MIN < lam < orc.LAMBDA_MAX) or err < orc.PT_ERROR_MIN:
            break
    return err, Pt, np.array(trace)


@functools.lru_cache(maxsize=None)
def yardstickOnGolden(tag, model, mask, maxIters=60):
    g = loadGolden(tag)
    return maskedDenseRefine(model, g["P0"], g["viewOffsets"], g["sensorPoints"], g["modelPoints"], maxIters,
                             bitsOf(mask))


def wellSeparatedPrefix(traceY):
    n = 0
    for row in traceY:
        if not (row[1] > 1e-13 and abs(row[2] - row[1]) > 1e-6 * row[1]):
            break
        n += 1
    return n


def checkMaskedRun(out, yard, P0, F, label, zeroResidual=False):
    """fixed entries bit-equal in P and in every trace row, count within +-2, accept column equal while well
    separated, final error within 1e-6 relative. zeroResidual: the fixed entries start at their true values on
    noise-free data, so both loops end through the stop rule err < 1e-12 (src/calibrate.py:168) with errors of 1e-14
    to 1e-18 -- rounding noise of the sums, where a relative bar says nothing: two final errors below the stop rule's
    own threshold count as equal there."""
    sse, P, iters, trace = out
    errY, PY, trY = yard
    print(f"{label}: iters {iters} (yardstick {trY.shape[0]}), sse {sse:.6e} (yardstick {errY:.6e}), "
          f"separated prefix {wellSeparatedPrefix(trY)}, max |P - PY| {np.abs(P - PY).max():.3e}")
    assert np.array_equal(P[F], P0[F]), label
    assert trace.shape[0] == iters
    for c in F:
        assert np.array_equal(trace[:, 5 + c], np.full(iters, P0[c])), (label, c)
    assert abs(iters - trY.shape[0]) <= 2, label
    n = min(wellSeparatedPrefix(trY), iters)
    assert n >= 3, label
    assert np.array_equal(trace[:n, 4], trY[:n, 4]), label
    if zeroResidual and sse < orc.PT_ERROR_MIN and errY < orc.PT_ERROR_MIN:
        return
    assert abs(sse - errY) <= 1e-6 * errY, label


# ---- 1. one step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", MASK_KEYS)
@pytest.mark.parametrize("case", ["radtan", "fisheye", "ragged200"])
def test_step_delta_is_the_step_of_the_column_deleted_problem(case, key):
    name = "radtan" if case == "ragged200" else case
    tag, model = ("g5_ragged200.npz", orc.RADTAN) if case == "ragged200" else GOLDENS[case]
    g = loadGolden(tag)
    offs, s, m, P0 = g["viewOffsets"], g["sensorPoints"], g["modelPoints"], g["P0"]
    mask = maskOf(key, name)
    F = bitsOf(mask)
    eng = cca.RefineEngine(name, "f64")
    eng.setProblem(offs, s, m)
    eng.setFixedShared(mask)
    assert eng.fixedShared == mask
    d = eng.stepDelta(P0, 1e-3)
    eng.close()
    dY = maskedDenseStep(model, P0, offs, s, m, 1e-3, F)
    rel = np.linalg.norm(d - dY) / np.linalg.norm(dY)
    print(f"{case} {key}: |d - dY| / |dY| = {rel:.3e}")
    assert np.all(d[F] == 0.0)
    assert rel < 1e-8


def test_mask_entry_points_reject_bad_arguments():
    for name, L in (("radtan", 10), ("fisheye", 9)):
        eng = cca.RefineEngine(name, "f64")
        assert eng.fixedShared == 0
        eng.setFixedShared((1 << L) - 1)                   # all L bits set is legal
        assert eng.fixedShared == (1 << L) - 1
        with pytest.raises(ValueError):                    # CALIB_E_INVALID from the library itself
            nat.check(eng._lib.calib_set_fixed_shared(eng._h, 1 << L))
        assert eng.fixedShared == (1 << L) - 1             # a refused mask changes nothing
        eng.setFixedShared(("skew", "focal"))
        assert eng.fixedShared == 0b111
        eng.close()


# ---- 2. whole refinements ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fused", "two_kernel"])
@pytest.mark.parametrize("key", MASK_KEYS)
@pytest.mark.parametrize("name", ["radtan", "fisheye"])
def test_masked_refinement_follows_the_yardstick(name, key, mode):
    tag, model = GOLDENS[name]
    g = loadGolden(tag)
    mask = maskOf(key, name)
    eng = cca.RefineEngine(name, "f64")
    eng.setProblem(g["viewOffsets"], g["sensorPoints"], g["modelPoints"])
    eng.setLmMode(mode)
    eng.setFixedShared(mask)
    out = eng.refine(g["P0"], 60)
    eng.close()
    checkMaskedRun(out, yardstickOnGolden(tag, model, mask), g["P0"], bitsOf(mask), f"{name} {key} {mode}")


@pytest.mark.parametrize("key", MASK_KEYS)
def test_masked_refinement_on_a_ragged_shard(key):
    g = loadGolden("g5_ragged200.npz")
    mask = maskOf(key, "radtan")
    # the "camera partly known" use: the fixed parameters sit at their true values, everything else starts perturbed
    # (the golden's P0). Held at P0's perturbed values instead, the minimum has a non-zero residual and the loop
    # ends by lambda leaving its range after wandering at the floor of the sums, where the count is decided by
    # summation order: the dense yardstick and a numpy Schur form of the same masked loop then take 31 and 37
    # (gamma), 35 and 23 (gamma, k3), 23 and 33 (uc, vc) iterations on this golden -- no count to hold a device to.
    F = bitsOf(mask)
    P0 = g["P0"].copy()
    P0[F] = g["Ptrue"][F]
    eng = cca.RefineEngine("radtan", "f64")
    eng.setProblem(g["viewOffsets"], g["sensorPoints"], g["modelPoints"])
    eng.setFixedShared(mask)
    out = eng.refine(P0, 60)
    eng.close()
    yard = maskedDenseRefine(orc.RADTAN, P0, g["viewOffsets"], g["sensorPoints"], g["modelPoints"], 60, bitsOf(mask))
    checkMaskedRun(out, yard, P0, F, f"ragged200 {key}", zeroResidual=True)


@pytest.mark.parametrize("stream", ["0", "1"])
def test_masked_refinement_in_the_stream_form(stream, monkeypatch):
    """one uniform shape large enough for the stream form of the fused kernel (c5's 88-point views, the wave count of
    tests/test_gpu_scale.py::test_stream_form_of_the_fused_kernel), every mask, stream form on and off"""
    monkeypatch.setenv("CALIB_FUSED_STREAM", stream)
    monkeypatch.setenv("CALIB_STREAM_WAVES", "9")
    cfg = dict(synthetic.CONFIGS["c2"], board=(11, 8, 0.04))
    sh = synthetic.makeShard(cfg, viewStart=7, numViews=53, noiseSigma=0.0)
    offs, s, m = sh["viewOffsets"], sh["sensorPoints"], sh["modelPoints"]
    for key in MASK_KEYS:
        mask = maskOf(key, "radtan")
        P0 = sh["P0"].copy()                               # as on the ragged shard: fixed at the truth, the rest perturbed
        P0[bitsOf(mask)] = sh["Ptrue"][bitsOf(mask)]
        eng = cca.RefineEngine("radtan", "f64")
        eng.setProblem(offs, s, m)
        assert (eng.fusedForm()[0] > 0) == (stream == "1")
        eng.setFixedShared(mask)
        out = eng.refine(P0, 60)
        eng.close()
        yard = maskedDenseRefine(orc.RADTAN, P0, offs, s, m, 60, bitsOf(mask))
        checkMaskedRun(out, yard, P0, bitsOf(mask), f"stream={stream} {key}", zeroResidual=True)


# ---- 3. zero skew ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["radtan", "fisheye"])
def test_zero_skew_recovers_the_goldens_parameters(name):
    tag, model = GOLDENS[name]
    g = loadGolden(tag)
    L = orc.numShared(model)
    assert g["P0"][2] != 0.0 and g["Atrue"][0, 1] == 0.0
    cal = cca.Calibrator(cca.RadialTangentialModel() if name == "radtan" else cca.FisheyeModel(), fixed={"gamma": 0.0})
    sse, P, iters, trace = cal.refinePacked(g["P0"], g["viewOffsets"], g["sensorPoints"], g["modelPoints"], 100)
    cal.close()
    print(f"{name}: {iters} iterations, sse {sse:.3e}, max |P - Pfinal| shared {np.abs(P[:L] - g['Pfinal'][:L]).max():.3e}")
    assert P[2] == 0.0 and np.all(trace[:, 5 + 2] == 0.0)
    assert np.abs(P[:L] - g["Pfinal"][:L]).max() < 1e-9


# ---- 4. mask 0 changes nothing ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["radtan", "fisheye"])
def test_mask_zero_is_bitwise_the_loop_without_a_mask(name):
    tag, model = GOLDENS[name]
    g = loadGolden(tag)
    outs = []
    for setIt in (True, False):
        eng = cca.RefineEngine(name, "f64")
        eng.setProblem(g["viewOffsets"], g["sensorPoints"], g["modelPoints"])
        if setIt:
            eng.setFixedShared(0b100)                      # and back: the handle's mask, not its history, counts
            eng.setFixedShared(0)
        d = eng.stepDelta(g["P0"], 1e-3)
        outs.append((d,) + eng.refine(g["P0"], 60))
        eng.close()
    a, b = outs
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3]
    assert np.array_equal(a[4], b[4])


# ---- 5. fp32 storage -------------------------------------------------------------------------------------------
def test_fp32_storage_holds_fixed_parameters_bitwise():
    tag, model = GOLDENS["radtan"]
    g = loadGolden(tag)
    mask = maskOf("gamma_lastk", "radtan")
    F = bitsOf(mask)
    outs = {}
    for dtype in ("f64", "f32"):
        eng = cca.RefineEngine("radtan", dtype)
        eng.setProblem(g["viewOffsets"], g["sensorPoints"], g["modelPoints"])
        eng.setFixedShared(mask)
        outs[dtype] = eng.refine(g["P0"], 60)
        eng.close()
    (sse64, P64, it64, tr64), (sse32, P32, it32, tr32) = outs["f64"], outs["f32"]
    scale = np.maximum(np.abs(P64[:10]), 1.0)
    scale[2] = abs(P64[0])
    rel = float(np.max(np.abs(P32[:10] - P64[:10]) / scale))
    print(f"fp32 vs fp64 masked: shared parameters {rel:.3e} relative, sse {sse32:.6e} vs {sse64:.6e}")
    assert np.array_equal(P32[F], g["P0"][F]) and np.array_equal(tr32[:, 5 + np.array(F)], np.tile(g["P0"][F], (it32, 1)))
    # the existing fp32 bar on the result (tests/test_gpu_scale.py: relIntr < 1e-6 against fp64): converged shared
    # parameters 1e-6 relative
    assert rel < 1e-6


# ---- 6. through the facade -------------------------------------------------------------------------------------
def _detections(g):
    offs = g["viewOffsets"]
    return [(g["sensorPoints"][a:b], g["modelPoints"][a:b]) for a, b in zip(offs[:-1], offs[1:])]


def test_facade_calibrate_camera_with_zero_skew(capsys):
    g = loadGolden("g2_config1_radtan.npz")
    dets = _detections(g)
    sse, A, W, k = cca.calibrateCamera(dets, "radtan", 100, fixed={"skew": 0.0})
    print(f"max |A - Atrue| {np.abs(A - g['Atrue']).max():.3e}, max |k - ktrue| {np.abs(np.array(k) - g['ktrue']).max():.3e}")
    assert A[0, 1] == 0.0
    assert np.abs(A - g["Atrue"]).max() < 1e-6 and np.abs(np.array(k) - g["ktrue"]).max() < 1e-6
    # Calibrator.calibrate prints per iteration (shouldPrint): that path takes the same mask
    out = capsys.readouterr().out
    assert "iter 0:" in out
    cal = cca.Calibrator(cca.RadialTangentialModel(), fixed=("k3",))
    A0, W0, k0 = cal.estimateCalibrationParameters(dets)
    sse2, A2, W2, k2 = cal.calibrate(dets, 100)
    assert k2[4] == k0[4] and np.all(cal.lastTrace[:, 5 + 9] == k0[4])
    assert A2[0, 1] != 0.0
    cal.close()
    with pytest.raises(ValueError):
        cca.calibrateCamera(dets, "fisheye", 5, fixed=("tangential",))


# ---- 7. sharded, real engines, two ranks on one GPU ------------------------------------------------------------
def _freePort():
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        return sock.getsockname()[1]


def _shardWorker(rank, world, port, outDir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0", RANK=str(rank),
                      WORLD_SIZE=str(world), CALIB_ALLREDUCE="torch", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from camera_calibration_amd import distributed
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = loadGolden("g3_unittest15.npz")
        sse, P, iters, trace = distributed.refineDistributed("radtan", g["P0"], g["viewOffsets"], g["sensorPoints"],
                                                             g["modelPoints"], 60, fixedShared=("gamma", "k3"))
        np.savez(os.path.join(outDir, f"r{rank}.npz"), sse=sse, P=P, iters=iters, trace=trace,
                 kind=distributed.refineDistributed.lastAllReduce)
    finally:
        dist.destroy_process_group()


def test_sharded_masked_refinement_two_ranks_on_one_gpu(tmp_path):
    """the launcher pattern of tests/test_gpu_multiproc.py (fresh spawned children, gloo, the torch carrier)"""
    import torch.multiprocessing as mp
    world = 2
    mp.spawn(_shardWorker, args=(world, _freePort(), str(tmp_path)), nprocs=world, join=True)
    outs = [np.load(os.path.join(tmp_path, f"r{r}.npz")) for r in range(world)]
    g = loadGolden("g3_unittest15.npz")
    P0, L = g["P0"], 10
    F = [2, 9]
    eng = cca.RefineEngine("radtan", "f64")
    eng.setProblem(g["viewOffsets"], g["sensorPoints"], g["modelPoints"])
    eng.setFixedShared(("gamma", "k3"))
    sseR, PR, itR, trR = eng.refine(P0, 60)
    eng.close()
    for o in outs:
        assert str(o["kind"]) == "torch"
        assert np.array_equal(o["P"][F], P0[F])                                # bit-equal on both ranks
        assert np.array_equal(o["trace"][:, 5 + np.array(F)], np.tile(P0[F], (int(o["iters"]), 1)))
        assert np.array_equal(o["P"], outs[0]["P"]) and np.array_equal(o["trace"], outs[0]["trace"])
    P, iters = outs[0]["P"], int(outs[0]["iters"])
    # between shard counts, as tests/test_gpu_multiproc.py::test_refine_distributed_real_engines_on_one_gpu
    n = min(5, iters, itR)
    assert np.array_equal(outs[0]["trace"][:n, 3], trR[:n, 3])
    assert np.allclose(outs[0]["trace"][:n, 1:3], trR[:n, 1:3], rtol=1e-9)
    assert abs(iters - itR) <= 2
    assert np.abs(P[:L] - PR[:L]).max() <= 1e-9 * max(1.0, np.abs(PR[:L]).max())
    assert np.abs(P - PR).max() <= 1e-7 * max(1.0, np.abs(PR).max())


# ---- 8. pose-only ----------------------------------------------------------------------------------------------
def posesYardstick(model, shared, poses0, offs, s, m, maxIters):
    """the reference's loop (src/calibrate.py:143-171) per view on the six view columns of orc.jacobianCompact
    -> (poses (M,6), error before the last update (M,), iterations (M,))"""
    L = orc.numShared(model)
    M = len(offs) - 1
    out, errs, its = np.array(poses0, dtype=np.float64).reshape(M, 6).copy(), np.zeros(M), np.zeros(M, dtype=int)
    for v in range(M):
        a, b = int(offs[v]), int(offs[v + 1])
        o1 = np.array([0, b - a])
        sv, mv = np.asarray(s)[a:b], np.asarray(m)[a:b]
        e, lam = out[v].copy(), orc.LAMBDA_INITIAL
        for it in range(maxIters):
            P = np.concatenate((shared, e))
            J = orc.jacobianCompact(model, P, o1, mv)[:, :, L:].reshape(-1, 6)
            r = (sv - orc.projectAllPoints(model, P, o1, mv)).reshape(-1, 1)
            JTJ = J.T @ J
            delta = (np.linalg.inv(JTJ + lam * np.diag(np.diagonal(JTJ))) @ J.T @ r).ravel()
            err = orc.reprojectionError(model, P, o1, sv, mv)
            err1 = orc.reprojectionError(model, np.concatenate((shared, e + delta)), o1, sv, mv)
            its[v], errs[v] = it + 1, err
            if err1 < err:
                e = e + delta
                lam /= 10
            else:
                lam *= 10
            if not (orc.LAMBDA_MIN < lam < orc.LAMBDA_MAX) or err < orc.PT_ERROR_MIN:
                break
        out[v] = e
    return out, errs, its


def transforms(model, shared, poses):
    return orc.decomposeParameterVector(np.concatenate((shared, np.asarray(poses).ravel())), model)[1]


def sharedTrue(g):
    A = g["Atrue"]
    return np.concatenate(([A[0, 0], A[1, 1], A[0, 1], A[0, 2], A[1, 2]], g["ktrue"]))


@pytest.mark.parametrize("name", ["radtan", "fisheye"])
def test_pose_only_refinement_vs_the_per_view_yardstick(name):
    tag, model = GOLDENS[name]
    g = loadGolden(tag)
    L = orc.numShared(model)
    offs, s, m = g["viewOffsets"], g["sensorPoints"], g["modelPoints"]
    shared, poses0 = sharedTrue(g), g["P0"][L:].reshape(-1, 6)
    sse, poses, iters, status = engine.refinePoses(engine.MODEL_IDS[name], shared, poses0, offs, s, m, 20)
    pY, eY, iY = posesYardstick(model, shared, poses0, offs, s, m, 20)
    W, WY = transforms(model, shared, poses), transforms(model, shared, pY)
    dY, dT = np.abs(W - WY).reshape(len(W), -1).max(axis=1), np.abs(W - g["Wtrue"]).reshape(len(W), -1).max(axis=1)
    yT = np.abs(WY - g["Wtrue"]).reshape(len(W), -1).max(axis=1)
    print(f"{name}: iters {iters.tolist()} (yardstick {iY.tolist()}), sse max {sse.max():.3e} (yardstick {eY.max():.3e})\n"
          f"  max |W - WY| {dY.max():.3e}, max |W - Wtrue| {dT.max():.3e}, yardstick to truth {yT.max():.3e}")
    assert np.all(status == 0)
    assert np.all(np.abs(iters - iY) <= 1)
    # measured: 6.7e-16 from the yardstick, 2.1e-15 / 1.0e-15 from Wtrue (the yardstick itself 2.2e-15 / 7.8e-16), so
    # the plain 1e-9 bar holds for every view and no view needs a bound derived from the stop threshold
    assert np.all(dY < 1e-9) and np.all(dT < 1e-9)
    # the Calibrator's form of the same call: (A, W, k) in, transforms out
    cal = cca.Calibrator(cca.RadialTangentialModel() if name == "radtan" else cca.FisheyeModel())
    W0 = orc.decomposeParameterVector(g["P0"], model)[1]
    sse2, W2, it2, st2 = cal.refinePoses(g["Atrue"], list(W0), g["ktrue"], _detections(g), 20)
    assert np.all(st2 == 0) and np.abs(np.array(W2) - g["Wtrue"]).max() < 1e-9
    # the global loop with every shared parameter fixed: one lambda and one decision for all views, the same poses
    P0 = np.concatenate((shared, poses0.ravel()))
    cal.setFixed("all")
    sseG, PG, itG, trG = cal.refinePacked(P0, offs, s, m, 60)
    cal.close()
    WG = orc.decomposeParameterVector(PG, model)[1]
    print(f"  global loop, fixed='all': {itG} iterations, sse {sseG:.3e}, max |WG - W| {np.abs(WG - W).max():.3e}")
    assert np.array_equal(PG[:L], shared)
    assert np.abs(WG - W).max() < 1e-9


def test_pose_only_refinement_ragged_batch_and_a_two_point_view():
    g = loadGolden("g5_ragged200.npz")
    offs, s, m = g["viewOffsets"], g["sensorPoints"], g["modelPoints"]
    L = 10
    shared, poses0 = g["Ptrue"][:L], g["P0"][L:].reshape(-1, 6)
    sse, poses, iters, status = engine.refinePoses(nat.MODEL_RADTAN, shared, poses0, offs, s, m, 20)
    pY, eY, iY = posesYardstick(orc.RADTAN, shared, poses0, offs, s, m, 20)
    W, WY = transforms(orc.RADTAN, shared, poses), transforms(orc.RADTAN, shared, pY)
    WT = transforms(orc.RADTAN, shared, g["Ptrue"][L:])
    print(f"ragged200: iters {np.bincount(iters).tolist()} (yardstick {np.bincount(iY).tolist()}), "
          f"max |W - WY| {np.abs(W - WY).max():.3e}, max |W - Wtrue| {np.abs(W - WT).max():.3e}, "
          f"yardstick to truth {np.abs(WY - WT).max():.3e}")
    assert np.all(status == 0) and np.all(np.abs(iters - iY) <= 1)
    assert np.abs(W - WY).max() < 1e-9 and np.abs(W - WT).max() < 1e-9
    # the same batch with view 3 cut down to two points: that view fails alone and keeps its input pose
    keep = np.ones(int(offs[-1]), dtype=bool)
    keep[int(offs[3]) + 2:int(offs[4])] = False
    counts = np.diff(offs).copy()
    counts[3] = 2
    offs2 = np.concatenate(([0], np.cumsum(counts)))
    sse2, poses2, iters2, status2 = engine.refinePoses(nat.MODEL_RADTAN, shared, poses0, offs2, s[keep], m[keep], 20)
    others = np.arange(len(counts)) != 3
    assert status2[3] == nat.E_SINGULAR and np.array_equal(poses2[3], poses0[3]) and iters2[3] == 0
    assert np.all(status2[others] == 0)
    assert np.array_equal(poses2[others], poses[others]) and np.array_equal(iters2[others], iters[others])
    assert np.array_equal(sse2[others], sse[others])
    with pytest.raises(ValueError):
        engine.refinePoses(nat.MODEL_RADTAN, shared, poses0, offs, s, m, 0)       # CALIB_E_INVALID


def test_estimate_poses_from_detections_with_a_known_camera():
    g = loadGolden("g2_config1_radtan.npz")
    sse, W, iters, status = cca.estimatePoses(_detections(g), "radtan", g["Atrue"], g["ktrue"])
    print(f"estimatePoses: iters {iters.tolist()}, max |W - Wtrue| {np.abs(np.array(W) - g['Wtrue']).max():.3e}")
    assert np.all(status == 0) and len(W) == len(g["Wtrue"])
    for we, wc in zip(g["Wtrue"], W):              # the bar of test_end_to_end_calibrate_matches_reference for W
        assert np.allclose(we, wc, atol=1e-6)
